"""A batch of QPs as a differentiable PyTorch layer: the forward pass is update -> solve -> polish on a live
BatchOSQP handle, the backward pass is BatchOSQP.adjoint (osqp_amd_batch_adjoint: one more solve with the KKT
matrix of the active rows, on the device).

Inputs and outputs are float64 tensors on the CPU or the GPU.  In this version they are staged through host numpy
arrays on their way to and from the handle (the C entry points take host pointers); device-pointer inputs are a
later change.  The solve, the polish and the adjoint themselves run on the device.
Tensors on the GPU take the same route (`.cpu()` in, `torch.as_tensor(..., device=...)` out); the tests exercise CPU
tensors only, so that path is untested.

A torch wheel may carry a HIP runtime of its own.  A process that imports torch before the library is first loaded
runs both on torch's copy; one that loads the library first maps two runtimes side by side, which host staging
does not mind, but a later `ctypes.CDLL("libamdhip64.so")` of the caller's then names torch's copy, not the
library's.  Import torch first (bench.py does) where that matters."""
import numpy as np
import torch
from scipy import sparse

from .batch import BatchOSQP


def _host(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy())


class _BatchQPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, Q, L, U, Px, Ax):
        args = tuple(_host(t) for t in (Q, L, U, Px, Ax))
        r = layer._solve(*args)
        ctx.layer, ctx.args, ctx.serial = layer, args, layer._serial
        ctx.set_materialize_grads(False)
        like = dict(dtype=Q.dtype, device=Q.device)
        return torch.as_tensor(r.x, **like), torch.as_tensor(r.y, **like)

    @staticmethod
    def backward(ctx, gX, gY):
        layer = ctx.layer
        need = ctx.needs_input_grad[1:]
        if not any(need) or (gX is None and gY is None):
            return (None,) * 6
        if layer._serial != ctx.serial:      # the handle has solved another problem since: bring this one back
            layer._solve(*ctx.args)
            ctx.serial = layer._serial
        ref = gX if gX is not None else gY
        dX = np.zeros((layer.h.B, layer.h.n)) if gX is None else _host(gX)
        a = layer.h.adjoint(dX, _host(gY), matrices=need[3] or need[4])
        layer.last_status_adjoint = a.status_adjoint
        outs = (a.dq, a.dl, a.du, a.dPx, a.dAx)
        return (None,) + tuple(torch.as_tensor(g, dtype=ref.dtype, device=ref.device) if w else None
                               for g, w in zip(outs, need))


class BatchQPLayer(torch.nn.Module):
    """x*(Q, L, U, Px, Ax) = argmin 1/2 x'Px + q'x  s.t.  l <= Ax <= u for a batch of QPs with the shared sparsity
    pattern of P (n x n; the upper triangle is used) and A (m x n), differentiable in every argument.

        layer = BatchQPLayer(P, A, engine="auto", eps_abs=1e-6, eps_rel=1e-6)
        X = layer(Q, L, U)                       # [B, n]; Q [B, n], L, U [B, m]
        X, Y = layer(Q, L, U, Ax=Ax, return_y=True)   # Px [B, nnz(triu P)], Ax [B, nnz(A)] in CSC order; None = P's, A's

    polish=True polishes the solved members after every solve (BatchOSQP.polish), so the point differentiated is the
    polished one where polish is accepted.  engine and **settings are BatchOSQP.setup's (the handle is set up at the
    first call and kept: later calls update it, and solves are warm-started unless warm_start=0).  Gradients come
    back for exactly the inputs that require them.  A gradient with respect to an off-diagonal Px slot counts both
    halves of the symmetric P.  Members whose solve did not end `solved` (or whose KKT matrix is rejected) get zero
    gradients; `last_status_adjoint` [B] (1 computed, -1 rejected, 0 not tried) and `last_results` say which.  Where active
    rows are linearly dependent or strict complementarity fails, the gradients are those of the guessed active set.

    Tensors are float64, on the CPU or the GPU; they are staged through host numpy arrays in this version."""

    def __init__(self, P, A, engine="auto", polish=True, **settings):
        super().__init__()
        self.P = sparse.triu(sparse.csc_matrix(P), format="csc"); self.P.sort_indices()
        self.A = sparse.csc_matrix(A); self.A.sort_indices()
        self.engine, self.polish, self.settings = engine, polish, settings
        self.h = None
        self._serial = 0
        self._own = [False, False]       # the handle holds per-member values of P / A given by a caller
        self.last_results = self.last_status_adjoint = None

    def _solve(self, Q, L, U, Px, Ax):
        if self.h is not None and self.h.B != Q.shape[0]:
            self.h.cleanup(); self.h = None
        if self.h is None:
            self.h = BatchOSQP().setup(self.P, self.A, Q, L, U, Px_all=Px, Ax_all=Ax, engine=self.engine, **self.settings)
        else:
            rc = self.h.update(Q=Q, L=L, U=U)
            if rc:
                raise RuntimeError("BatchOSQP.update failed (%d)" % rc)
            # values a caller gave last time and not this time go back to the layer's own
            vP = Px if Px is not None else (self.P.data if self._own[0] else None)
            vA = Ax if Ax is not None else (self.A.data if self._own[1] else None)
            if vP is not None or vA is not None:
                rc = self.h.update_matrices(Px=vP, Ax=vA)
                if rc:
                    raise RuntimeError("BatchOSQP.update_matrices failed (%d)" % rc)
        self._own = [Px is not None, Ax is not None]
        self.h.solve(fetch=False)
        self.last_results = self.h.polish() if self.polish else self.h.results()
        self._serial += 1
        return self.last_results

    def forward(self, Q, L, U, Px=None, Ax=None, return_y=False):
        B = Q.shape[0] if Q.dim() == 2 else -1
        n, m = self.P.shape[0], self.A.shape[0]
        for name, t, cols in (("Q", Q, n), ("L", L, m), ("U", U, m), ("Px", Px, self.P.nnz), ("Ax", Ax, self.A.nnz)):
            if t is None:
                continue
            if t.dtype != torch.float64:
                raise TypeError("%s must be a float64 tensor, not %s" % (name, t.dtype))
            if tuple(t.shape) != (B, cols):
                raise ValueError("%s must be [B, %d], not %s" % (name, cols, tuple(t.shape)))
        X, Y = _BatchQPFunction.apply(self, Q, L, U, Px, Ax)
        return (X, Y) if return_y else X

    def cleanup(self):
        if self.h is not None:
            self.h.cleanup(); self.h = None
