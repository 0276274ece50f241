"""QPs as differentiable PyTorch layers: BatchQPLayer over the batch engines and, at the end of the file, QPLayer over the
single-QP engine (OSQP.adjoint / OSQP.tangent).

A batch of QPs as a differentiable PyTorch layer: the forward pass is update -> solve -> polish on a live
BatchOSQP handle, the backward pass is BatchOSQP.adjoint (osqp_amd_batch_adjoint: one more solve with the KKT
matrix of the active rows, on the device), and forward-mode tangents come from BatchOSQP.tangent the same way.

Inputs and outputs are float64 tensors on the CPU or the GPU, and the route follows Q (`layer.last_route`).
CPU tensors ("host") are staged through numpy arrays on their way to and from the handle.  CUDA tensors ("device") set
the handle up once from host copies (setup takes host pointers) on the tensors' device; every later call on the live
handle hands the tensors' device pointers to the handle (the osqp_amd_batch_*_dev entry points through
BatchOSQP.update / update_matrices / results_into / adjoint_into): no [B, .] array crosses to the host, forward or
backward, and the outputs are tensors on that device.  The handle works on a stream of its own, so the layer
synchronises torch's current stream before each hand-over, and every call returns with the handle's work complete.
The solve, the polish and the adjoint themselves run on the device on either route.

A torch wheel may carry a HIP runtime of its own.  A process that imports torch before the library is first loaded
runs both on torch's copy; one that loads the library first maps two runtimes side by side.  Host staging does not
mind that, but the device route does: torch's allocations are then unknown to the library's runtime, the pointer check
of the _dev calls refuses them (error 1) and the layer raises.  A later `ctypes.CDLL("libamdhip64.so")` of the
caller's likewise names torch's copy, not the library's.  Import torch first (bench.py does)."""
import numpy as np
import torch
from types import SimpleNamespace

from scipy import sparse

from .batch import BatchOSQP


def _host(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy())


def _dev(t):
    return None if t is None else t.detach().contiguous()


def _hand_over(device):
    """The handle reads and writes on its own stream: what torch has queued for these tensors has to be done first."""
    torch.cuda.current_stream(device).synchronize()


class _HostSide:
    """The array adapter of the host route: what a layer does with tensors on their way to and from a handle that takes
    and returns host numpy arrays (BatchOSQP's host forms, OSQP).  `like`: the dtype and device the outputs take."""
    route, index, where = "host", None, {}
    update_failed = "BatchOSQP.update failed (%d)%s"
    take = staticmethod(_host)                   # a tensor as the handle takes it
    host = staticmethod(lambda a: a)             # ... and what take() gave as setup and _class_clash take it
    hand_over = staticmethod(lambda: None)       # (numpy arrays are complete when they are made)
    bounds = staticmethod(lambda L, U, m: (L, U))

    def __init__(self, like):
        self.like = dict(dtype=like.dtype, device=like.device)

    def save(self, ctx, tensors, args):
        ctx.args = args

    def saved(self, ctx):
        return ctx.args

    def outputs(self, r):
        return torch.as_tensor(r.x, **self.like), torch.as_tensor(r.y, **self.like)

    def own(self, layer, which):
        return (layer.P if which == "P" else layer.A).data

    def results(self, h, polish):
        return h.polish() if polish else h.results()

    def adjoint(self, layer, gX, gY, need, ref):
        """(dq, dl, du, dPx, dAx) -- None where not needed --, and the call's result for the layer's status attributes."""
        h = layer.h
        dX = np.zeros(((h.B,) if layer.batched else ()) + (h.n,)) if gX is None else _host(gX)
        a = h.adjoint(dX, _host(gY), matrices=need[3] or need[4])
        return [torch.as_tensor(g, dtype=ref.dtype, device=ref.device) if w else None
                for g, w in zip((a.dq, a.dl, a.du, a.dPx, a.dAx), need)], a

    def tangent(self, layer, tangents):
        r = layer.h.tangent(*(_host(t) for t in tangents))
        like = dict(dtype=torch.float64, device=next((t.device for t in tangents if t is not None), "cpu"))
        return torch.as_tensor(r.dx, **like), torch.as_tensor(r.dy, **like), r


class _DeviceSide:
    """The array adapter of the device route (BatchQPLayer on CUDA tensors): contiguous tensors go to the handle's _dev
    forms as they are, outputs are torch.empty on the device and filled by the _into calls, and torch's current stream is
    synchronised before every hand-over (the handle works on a stream of its own)."""
    route, take = "device", staticmethod(_dev)
    host = staticmethod(_host)
    update_failed = ("BatchOSQP.update failed (%d: some lower bound exceeds its upper bound, or a tensor is not device memory "
                     "the library's HIP runtime knows -- import torch before the library is first loaded)%s")

    def __init__(self, like):
        self.device = like.device
        self.index = like.device.index if like.device.index is not None else torch.cuda.current_device()
        self.where = dict(device=self.index)

    def hand_over(self):
        _hand_over(self.device)

    def new(self, *shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def save(self, ctx, tensors, args):
        ctx.save_for_backward(*tensors)
        ctx.save_for_forward(*tensors)           # (jvp sees only these)

    def saved(self, ctx):
        return tuple(_dev(t) for t in ctx.saved_tensors)

    def outputs(self, r):
        # (tensor objects of their own, so that last_results stays outside the graph; they share its storage, as the
        # host route's outputs share the numpy arrays of last_results)
        return r.x.detach(), r.y.detach()

    def bounds(self, L, U, m):
        return (L, U) if m else (None, None)

    def own(self, layer, which):
        if which not in layer._vals or layer._vals[which].device != self.device:
            layer._vals[which] = torch.as_tensor((layer.P if which == "P" else layer.A).data, dtype=torch.float64,
                                                 device=self.device)
        return layer._vals[which]

    def results(self, h, polish):
        if polish:
            h.polish(fetch=False)
        X, Y, sp = self.new(h.B, h.n), self.new(h.B, h.m), self.new(h.B, dtype=torch.int32)
        self.hand_over()
        h.results_into(X=X, Y=Y if h.m else None, status_polish=sp)
        return SimpleNamespace(x=X, y=Y, status_polish=sp)

    def adjoint(self, layer, gX, gY, need, ref):
        h, m = layer.h, layer.h.m > 0
        # both inputs are made contiguous here, before the hand-over: a copy queued on torch's stream after it
        # would race with the handle's stream (the gradient of a sum is an expanded, non-contiguous tensor)
        dX = torch.zeros((h.B, h.n), dtype=torch.float64, device=self.device) if gX is None else _dev(gX)
        dY = _dev(gY) if m else None
        g = dict(dq=self.new(h.B, h.n), dl=self.new(h.B, h.m) if m else None, du=self.new(h.B, h.m) if m else None,
                 dPx=self.new(h.B, h.Pu.nnz) if need[3] else None, dAx=self.new(h.B, h.Ah.nnz) if need[4] else None)
        sa = self.new(h.B, dtype=torch.int32)
        self.hand_over()
        h.adjoint_into(dX, dY, status_adjoint=sa, **g)
        zero = lambda w: self.new(h.B, 0).zero_() if w else None        # (m = 0: the empty gradients of L, U)
        return [g["dq"], g["dl"] if m else zero(need[1]), g["du"] if m else zero(need[2]), g["dPx"], g["dAx"]], \
            SimpleNamespace(status_adjoint=sa)

    def tangent(self, layer, tangents):
        h, m = layer.h, layer.h.m > 0
        tQ, tL, tU, tPx, tAx = tangents
        # made contiguous before the hand-over, as in adjoint
        t = dict(dQ=_dev(tQ), dL=_dev(tL) if m else None, dU=_dev(tU) if m else None, dPx=_dev(tPx), dAx=_dev(tAx))
        tX, tY, st = self.new(h.B, h.n), self.new(h.B, h.m), self.new(h.B, dtype=torch.int32)
        self.hand_over()
        h.tangent_into(tX, tY if m else None, status_tangent=st, **t)
        return tX, tY, SimpleNamespace(status_tangent=st)


def _bring_back(ctx):
    """The layer of a graph, its handle holding the graph's problem: where the handle has solved another one since, this
    one is solved again."""
    layer = ctx.layer
    if layer._serial != ctx.serial:
        layer._solve(ctx.side, *ctx.side.saved(ctx))
        ctx.serial = layer._serial
    return layer


class _QPFunction(torch.autograd.Function):
    """Both layers' autograd function: the route of a call is the adapter the layer chooses for its first input."""

    @staticmethod
    def forward(ctx, layer, Q, L, U, Px, Ax):
        ctx.layer, ctx.side = layer, layer._side(Q)
        args = tuple(ctx.side.take(t) for t in (Q, L, U, Px, Ax))
        ctx.side.save(ctx, (Q, L, U, Px, Ax), args)
        ctx.set_materialize_grads(False)
        r = layer._solve(ctx.side, *args)
        ctx.serial = layer._serial
        return ctx.side.outputs(r)

    @staticmethod
    def backward(ctx, gX, gY):
        need = ctx.needs_input_grad[1:]
        if not any(need) or (gX is None and gY is None):
            return (None,) * 6
        layer = _bring_back(ctx)
        outs, a = ctx.side.adjoint(layer, gX, gY, need, gX if gX is not None else gY)
        layer._note("adjoint", a)
        outs = outs[:3] + [layer._shared_grad(g) for g in outs[3:]]
        return (None,) + tuple(g if w else None for g, w in zip(outs, need))

    @staticmethod
    def jvp(ctx, _, tQ, tL, tU, tPx, tAx):
        """Forward mode (torch.autograd.forward_ad): the tangents of X and Y from those of Q, L, U, Px, Ax (None = 0)
        by the handle's tangent on the host route and tangent_into on the device route."""
        layer = ctx.layer
        tPx, tAx = layer._shared_tangent(tPx), layer._shared_tangent(tAx)
        _bring_back(ctx)
        tX, tY, r = ctx.side.tangent(layer, (tQ, tL, tU, tPx, tAx))
        layer._note("tangent", r)
        return tX, tY


_BatchQPFunction = _QPFunction       # (the name it had while each layer had a function of its own)


class _Layer(torch.nn.Module):
    """What BatchQPLayer and QPLayer share: the pattern of P and A, one live handle `h`, which of P / A hold values a
    caller gave (`_own`), the count of solves (`_serial`: a graph whose count is not the layer's has to bring its problem
    back before it is differentiated) and the checks of forward.  `batched`: shapes carry a leading B."""
    batched = True

    def __init__(self, P, A):
        super().__init__()
        self.P = sparse.triu(sparse.csc_matrix(P), format="csc"); self.P.sort_indices()
        self.A = sparse.csc_matrix(A); self.A.sort_indices()
        self.h = None
        self._serial = 0
        self._own = [False, False]       # the handle holds values of P / A given by a caller
        self.last_results = self.last_status_adjoint = self.last_status_tangent = None

    def _side(self, Q):
        return _HostSide(Q)

    def _shared_grad(self, g):
        return g

    def _shared_tangent(self, t):
        return t

    def _note(self, which, r):
        setattr(self, "last_status_" + which, getattr(r, "status_" + which))

    def _values(self, side, Px, Ax):
        """The values to bring to a live handle: the caller's, or -- where a caller gave some last time and none this
        time -- the layer's own again; None: the handle holds the right ones."""
        return (Px if Px is not None else (side.own(self, "P") if self._own[0] else None),
                Ax if Ax is not None else (side.own(self, "A") if self._own[1] else None))

    def _solved(self, results, Px, Ax):
        self._own = [Px is not None, Ax is not None]
        self.last_results = results
        self._serial += 1
        return results

    def _check(self, tensors, shared=False):
        """dtype, shape and device of the inputs of forward; shared: Px / Ax may be the [k] values of one shared model."""
        names = ("Q", "L", "U", "Px", "Ax") if self.batched else ("q", "l", "u", "Px", "Ax")
        first = tensors[0]
        lead = (first.shape[0] if first.dim() == 2 else -1,) if self.batched else ()
        n, m = self.P.shape[0], self.A.shape[0]
        for name, t, cols in zip(names, tensors, (n, m, m, self.P.nnz, self.A.nnz)):
            if t is None:
                continue
            if t.dtype != torch.float64:
                raise TypeError("%s must be a float64 tensor, not %s" % (name, t.dtype))
            if shared and name in ("Px", "Ax") and t.dim() == 1:       # the shared model's values
                if tuple(t.shape) != (cols,):
                    raise ValueError("%s must be [%d] (the shared model of engine='common'), not %s" % (name, cols, tuple(t.shape)))
            elif tuple(t.shape) != lead + (cols,):
                raise ValueError("%s must be [%s%d], not %s" % (name, "B, " if self.batched else "", cols, tuple(t.shape)))
            if t.device != first.device:
                raise ValueError("%s is on %s and %s on %s: every tensor of a call lives on one device"
                                 % (name, t.device, names[0], first.device))

    def cleanup(self):
        if self.h is not None:
            self.h.cleanup(); self.h = None


class BatchQPLayer(_Layer):
    """x*(Q, L, U, Px, Ax) = argmin 1/2 x'Px + q'x  s.t.  l <= Ax <= u for a batch of QPs with the shared sparsity
    pattern of P (n x n; the upper triangle is used) and A (m x n), differentiable in every argument.

        layer = BatchQPLayer(P, A, engine="auto", eps_abs=1e-6, eps_rel=1e-6)
        X = layer(Q, L, U)                       # [B, n]; Q [B, n], L, U [B, m]
        X, Y = layer(Q, L, U, Ax=Ax, return_y=True)   # Px [B, nnz(triu P)], Ax [B, nnz(A)] in CSC order; None = P's, A's

    polish=True polishes the solved members after every solve (BatchOSQP.polish), so the point differentiated is the
    polished one where polish is accepted.  engine and **settings are BatchOSQP.setup's (the handle is set up at the
    first call and kept: later calls update it, and solves are warm-started unless warm_start=0).  engine="common" (one
    model, many right-hand sides) needs shared_kkt=True, takes Px [nnz(triu P)] and Ax [nnz(A)] as the values of the one
    shared model (1-D; later calls bring them to the live handle through BatchOSQP.update_model, their gradient is the
    sum over the members and a tangent counts for every member) and no per-member [B, k] values, and raises RuntimeError
    naming member and row when the bounds of a call give a row different classes in two members.  Gradients come
    back for exactly the inputs that require them.  A gradient with respect to an off-diagonal Px slot counts both
    halves of the symmetric P.  Members whose solve did not end `solved` (or whose KKT matrix is rejected) get zero
    gradients; `last_status_adjoint` [B] (1 computed, -1 rejected, 0 not tried) and `last_results` say which.  Where active
    rows are linearly dependent or strict complementarity fails, the gradients are those of the guessed active set.
    Forward mode works too: under `torch.autograd.forward_ad.dual_level()` the tangents of X and Y come from
    BatchOSQP.tangent (an input without a tangent counts as zero; `last_status_tangent` [B] as `last_status_adjoint`).

    Tensors are float64, all on the CPU (staged through host numpy arrays) or all on one GPU: CUDA tensors set the handle
    up on their device, and every later call and every backward pass on the live handle runs without a host copy of
    any [B, .] array; X, Y and the gradients are then tensors on that device, `last_results` carries device tensors
    x, y, status_polish (int32) and `last_status_adjoint` is one too.  `last_route` says which route the last call
    took: "host" or "device"."""

    def __init__(self, P, A, engine="auto", polish=True, **settings):
        if engine == "common" and not settings.get("shared_kkt"):
            raise ValueError("BatchQPLayer needs polish and adjoint, which the common-K engine (engine='common') does not "
                             "serve without its shared KKT pieces: pass shared_kkt=True, or use engine='auto' or 'streamed'")
        super().__init__(P, A)
        self.engine, self.polish, self.settings = engine, polish, settings
        self.last_route = None
        self._device = None              # device route: the device index the handle was set up on
        self._vals = {}                  # the layer's own P / A values as tensors on the handle's device

    def _side(self, Q):
        return _DeviceSide(Q) if Q.is_cuda else _HostSide(Q)

    def _shared_grad(self, g):
        """engine="common": the gradient of a shared value is the sum over the members of the adjoint's [B, k] rows."""
        return g.sum(0) if self.engine == "common" and g is not None else g

    def _shared_tangent(self, t):
        """engine="common": the tangent of a shared value, [k], as the [B, k] array tangent / tangent_into take."""
        return t.expand(self.h.B, -1) if self.engine == "common" and t is not None else t

    def _setup(self, Q, L, U, Px, Ax, **where):
        """The handle from host arrays.  engine="common": Px / Ax are the shared model's values, [k]."""
        if self.engine != "common":
            return BatchOSQP().setup(self.P, self.A, Q, L, U, Px_all=Px, Ax_all=Ax, engine=self.engine, **where, **self.settings)
        with_values = lambda M, v: M if v is None else sparse.csc_matrix((v, M.indices, M.indptr), shape=M.shape)
        return BatchOSQP().setup(with_values(self.P, Px), with_values(self.A, Ax), Q, L, U, engine=self.engine, **where,
                                 **self.settings)

    def _update_values(self, vP, vA):
        if self.engine == "common":
            rc, call = self.h.update_model(Px=vP, Ax=vA), "update_model"
        else:
            rc, call = self.h.update_matrices(Px=vP, Ax=vA), "update_matrices"
        if rc:
            raise RuntimeError("BatchOSQP.%s failed (%d)" % (call, rc))

    def _solve(self, side, Q, L, U, Px, Ax):
        """update -> solve -> polish -> results on the live handle, from what side.take() made of the inputs.  The first
        call, and one with another B or (device route) on another device, sets the handle up from host copies."""
        self.last_route = side.route
        if self.h is not None and (self.h.B != Q.shape[0] or (side.index is not None and self._device != side.index)):
            self.h.cleanup(); self.h = None
        m = self.A.shape[0] > 0
        side.hand_over()
        if self.h is None:
            self.h = self._setup(*(side.host(t) for t in (Q, L, U, Px, Ax)), **side.where)
            self._device = side.index
        else:
            Lb, Ub = side.bounds(L, U, m)
            rc = self.h.update(Q=Q, L=Lb, U=Ub)
            if rc:
                raise RuntimeError(side.update_failed % (rc, self._class_clash(side.host(L), side.host(U)) if m else ""))
            vP, vA = self._values(side, Px, Ax)
            if vP is not None or vA is not None:
                side.hand_over()
                self._update_values(vP, vA)
        self.h.solve(fetch=False)
        return self._solved(side.results(self.h, self.polish), Px, Ax)

    def _class_clash(self, L, U):
        """Why a common-K handle refused the bounds L, U [B, m] (host arrays): the first member and row whose class
        (loose / inequality / equality, on the scaled bounds as src/auxil.c:76-98 takes it) differs from member 0's;
        "" when the classes agree or the handle is of another engine."""
        if self.engine != "common" or L is None or U is None or not L.shape[1]:
            return ""
        E = self.h.member_workspace(0)["E"]
        ls, us = np.maximum(L, -1e30) * E, np.minimum(U, 1e30) * E
        cls = np.where((ls < -1e26) & (us > 1e26), -1, np.where(us - ls < 1e-4, 1, 0))
        bad = np.argwhere(cls != cls[0])
        if not bad.size:
            return ""
        return (": row %d of member %d has another class (loose / inequality / equality) than in member 0 -- the common-K "
                "engine needs one class per row over the batch" % (bad[0][1], bad[0][0]))

    def forward(self, Q, L, U, Px=None, Ax=None, return_y=False):
        common = self.engine == "common"
        self._check((Q, L, U, Px, Ax), shared=common)
        if common and any(t is not None and t.dim() != 1 for t in (Px, Ax)):
            raise ValueError("engine='common' shares P and A over the batch: the layer takes no Px / Ax per member ([B, k]); "
                             "pass the shared model's values as [k]")
        X, Y = _QPFunction.apply(self, Q, L, U, Px, Ax)
        return (X, Y) if return_y else X


class QPLayer(_Layer):
    """x*(q, l, u, Px, Ax) = argmin 1/2 x'Px + q'x  s.t.  l <= Ax <= u for ONE sparse QP on the single-QP engine (the
    engine of the large problems: no limit on n), differentiable in every argument.

        layer = QPLayer(P, A, eps_abs=1e-6, eps_rel=1e-6)
        x = layer(q, l, u)                            # [n]; q [n], l, u [m]
        x, y = layer(q, l, u, Ax=Ax, return_y=True)   # Px [nnz(triu P)], Ax [nnz(A)] in CSC order; None = P's, A's

    The forward pass is update -> solve on one live `OSQP` handle (set up at the first call and kept; **settings are
    OSQP.setup's, with polish=1 unless given), so the point differentiated is the polished one where polish is accepted.
    The backward pass is OSQP.adjoint, forward-mode tangents (`torch.autograd.forward_ad`) are OSQP.tangent; both share
    the KKT instance of the solved problem.  Gradients come back for exactly the inputs that require them; a gradient
    with respect to an off-diagonal Px slot counts both halves of the symmetric P.  A solve that did not end `solved`
    (or a failed KKT solve) gives zero gradients: `last_status_adjoint` / `last_status_tangent` (1 computed, -1 failed,
    0 not tried), `last_kkt_res` and `last_results` say which.

    Tensors are float64 on the CPU or on a GPU.  Tensors of either device are staged through host numpy arrays on their
    way to and from the handle (the single-QP engine's C ABI takes host pointers; a device-array route exists for the
    batch engines only, BatchQPLayer): the outputs and gradients come back on the inputs' device."""

    batched = False

    def __init__(self, P, A, **settings):
        super().__init__(P, A)
        self.settings = dict(polish=1, **settings) if "polish" not in settings else dict(settings)
        self.last_kkt_res = None

    def _note(self, which, r):
        super()._note(which, r)
        self.last_kkt_res = r.kkt_res

    def _solve(self, side, q, l, u, Px, Ax):
        from . import OSQP
        if self.h is None:
            P = self.P if Px is None else sparse.csc_matrix((Px, self.P.indices, self.P.indptr), shape=self.P.shape)
            A = self.A if Ax is None else sparse.csc_matrix((Ax, self.A.indices, self.A.indptr), shape=self.A.shape)
            self.h = OSQP().setup(P=P, q=q, A=A, l=l, u=u, **self.settings)
        else:
            vP, vA = self._values(side, Px, Ax)
            rc = self.h.update(q=q, l=l, u=u, Px=vP, Ax=vA)
            if rc:
                raise RuntimeError("OSQP.update failed (%d)" % rc)
        return self._solved(self.h.solve(), Px, Ax)

    def forward(self, q, l, u, Px=None, Ax=None, return_y=False):
        self._check((q, l, u, Px, Ax))
        x, y = _QPFunction.apply(self, q, l, u, Px, Ax)
        return (x, y) if return_y else x
