"""One-QP-per-stream batches: every `OSQP` workspace owns a HIP stream, so several
independent QPs of any size can be in flight on one GPU.  `osqp_solve` blocks its
calling thread between windows, therefore the solves are driven from a small
thread pool (ctypes drops the GIL inside the C call).  For many *small* QPs with
one sparsity pattern use `BatchOSQP` instead (one workgroup per QP)."""
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
from scipy import sparse


def solve_many(solvers, max_workers=4):
    """Solve the given set-up `OSQP` objects concurrently; returns their results in order."""
    if len(solvers) <= 1 or max_workers <= 1:
        return [s.solve() for s in solvers]
    with ThreadPoolExecutor(max_workers=min(max_workers, len(solvers))) as ex:
        return list(ex.map(lambda s: s.solve(), solvers))


class PerMemberBatch:
    """The one-engine-per-member route of BatchOSQP (engine="auto", n above the tiled kernel's size): one `OSQP` per
    member, solved through solve_many.  BatchOSQP keeps it as `_many` and hands over arguments it has checked already, as
    the batch engines get them: contiguous float64 host arrays, bounds clamped, L <= U.  The calls that go member by
    member return the first non-zero code of a member and leave its index in `last_update_failed` (None: none)."""

    def __init__(self, P, A, Q, L, U, Px_all, Ax_all, device, settings):
        from . import OSQP, engine_options, set_engine_options
        self.B, self.m = L.shape
        self.members, self._last, self.last_update_failed = [], None, None
        old = engine_options()["device"]
        set_engine_options(device=device)
        try:
            Pf, Af = sparse.csc_matrix(P), sparse.csc_matrix(A)
            for b in range(self.B):
                Pb, Ab = Pf.copy(), Af.copy()
                if Px_all is not None:
                    Pb = sparse.triu(Pf, format="csc"); Pb.sort_indices(); Pb.data = Px_all[b].copy()
                if Ax_all is not None:
                    Ab.sort_indices(); Ab.data = Ax_all[b].copy()
                try:
                    self.members.append(OSQP().setup(P=Pb, q=Q[b], A=Ab, l=L[b], u=U[b], **settings))
                except ValueError as e:       # e.g. error 5 (non-convex member), as the kernel path reports it
                    self.cleanup()
                    raise ValueError("%s (QP %d of the batch)" % (e, b)) from None
        finally:
            set_engine_options(device=old)

    def _each(self, call):
        self.last_update_failed = None
        for b, s in enumerate(self.members):
            rc = call(b, s)
            if rc:
                self.last_update_failed = b
                return rc
        return 0

    def update(self, Q, L, U):
        row = lambda V, b: None if V is None else V[b]
        return self._each(lambda b, s: s.update(q=row(Q, b), l=row(L, b), u=row(U, b)))

    def update_matrices(self, Px, Px_idx, pper, Ax, Ax_idx, aper):
        """As check_matrix_update returns them: values [k] or, with the per-member flag, [B, k]."""
        return self._each(lambda b, s: s.update(Px=None if Px is None else (Px[b] if pper else Px), Px_idx=Px_idx,
                                                Ax=None if Ax is None else (Ax[b] if aper else Ax), Ax_idx=Ax_idx))

    def update_rho(self, rho, per):
        """rho: [B] (per) or [1] values; 1, with nothing changed, when one of them is <= 0 (as the batch engines answer)."""
        if np.any(rho <= 0):
            return 1
        return self._each(lambda b, s: s.update_rho(rho[b if per else 0]))

    def warm_start(self, X, Y):
        return self._each(lambda b, s: s.warm_start(x=None if X is None else X[b], y=None if Y is None else Y[b]))

    def solve(self):
        self._last = solve_many(self.members, max_workers=8)

    def results(self):
        """The members' last results as the arrays of BatchOSQP.results (info_raw [B, 8] in the order of INFO_FIELDS)."""
        rs = self._last
        info = np.array([[r.info.iter, r.info.status_val, r.info.obj_val, r.info.pri_res, r.info.dua_res, r.info.rho_updates,
                          r.info.rho_estimate, s.settings().rho] for r, s in zip(rs, self.members)], dtype=np.float64)
        return SimpleNamespace(x=np.array([r.x for r in rs]), y=np.array([r.y for r in rs]).reshape(self.B, self.m),
                               dual_inf_cert=np.array([r.dual_inf_cert for r in rs]),
                               prim_inf_cert=np.array([r.prim_inf_cert for r in rs]).reshape(self.B, self.m), info_raw=info)

    def cleanup(self):
        for s in self.members:
            s.cleanup()
        self.members = []
