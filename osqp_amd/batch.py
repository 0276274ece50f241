"""Batched solves of many small QPs with a shared sparsity pattern (MPC-style,
BASELINE config 4) -- ctypes plumbing over include/osqp_amd_batch.h.  One
workgroup per QP on the GPU; see osqp_amd/csrc/batch.hip."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
from scipy import sparse

from . import _abi as abi
from ._lib import lib

BATCH_MAX_N = 128     # register-tiled K^-1 of the batch kernel (batch.hip)
STREAMED_MAX_N = 1024  # streamed-inverse engine (batch_streamed.h)
ENGINES = {"tiled": 0, "streamed": 1}   # OSQP_AMD_BATCH_TILED / _STREAMED
INFO_FIELDS = ["iter", "status_val", "obj_val", "pri_res", "dua_res", "rho_updates", "rho_estimate", "rho"]


def _bind(L):
    H = C.c_void_p
    L.osqp_amd_batch_setup.restype = abi.c_int
    L.osqp_amd_batch_setup.argtypes = [C.POINTER(H), abi.c_int, C.POINTER(abi.csc), C.POINTER(abi.csc),
                                       abi.c_float_p, abi.c_float_p, abi.c_float_p, abi.c_float_p,
                                       abi.c_float_p, C.POINTER(abi.OSQPSettings), abi.c_int]
    L.osqp_amd_batch_update.restype = abi.c_int
    L.osqp_amd_batch_update.argtypes = [H, abi.c_float_p, abi.c_float_p, abi.c_float_p]
    L.osqp_amd_batch_update_matrices.restype = abi.c_int
    L.osqp_amd_batch_update_matrices.argtypes = [H, abi.c_float_p, abi.c_int_p, abi.c_int, abi.c_int,
                                                 abi.c_float_p, abi.c_int_p, abi.c_int, abi.c_int]
    L.osqp_amd_batch_update_rho.restype = abi.c_int
    L.osqp_amd_batch_update_rho.argtypes = [H, abi.c_float_p, abi.c_int]
    L.osqp_amd_batch_warm_start.restype = abi.c_int
    L.osqp_amd_batch_warm_start.argtypes = [H, abi.c_float_p, abi.c_float_p]
    L.osqp_amd_batch_solve.restype = abi.c_int
    L.osqp_amd_batch_solve.argtypes = [H]
    L.osqp_amd_batch_polish.restype = abi.c_int
    L.osqp_amd_batch_polish.argtypes = [H, abi.c_int_p]
    L.osqp_amd_batch_adjoint.restype = abi.c_int
    L.osqp_amd_batch_adjoint.argtypes = [H] + [abi.c_float_p] * 7 + [abi.c_int_p] * 2
    L.osqp_amd_batch_get.restype = abi.c_int
    L.osqp_amd_batch_get.argtypes = [H, abi.c_float_p, abi.c_float_p, abi.c_float_p, abi.c_float_p, abi.c_float_p]
    L.osqp_amd_batch_cleanup.restype = None
    L.osqp_amd_batch_cleanup.argtypes = [H]
    L.osqp_amd_batch_setup_engine.restype = abi.c_int
    L.osqp_amd_batch_setup_engine.argtypes = [C.POINTER(H), abi.c_int, abi.c_int, C.POINTER(abi.csc), C.POINTER(abi.csc),
                                              abi.c_float_p, abi.c_float_p, abi.c_float_p, abi.c_float_p,
                                              abi.c_float_p, C.POINTER(abi.OSQPSettings), abi.c_int]
    L.osqp_amd_batch_shape.restype = abi.c_int
    L.osqp_amd_batch_shape.argtypes = [H, abi.c_int_p, abi.c_int_p]
    L.osqp_amd_batch_rounds.restype = abi.c_int
    L.osqp_amd_batch_rounds.argtypes = [H, abi.c_int_p, abi.c_int_p]
    L.osqp_amd_batch_member.restype = abi.c_int
    L.osqp_amd_batch_member.argtypes = [H, abi.c_int] + [abi.c_float_p] * 4 + [abi.c_int_p] + [abi.c_float_p] * 3 + [abi.c_int_p]


def _p(a):
    return C.cast(None, abi.c_float_p) if a is None else abi.fptr(a)


def check_matrix_update(B, nnzP, nnzA, Px=None, Px_idx=None, Ax=None, Ax_idx=None):
    """Shape and index checks of BatchOSQP.update_matrices, as interface.py: update makes them for one QP (the C
    entry point reads what the shapes promise).  A 1-D value array is shared by the batch, a 2-D one is [B, k];
    without an index list k is the matrix's nnz, with one it is the list's length.  Returns the arrays as the C
    side takes them: (Px, Px_idx, P per-member flag, Ax, Ax_idx, A per-member flag)."""
    out = []
    for name, V, I, nnz in (("P", Px, Px_idx, nnzP), ("A", Ax, Ax_idx, nnzA)):
        if V is None:
            if I is not None:
                raise ValueError("%sx_idx given without %sx" % (name, name))
            out += [None, None, 0]
            continue
        V = abi.as_f64(V)
        if V.ndim not in (1, 2):
            raise ValueError("%sx must be [k] (shared) or [B, k] (per member)" % name)
        if V.ndim == 2 and V.shape[0] != B:
            raise ValueError("%sx has %d rows, the batch has %d members" % (name, V.shape[0], B))
        k = V.shape[-1]
        if I is None:
            if k != nnz:
                raise ValueError("%sx has %d values per member, %s has %d non-zeros (pass %sx_idx for a partial update)"
                                 % (name, k, name, nnz, name))
        else:
            I = abi.as_i64(I)
            if I.ndim != 1 or I.size != k:
                raise ValueError("%sx_idx must be a vector as long as a member's %sx" % (name, name))
            if I.size and (I.min() < 0 or I.max() >= nnz):
                raise ValueError("%sx_idx out of range [0, %d)" % (name, nnz))
        out += [V, I, int(V.ndim == 2)]
    return tuple(out)


def check_adjoint(B, n, m, dX, dY=None):
    """Shape checks of BatchOSQP.adjoint, as update makes them: dX [B, n], dY [B, m] or None.  Returns the arrays as
    the C side takes them."""
    dX = abi.as_f64(dX)
    dY = None if dY is None else abi.as_f64(dY)
    if dX.shape != (B, n) or (dY is not None and dY.shape != (B, m)):
        raise ValueError("adjoint arrays must be dX [B, n], dY [B, m]")
    return dX, dY


class BatchOSQP:
    def __init__(self):
        self._lib = lib()
        _bind(self._lib)
        self._h = None
        self._status_polish = None

    def setup(self, P, A, Q, L, U, Px_all=None, Ax_all=None, device=None, engine="auto", **settings):
        """P (n x n, any triangle content; upper triangle is used), A (m x n): shared
        pattern/values.  Q [B, n], L, U [B, m].  Px_all / Ax_all [B, nnz] optional
        per-QP values in CSC order of triu(P) / A.  engine: "auto" (the register-tiled kernel for
        n <= 128, one single-QP engine per member above) or "streamed" (the streamed-inverse batch
        engine, K^-1 in HBM, any n <= 1024)."""
        from . import engine_options
        if engine not in ("auto", "streamed"):
            raise ValueError("engine must be 'auto' or 'streamed', not %r" % (engine,))
        self.engine = engine
        # neither path may hand back an unpolished or unclocked answer to a caller who asked for one: the batch
        # kernel implements neither, so both paths refuse them (OSQP_SETTINGS_VALIDATION_ERROR = 2)
        for k in ("polish", "time_limit"):
            if settings.get(k, 0) and settings[k] > 0:
                raise ValueError("osqp_amd_batch_setup failed with error 2: %s is not implemented by the batched engine" % k)
        self.Pu = abi.CscHolder(sparse.triu(P, format="csc"))
        self.Ah = abi.CscHolder(A)
        Q = abi.as_f64(Q)
        self.B, self.n = Q.shape
        self.m = self.Ah.m
        L = np.maximum(abi.as_f64(L), -abi.OSQP_INFTY)
        U = np.minimum(abi.as_f64(U), abi.OSQP_INFTY)
        if L.shape != (self.B, self.m) or U.shape != (self.B, self.m) or self.Pu.n != self.n or self.Ah.n != self.n:
            raise ValueError("dimension mismatch: Q [B, n], L, U [B, m], P n x n, A m x n")
        if np.any(L > U):
            raise ValueError("lower bound greater than upper bound")          # validate_data, src/auxil.c:868-875
        for nm, V, nnz in (("Px_all", Px_all, self.Pu.nnz), ("Ax_all", Ax_all, self.Ah.nnz)):
            if V is not None and np.shape(V) != (self.B, nnz):
                raise ValueError("%s must be [B, %d]" % (nm, nnz))
        st = abi.OSQPSettings()
        self._lib.osqp_set_default_settings.restype = None
        self._lib.osqp_set_default_settings.argtypes = [C.POINTER(abi.OSQPSettings)]
        self._lib.osqp_set_default_settings(C.byref(st))
        st.verbose = 0
        for k, v in settings.items():
            if k not in abi.SETTING_NAMES:
                raise ValueError("unknown setting %r" % k)
            setattr(st, k, v)
        if Px_all is not None:
            Px_all = abi.as_f64(Px_all)
        if Ax_all is not None:
            Ax_all = abi.as_f64(Ax_all)
        if device is None:
            device = engine_options()["device"]
        self._many = None
        if engine == "auto" and self.n > BATCH_MAX_N:
            # The one-workgroup-per-QP kernel keeps K^-1 in registers (n <= 128).  Larger members of a batch go
            # one QP per HIP stream through the single-QP engine (osqp_amd/multi.py): same results, the PCG path.
            from . import OSQP, set_engine_options
            old = engine_options()["device"]
            set_engine_options(device=device)
            try:
                Pf, Af = sparse.csc_matrix(P), sparse.csc_matrix(A)
                self._many = []
                for b in range(self.B):
                    Pb, Ab = Pf.copy(), Af.copy()
                    if Px_all is not None:
                        Pb = sparse.triu(Pf, format="csc"); Pb.sort_indices(); Pb.data = Px_all[b].copy()
                    if Ax_all is not None:
                        Ab.sort_indices(); Ab.data = Ax_all[b].copy()
                    try:
                        self._many.append(OSQP().setup(P=Pb, q=Q[b], A=Ab, l=L[b], u=U[b], **settings))
                    except ValueError as e:       # e.g. error 5 (non-convex member), as the kernel path reports it
                        for s in self._many:
                            s.cleanup()
                        self._many = None
                        raise ValueError("%s (QP %d of the batch)" % (e, b)) from None
            finally:
                set_engine_options(device=old)
            self._last = None
            return self
        h = C.c_void_p()
        if engine == "streamed":
            rc = self._lib.osqp_amd_batch_setup_engine(C.byref(h), ENGINES["streamed"], self.B, C.byref(self.Pu.struct),
                                                       C.byref(self.Ah.struct), _p(Px_all), _p(Ax_all), abi.fptr(Q),
                                                       _p(L if self.m else None), _p(U if self.m else None), C.byref(st),
                                                       device)
            if rc:
                raise ValueError("osqp_amd_batch_setup_engine failed with error %d" % rc)
        else:
            rc = self._lib.osqp_amd_batch_setup(C.byref(h), self.B, C.byref(self.Pu.struct), C.byref(self.Ah.struct),
                                                _p(Px_all), _p(Ax_all), abi.fptr(Q), _p(L if self.m else None),
                                                _p(U if self.m else None), C.byref(st), device)
            if rc:
                raise ValueError("osqp_amd_batch_setup failed with error %d" % rc)
        self._h = h
        return self

    def shape(self):
        """(engine, NP) of a kernel batch: engine 0 = tiled, 1 = streamed; K^-1 is NP x NP (padded)."""
        e = np.zeros(1, np.int64); npo = np.zeros(1, np.int64)
        if self._lib.osqp_amd_batch_shape(self._h, abi.iptr(e), abi.iptr(npo)):
            raise RuntimeError("osqp_amd_batch_shape failed")
        return int(e[0]), int(npo[0])

    def rounds(self):
        """Of the last solve: (launches of the ADMM loop, members whose K^-1 solve is refined)."""
        r = np.zeros(1, np.int64); f = np.zeros(1, np.int64)
        if self._lib.osqp_amd_batch_rounds(self._h, abi.iptr(r), abi.iptr(f)):
            raise RuntimeError("osqp_amd_batch_rounds failed")
        return int(r[0]), int(f[0])

    def _many_update(self, Q, L, U):
        # the first failing member's code comes back (and which member it was stays readable in `last_update_failed`)
        self.last_update_failed = None
        for b, s in enumerate(self._many):
            rc = s.update(q=None if Q is None else Q[b], l=None if L is None else L[b], u=None if U is None else U[b])
            if rc:
                self.last_update_failed = b
                return rc
        return 0

    def _many_results(self):
        rs = self._last
        X = np.array([r.x for r in rs]); Y = np.array([r.y for r in rs]).reshape(self.B, self.m)
        info = np.array([[r.info.iter, r.info.status_val, r.info.obj_val, r.info.pri_res, r.info.dua_res, r.info.rho_updates,
                          r.info.rho_estimate, s.settings().rho] for r, s in zip(rs, self._many)], dtype=np.float64)
        out = SimpleNamespace(x=X, y=Y, dual_inf_cert=np.array([r.dual_inf_cert for r in rs]),
                              prim_inf_cert=np.array([r.prim_inf_cert for r in rs]).reshape(self.B, self.m), info_raw=info)
        for k, name in enumerate(INFO_FIELDS):
            col = info[:, k]
            setattr(out, name, col.astype(np.int64) if name in ("iter", "status_val", "rho_updates") else col)
        return out

    def update(self, Q=None, L=None, U=None):
        Q = None if Q is None else abi.as_f64(Q)
        L = None if L is None else np.maximum(abi.as_f64(L), -abi.OSQP_INFTY)
        U = None if U is None else np.minimum(abi.as_f64(U), abi.OSQP_INFTY)
        if (Q is not None and Q.shape != (self.B, self.n)) or (L is not None and L.shape != (self.B, self.m)) or \
           (U is not None and U.shape != (self.B, self.m)):
            raise ValueError("update arrays must be Q [B, n], L [B, m], U [B, m]")
        if L is not None and U is not None and np.any(L > U):
            raise ValueError("lower bound greater than upper bound")
        if self._many is not None:
            return self._many_update(Q, L, U)
        return int(self._lib.osqp_amd_batch_update(self._h, _p(Q), _p(L), _p(U)))

    def _many_each(self, call):
        # as _many_update: the first failing member's code comes back
        self.last_update_failed = None
        for b, s in enumerate(self._many):
            rc = call(b, s)
            if rc:
                self.last_update_failed = b
                return rc
        return 0

    def update_matrices(self, Px=None, Px_idx=None, Ax=None, Ax_idx=None):
        """osqp_update_P / _A / _P_A for every QP: new values on the pattern of setup.  Px / Ax: [k] (shared by the
        batch) or [B, k] (per member); k = nnz of triu(P) / A in CSC order, or the length of Px_idx / Ax_idx (slots, one
        list for the batch).  Scaling is recomputed; rho, row classes and iterates stay.  Returns the C return code
        (5: some member's new K is not positive definite; solve then refuses until an update succeeds)."""
        Px, Px_idx, pper, Ax, Ax_idx, aper = check_matrix_update(self.B, self.Pu.nnz, self.Ah.nnz, Px, Px_idx, Ax, Ax_idx)
        if Px is None and Ax is None:
            return 0
        if self._many is not None:
            return self._many_each(lambda b, s: s.update(Px=None if Px is None else (Px[b] if pper else Px), Px_idx=Px_idx,
                                                         Ax=None if Ax is None else (Ax[b] if aper else Ax), Ax_idx=Ax_idx))
        ip = lambda a: C.cast(None, abi.c_int_p) if a is None else abi.iptr(a)
        return int(self._lib.osqp_amd_batch_update_matrices(
            self._h, _p(Px), ip(Px_idx), 0 if Px is None else Px.shape[-1], pper,
            _p(Ax), ip(Ax_idx), 0 if Ax is None else Ax.shape[-1], aper))

    def update_rho(self, rho):
        """osqp_update_rho for every QP: a scalar, or [B] values.  Returns 1 (nothing changed) when a value is <= 0."""
        rho = np.asarray(rho, dtype=np.float64)
        if rho.shape not in ((), (self.B,)):
            raise ValueError("rho must be a scalar or [B]")
        per = int(rho.ndim == 1)
        rho = np.ascontiguousarray(rho.reshape(-1))
        if self._many is not None:
            if np.any(rho <= 0):
                return 1
            return self._many_each(lambda b, s: s.update_rho(rho[b if per else 0]))
        return int(self._lib.osqp_amd_batch_update_rho(self._h, abi.fptr(rho), per))

    def warm_start(self, X=None, Y=None):
        """osqp_warm_start (_x, _y) for every QP: X [B, n], Y [B, m], unscaled; turns the warm_start setting on."""
        X = None if X is None else abi.as_f64(X)
        Y = None if Y is None else abi.as_f64(Y)
        if (X is not None and X.shape != (self.B, self.n)) or (Y is not None and Y.shape != (self.B, self.m)):
            raise ValueError("warm start arrays must be X [B, n], Y [B, m]")
        if self._many is not None:
            return self._many_each(lambda b, s: s.warm_start(x=None if X is None else X[b], y=None if Y is None else Y[b]))
        return int(self._lib.osqp_amd_batch_warm_start(self._h, _p(X), _p(Y if self.m else None)))

    def solve(self, fetch=True):
        if self._many is not None:
            from .multi import solve_many
            self._last = solve_many(self._many, max_workers=8)
            return self._many_results() if fetch else None
        self._status_polish = None
        rc = self._lib.osqp_amd_batch_solve(self._h)
        if rc:
            raise RuntimeError("osqp_amd_batch_solve failed (%d)" % rc)
        return self.results() if fetch else None

    def polish(self):
        """Polish (src/polish.c) on the device for every member whose last solve ended `solved`, with the handle's
        `delta` and `polish_refine_iter`.  Returns results() -- x, y, obj_val, pri_res, dua_res of the accepted
        members are the polished ones -- with `status_polish` [B]: 1 accepted, -1 tried and rejected (nothing of
        that member changed), 0 not tried.  Needs a solve since setup or the last update."""
        if self._many is not None:
            raise RuntimeError("this batch runs one single-QP engine per member (n > %d): polish is a call of the batch "
                               "engines; set the batch up with engine=\"streamed\"" % BATCH_MAX_N)
        sp = np.zeros(self.B, np.int64)
        rc = self._lib.osqp_amd_batch_polish(self._h, abi.iptr(sp))
        if rc:
            raise RuntimeError("osqp_amd_batch_polish failed (%d)%s" % (rc, ": no solve has run on the current problem"
                                                                        if rc == 7 else ""))
        self._status_polish = sp
        return self.results()

    def adjoint(self, dX, dY=None, matrices=False):
        """Adjoint derivatives of the solution on the device, for every member whose last solve ended `solved`: from
        dX = dl/dx [B, n] and dY = dl/dy [B, m] (None = 0) of a scalar l, a namespace with dq [B, n], dl, du [B, m],
        dPx [B, nnzP] and dAx [B, nnzA] (CSC order of triu(P) / A; None unless matrices=True; an off-diagonal dPx slot
        stands for both halves of P), active [B, m] (-1 active at the lower bound, +1 at the upper, 0 inactive) and
        status_adjoint [B]: 1 computed, -1 a KKT pivot of the wrong sign, 0 not tried (the member did not end
        `solved`); the gradients of members that are not 1 are 0.  The point differentiated is the one the handle
        holds: the polished one where polish() was accepted, the ADMM iterate otherwise.  Changes nothing in the
        handle.  Needs a solve since setup or the last update."""
        if self._many is not None:
            raise RuntimeError("this batch runs one single-QP engine per member (n > %d): adjoint is a call of the batch "
                               "engines; set the batch up with engine=\"streamed\"" % BATCH_MAX_N)
        B, n, m = self.B, self.n, self.m
        dX, dY = check_adjoint(B, n, m, dX, dY)
        dq = np.zeros((B, n)); dl = np.zeros((B, max(m, 1))); du = np.zeros((B, max(m, 1)))
        dPx = np.zeros((B, max(self.Pu.nnz, 1))) if matrices else None
        dAx = np.zeros((B, max(self.Ah.nnz, 1))) if matrices else None
        act = np.zeros((B, max(m, 1)), np.int64); sa = np.zeros(B, np.int64)
        rc = self._lib.osqp_amd_batch_adjoint(self._h, abi.fptr(dX), _p(dY if m else None), abi.fptr(dq), abi.fptr(dl),
                                              abi.fptr(du), _p(dPx), _p(dAx), abi.iptr(act), abi.iptr(sa))
        if rc:
            raise RuntimeError("osqp_amd_batch_adjoint failed (%d)%s" % (rc, ": no solve has run on the current problem"
                                                                         if rc == 7 else ""))
        return SimpleNamespace(dq=dq, dl=dl[:, :m], du=du[:, :m], dPx=None if dPx is None else dPx[:, :self.Pu.nnz],
                               dAx=None if dAx is None else dAx[:, :self.Ah.nnz], active=act[:, :m], status_adjoint=sa)

    def results(self):
        if self._many is not None:
            return self._many_results()
        X = np.zeros((self.B, self.n)); Y = np.zeros((self.B, max(self.m, 1)))
        info = np.zeros((self.B, 8)); DX = np.zeros((self.B, self.n)); DY = np.zeros((self.B, max(self.m, 1)))
        rc = self._lib.osqp_amd_batch_get(self._h, abi.fptr(X), abi.fptr(Y), abi.fptr(info), abi.fptr(DX), abi.fptr(DY))
        if rc:
            raise RuntimeError("osqp_amd_batch_get failed (%d)" % rc)
        out = SimpleNamespace(x=X, y=Y[:, :self.m], dual_inf_cert=DX, prim_inf_cert=DY[:, :self.m], info_raw=info)
        out.status_polish = np.zeros(self.B, np.int64) if self._status_polish is None else self._status_polish.copy()
        for k, name in enumerate(INFO_FIELDS):
            col = info[:, k]
            setattr(out, name, col.astype(np.int64) if name in ("iter", "status_val", "rho_updates") else col)
        return out

    def member_workspace(self, qp):
        """Test hook: member qp's workspace as the last setup / update / solve left it -- D, E, c, rho (scalar),
        ctype (-1 free, 0 inequality, 1 equality), scaled Pv / Av (CSC order of triu(P) / A) and the kernel's
        K^-1 as an NP x NP matrix (padded with identity to NP = 64 or 128; the streamed engine: n rounded up to 32)."""
        if self._many is not None:
            raise RuntimeError("this batch runs one single-QP engine per member (n > %d): there is no packed batch "
                               "workspace to read" % BATCH_MAX_N)
        NP = self.shape()[1]
        D = np.zeros(self.n); E = np.zeros(max(self.m, 1)); c = np.zeros(1); rho = np.zeros(1)
        ct = np.zeros(max(self.m, 1), np.int64); Pv = np.zeros(max(self.Pu.nnz, 1)); Av = np.zeros(max(self.Ah.nnz, 1))
        K = np.zeros((NP, NP)); npo = np.zeros(1, np.int64)
        rc = self._lib.osqp_amd_batch_member(self._h, int(qp), abi.fptr(D), abi.fptr(E), abi.fptr(c), abi.fptr(rho), abi.iptr(ct),
                                             abi.fptr(Pv), abi.fptr(Av), abi.fptr(K), abi.iptr(npo))
        if rc:
            raise RuntimeError("osqp_amd_batch_member failed (%d)" % rc)
        assert int(npo[0]) == NP
        return dict(D=D, E=E[:self.m], c=float(c[0]), rho=float(rho[0]), ctype=ct[:self.m], Pv=Pv[:self.Pu.nnz],
                    Av=Av[:self.Ah.nnz], Kinv=K, NP=NP)

    def device_arrays(self):
        """The result arrays as they sit in HBM -- X [B, n], Y [B, m], info8 [B, 8] -- as objects carrying
        `__cuda_array_interface__` (no copy; `torch.as_tensor(a, device="cuda")` wraps them for a device-side
        gather).  Valid until the next solve / cleanup."""
        if self._many is not None:
            raise RuntimeError("this batch runs one single-QP engine per member (n > %d): its results are host arrays "
                               "(results()); there is no packed device image to wrap" % BATCH_MAX_N)
        f = self._lib.osqp_amd_batch_device_ptrs
        f.restype = abi.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        px, py, pi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if f(self._h, C.byref(px), C.byref(py), C.byref(pi)):
            raise RuntimeError("osqp_amd_batch_device_ptrs failed")

        class _Dev:
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = dict(shape=shape, typestr="<f8", data=(int(ptr), False), version=2, strides=None)
        return _Dev(px.value, (self.B, self.n)), _Dev(py.value, (self.B, max(self.m, 1))), _Dev(pi.value, (self.B, 8))

    def cleanup(self):
        if getattr(self, "_many", None):
            for s in self._many:
                s.cleanup()
            self._many = None
        if self._h is not None:
            self._lib.osqp_amd_batch_cleanup(self._h)
            self._h = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass
