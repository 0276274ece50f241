"""Host-side object interface over the C ABI, shaped like the reference's Python
wrapper (docs/interfaces/python.rst in the reference: `OSQP().setup(P, q, A, l,
u, **settings)`, `.solve()`, `.update(...)`, `.warm_start(...)`,
`.update_settings(...)`).  All numerics happen behind the C ABI in
libosqp_amd.so (HIP); this file only marshals arrays.

`SolverHandle` is library-agnostic (library + symbol prefix) so the tests can
drive a second library with the same ABI through exactly the same Python code path.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
from scipy import sparse

from . import _abi as abi
from .batch import VERIFY_FIELDS


class Results(SimpleNamespace):
    pass


def check_adjoint(n, m, dx, dy=None):
    """Shape checks of SolverHandle.adjoint: dx [n], dy [m] or None.  Returns the arrays as the C side takes them."""
    dx = abi.as_f64(dx)
    dy = None if dy is None else abi.as_f64(dy)
    if dx.shape != (n,) or (dy is not None and dy.shape != (m,)):
        raise ValueError("adjoint arrays must be dx [%d], dy [%d]" % (n, m))
    return dx, dy


def check_tangent(n, m, nnzP, nnzA, dq=None, dl=None, du=None, dPx=None, dAx=None):
    """Shape checks of SolverHandle.tangent: every given array is [k] (one direction) or [D, k] (D directions), k = n for dq,
    m for dl and du, nnzP for dPx, nnzA for dAx; all given arrays agree on the form and on D.  Returns (dq, dl, du, dPx,
    dAx, D, flat) with contiguous float64 arrays: flat is True for the [k] form (D = 1), and when nothing is given."""
    cols = dict(dq=n, dl=m, du=m, dPx=nnzP, dAx=nnzA)
    out, forms = {}, {}
    for name, a in dict(dq=dq, dl=dl, du=du, dPx=dPx, dAx=dAx).items():
        if a is None:
            out[name] = None
            continue
        a = abi.as_f64(a)
        if a.ndim not in (1, 2) or a.shape[-1] != cols[name] or (a.ndim == 2 and a.shape[0] < 1):
            raise ValueError("%s must be [%d] or [D, %d], not %s" % (name, cols[name], cols[name], a.shape))
        forms[name] = None if a.ndim == 1 else a.shape[0]
        out[name] = a
    if len(set(forms.values())) > 1:
        raise ValueError("tangent arrays must all be [k] or all [D, k] with one D: %s"
                         % ", ".join("%s %s" % (k, "[k]" if d is None else "D = %d" % d) for k, d in forms.items()))
    D = next(iter(forms.values()), None)
    if D is not None and D > 65535:
        raise ValueError("at most 65535 directions per call, not %d" % D)
    return tuple(out[k] for k in ("dq", "dl", "du", "dPx", "dAx")) + (1 if D is None else int(D), D is None)


def _opt(a, ptr=None):
    return C.cast(None, ptr or abi.c_float_p) if a is None else abi.fptr(a)


class SolverHandle:
    def __init__(self, lib, prefix=""):
        self._lib = lib
        self._prefix = prefix
        self._api = abi.bind_api(lib, prefix)
        self._work = None
        self._keep = None
        self.n = self.m = 0

    # ------------------------------------------------------------------ setup
    def default_settings(self):
        s = abi.OSQPSettings()
        self._api["set_default_settings"](C.byref(s))
        s.verbose = 0
        return s

    def setup(self, P=None, q=None, A=None, l=None, u=None, **settings):
        if self._work is not None:
            raise ValueError("solver already set up")
        if P is None and q is None:
            raise ValueError("P and q cannot both be missing")
        n = P.shape[0] if P is not None else len(q)
        if P is None:
            P = sparse.csc_matrix((n, n))
        if q is None:
            q = np.zeros(n)
        if A is None:
            A = sparse.csc_matrix((0, n))
            l = np.zeros(0)
            u = np.zeros(0)
        m = A.shape[0]
        if l is None:
            l = -np.inf * np.ones(m)
        if u is None:
            u = np.inf * np.ones(m)
        Pu = abi.CscHolder(sparse.triu(P, format="csc"))
        Ah = abi.CscHolder(A)
        qv = abi.as_f64(q)
        lv = np.maximum(abi.as_f64(l), -abi.OSQP_INFTY)
        uv = np.minimum(abi.as_f64(u), abi.OSQP_INFTY)
        if qv.shape != (n,) or lv.shape != (m,) or uv.shape != (m,):
            raise ValueError("dimension mismatch")
        if m == 0:  # keep pointers non-NULL like malloc(0) callers do
            lv = np.zeros(1)
            uv = np.zeros(1)
        data = abi.OSQPData(n, m, C.pointer(Pu.struct), C.pointer(Ah.struct),
                            abi.fptr(qv), abi.fptr(lv), abi.fptr(uv))
        st = self.default_settings()
        for k, v in settings.items():
            if k not in abi.SETTING_NAMES:
                raise ValueError("unknown setting %r" % k)
            setattr(st, k, v)
        work = C.POINTER(abi.OSQPWorkspace)()
        rc = self._api["setup"](C.byref(work), C.byref(data), C.byref(st))
        self._keep = (Pu, Ah, qv, lv, uv)
        if rc != 0:
            if work:
                self._api["cleanup"](work)
            raise ValueError("osqp_setup failed with error %d" % rc)
        self._work = work
        self.n, self.m = n, m
        self.nnzP, self.nnzA = Pu.nnz, Ah.nnz
        return self

    # ------------------------------------------------------------------ solve
    def _vec(self, ptr, k):
        if k == 0:
            return np.zeros(0)
        return np.ctypeslib.as_array(ptr, shape=(k,)).copy()

    def solve(self):
        w = self._work
        rc = self._api["solve"](w)
        info = w.contents.info.contents
        sol = w.contents.solution.contents
        fields = {f[0]: getattr(info, f[0]) for f in abi.OSQPInfo._fields_}
        fields["status"] = info.status.decode()
        res = Results(x=self._vec(sol.x, self.n), y=self._vec(sol.y, self.m),
                      info=SimpleNamespace(**fields), exitflag=int(rc),
                      prim_inf_cert=self._vec(w.contents.delta_y, self.m),
                      dual_inf_cert=self._vec(w.contents.delta_x, self.n))
        return res

    # ---------------------------------------------------------------- updates
    def update(self, q=None, l=None, u=None, Px=None, Px_idx=None, Ax=None, Ax_idx=None):
        w = self._work
        rc = 0
        if q is not None:
            q = abi.as_f64(q)
            if q.shape != (self.n,):
                raise ValueError("q must have %d entries" % self.n)
            rc |= self._api["update_lin_cost"](w, abi.fptr(q))
        if l is not None:
            l = np.maximum(abi.as_f64(l), -abi.OSQP_INFTY)
            if l.shape != (self.m,):
                raise ValueError("l must have %d entries" % self.m)
        if u is not None:
            u = np.minimum(abi.as_f64(u), abi.OSQP_INFTY)
            if u.shape != (self.m,):
                raise ValueError("u must have %d entries" % self.m)
        if l is not None and u is not None:
            rc |= self._api["update_bounds"](w, abi.fptr(l), abi.fptr(u))
        elif l is not None:
            rc |= self._api["update_lower_bound"](w, abi.fptr(l))
        elif u is not None:
            rc |= self._api["update_upper_bound"](w, abi.fptr(u))

        def idx(a):
            if a is None:
                return None, C.cast(None, abi.c_int_p)
            a = abi.as_i64(a)
            return a, abi.iptr(a)

        def check(vals, ind, nnz, name):
            # the C entry points trust their arguments like the reference's (osqp.c:1012-1169 reads nnz values when no
            # index array is given and never range-checks the indices): refuse what would read or write out of bounds
            if vals.ndim != 1:
                raise ValueError("%sx must be a vector" % name)
            if ind is None:
                if vals.size != nnz:
                    raise ValueError("%sx has %d values, %s has %d non-zeros (pass %sx_idx for a partial update)" % (name, vals.size, name, nnz, name))
            else:
                if ind.shape != vals.shape:
                    raise ValueError("%sx and %sx_idx differ in length" % (name, name))
                if ind.size and (ind.min() < 0 or ind.max() >= nnz):
                    raise ValueError("%sx_idx out of range [0, %d)" % (name, nnz))

        if Px is not None and Ax is not None:
            Px = abi.as_f64(Px); Ax = abi.as_f64(Ax)
            pi, pip = idx(Px_idx); ai, aip = idx(Ax_idx)
            check(Px, pi, self.nnzP, "P"); check(Ax, ai, self.nnzA, "A")
            rc |= self._api["update_P_A"](w, abi.fptr(Px), pip, len(Px), abi.fptr(Ax), aip, len(Ax))
        elif Px is not None:
            Px = abi.as_f64(Px)
            pi, pip = idx(Px_idx)
            check(Px, pi, self.nnzP, "P")
            rc |= self._api["update_P"](w, abi.fptr(Px), pip, len(Px))
        elif Ax is not None:
            Ax = abi.as_f64(Ax)
            ai, aip = idx(Ax_idx)
            check(Ax, ai, self.nnzA, "A")
            rc |= self._api["update_A"](w, abi.fptr(Ax), aip, len(Ax))
        return int(rc)

    def update_rho(self, rho):
        return int(self._api["update_rho"](self._work, float(rho)))

    def update_settings(self, **kw):
        """Post-setup setting changes (reference osqp.c:1339-1617 setters)."""
        st = self._work.contents.settings.contents
        for k, v in kw.items():
            if k == "rho":
                self.update_rho(v)
                continue
            if k in ("sigma", "scaling", "linsys_solver", "adaptive_rho",
                     "adaptive_rho_interval", "adaptive_rho_tolerance", "adaptive_rho_fraction"):
                raise ValueError("%s cannot be changed after setup" % k)
            setter = getattr(self._lib, self._prefix + "osqp_update_" + k, None)
            if setter is not None:
                tp = dict(abi.OSQPSettings._fields_)[k]
                setter.restype = abi.c_int
                setter.argtypes = [C.POINTER(abi.OSQPWorkspace), tp]
                if setter(self._work, v) != 0:
                    raise ValueError("invalid value for %s" % k)
            else:
                setattr(st, k, v)

    def warm_start(self, x=None, y=None):
        w = self._work
        if (x is not None and np.shape(x) != (self.n,)) or (y is not None and np.shape(y) != (self.m,)):
            raise ValueError("warm start vectors must have %d (x) and %d (y) entries" % (self.n, self.m))
        if x is not None and y is not None:
            x = abi.as_f64(x); y = abi.as_f64(y)
            return int(self._api["warm_start"](w, abi.fptr(x), abi.fptr(y)))
        if x is not None:
            x = abi.as_f64(x)
            return int(self._api["warm_start_x"](w, abi.fptr(x)))
        if y is not None:
            y = abi.as_f64(y)
            return int(self._api["warm_start_y"](w, abi.fptr(y)))
        return 0

    # ------------------------------------------------------------ derivatives
    def _sens(self, name):
        if name not in self._api:
            raise NotImplementedError("this library has no osqp_amd_%s" % name)
        return self._api[name]

    @staticmethod
    def _sens_fail(name, rc):
        raise RuntimeError("%s failed (%d)%s" % (name, rc, ": no solve has run on the current problem" if rc == 7 else ""))

    def adjoint(self, dx, dy=None, matrices=False):
        """Adjoint derivatives of the solution (osqp_amd_adjoint): from dx = dl/dx [n] and dy = dl/dy [m] (None = 0) of a
        scalar l, a namespace with dq [n], dl, du [m], dPx [nnzP] and dAx [nnzA] (CSC order of triu(P) / A; None unless
        matrices=True; an off-diagonal dPx slot stands for both halves of P), active [m] (-1 active at the lower bound, +1
        at the upper, 0 inactive), status_adjoint (1 computed, -1 a linear solve failed, 0 not tried: the solve did not end
        `solved`; the gradients are 0 unless it is 1) and kkt_res (the scaled KKT residual the refined solve ended at,
        relative to its right-hand side).  The point differentiated is the one the handle holds: the polished one where
        polish ran and was accepted, the ADMM iterate otherwise.  Changes nothing in the handle.  Needs a solve since
        setup or the last update or warm start; the KKT instance the first call builds serves every later adjoint() and
        tangent() until then."""
        n, m = self.n, self.m
        dx, dy = check_adjoint(n, m, dx, dy)
        f = self._sens("adjoint")
        dq = np.zeros(n); dl = np.zeros(max(m, 1)); du = np.zeros(max(m, 1))
        dPx = np.zeros(max(self.nnzP, 1)) if matrices else None
        dAx = np.zeros(max(self.nnzA, 1)) if matrices else None
        act = np.zeros(max(m, 1), np.int64); st = np.zeros(1, np.int64); kr = np.zeros(1)
        rc = f(self._work, abi.fptr(dx), _opt(dy if m else None), abi.fptr(dq), abi.fptr(dl), abi.fptr(du), _opt(dPx), _opt(dAx),
               abi.iptr(act), abi.iptr(st), abi.fptr(kr))
        if rc:
            self._sens_fail("osqp_amd_adjoint", rc)
        return SimpleNamespace(dq=dq, dl=dl[:m], du=du[:m], dPx=None if dPx is None else dPx[:self.nnzP],
                               dAx=None if dAx is None else dAx[:self.nnzA], active=act[:m], status_adjoint=int(st[0]),
                               kkt_res=float(kr[0]))

    def tangent(self, dq=None, dl=None, du=None, dPx=None, dAx=None):
        """Forward sensitivities of the solution (osqp_amd_tangent): from tangents of the data -- dq [n], dl, du [m], dPx
        [nnzP], dAx [nnzA] (CSC order of triu(P) / A; an off-diagonal dPx slot stands for both halves of P), or each of
        them [D, k] for D directions that share the KKT instance; None = 0 -- a namespace with dx [n] and dy [m] (or
        [D, .]), active [m], status_tangent (as adjoint()'s status) and kkt_res [D] (a float for the [k] form).  Only the
        tangent of the bound a row is active at counts (dl = du on an equality row).  The point, the instance and what the
        call needs are adjoint()'s.  Changes nothing in the handle."""
        n, m = self.n, self.m
        dq, dl, du, dPx, dAx, D, flat = check_tangent(n, m, self.nnzP, self.nnzA, dq, dl, du, dPx, dAx)
        f = self._sens("tangent")
        dx = np.zeros((D, n)); dy = np.zeros((D, max(m, 1)))
        act = np.zeros(max(m, 1), np.int64); st = np.zeros(1, np.int64); kr = np.zeros(D)
        rc = f(self._work, D, _opt(dq), _opt(dl if m else None), _opt(du if m else None), _opt(dPx), _opt(dAx), abi.fptr(dx),
               _opt(dy if m else None), abi.iptr(act), abi.iptr(st), abi.fptr(kr))
        if rc:
            self._sens_fail("osqp_amd_tangent", rc)
        dy = dy[:, :m]
        return SimpleNamespace(dx=dx[0] if flat else dx, dy=dy[0] if flat else dy, active=act[:m], status_tangent=int(st[0]),
                               kkt_res=float(kr[0]) if flat else kr)

    def sens_info(self):
        """For the tests: KKT instances built since setup, whether one is alive, its active rows, linear solves since setup."""
        out = np.zeros(4, np.int64)
        rc = self._sens("sens_info")(self._work, abi.iptr(out))
        if rc:
            self._sens_fail("osqp_amd_sens_info", rc)
        return dict(built=int(out[0]), alive=int(out[1]), active_rows=int(out[2]), solves=int(out[3]))

    def polish_info(self):
        """For the tests: polish instances run since setup, the linear-solve form the last one took (hipeng_resident_info [9];
        -1: none yet), its active rows, and its give-ups plus negative-curvature stops (0: the form served every solve)."""
        out = np.zeros(4, np.int64)
        rc = self._sens("polish_info")(self._work, abi.iptr(out))
        if rc:
            self._sens_fail("osqp_amd_polish_info", rc)
        return dict(runs=int(out[0]), form=int(out[1]), active_rows=int(out[2]), troubles=int(out[3]))

    def sens_engine(self):
        """Raw engine handle of the live KKT instance of adjoint() / tangent() (None: none alive), as OSQP.engine() is of
        the handle's own engine."""
        return self._sens("sens_engine")(self._work)

    # ----------------------------------------------------------------- verify
    def verify(self, x=None, y=None, dx=None, dy=None, eps_abs=None, eps_rel=None):
        """The verdict on a point against the raw problem the handle holds now, computed on the device from P, q, A, l, u as
        given and last updated -- nothing of the scaling, rho, the linear-solve form or the engine's iterates
        (include/osqp_amd.h: osqp_amd_verify).  x [n], y [m]: the point, unscaled; dx [n], dy [m]: certificates; None = the
        handle's own, what solve() returned as x, y, dual_inf_cert, prim_inf_cert.  eps_abs, eps_rel: the tolerances of
        eps_pri and eps_dua (None: the handle's settings).  Needs no solve and changes nothing in the handle.  Returns a
        namespace with one scalar per slot (batch.VERIFY_FIELDS): obj, pri_res, dua_res, norm_ax, norm_z, norm_px, norm_aty,
        norm_q, eps_pri, eps_dua, comp, dual_obj, gap (float) and optimal, prim_inf, dual_inf (bool), and V [16], the record
        as the device wrote it."""
        if "verify" not in self._api:
            raise NotImplementedError("this library has no osqp_amd_verify")
        arr = {}
        for name, a, k in (("x", x, self.n), ("y", y, self.m), ("dx", dx, self.n), ("dy", dy, self.m)):
            if a is not None:
                a = abi.as_f64(a)
                if a.shape != (k,):
                    raise ValueError("%s must have %d entries, not shape %s" % (name, k, a.shape))
                if k == 0:
                    a = np.zeros(1)      # (a pointer that is not NULL: the array is the caller's, empty as it is)
            arr[name] = a
        eps = []
        for name, e in (("eps_abs", eps_abs), ("eps_rel", eps_rel)):
            if e is not None and not (np.isfinite(e) and e >= 0):
                raise ValueError("%s must be a finite number >= 0 or None (the handle's setting), not %r" % (name, e))
            eps.append(-1.0 if e is None else float(e))
        V = np.zeros(len(VERIFY_FIELDS))
        rc = self._api["verify"](self._work, _opt(arr["x"]), _opt(arr["y"]), _opt(arr["dx"]), _opt(arr["dy"]), eps[0], eps[1],
                                 abi.fptr(V))
        if rc:
            raise RuntimeError("osqp_amd_verify failed (%d)" % rc)
        out = SimpleNamespace(V=V)
        for k, name in enumerate(VERIFY_FIELDS):
            setattr(out, name, bool(V[k] != 0.0) if k >= 13 else float(V[k]))
        return out

    def verify_info(self):
        """For the tests: verify() calls served since setup and, since the first of them, uploads of P values, of A values
        and of q / l / u (one counter; each vector counts one)."""
        if "verify_info" not in self._api:
            raise NotImplementedError("this library has no osqp_amd_verify_info")
        out = np.zeros(4, np.int64)
        rc = self._api["verify_info"](self._work, abi.iptr(out))
        if rc:
            raise RuntimeError("osqp_amd_verify_info failed (%d)" % rc)
        return dict(calls=int(out[0]), uploads_P=int(out[1]), uploads_A=int(out[2]), uploads_qlu=int(out[3]))

    # -------------------------------------------------------------- accessors
    @property
    def work(self):
        return self._work.contents

    def settings(self):
        return self._work.contents.settings.contents

    def cleanup(self):
        if self._work is not None:
            self._api["cleanup"](self._work)
            self._work = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass
