"""ctypes view of the C shim include/osqp_amd_engine.h, shared by the kernel-level GPU tests (test_gpu_direct_solve_edges.py,
test_gpu_engine_kernels.py, test_gpu_pcg_edges.py, test_gpu_elim_edges.py).  Nothing here computes a reference; Engine.reference() only hands the current (P, A, sigma, rho) to
tests/_kkt_reference.py."""
import ctypes as C
import os

import numpy as np
from scipy import sparse

from tests._kkt_reference import KKTReference

SIGMA = 1e-6
PCG_STOP = 1e-10


class HipengParams(C.Structure):          # include/osqp_amd_engine.h: hipeng_params
    _fields_ = [("sigma", C.c_double), ("alpha", C.c_double), ("pcg_eps_rel", C.c_double), ("pcg_eps_abs", C.c_double),
                ("pcg_max_iter", C.c_longlong), ("no_restart", C.c_longlong)]


SCALAR_FIELDS = ("pri_res_u", "pri_res_s", "z_u", "z_s", "Ax_u", "Ax_s", "dua_res_u", "dua_res_s", "q_u", "q_s", "Aty_u", "Aty_s",
                 "Px_u", "Px_s", "obj_scaled", "dy_norm_u", "dy_norm_s", "dy_lhs", "dx_norm_u", "dx_norm_s", "q_dx")
CERT_FIELDS = ("Atdy_u", "Atdy_s", "Pdx_u", "Pdx_s", "Adx_viol")


class HipengScalars(C.Structure):         # hipeng_scalars
    _fields_ = [(k, C.c_double) for k in SCALAR_FIELDS + CERT_FIELDS]


class HipengStats(C.Structure):           # hipeng_stats
    _fields_ = [(k, C.c_longlong) for k in ("admm_done", "pcg_iters_total", "pcg_iters_last", "pcg_iters_max", "pcg_forced",
                                            "graph_launches", "kernels_per_pcg_iter", "neg_curvature", "resident")]


class _env:
    def __init__(self, **kw): self.kw = kw
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            os.environ[k] = str(v)
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _lib():
    import osqp_amd
    from osqp_amd import _abi
    L = osqp_amd.lib()
    vp, fp, ll = C.c_void_p, _abi.c_float_p, C.c_longlong
    for name, args in (("hipeng_create", [C.POINTER(vp), C.POINTER(_abi.csc), C.POINTER(_abi.csc), fp, fp, fp, fp, C.POINTER(HipengParams), C.c_int]),
                       ("hipeng_kkt_solve", [vp, fp]), ("hipeng_kkt_solve_unrefined", [vp, fp]), ("hipeng_upload_rho", [vp, fp]),
                       ("hipeng_upload_matrices", [vp, C.POINTER(_abi.csc), C.POINTER(_abi.csc)]),
                       ("hipeng_set_params", [vp, C.POINTER(HipengParams)]), ("hipeng_resident_info", [vp, C.POINTER(C.c_longlong)]),
                       ("hipeng_ruiz_scale", [vp, ll, fp, fp, fp, fp, fp, fp, fp, fp]), ("hipeng_matrices_changed", [vp]),
                       ("hipeng_set_iterates", [vp, fp, fp]), ("hipeng_set_z", [vp, fp]), ("hipeng_run_admm", [vp, ll]),
                       ("hipeng_residuals", [vp, C.POINTER(HipengScalars)]),
                       ("hipeng_certificates", [vp, C.c_double, C.c_int, C.POINTER(HipengScalars)]),
                       ("hipeng_download", [vp, fp, fp, fp, fp, fp, C.c_int]), ("hipeng_spmv", [vp, C.c_int, fp, fp]),
                       ("hipeng_get_stats", [vp, C.POINTER(HipengStats)]), ("hipeng_pcg_layout", [vp, C.POINTER(C.c_longlong)]),
                       ("hipeng_is_split", [vp]), ("hipeng_upload_q", [vp, fp]), ("hipeng_upload_bounds", [vp, fp, fp]),
                       ("hipeng_cold_start", [vp]), ("hipeng_row_eliminated", [vp, ll]), ("hipeng_elim_peek", [vp, C.c_int, fp])):
        f = getattr(L, name)
        f.restype, f.argtypes = C.c_int, args
    L.hipeng_destroy.restype, L.hipeng_destroy.argtypes = None, [vp]
    L.hipeng_elim_count.restype, L.hipeng_elim_count.argtypes = C.c_longlong, [vp]
    L.hipeng_resident_dump.restype, L.hipeng_resident_dump.argtypes = C.c_longlong, [vp, vp, vp, vp, ll]
    return L


class Engine:
    """One hipeng on device 0 and the refined reference of its current (P, A, sigma, rho)."""

    def __init__(self, Pu, A, rho, sigma=SIGMA, env=None, q=None, l=None, u=None, alpha=1.6, pcg_eps_rel=PCG_STOP, pcg_max_iter=None):
        from osqp_amd import _abi
        self.L, self.abi = _lib(), _abi
        self.n, self.m = Pu.shape[0], A.shape[0]
        # (rho None: created without a rho vector, as the solver's set-up does before it scales; set_rho() follows)
        self.Pu, self.A, self.rho, self.sigma = sparse.csc_matrix(Pu), sparse.csc_matrix(A), None if rho is None else np.asarray(rho, float), sigma
        self._hold = [_abi.CscHolder(self.Pu), _abi.CscHolder(self.A)]
        self.prm = HipengParams(sigma, alpha, pcg_eps_rel, 1e-15, max(20000, 10 * self.n) if pcg_max_iter is None else pcg_max_iter, 0)
        r = None if rho is None else _abi.as_f64(self.rho)
        raw = [None if v is None else _abi.as_f64(v) for v in (q, l, u)]
        self.h = C.c_void_p()
        with _env(**(env or {})):
            rc = self.L.hipeng_create(C.byref(self.h), C.byref(self._hold[0].struct), C.byref(self._hold[1].struct),
                                      *[None if v is None else _abi.fptr(v) for v in raw], None if r is None else _abi.fptr(r), C.byref(self.prm), 0)
        assert rc == 0, rc
        self.ref = None

    def close(self):
        if self.h:
            self.L.hipeng_destroy(self.h)
            self.h = C.c_void_p()

    def info(self):
        out = (C.c_longlong * 16)()
        assert self.L.hipeng_resident_info(self.h, out) == 0
        return list(out)

    def layout(self):
        """hipeng_pcg_layout: [0] dense blocks of P, [1] rows inside them, [2] stream blocks, [3] long rows, [4] huge rows of A,
        [5] huge rows folded into k_cg_B, [6] split, [7] A / [8] M / [9] the matrix k_cg_B streams has 16-bit column ids,
        [10] long rows of that matrix, [11] gridA, [12] gridM."""
        out = (C.c_longlong * 16)()
        assert self.L.hipeng_pcg_layout(self.h, out) == 0
        return list(out)

    def is_split(self):
        return int(self.L.hipeng_is_split(self.h))

    def resident_dump(self):
        """hipeng_resident_dump: K as k_pcg_resident holds it, as a dense array."""
        nnz = int(self.info()[4])
        row, col, val = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
        assert self.L.hipeng_resident_dump(self.h, row.ctypes.data, col.ctypes.data, val.ctypes.data, nnz) == nnz
        assert len(set(zip(row.tolist(), col.tolist()))) == nnz
        return sparse.coo_matrix((val, (row, col)), shape=(self.n, self.n)).toarray()

    def elim(self):
        return int(self.L.hipeng_elim_count(self.h))

    def row_eliminated(self, i):
        return int(self.L.hipeng_row_eliminated(self.h, int(i)))

    def elim_peek(self, which):
        """hipeng_elim_peek: "rhoe", "ecoef", "edinv" or "xte", one value per row of A."""
        out = np.zeros(max(self.m, 1))
        assert self.L.hipeng_elim_peek(self.h, ("rhoe", "ecoef", "edinv", "xte").index(which), self._p(out)) == 0
        return out[: self.m]

    def upload_q(self, q):
        q = self.abi.as_f64(q)
        assert self.L.hipeng_upload_q(self.h, self._p(q)) == 0

    def upload_bounds(self, l, u):
        l, u = self.abi.as_f64(l), self.abi.as_f64(u)
        assert self.L.hipeng_upload_bounds(self.h, self._p(l), self._p(u)) == 0

    def cold_start(self):
        assert self.L.hipeng_cold_start(self.h) == 0

    def set_rho(self, rho):
        self.rho = np.asarray(rho, float)
        r = self.abi.as_f64(self.rho)
        assert self.L.hipeng_upload_rho(self.h, self.abi.fptr(r)) == 0
        self.ref = None

    def set_sigma(self, sigma):
        self.sigma = self.prm.sigma = sigma
        assert self.L.hipeng_set_params(self.h, C.byref(self.prm)) == 0
        self.ref = None

    def set_matrices(self, Pu, A):
        Pu, A = sparse.csc_matrix(Pu), sparse.csc_matrix(A)
        hp, ha = self.abi.CscHolder(Pu), self.abi.CscHolder(A)
        assert (hp.nnz, ha.nnz) == (self._hold[0].nnz, self._hold[1].nnz)
        assert self.L.hipeng_upload_matrices(self.h, C.byref(hp.struct), C.byref(ha.struct)) == 0
        self.Pu, self.A, self._hold = Pu, A, [hp, ha]
        self.ref = None

    def reference(self):
        if self.ref is None:
            self.ref = KKTReference(self.Pu, self.A, self.sigma, self.rho)
        return self.ref

    def solve(self, b, refined=True):
        out = self.abi.as_f64(b).copy()
        f = self.L.hipeng_kkt_solve if refined else self.L.hipeng_kkt_solve_unrefined
        assert f(self.h, self.abi.fptr(out)) == 0
        return out

    def check(self, tag, form, route=None, seed=0, nrhs=2):
        """Assert the form (and, where given, the route) in use, then the bar for it on nrhs right-hand sides; returns the worst
        ratio.  Where no route is given, which one serves depends on how far the sweeps' inverse is off its probes -- close to the
        thresholds on well-conditioned systems, and the formation of S sums with atomics -- and the bar holds on either."""
        inf = self.info()
        if isinstance(form, (set, tuple)):
            assert inf[9] in form, (tag, inf)
        else:
            assert inf[9] == form, (tag, "form", inf[9], "expected", form, inf)
        if route is not None and inf[9] == 4:
            assert inf[5] == route, (tag, "route", inf[5], "expected", route)
        ref = self.reference()
        rng = np.random.default_rng(seed)
        worst = 0.0
        for k in range(nrhs):
            b = rng.standard_normal(self.n + self.m) * (1.0 if k == 0 else rng.uniform(0.1, 10.0, self.n + self.m))
            _, _, plain = ref.solve(b)
            for refined in (False, True):
                out = self.solve(b, refined)
                if inf[9] in (3, 4):
                    err = ref.forward_error(out)
                    yard = plain if refined else ref.inverse_error(b)
                    bar = 10.0 * yard + 1e-14
                    what = f"fwd {err:.2e} {'numpy' if refined else 'inv(K)'} {yard:.2e}"
                else:
                    err = ref.residual(out[: self.n], b)
                    bar = 10.0 * PCG_STOP
                    what = f"res {err:.2e}"
                ratio = err / bar
                worst = max(worst, ratio)
                route_s = "" if inf[9] != 4 else (" chol" if inf[5] else " sweep")
                kind = "refined" if refined else "unrefined"
                print(f"[direct-edges] {tag}: {kind} form {inf[9]}{route_s} n3={inf[3]} n15={inf[15]} {what} ratio {ratio:.3f}")
                assert err <= bar, (tag, kind, inf[9], inf[5], err, bar, plain)
        return worst

    # ---- the calls of the scaling / residual / certificate / ADMM-step tests ----
    def _p(self, a):
        return self.abi.fptr(a)

    def ruiz_scale(self, passes):
        """hipeng_ruiz_scale: dict of D, E, c, q, l, u, Px, Ax (the matrices' values in the CSC order given to hipeng_create)."""
        n, m = self.n, self.m
        o = dict(D=np.zeros(n), E=np.zeros(max(m, 1)), q=np.zeros(n), l=np.zeros(max(m, 1)), u=np.zeros(max(m, 1)),
                 Px=np.zeros(max(self._hold[0].nnz, 1)), Ax=np.zeros(max(self._hold[1].nnz, 1)))
        c = C.c_double(0.0)
        rc = self.L.hipeng_ruiz_scale(self.h, passes, self._p(o["D"]), self._p(o["E"]), C.byref(c), self._p(o["q"]), self._p(o["l"]),
                                      self._p(o["u"]), self._p(o["Px"]), self._p(o["Ax"]))
        assert rc == 0, rc
        for k in ("E", "l", "u"):
            o[k] = o[k][:m]
        o["Px"], o["Ax"] = o["Px"][: self._hold[0].nnz], o["Ax"][: self._hold[1].nnz]
        o["c"] = c.value
        return o

    def matrices_changed(self):
        assert self.L.hipeng_matrices_changed(self.h) == 0

    def set_iterates(self, x, y, z=None):
        x, y = self.abi.as_f64(x), self.abi.as_f64(y if self.m else np.zeros(1))
        assert self.L.hipeng_set_iterates(self.h, self._p(x), self._p(y)) == 0
        if z is not None and self.m:
            z = self.abi.as_f64(z)
            assert self.L.hipeng_set_z(self.h, self._p(z)) == 0

    def run_admm(self, count=1):
        assert self.L.hipeng_run_admm(self.h, count) == 0

    def stats(self):
        st = HipengStats()
        assert self.L.hipeng_get_stats(self.h, C.byref(st)) == 0
        return {k: int(getattr(st, k)) for k, _ in HipengStats._fields_}

    def residuals(self):
        sc = HipengScalars()
        assert self.L.hipeng_residuals(self.h, C.byref(sc)) == 0
        return {k: float(getattr(sc, k)) for k in SCALAR_FIELDS}

    def certificates(self, eps_dx, unscaled):
        sc = HipengScalars()
        assert self.L.hipeng_certificates(self.h, float(eps_dx), int(unscaled), C.byref(sc)) == 0
        return {k: float(getattr(sc, k)) for k in CERT_FIELDS}

    def download(self, dy_projected=False):
        """x, y, z, dx, dy (dy: the raw delta_y of the last iteration, or its projection left by hipeng_residuals)."""
        n, m = self.n, self.m
        x, dx = np.zeros(n), np.zeros(n)
        y, z, dy = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(max(m, 1))
        assert self.L.hipeng_download(self.h, self._p(x), self._p(y), self._p(z), self._p(dx), self._p(dy), int(dy_projected)) == 0
        return x, y[:m], z[:m], dx, dy[:m]

    def spmv(self, which, v):
        """which = 0: A v (CSR copy of A), 1: A' v (the A' part of M), 2: P v."""
        v = self.abi.as_f64(v)
        out = np.zeros(max(self.m if which == 0 else self.n, 1))
        assert self.L.hipeng_spmv(self.h, which, self._p(v), self._p(out)) == 0
        return out[: self.m if which == 0 else self.n]
