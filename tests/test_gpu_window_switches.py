"""GPU tests, through the C ABI, of the two switches that take work out of a window of ADMM iterations without touching an operand:

  OSQP_AMD_FUSED_CHECK            the window's prologue, hipeng_cold_start and the reset of the PCG start history are one launch
                                  each; hipeng_run_admm_check brings the residual scalars back with the window's own wait
                                  (tests/test_gpu_fused_check.py drives it through osqp_solve).
  OSQP_AMD_INIT_RESIDENT_STORES   k_pcg_init of the resident graphs stores r0 and u0 = Minv r0 in the exchanged vector's layout only
                                  (r0pos, u0pos: whole lines per workgroup of the resident launch), and k_pcg_resident reads its own
                                  rows from there instead of from init_r (stride 4) and init_z.

Each switch is read when the engine is created.  For every case two engines on the same data, one with the switch on (the default)
and one with it off, are stepped side by side: x, y, z after each of 30 ADMM iterations, then after a new rho, a warm start and a
new q (three iterations each), the PCG iteration counts, State::tol2 (hipeng_resident_start_peek), the residual scalars and both
certificates must agree in every bit.  Every case asserts first that the resident form is in use and that no launch gave up.

Cases: one workgroup of 60 and of 61 rows (even and odd; 61 rows and the three riding partials fill the 64 lanes), n = 62 (two
workgroups), `tiny3` (gridM = 1), `m0` (no constraints), `offtile`, res_e8 and res_e20 (E = 8 and 20, n = 427 and 610: no multiple
of 64), res_e64 (gridM = 610 > 64), res_gone_e8 (eliminated slacks).  `tiny3` and `m0` are stepped on until a solve starts
converged (no PCG iteration), as tests/test_gpu_resident_startup.py finds one."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

from tests import _elim_cases as EC
from tests import _engine_reference as R
from tests import _iteration_chain_worker as W
from tests import _pcg_cases as PC
from tests._hipeng import Engine, HipengScalars, SCALAR_FIELDS
from tests.test_gpu_resident_last_trip import ALPHA, _res_env
from tests.test_gpu_resident_startup import _on_resident, peek

pytestmark = pytest.mark.gpu

SWITCHES = ("OSQP_AMD_FUSED_CHECK", "OSQP_AMD_INIT_RESIDENT_STORES")
CHAIN = 30


def _small(n, m, seed):
    """Tridiagonal SPD P (every variable coupled: nothing is eliminated), m rows of A with three entries each."""
    rng = np.random.default_rng(seed)
    d, o = rng.uniform(2.0, 3.0, n), np.full(n - 1, -0.5)
    Pu = sparse.csc_matrix(sparse.diags([d, o], [0, 1]))
    Pu.sort_indices()
    rows = np.repeat(np.arange(m), 3)
    cols = np.concatenate([np.sort(rng.choice(n, 3, replace=False)) for _ in range(m)])
    A = sparse.csc_matrix((rng.uniform(0.5, 1.0, rows.size) * rng.choice([-1.0, 1.0], rows.size), (rows, cols)), shape=(m, n))
    A.sort_indices()
    return dict(name="small%d" % n, n=n, m=m, Pu=Pu, A=A, q=rng.standard_normal(n), l=-np.ones(m), u=np.ones(m), rho=np.full(m, R.RHO),
                x=rng.standard_normal(n), y=rng.standard_normal(m) * 0.05, z=rng.standard_normal(m))


CASES = {                                     # name -> (case, environment, workgroups (None: whatever the plan gives))
    "rows60": (lambda: _small(60, 30, 60), lambda c: W.ENVS["resident"], 1),
    "rows61": (lambda: _small(61, 30, 61), lambda c: W.ENVS["resident"], 1),
    "rows62": (lambda: _small(62, 30, 62), lambda c: W.ENVS["resident"], None),
    "tiny3": (lambda: R.make_case("tiny3"), lambda c: W.ENVS["resident"], None),
    "m0": (lambda: R.make_case("m0"), lambda c: W.ENVS["resident"], None),
    "offtile": (lambda: R.make_case("offtile"), lambda c: W.ENVS["resident"], None),
    "res_e8": (lambda: PC.make("res_e8"), _res_env, None),
    "res_e20": (lambda: PC.make("res_e20"), _res_env, None),
    "res_e64": (lambda: PC.make("res_e64"), _res_env, None),
    "res_gone_e8": (lambda: EC.make("res_gone_e8"), _res_env, None),
}


def _open(c, env):
    e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=env, q=c["q"], l=c["l"], u=c["u"], alpha=ALPHA, pcg_eps_rel=PC.PCG_EPS,
               pcg_max_iter=20000)
    try:
        e.ruiz_scale(10)
        e.matrices_changed()
        e.set_rho(c["rho"])
    except BaseException:
        e.close()
        raise
    return e


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _same_state(tag, on, off):
    for k, a, b in zip("xyz", on.download(False)[:3], off.download(False)[:3]):
        diff = int((_bits(a) != _bits(b)).sum())
        assert diff == 0, (tag, k, diff, "elements differ")
    sa, sb = on.stats(), off.stats()
    for k in ("admm_done", "pcg_iters_total", "pcg_iters_last", "pcg_iters_max", "pcg_forced", "neg_curvature", "resident"):
        assert sa[k] == sb[k], (tag, k, sa, sb)
    assert _bits([peek(on)[2]])[0] == _bits([peek(off)[2]])[0], (tag, "tol2")
    return sa


def _same_scalars(tag, on, off):
    ra, rb = on.residuals(), off.residuals()
    for k in SCALAR_FIELDS:
        assert _bits([ra[k]])[0] == _bits([rb[k]])[0], (tag, k, ra[k], rb[k])
    for unscaled in (0, 1):
        ca, cb = on.certificates(1e-4 * max(ra["dx_norm_s"], 1e-300), unscaled), off.certificates(1e-4 * max(rb["dx_norm_s"], 1e-300), unscaled)
        for k in ca:
            assert _bits([ca[k]])[0] == _bits([cb[k]])[0], (tag, "certificates", unscaled, k)


def _pair(name, switch):
    make, env, nwg = CASES[name]
    c = make()
    base = dict(env(c))
    on = _open(c, dict(base, **{switch: 1}))
    try:
        off = _open(c, dict(base, **{switch: 0}))
    except BaseException:
        on.close()
        raise
    return c, on, off, nwg


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("name", list(CASES))
def test_bit_identity(name, switch):
    c, on, off, nwg = _pair(name, switch)
    try:
        for e in (on, off):
            _on_resident(e, (name, switch), c["claims"]["nwg"] if "claims" in c and "nwg" in c["claims"] else nwg)
        assert name != "rows62" or on.info()[3] >= 2, (name, on.info()[:11])      # (61 rows at the most per workgroup)
        assert on.elim() == off.elim() and (on.elim() > 0) == (name == "res_gone_e8"), (name, on.elim())
        print(f"[window-switches] {name} {switch}: n {on.n}, m {on.m}, workgroups {on.info()[3]}, E {on.info()[2]}, gridM {on.layout()[12]}")
        x0, y0, z0 = (c["x"], c["y"], c["z"]) if "x" in c else R.iterates(c)
        for e in (on, off):
            e.set_iterates(x0, y0, z0)
        for k in range(1, CHAIN + 1):
            on.run_admm(1); off.run_admm(1)
            _same_state((name, switch, k), on, off)
        rng = np.random.default_rng(7)
        # a new rho (the operator and the preconditioner are formed again), a warm start, a new q: three iterations after each
        rho2 = np.asarray(c["rho"], float) * 3.0
        for e in (on, off):
            e.set_rho(rho2)
        for k in range(3):
            on.run_admm(1); off.run_admm(1)
            _same_state((name, switch, "rho", k), on, off)
        x1, y1 = rng.standard_normal(on.n), rng.standard_normal(on.m) * 0.05
        for e in (on, off):
            e.set_iterates(x1, y1)
        for k in range(3):
            on.run_admm(1); off.run_admm(1)
            _same_state((name, switch, "warm", k), on, off)
        q1 = np.asarray(c["q"], float) * 1.5 + 0.1
        for e in (on, off):
            e.upload_q(q1)
        on.run_admm(3); off.run_admm(3)
        _same_state((name, switch, "q"), on, off)
        # a cold start and a longer window
        for e in (on, off):
            e.cold_start()
        on.run_admm(7); off.run_admm(7)
        _same_state((name, switch, "cold"), on, off)
        _same_scalars((name, switch), on, off)
        for e in (on, off):
            _on_resident(e, (name, switch, "end"))
    finally:
        on.close(); off.close()


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("name", ["tiny3", "m0"])
def test_solve_that_starts_converged(name, switch, limit=500):
    c, on, off, _ = _pair(name, switch)
    try:
        x0, y0, z0 = R.iterates(c)
        for e in (on, off):
            _on_resident(e, (name, switch))
            e.set_iterates(x0, y0, z0)
        found = None
        for k in range(1, limit + 1):
            on.run_admm(1); off.run_admm(1)
            st = _same_state((name, switch, k), on, off)
            if found is not None and k >= found + 2:
                break
            if found is None and st["pcg_iters_last"] == 0:
                found = k
        assert found is not None and found < limit, (name, switch, "no start vector passed the stop test")
        print(f"[window-switches] {name} {switch}: the solve of iteration {found} started converged")
        for e in (on, off):
            _on_resident(e, (name, switch, "end"))
    finally:
        on.close(); off.close()


@pytest.mark.parametrize("name", ["rows61", "res_e20", "m0"])
def test_run_admm_check_brings_the_scalars_of_hipeng_residuals(name):
    """hipeng_run_admm_check on a window of seven iterations: *have = 1, and the scalars are those hipeng_residuals gives right
    after it, in every bit; with the switch off *have = 0 and the output is left alone."""
    make, env, _ = CASES[name]
    c = make()
    for switch in (1, 0):
        e = _open(c, dict(env(c), OSQP_AMD_FUSED_CHECK=switch))
        try:
            _on_resident(e, (name, switch))
            f = e.L.hipeng_run_admm_check
            f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_longlong, C.POINTER(HipengScalars), C.POINTER(C.c_int)]
            x0, y0, z0 = (c["x"], c["y"], c["z"]) if "x" in c else R.iterates(c)
            e.set_iterates(x0, y0, z0)
            sc, have = HipengScalars(), C.c_int(-1)
            sc.obj_scaled = 12345.0
            assert f(e.h, 7, C.byref(sc), C.byref(have)) == 0
            _on_resident(e, (name, switch, "after"))
            assert e.stats()["admm_done"] == 7
            want = e.residuals()
            if switch:
                assert have.value == 1
                for k in SCALAR_FIELDS:
                    assert _bits([getattr(sc, k)])[0] == _bits([want[k]])[0], (name, k, getattr(sc, k), want[k])
            else:
                assert have.value == 0 and sc.obj_scaled == 12345.0
        finally:
            e.close()
