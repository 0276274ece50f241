"""GPU tests of the dense-direct GEMM kernels and both inversion routes on their own (csrc/dense_direct.h), through the hooks of
csrc/dense_direct_host.h: hipeng_dense_gemm_selftest launches k_dd_gemm_tn / k_dd_gemm_tn_lds by name with every argument
explicit, hipeng_dense_invert_route runs dd_invert_sweep / dd_invert_chol on either kernel.  References, bars and case tables:
tests/_dense_reference.py (held to account on the CPU by tests/test_dense_reference_host.py).

  GEMM: every written entry within (K + 5) 2^-53 (|beta||C0| + |alpha| |T|' |w| |B|) of the long-double product -- a theorem, no
        margin --, every masked entry (skip ranges, tiles above the diagonal under `lower`, rows >= M, columns >= N) bit-equal
        to the sentinel C0.
  Inversion: max |Ainv - truth| and max |Ainv A - I| within 10 x those of the same route's float64 numpy restatement on the same
        matrix + n 2^-53 max|A^-1|; Ainv == Ainv' to the bit.
  Verdicts: a pivot that is not positive comes back as 1, from either route on either kernel, without a HIP error.
  The switches that are read once per process (OSQP_AMD_DENSE_GEMM_LDS=0, OSQP_AMD_DENSE_CHOL=1) inside an engine: a fresh child
  process each (tests/_dense_switch_worker.py).

Every case prints its worst err / bound for the record (pytest -s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _dense_reference as DR

pytestmark = pytest.mark.gpu

HIPENG_ERR_ARG = -103
KERNELS = ((0, "k_dd_gemm_tn"), (1, "k_dd_gemm_tn_lds"))
ROUTES = ((DR.SWEEP, "sweeps"), (DR.CHOL, "cholesky"))
GEMMS = ((0, "global"), (1, "lds"))


def _lib():
    import osqp_amd
    L = osqp_amd.lib()
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    L.hipeng_dense_gemm_selftest.restype = i
    L.hipeng_dense_gemm_selftest.argtypes = [i, i, i, i, vp, i, vp, i, vp, vp, i, d, d, i, i, i, i, i, i, i]
    L.hipeng_dense_invert_route.restype, L.hipeng_dense_invert_route.argtypes = i, [i, vp, vp, i, i]
    return L


def _gemm(L, kernel, c, **over):
    """One launch on a copy of the case's C0; returns (status, C)."""
    a = dict(c, **over)
    out = np.ascontiguousarray(a["C0"]).copy()
    w = a["w"]
    rc = L.hipeng_dense_gemm_selftest(kernel, a["M"], a["N"], a["K"], a["T"].ctypes.data, a["ldt"], a["B"].ctypes.data, a["ldb"],
                                      None if w is None else w.ctypes.data, out.ctypes.data, a["ldc"], a["alpha"], a["beta"],
                                      a["sr"][0], a["sr"][1], a["sc"][0], a["sc"][1], a["lower"], a["kmode"], a["ksl"])
    return rc, out


@pytest.mark.parametrize("name", list(DR.GEMM_CASES))
def test_gemm_kernels_against_long_double(gpu_lib, name):
    L = _lib()
    c = DR.GEMM_CASES[name]
    ref, untouched, bound = DR.gemm_reference(c)
    for kernel, kname in KERNELS:
        rc, got = _gemm(L, kernel, c)
        assert rc == 0, (name, kname, rc)
        worst, changed = DR.gemm_miss(got, c, ref, untouched, bound)
        print(f"[dense-kernels] gemm {name} {kname}: worst err/bound {worst:.3f}, {changed} of {int(untouched.sum())} masked entries changed")
        assert changed == 0, (name, kname, changed)
        assert not np.isnan(got[~untouched]).any(), (name, kname)
        assert worst <= 1.0, (name, kname, worst)


def test_gemm_hook_refuses_what_the_kernels_do_not_support(gpu_lib):
    """Odd strides (the double2 loads of the LDS kernel), a stride below its extent, split K outside 128 rows: HIPENG_ERR_ARG and
    C as it was."""
    L = _lib()
    c = DR.GEMM_CASES["guards"]
    for kernel, _ in KERNELS:
        for over in (dict(ldt=255), dict(ldb=255), dict(ldc=255), dict(ldt=128), dict(ldb=252), dict(ldc=252), dict(ksl=16)):
            rc, got = _gemm(L, kernel, c, **over)
            assert rc == HIPENG_ERR_ARG, (kernel, over, rc)
            assert np.array_equal(got.view(np.uint64), c["C0"].view(np.uint64))


@pytest.mark.parametrize("gemm,gname", GEMMS)
@pytest.mark.parametrize("route,rname", ROUTES)
@pytest.mark.parametrize("name", DR.INVERT_NAMES)
def test_inversion_routes_against_their_restatement(gpu_lib, name, route, rname, gemm, gname):
    L = _lib()
    c = DR.invert_case(name)
    n = c["n"]
    Ainv = np.zeros((n, n))
    assert L.hipeng_dense_invert_route(n, c["A"].ctypes.data, Ainv.ctypes.data, route, gemm) == 0
    e, own, bar = DR.invert_errors(c, Ainv), c[route]["err"], c[route]["bar"]
    print(f"[dense-kernels] invert {name} {rname} {gname}: |Ainv - truth| {e[0]:.2e} = {e[0] / own[0]:.2f} x restatement, {e[0] / bar[0]:.3f} x bar; "
          f"|Ainv A - I| {e[1]:.2e} = {e[1] / own[1]:.2f} x restatement, {e[1] / bar[1]:.3f} x bar")
    assert e[0] <= bar[0] and e[1] <= bar[1], (name, rname, gname, e, bar)
    assert np.array_equal(Ainv, Ainv.T), (name, rname, gname)            # both routes end in k_dd_mirror


def test_pivot_verdicts_of_both_routes(gpu_lib):
    L = _lib()
    for tag, A, verdict in DR.verdict_cases():
        for route, rname in ROUTES:
            for gemm, gname in GEMMS:
                Ainv = np.zeros_like(A)
                rc = L.hipeng_dense_invert_route(256, A.ctypes.data, Ainv.ctypes.data, route, gemm)
                assert rc == verdict, (tag, rname, gname, rc)
                if verdict == 0:
                    assert np.array_equal(Ainv, np.eye(256)), (tag, rname, gname)


def test_dormant_switches_inside_an_engine(gpu_lib):
    """OSQP_AMD_DENSE_GEMM_LDS=0 (k_dd_gemm_tn behind every product of an engine) and OSQP_AMD_DENSE_CHOL=1 (the Cholesky route
    first): one fresh child process each, one at a time; a child that fails, is killed or times out fails the test there."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dense_switch_worker.py")
    for mode, key, val in (("gemm_global", "OSQP_AMD_DENSE_GEMM_LDS", "0"), ("chol_first", "OSQP_AMD_DENSE_CHOL", "1")):
        env = {k: v for k, v in os.environ.items() if k not in ("OSQP_AMD_DENSE_GEMM_LDS", "OSQP_AMD_DENSE_CHOL")}
        env[key] = val
        p = subprocess.run([sys.executable, worker, mode], env=env, capture_output=True, text=True, timeout=300)
        print(p.stdout)
        assert p.returncode == 0, (mode, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        assert f"[dense-switch] {mode}: ok" in p.stdout
