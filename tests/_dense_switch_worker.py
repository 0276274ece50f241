"""Child process of tests/test_gpu_dense_kernels.py::test_dormant_switches_inside_an_engine.  The two switches it is about are
read once per process (dd_gemm: OSQP_AMD_DENSE_GEMM_LDS, dd_refresh: OSQP_AMD_DENSE_CHOL), so each setting needs a process that
has not refreshed a dense-direct engine yet.  argv[1]: "gemm_global" (the parent set OSQP_AMD_DENSE_GEMM_LDS=0) or "chol_first"
(OSQP_AMD_DENSE_CHOL=1).  Asserts hipeng_dense_switches before and after the first engine, then holds three cases of
tests/test_gpu_direct_solve_edges.py to the bars of Engine.check; prints the ratios; exit status 0 = all held."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {"gemm_global": ("OSQP_AMD_DENSE_GEMM_LDS", "0", [0, 0]), "chol_first": ("OSQP_AMD_DENSE_CHOL", "1", [1, 1])}
DD_ENV = dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=2)


def main(mode):
    key, val, want = MODES[mode]
    assert os.environ.get(key) == val, (key, os.environ.get(key))
    import osqp_amd
    from tests._direct_problems import dd_problem
    from tests._hipeng import Engine
    L = osqp_amd.lib()
    L.hipeng_dense_switches.restype, L.hipeng_dense_switches.argtypes = C.c_int, [C.POINTER(C.c_int)]

    def switches():
        out = (C.c_int * 2)()
        assert L.hipeng_dense_switches(out) == 0
        return list(out)

    assert switches() == [-1, -1], switches()
    cases = (("dd na=129", lambda: dd_problem(129, seed=129)),
             ("dd na=1025", lambda: dd_problem(1025, seed=1025)),
             ("dd slacks pyy=0.0 b2", lambda: dd_problem(150, seed=2, nslack=20, pyy=0.0, b2_nbrs=(2, 8, 9))))
    for tag, make in cases:
        e = Engine(*make(), env=DD_ENV)
        try:
            assert switches() == want, (tag, switches(), want)
            # chol_first: the Cholesky route serves; gemm_global: whichever route the probes chose is held to the bar
            worst = e.check(f"{mode}: {tag}", 4, 1 if mode == "chol_first" else None)
            print(f"[dense-switch] {mode}: {tag}: route {e.info()[5]} worst err/bar {worst:.3f}")
        finally:
            e.close()
    assert switches() == want
    print(f"[dense-switch] {mode}: ok")


if __name__ == "__main__":
    main(sys.argv[1])
