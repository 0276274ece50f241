"""Iterates of the engine on the small seeded cases, to compare two builds bit for bit.

  python tools/iterate_bits.py run OUT.npz        x, y, z after 3 and after 30 ADMM iterations of every case of
                                                  tests/_engine_reference.make_case below, on the launch-per-step kernels
                                                  (OSQP_AMD_RESIDENT=0 OSQP_AMD_DENSE_DIRECT=0) and with the defaults;
                                                  and x, y of a Lasso QP (150 features, 300 data points: its 300 residual
                                                  variables are eliminated from the linear system) solved through the solver
                                                  on the launch-per-step kernels and on the resident PCG
  python tools/iterate_bits.py cmp A.npz B.npz    one line per array: elements whose bits differ; exit status 1 if any does

A change that claims to leave the arithmetic alone (profiles/iter_kernels_chain_identity.txt) runs `run` at both commits."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("tiny3", "m0", "offtile", "empty", "long", "huge", "bounds")
ENVS = (("steps", dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=0)), ("default", {}))


def run(out):
    from tests import _engine_reference as R
    from tests._hipeng import Engine
    res = {}
    for name in CASES:
        c = R.make_case(name)
        for env_name, env in ENVS:
            e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=env, q=c["q"], l=c["l"], u=c["u"], alpha=1.6, pcg_eps_rel=1e-12,
                       pcg_max_iter=20000)
            try:
                e.ruiz_scale(10)
                e.matrices_changed()
                e.set_rho(c["rho"])
                x0, y0, z0 = R.iterates(c)
                e.set_iterates(x0, y0, z0)
                done = 0
                for count in (3, 30):
                    e.run_admm(count - done)
                    done = count
                    x, y, z, _, _ = e.download(False)
                    for k, v in (("x", x), ("y", y), ("z", z)):
                        res[f"{name}/{env_name}/{count}/{k}"] = v
                inf, st = e.info(), e.stats()
                print(f"{name}/{env_name}: form {inf[9]} in use {inf[1]} gave up {inf[10]}, PCG iterations of the last solve {st['pcg_iters_last']}")
            finally:
                e.close()
    # engines with eliminated variables (Ctx::nelim): the solver's own path, PCG forms only (OSQP_AMD_DENSE_SMALL=0)
    import ctypes as C
    import osqp_amd
    from osqp_amd.problems import lasso_qp
    L = osqp_amd.lib()
    L.hipeng_elim_count.restype, L.hipeng_elim_count.argtypes = C.c_longlong, [C.c_void_p]
    pb = lasso_qp(150, 300, density=0.15, seed=3)
    data = {k: pb[k] for k in "PqAlu"}
    for resident in (0, 1):
        old = {k: os.environ.get(k) for k in ("OSQP_AMD_RESIDENT", "OSQP_AMD_DENSE_SMALL")}
        os.environ.update(OSQP_AMD_RESIDENT=str(resident), OSQP_AMD_DENSE_SMALL="0")
        try:
            sg = osqp_amd.OSQP().setup(**data, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        r = sg.solve()
        tag = "lasso150x300/" + ("resident" if resident else "steps")
        res[tag + "/x"], res[tag + "/y"] = np.asarray(r.x, float), np.asarray(r.y, float)
        res[tag + "/iter"] = np.array([float(r.info.iter), float(sg.stats()["pcg_iters_total"])])
        print(f"{tag}: eliminated {int(L.hipeng_elim_count(sg.engine()))}, resident {sg.stats()['resident']}, status {r.info.status}, "
              f"iterations {r.info.iter}, PCG iterations {sg.stats()['pcg_iters_total']}")
    np.savez(out, **res)


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    for k in sorted(set(A.files) | set(B.files)):
        if k not in A.files or k not in B.files:
            print(f"{k}: missing in one file"); bad += 1
            continue
        va, vb = A[k].astype(np.float64), B[k].astype(np.float64)
        d = int((va.view(np.uint64) != vb.view(np.uint64)).sum()) if va.shape == vb.shape else -1
        print(f"{k}: {va.size} elements, {d} differ")
        bad += d != 0
    print("identical" if not bad else f"{bad} arrays differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
