"""Shared set-up of tests/test_gpu_iteration_chain.py, and the child process of its segment test: the number of segments per
graph (OSQP_AMD_GRAPH_SEGS) is read when an engine is created; the single-segment run has a process of its own, with the variable
set for all of it.

  python tests/_iteration_chain_worker.py CASE ENV COUNT OUT.npz      (ENV: steps | default | resident)
runs COUNT ADMM iterations in one hipeng_run_admm call and saves x, y, z."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _engine_reference as R

PCG_EPS = 1e-12
ENVS = dict(steps=dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=0), default={},
            resident=dict(OSQP_AMD_RESIDENT_MIN_N=1, OSQP_AMD_DENSE_DIRECT=0))     # the resident PCG far below its size


def open_case(c, env, alpha=1.6, pcg_eps_rel=PCG_EPS, rho=None):
    """Engine on case c in the order of the solver's set-up (create, ten Ruiz sweeps, rho), the seeded iterates loaded.
    Returns (engine, dict of what Ruiz returned, Problem of the scaled data, (x0, y0, z0))."""
    from tests._hipeng import Engine
    e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=ENVS[env], q=c["q"], l=c["l"], u=c["u"], alpha=alpha,
               pcg_eps_rel=pcg_eps_rel, pcg_max_iter=20000)
    o = e.ruiz_scale(10)
    e.matrices_changed()
    e.set_rho(c["rho"] if rho is None else rho)
    Pu, A = c["Pu"].copy(), c["A"].copy()
    Pu.data, A.data = o["Px"].copy(), o["Ax"].copy()
    pb = R.Problem(Pu, A, o["q"], o["l"], o["u"], o["D"], o["E"])
    x0, y0, z0 = R.iterates(c)
    e.set_iterates(x0, y0, z0)
    return e, o, pb, (x0, y0, z0)


def main(argv):
    name, env, count, out = argv[0], argv[1], int(argv[2]), argv[3]
    e, _, _, _ = open_case(R.make_case(name), env)
    try:
        e.run_admm(count)
        x, y, z, _, _ = e.download(False)
        st = e.stats()
    finally:
        e.close()
    np.savez(out, x=x, y=y, z=z, launches=st["graph_launches"])


if __name__ == "__main__":
    main(sys.argv[1:])
