"""Time of the derivative calls of the single-QP engine at config 2's size (random sparse QP, n = 10 000, m = 20 000):
  solve:     a cold solve of the handle with polish = 1 (setup excluded; polish builds and frees its own KKT instance);
  adjoint:   OSQP.adjoint(dx, dy) without and with the matrix gradients;
  tangent:   OSQP.tangent with D = 1 and with D = 8 directions (all five tangents), first call and second call on the
             same solve.
Each repetition is a fresh cold solve; the FIRST derivative call after it builds the KKT instance (Ared, a polish-mode
plugin instance), every later one reuses it, so the calls are timed in two orders: adjoint first, and tangent first.
Medians over --reps after --warmup untimed repetitions.
usage: python tools/single_sens_time.py [--n 10000] [--m 20000] [--reps 3] [--warmup 1]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import osqp_amd  # noqa: E402
from osqp_amd.problems import random_sparse_qp  # noqa: E402

D = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    pb = random_sparse_qp(a.n, a.m, seed=1)
    h = osqp_amd.OSQP().setup(**pb, polish=1, warm_start=0)
    n, m = h.n, h.m
    rng = np.random.default_rng(0)
    gx, gy = rng.standard_normal(n), rng.standard_normal(m)
    tan = [rng.standard_normal((D, k)) for k in (n, m, m, h.nnzP, h.nnzA)]
    one = [v[0].copy() for v in tan]
    keys = ("solve", "adjoint (first call: builds the instance)", "adjoint + matrices", "tangent D=1", "tangent D=%d" % D,
            "tangent D=%d again" % D, "solve (2)", "tangent D=1 (first call: builds the instance)", "tangent D=1 again", "adjoint")
    t = {k: [] for k in keys}
    for k in range(a.warmup + a.reps):
        c = [time.perf_counter()]
        r = h.solve(); c.append(time.perf_counter())
        solves0 = h.sens_info()["solves"]
        g0 = h.adjoint(gx, gy); c.append(time.perf_counter())
        g1 = h.adjoint(gx, gy, matrices=True); c.append(time.perf_counter())
        t1 = h.tangent(*one); c.append(time.perf_counter())
        t8 = h.tangent(*tan); c.append(time.perf_counter())
        h.tangent(*tan); c.append(time.perf_counter())
        info = h.sens_info()
        info["solves"] -= solves0
        h.solve(); c.append(time.perf_counter())
        h.tangent(*one); c.append(time.perf_counter())
        h.tangent(*one); c.append(time.perf_counter())
        h.adjoint(gx, gy); c.append(time.perf_counter())
        if k >= a.warmup:
            for key, v in zip(keys, np.diff(c)):
                t[key].append(v)
    assert np.array_equal(t1.dx, t8.dx[0]) and np.array_equal(g0.dq, g1.dq)
    print("random sparse QP n=%d m=%d nnz(P)=%d nnz(A)=%d, %d repetitions after %d warm-up; status %s, polish %d, iterations %d"
          % (n, m, h.nnzP, h.nnzA, a.reps, a.warmup, r.info.status, r.info.status_polish, r.info.iter))
    for key in keys:
        v = t[key]
        print("    %-46s: median %9.3f ms (min %.3f, max %.3f)" % (key, 1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)))
    print("    status_adjoint %d status_tangent %d, active rows %d, kkt_res adjoint %.1e tangent %.1e .. %.1e; linear solves of the five calls after the first solve (19 refined solves) %d"
          % (g1.status_adjoint, t8.status_tangent, info["active_rows"], g1.kkt_res, t8.kkt_res.min(), t8.kkt_res.max(), info["solves"]))
    h.cleanup()


if __name__ == "__main__":
    main()
