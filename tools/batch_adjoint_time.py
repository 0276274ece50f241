"""Time of the adjoint call on a solved and polished batch: for config 4 (1024 x n = 120, m = 240, tiled engine)
and for the streamed engine at n = 300, m = 600, B = 1024,
  solve:    a cold solve of the handle (setup excluded);
  polish:   BatchOSQP.polish() on the solved handle;
  adjoint:  BatchOSQP.adjoint(dX, dY) on the polished handle, without and with the matrix gradients (host arrays in
            and out: the copies are part of the call).
Every repetition is a fresh cold solve, one polish and the two adjoint calls; medians over --reps after --warmup
untimed ones.
usage: python tools/batch_adjoint_time.py [--reps 5] [--warmup 1] [--B 1024]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import osqp_amd  # noqa: E402
from osqp_amd.problems import mpc_batch  # noqa: E402
from tools.batch_streamed_time import problem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--B", type=int, default=1024)
    a = ap.parse_args()
    s, Q, L, U = mpc_batch(batch=a.B)
    legs = [("tiled, config 4 (n=120, m=240)", "auto", s["P"], s["A"], Q, L, U),
            ("streamed (n=300, m=600)", "streamed") + tuple(problem(300, 600, a.B, seed=300))]
    rng = np.random.default_rng(0)
    for name, engine, P, A, Q, L, U in legs:
        h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, warm_start=0)
        dX, dY = rng.standard_normal(Q.shape), rng.standard_normal(L.shape)
        t = {k: [] for k in ("solve", "polish", "adjoint", "adjoint+matrices")}
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            h.solve(fetch=False)
            t1 = time.perf_counter()
            r = h.polish()
            t2 = time.perf_counter()
            g = h.adjoint(dX, dY)
            t3 = time.perf_counter()
            gm = h.adjoint(dX, dY, matrices=True)
            t4 = time.perf_counter()
            if k >= a.warmup:
                for key, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    t[key].append(v)
        assert np.array_equal(g.dq, gm.dq)
        med = {k: statistics.median(v) for k, v in t.items()}
        print("%s, B=%d, %d repetitions after %d warm-up:" % (name, a.B, a.reps, a.warmup))
        for k, v in t.items():
            print("    %-17s: median %9.3f ms (min %.3f, max %.3f)" % (k, 1e3 * med[k], 1e3 * min(v), 1e3 * max(v)))
        sa = g.status_adjoint
        print("    solved %d, polish accepted %d; adjoint computed %d, rejected %d, skipped %d; active rows per member %.1f"
              % (int(np.sum(r.status_val == 1)), int(np.sum(r.status_polish == 1)), int(np.sum(sa == 1)), int(np.sum(sa == -1)),
                 int(np.sum(sa == 0)), np.count_nonzero(g.active, axis=1).mean()))
        print("    adjoint / polish = %.2f; adjoint / cold solve = %.2f" % (med["adjoint"] / med["polish"], med["adjoint"] / med["solve"]))
        sys.stdout.flush()
        h.cleanup()


if __name__ == "__main__":
    main()
