"""Time of the tangent call on a solved and polished batch: for config 4 (1024 x n = 120, m = 240, tiled engine)
and for the streamed engine at n = 300, m = 600, B = 1024,
  solve:    a cold solve of the handle (setup excluded);
  polish:   BatchOSQP.polish() on the solved handle;
  adjoint:  BatchOSQP.adjoint(dX, dY) on the polished handle (one row of the Jacobian);
  tangent:  BatchOSQP.tangent(dQ, dL, dU) with D = 1 and with D = 8 directions per member (one and eight columns; the
            eight share one KKT inversion), and with D = 8 and the matrix tangents too (host arrays in and out: the
            copies are part of the call).
Every repetition is a fresh cold solve, one polish, one adjoint and the three tangent calls; medians over --reps after
--warmup untimed ones.
usage: python tools/batch_tangent_time.py [--reps 5] [--warmup 1] [--B 1024]"""
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

D = 8


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
        B, n, m = h.B, h.n, h.m
        dX, dY = rng.standard_normal((B, n)), rng.standard_normal((B, m))
        dQ, dL, dU = (rng.standard_normal((B, D, k)) for k in (n, m, m))
        dPx, dAx = rng.standard_normal((B, D, h.Pu.nnz)), rng.standard_normal((B, D, h.Ah.nnz))
        one = dict(dQ=dQ[:, 0].copy(), dL=dL[:, 0].copy(), dU=dU[:, 0].copy())
        t = {k: [] for k in ("solve", "polish", "adjoint", "tangent D=1", "tangent D=%d" % D, "tangent D=%d+matrices" % D)}
        for k in range(a.warmup + a.reps):
            c = [time.perf_counter()]
            h.solve(fetch=False); c.append(time.perf_counter())
            r = h.polish(); c.append(time.perf_counter())
            g = h.adjoint(dX, dY); c.append(time.perf_counter())
            t1 = h.tangent(**one); c.append(time.perf_counter())
            t8 = h.tangent(dQ=dQ, dL=dL, dU=dU); c.append(time.perf_counter())
            h.tangent(dQ=dQ, dL=dL, dU=dU, dPx=dPx, dAx=dAx); c.append(time.perf_counter())
            if k >= a.warmup:
                for key, v in zip(t, np.diff(c)):
                    t[key].append(v)
        assert np.array_equal(t1.dx, t8.dx[:, 0]) and np.array_equal(t1.dy, t8.dy[:, 0])
        med = {k: statistics.median(v) for k, v in t.items()}
        print("%s, B=%d, %d repetitions after %d warm-up:" % (name, a.B, a.reps, a.warmup))
        for k, v in t.items():
            print("    %-21s: median %9.3f ms (min %.3f, max %.3f)" % (k, 1e3 * med[k], 1e3 * min(v), 1e3 * max(v)))
        st = t1.status_tangent
        print("    solved %d, polish accepted %d; tangent computed %d, rejected %d, skipped %d; active rows per member %.1f"
              % (int(np.sum(r.status_val == 1)), int(np.sum(r.status_polish == 1)), int(np.sum(st == 1)), int(np.sum(st == -1)),
                 int(np.sum(st == 0)), np.count_nonzero(t1.active, axis=1).mean()))
        print("    tangent D=1 / adjoint = %.2f; tangent D=%d / (%d x tangent D=1) = %.2f; tangent D=1 / cold solve = %.2f"
              % (med["tangent D=1"] / med["adjoint"], D, D, med["tangent D=%d" % D] / (D * med["tangent D=1"]),
                 med["tangent D=1"] / med["solve"]))
        assert np.array_equal(g.active, t1.active)
        sys.stdout.flush()
        h.cleanup()


if __name__ == "__main__":
    main()
