"""Time of polish on a solved batch: for config 4 (1024 x n = 120, m = 240, tiled engine) and for the streamed
engine at n = 300, m = 600, B = 1024,
  solve:   a cold solve of the handle (setup excluded);
  polish:  BatchOSQP.polish() on the solved handle, results left on the device (the C call ends in a stream synchronise);
  single:  the only route to a polished member before -- one single-QP engine per member with polish=1 -- as the
           setup-excluded solve time per member over a sample of --sample members, scaled to the batch.
Every repetition is a fresh cold solve followed by one polish; medians over --reps after --warmup untimed ones.
usage: python tools/batch_polish_time.py [--reps 5] [--warmup 1] [--B 1024] [--sample 64]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import osqp_amd  # noqa: E402
from osqp_amd import abi  # noqa: E402
from osqp_amd.problems import mpc_batch  # noqa: E402
from tools.batch_streamed_time import problem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    s, Q, L, U = mpc_batch(batch=a.B)
    legs = [("tiled, config 4 (n=120, m=240)", "auto", s["P"], s["A"], Q, L, U),
            ("streamed (n=300, m=600)", "streamed") + tuple(problem(300, 600, a.B, seed=300))]
    for name, engine, P, A, Q, L, U in legs:
        h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, warm_start=0)
        sp = np.zeros(a.B, np.int64)
        t_solve, t_pol = [], []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            h.solve(fetch=False)
            t1 = time.perf_counter()
            rc = h._lib.osqp_amd_batch_polish(h._h, abi.iptr(sp))
            t2 = time.perf_counter()
            assert rc == 0, rc
            if k >= a.warmup:
                t_solve.append(t1 - t0); t_pol.append(t2 - t1)
        r = h.results()
        ms, mp = statistics.median(t_solve), statistics.median(t_pol)
        k = min(a.sample, a.B)
        t_one = 0.0
        agree = 0
        for b in range(k):
            one = osqp_amd.OSQP().setup(P=P, q=Q[b], A=A, l=L[b], u=U[b], polish=1)
            t0 = time.perf_counter()
            ro = one.solve()
            t_one += time.perf_counter() - t0
            agree += int(ro.info.status_polish == sp[b])
            one.cleanup()
        print("%s, B=%d, %d repetitions after %d warm-up:" % (name, a.B, a.reps, a.warmup))
        print("    cold solve                   : median %9.3f ms (min %.3f, max %.3f), mean iterations %.1f, solved %d"
              % (1e3 * ms, 1e3 * min(t_solve), 1e3 * max(t_solve), r.iter.mean(), int(np.sum(r.status_val == 1))))
        print("    polish()                     : median %9.3f ms (min %.3f, max %.3f); accepted %d, rejected %d, skipped %d;"
              " worst polished residuals %.1e / %.1e"
              % (1e3 * mp, 1e3 * min(t_pol), 1e3 * max(t_pol), int(np.sum(sp == 1)), int(np.sum(sp == -1)), int(np.sum(sp == 0)),
                 r.pri_res[sp == 1].max() if np.any(sp == 1) else float("nan"), r.dua_res[sp == 1].max() if np.any(sp == 1) else float("nan")))
        print("    OSQP(polish=1), one per member: %9.3f ms per member over %d members = %.1f ms for the batch (solve + polish,"
              " setup excluded); status_polish agrees on %d of %d" % (1e3 * t_one / k, k, 1e3 * t_one / k * a.B, agree, k))
        print("    polish / cold solve = %.2f; per-member route / (cold solve + polish) = %.1f"
              % (mp / ms, (t_one / k * a.B) / (ms + mp)))
        sys.stdout.flush()
        h.cleanup()


if __name__ == "__main__":
    main()
