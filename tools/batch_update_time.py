"""Time of a matrix-value update on a live batch against the only route there was before it: for config 4
(1024 x n = 120, m = 240, tiled engine) and for the streamed engine at n = 300, m = 600, B = 1024,
  update:  update_matrices(per-member A values) + warm solve on the live handle
  rebuild: cleanup + setup with the same values + cold solve.
Both legs alternate inside one process; every timed call ends in a stream synchronise inside the library, the clock
is the host's.  Medians over --reps repetitions after --warmup untimed ones.
usage: python tools/batch_update_time.py [--reps 20] [--warmup 3] [--B 1024]"""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=1024)
    a = ap.parse_args()
    s, Q, L, U = mpc_batch(batch=a.B)
    legs = [("tiled, config 4 (n=120, m=240)", "auto", s["P"], s["A"], Q, L, U),
            ("streamed (n=300, m=600)", "streamed") + tuple(problem(300, 600, a.B, seed=300))]
    for name, engine, P, A, Q, L, U in legs:
        A = A.tocsc(); A.sort_indices()
        rng = np.random.default_rng(1)
        Ax = [A.data * rng.uniform(0.9, 1.1, (a.B, A.nnz)) for _ in range(2)]      # a re-linearised model: +-10 % per member
        live = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, Ax_all=Ax[1], engine=engine)
        live.solve(fetch=False)
        other = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, Ax_all=Ax[1], engine=engine)
        other.solve(fetch=False)
        t_upd, t_new, it_upd, it_new = [], [], [], []
        for k in range(a.warmup + a.reps):
            v = Ax[k % 2]
            t0 = time.perf_counter()
            rc = live.update_matrices(Ax=v); live.solve(fetch=False)
            t1 = time.perf_counter()
            other.cleanup()
            other = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, Ax_all=v, engine=engine); other.solve(fetch=False)
            t2 = time.perf_counter()
            assert rc == 0
            if k >= a.warmup:
                t_upd.append(t1 - t0); t_new.append(t2 - t1)
                ru, rn = live.results(), other.results()
                differ = int(np.sum(ru.status_val != rn.status_val))
                it_upd.append(float(ru.iter.mean())); it_new.append(float(rn.iter.mean()))
        mu, mn = statistics.median(t_upd), statistics.median(t_new)
        print("%s, B=%d, %d repetitions after %d warm-up:" % (name, a.B, a.reps, a.warmup))
        print("    update_matrices + warm solve : median %8.3f ms (min %.3f, max %.3f), mean iterations %.1f"
              % (1e3 * mu, 1e3 * min(t_upd), 1e3 * max(t_upd), statistics.mean(it_upd)))
        print("    cleanup + setup + cold solve : median %8.3f ms (min %.3f, max %.3f), mean iterations %.1f"
              % (1e3 * mn, 1e3 * min(t_new), 1e3 * max(t_new), statistics.mean(it_new)))
        print("    update route / rebuild route = %.3f; members whose status differs between the routes (last repetition): %d" % (mu / mn, differ))
        sys.stdout.flush()
        live.cleanup(); other.cleanup()


if __name__ == "__main__":
    main()
