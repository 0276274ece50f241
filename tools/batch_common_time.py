"""Timing of the common-K batch engine (BatchOSQP(engine="common")) against the streamed engine on the same problems in
the same run: B = 1024, m = 2n (capped by the engines' LDS limit), n = 150, 300, 600, 1000, plus config 4's size
(n = 120, m = 240) where the tiled engine (engine="auto") runs too.  The problems are of the common-class family: one
model, one class per row for the batch, per member its own q, bounds and feasible point.

Per shape and engine: one handle; a warm-up solve (code objects, LDS limits), then `--repeats` cold solves (zero
iterates: warm_start = 0) and `--repeats` warm solves (from the last iterates), the engines alternating; each solve
ends in a stream synchronise inside osqp_amd_batch_solve.  The median is reported with the spread.
usage: python tools/batch_common_time.py [--n 120,150,300,600,1000] [--B 1024] [--repeats 3] [--engines common,streamed]
Kernel split, in a run of its own (tracing slows the host):
  rocprofv3 --kernel-trace --stats -d <dir> -o common -- python tools/batch_common_time.py --n 1000 --engines common --repeats 1"""
import argparse
import os
import sys
import time

import numpy as np
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import osqp_amd  # noqa: E402


def problem(n, m, B, seed):
    """Shared diagonally dominant P and sparse A (1-3 entries per row); one class per row for the batch (70 %
    inequality, 10 % equality, 15 % one-sided, 5 % free); per member q, a feasible point and bound widths."""
    rng = np.random.default_rng(seed)
    off = sparse.triu(sparse.random(n, n, density=min(1.0, 3.0 / n), random_state=rng, format="csc"), 1)
    off.data = rng.uniform(-0.3, 0.3, off.nnz)
    full = off + off.T
    d = 1.0 + np.asarray(abs(full).sum(axis=1)).ravel() + rng.uniform(0, 2, n)
    P = sparse.triu(full + sparse.diags(d), format="csc")
    rows, cols, vals = [], [], []
    for i in range(m):
        k = min(n, 1 + i % 3)
        c = rng.choice(n, k, replace=False)
        rows += [i] * k; cols += list(c); vals += list(rng.standard_normal(k))
    A = sparse.csc_matrix((vals, (rows, cols)), shape=(m, n))
    cls = rng.choice(4, m, p=[0.7, 0.1, 0.15, 0.05])
    side = rng.random(m) < 0.5
    AX = (A @ rng.standard_normal((n, B))).T
    Q = rng.standard_normal((B, n))
    L = AX - rng.uniform(0.05, 1.0, (B, m)); U = AX + rng.uniform(0.05, 1.0, (B, m))
    L[:, cls == 1] = U[:, cls == 1] = AX[:, cls == 1]
    L[:, (cls == 2) & side] = -np.inf; U[:, (cls == 2) & ~side] = np.inf
    L[:, cls == 3] = -np.inf; U[:, cls == 3] = np.inf
    return P, A, Q, L, U


def timed(h):
    t0 = time.perf_counter()
    h.solve(fetch=False)                  # returns with the handle's stream synchronised
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="120,150,300,600,1000")
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--engines", default="common,streamed")
    a = ap.parse_args()
    for n in (int(v) for v in a.n.split(",")):
        NP = (n + 31) // 32 * 32
        m = min(2 * n, (160 * 1024 - 8 * (7 * NP + 320)) // 92)
        P, A, Q, L, U = problem(n, m, a.B, seed=n)
        engines = a.engines.split(",") + (["auto"] if n <= 128 and a.engines == "common,streamed" else [])
        hs, setup = {}, {}
        for e in engines:
            t0 = time.perf_counter()
            hs[e] = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=e, warm_start=0)
            setup[e] = time.perf_counter() - t0
            hs[e].solve(fetch=False)      # warm-up
        cold = {e: [] for e in engines}; warm = {e: [] for e in engines}
        for _ in range(a.repeats):
            for e in engines:
                cold[e].append(timed(hs[e]))
        info = {e: hs[e].results() for e in engines}
        rounds = {e: hs[e].rounds() for e in engines}
        for e in engines:
            hs[e].warm_start()            # from here on every solve starts from the last iterates
        for _ in range(a.repeats):
            for e in engines:
                warm[e].append(timed(hs[e]))
        print("n=%d m=%d B=%d NP=%d" % (n, m, a.B, NP))
        for e in engines:
            r, c, w = info[e], np.array(cold[e]), np.array(warm[e])
            it = r.iter.astype(float)
            print("  %-8s setup %.3f s | cold %.2f ms (min %.2f max %.2f) %.0f QPs/s | warm %.2f ms (min %.2f max %.2f) | "
                  "iterations mean %.1f max %d | solved %d/%d | rho updates mean %.2f | rounds %d (inversions %d) refined %d"
                  % (e, setup[e], 1e3 * np.median(c), 1e3 * c.min(), 1e3 * c.max(), a.B / np.median(c),
                     1e3 * np.median(w), 1e3 * w.min(), 1e3 * w.max(), it.mean(), it.max(),
                     int((r.status_val == 1).sum()), a.B, r.rho_updates.mean(), rounds[e][0], rounds[e][0] - 1, rounds[e][1]))
        if "common" in engines and "streamed" in engines:
            print("  common / streamed: cold %.2fx, per iteration %.2fx (%.1f vs %.1f us per ADMM iteration of the batch)"
                  % (np.median(cold["streamed"]) / np.median(cold["common"]),
                     (np.median(cold["streamed"]) / info["streamed"].iter.max()) / (np.median(cold["common"]) / info["common"].iter.max()),
                     1e6 * np.median(cold["common"]) / info["common"].iter.max(),
                     1e6 * np.median(cold["streamed"]) / info["streamed"].iter.max()))
        for h in hs.values():
            h.cleanup()
        sys.stdout.flush()


if __name__ == "__main__":
    main()
