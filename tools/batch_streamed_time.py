"""Timing of the streamed-inverse batch engine (BatchOSQP(engine="streamed")) at B = 1024 and n = 150, 300, 600,
1000 (m = 2n, capped by the engine's LDS limit), against the per-member path (one single-QP engine per member,
eight streams) on a sample of 64 members.
usage: python tools/batch_streamed_time.py [--n 150,300,600,1000] [--B 1024] [--sample 64]"""
import argparse
import os
import sys
import time

import numpy as np
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import osqp_amd  # noqa: E402

HBM_TBS = 8.0     # MI355X peak HBM bandwidth, TB/s


def problem(n, m, B, seed):
    """Shared diagonally dominant P and sparse A (1-3 entries per row); per member q and a mix of row classes."""
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
    ax = A @ rng.standard_normal(n)
    Q = rng.standard_normal((B, n))
    L = np.tile(ax - 1.0, (B, 1)) - rng.uniform(0, 1, (B, m))
    U = np.tile(ax + 1.0, (B, 1)) + rng.uniform(0, 1, (B, m))
    eq = rng.random((B, m)) < 0.1
    L[eq] = U[eq] = np.tile(ax, (B, 1))[eq]
    return P, A, Q, L, U


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="150,300,600,1000")
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    for n in (int(v) for v in a.n.split(",")):
        NP = (n + 31) // 32 * 32
        m = min(2 * n, (160 * 1024 - 8 * (7 * NP + 320)) // 92)
        P, A, Q, L, U = problem(n, m, a.B, seed=n)
        t0 = time.perf_counter()
        bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="streamed")
        t1 = time.perf_counter()
        bs.solve(fetch=False)
        t2 = time.perf_counter()
        rounds, refined = bs.rounds()
        r = bs.results()
        t3 = time.perf_counter()
        bs.solve(fetch=False)
        t4 = time.perf_counter()
        cold, warm = t2 - t1, t4 - t3
        it = r.iter.astype(float)
        kbytes = 8.0 * NP * NP * it.sum()
        print("n=%d m=%d B=%d NP=%d: setup %.3f s, cold solve %.1f ms, warm solve %.1f ms, %.0f QPs/s (cold)"
              % (n, m, a.B, NP, t1 - t0, 1e3 * cold, 1e3 * warm, a.B / cold))
        print("    iterations mean %.1f max %d, rho updates mean %.2f, loop rounds %d, refined members %d"
              % (it.mean(), it.max(), r.rho_updates.mean(), rounds, refined))
        print("    K^-1 streamed, one pass per member-iteration: %.2f GB = %.1f ms at %.0f TB/s; the cold solve moved "
              "it at %.2f TB/s" % (kbytes / 1e9, 1e3 * kbytes / (HBM_TBS * 1e12), HBM_TBS, kbytes / cold / 1e12))
        bs.cleanup()
        S = min(a.sample, a.B)
        sp = osqp_amd.BatchOSQP().setup(P, A, Q[:S], L[:S], U[:S])      # n > 128: one single-QP engine per member
        t5 = time.perf_counter()
        rp = sp.solve()
        t6 = time.perf_counter()
        per = (t6 - t5) / S
        print("    per-member path, a SAMPLE of %d members: %.1f ms, %.0f QPs/s; streamed (cold) / per-member = %.1fx; "
              "iteration counts equal on the sample: %s"
              % (S, 1e3 * (t6 - t5), 1.0 / per, (a.B / cold) * per, bool(np.array_equal(rp.iter, r.iter[:S]))))
        sp.cleanup()
        sys.stdout.flush()


if __name__ == "__main__":
    main()
