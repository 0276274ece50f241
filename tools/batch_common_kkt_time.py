"""Time of polish, adjoint and tangent on the shared KKT pieces of the common-K engine (osqp_amd_batch_common_kkt) against
the streamed engine's full-KKT route on the same batch: B = 1024, m = 2n capped by the LDS limit, n = 300 / 600 / 1000,
the family of tools/batch_common_time.py, default settings.  Two legs, one process each, one after the other on the same
device:
  common    this tree, engine="common": setup, then shared_kkt(True) timed (H pivots and Wt together: the call returns
            with the stream synchronised; a second handle on the same P without rows times H alone, the
            difference is Wt), then per repetition a cold solve, polish, adjoint D = 1 (it builds the members' S^-1),
            adjoint D = 8 and tangent D = 8 (both on the kept inversion when one chunk holds the batch);
  streamed  --parent-tree DIR, a built checkout of the parent commit, engine="streamed": the same four calls.
Host arrays in and out: the copies are part of every call, every call returns with the handle's stream synchronised.
Medians over --reps after --warmup untimed repetitions.  Also printed: active rows per member (mean, max), NS against
NPOL, bytes of the KKT buffer of each route and the chunks they make under OSQP_AMD_BATCH_POLISH_CAP_BYTES (8 GiB).
--parent-n: the sizes of the streamed leg (its matrices of order n + mred make n = 1000 take minutes per repetition).
usage: python tools/batch_common_kkt_time.py [--parent-tree DIR] [--n 300,600,1000] [--parent-n 300,600] [--reps 3] [--warmup 1] [--B 1024]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 8 << 30


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    sys.path.insert(1, ROOT)
    import osqp_amd
    from tools.batch_common_time import problem
    common = a.leg == "common"
    rng = np.random.default_rng(0)
    for n in (int(v) for v in a.n.split(",")):
        m = min(2 * n, 1129)
        P, A, Q, L, U = problem(n, m, a.B, seed=n)
        kw = dict(engine="common") if common else dict(engine="streamed")
        h, t_setup = clock(lambda: osqp_amd.BatchOSQP().setup(P, A, Q, L, U, warm_start=0, **kw))
        line = "  n=%d m=%d B=%d: setup %.3f s" % (n, m, a.B, t_setup)
        if common:
            _, t_on = clock(lambda: h.shared_kkt(True))
            h.shared_kkt(False)
            _, t_on2 = clock(lambda: h.shared_kkt(True))
            line += " | shared_kkt(True) %.1f ms first, %.1f ms again after shared_kkt(False)" % (1e3 * t_on, 1e3 * t_on2)
            h0 = osqp_amd.BatchOSQP().setup(P, A[:0], Q[:2], np.zeros((2, 0)), np.zeros((2, 0)), engine="common")
            h0.shared_kkt(True); h0.shared_kkt(False)
            _, t_h = clock(lambda: h0.shared_kkt(True))
            line += " | H alone (a handle without rows) %.1f ms, so Wt ~ %.1f ms" % (1e3 * t_h, 1e3 * max(t_on2 - t_h, 0.0))
            h0.cleanup()
        print(line)
        B, nn, mm = h.B, h.n, h.m
        gx, gy = rng.standard_normal((B, 8, nn)), rng.standard_normal((B, 8, mm))
        dQ = rng.standard_normal((B, 8, nn))
        keys = ["solve", "polish", "adjoint D=1", "adjoint D=8", "tangent D=8"]
        t = {k: [] for k in keys}
        for k in range(a.warmup + a.reps):
            c = [time.perf_counter()]
            h.solve(fetch=False); c.append(time.perf_counter())
            r = h.polish(); c.append(time.perf_counter())
            g = h.adjoint(np.ascontiguousarray(gx[:, 0]), np.ascontiguousarray(gy[:, 0])); c.append(time.perf_counter())
            h.adjoint(gx, gy); c.append(time.perf_counter())
            h.tangent(dQ=dQ); c.append(time.perf_counter())
            if k >= a.warmup:
                for key, v in zip(keys, np.diff(c)):
                    t[key].append(v)
        for k, v in t.items():
            print("    %-12s: median %9.3f ms (min %.3f, max %.3f)" % (k, 1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)))
        mred = np.count_nonzero(g.active, axis=1)[g.status_adjoint != 0]
        mmax = int(mred.max()) if mred.size else 0
        NPOL, NS = (nn + mmax + 31) & ~31, max(32, (mmax + 31) & ~31)
        order = NS if common else NPOL
        per = order * order * 8
        chunk = max(1, min(int(mred.size), CAP // per))
        info = h.kkt_info()
        print("    solved %d, polish accepted %d, adjoint computed %d rejected %d | active rows mean %.1f max %d | NS %d NPOL %d | "
              "KKT buffer %d x %d doubles per member = %.2f GiB for the batch, %d chunk(s) | kept %d, builds per repetition %.1f"
              % (int(np.sum(r.status_val == 1)), int(np.sum(r.status_polish == 1)), int(np.sum(g.status_adjoint == 1)),
                 int(np.sum(g.status_adjoint == -1)), mred.mean() if mred.size else 0.0, mmax, NS, NPOL, order, order,
                 per * mred.size / 2.0 ** 30, -(-int(mred.size) // chunk), info.kept, info.builds / (a.warmup + a.reps)))
        sys.stdout.flush()
        h.cleanup()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="300,600,1000")
    ap.add_argument("--parent-n", default="300,600")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the streamed leg)")
    ap.add_argument("--leg", choices=["common", "streamed"], help="run one leg in this process (what the tool starts itself)")
    ap.add_argument("--tree", help="with --leg streamed: the tree to import from")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup), "--B", str(a.B)]
    runs = [("common-K engine with the shared KKT pieces (this tree)", ["--leg", "common", "--n", a.n])]
    if a.parent_tree:
        runs.append(("streamed engine, full KKT route (parent commit)", ["--leg", "streamed", "--tree", a.parent_tree, "--n", a.parent_n]))
    for title, args in runs:
        print(title + ":")
        sys.stdout.flush()
        subprocess.run(base + args, check=True, timeout=900)


if __name__ == "__main__":
    main()
