"""Time of a matrix-value update for chosen members of a live batch against the whole-batch call that was the only route
before: config 4 (1024 x n = 120, m = 240, tiled engine) and the streamed engine at n = 300, m = 600, B = 1024.  Per
repetition, on one live handle with per-member A values (a re-linearised model: +-10 % per member):
  members |S|   update_matrices(Ax=[|S|, k], members=S) for |S| = 1, 16, 64 spread over the batch, then a warm solve();
  whole batch   update_matrices(Ax=[B, k]), then a warm solve();
  cold solve    solve() on a second handle set up with warm_start=0.
Every timed call ends in a stream synchronise inside the library; the clock is the host's.  A round is one process: medians
over --reps repetitions after --warmup untimed ones.  The tool runs --rounds rounds and prints, per leg, the range of the
rounds' medians.  With --parent-tree DIR (a built checkout of the parent commit) every round runs three processes one
after the other: this tree with all legs, this tree with the whole-batch leg and the cold solve only, and the parent with
those two -- the same calls on the same handle states, so that the two builds can be compared: this tree's must stay
inside the parent's own range (the median over its rounds between the parent's fastest and slowest round).
usage: python tools/batch_update_members_time.py [--parent-tree DIR] [--rounds 6] [--reps 5] [--warmup 1] [--B 1024]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 16, 64)


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    from osqp_amd.problems import mpc_batch
    from tools.batch_streamed_time import problem
    s, Q, L, U = mpc_batch(batch=a.B)
    legs = [("tiled, config 4 (n=120, m=240)", "auto", s["P"], s["A"], Q, L, U),
            ("streamed (n=300, m=600)", "streamed") + tuple(problem(300, 600, a.B, seed=300))]
    out = {}
    for name, engine, P, A, Q, L, U in legs:
        A = A.tocsc(); A.sort_indices()
        rng = np.random.default_rng(1)
        Ax = [A.data * rng.uniform(0.9, 1.1, (a.B, A.nnz)) for _ in range(2)]
        live = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, Ax_all=Ax[1], engine=engine)
        live.solve(fetch=False)
        cold = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, Ax_all=Ax[1], engine=engine, warm_start=0)
        lists = [] if a.whole_only else [np.unique(np.linspace(0, a.B - 1, k).astype(np.int64)) for k in SIZES if k <= a.B]
        t = {}
        for k in range(a.warmup + a.reps):
            v = Ax[k % 2]
            c = {}
            for S in lists:
                rows = np.ascontiguousarray(v[S])
                t0 = time.perf_counter()
                rc = live.update_matrices(Ax=rows, members=S)
                t1 = time.perf_counter()
                live.solve(fetch=False)
                t2 = time.perf_counter()
                assert rc == 0
                c["update_matrices(members=S), |S| = %d" % S.size] = t1 - t0
                c["  warm solve after it, |S| = %d" % S.size] = t2 - t1
            t0 = time.perf_counter()
            rc = live.update_matrices(Ax=v)
            t1 = time.perf_counter()
            live.solve(fetch=False)
            t2 = time.perf_counter()
            cold.solve(fetch=False)
            t3 = time.perf_counter()
            assert rc == 0
            c["update_matrices, whole batch [B, k]"] = t1 - t0
            c["  warm solve after it"] = t2 - t1
            c["cold solve"] = t3 - t2
            if k >= a.warmup:
                for key, val in c.items():
                    t.setdefault(key, []).append(val)
        out[name] = {key: 1e3 * statistics.median(val) for key, val in t.items()}
        live.cleanup(); cold.cleanup()
    print("ROUND " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the parent's rounds)")
    ap.add_argument("--leg", action="store_true", help="run one round in this process (what the tool starts itself)")
    ap.add_argument("--whole-only", action="store_true", help="with --leg: the legs the parent commit has")
    ap.add_argument("--tree", help="with --leg: the tree to import from")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    base = [sys.executable, os.path.abspath(__file__), "--leg", "--reps", str(a.reps), "--warmup", str(a.warmup), "--B", str(a.B)]
    trees = [("this tree", [])]
    if a.parent_tree:
        trees.append(("this tree, whole-batch legs only", ["--whole-only"]))
        trees.append(("parent commit", ["--whole-only", "--tree", a.parent_tree]))
    rounds = {title: [] for title, _ in trees}
    for r in range(a.rounds):
        for title, args in trees:                           # the builds alternate
            p = subprocess.run(base + args, check=True, timeout=900, stdout=subprocess.PIPE, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROUND ")][-1]
            rounds[title].append(json.loads(line[6:]))
            print("round %d, %s: done" % (r + 1, title))
            sys.stdout.flush()
    print("B=%d, %d rounds (one process each, alternating), medians of %d repetitions after %d warm-up; "
          "range of the rounds' medians in ms:" % (a.B, a.rounds, a.reps, a.warmup))
    for title, _ in trees:
        print(title + ":")
        for name in rounds[title][0]:
            print("  " + name)
            for key in rounds[title][0][name]:
                v = [rd[name][key] for rd in rounds[title]]
                print("    %-44s: %9.3f .. %9.3f" % (key, min(v), max(v)))
    if a.parent_tree:
        print("this tree against the parent's own range (inside: the median over this tree's rounds lies between the parent's "
              "fastest and slowest round; then this tree's slowest round against the parent's slowest):")
        for name in rounds["parent commit"][0]:
            for key in rounds["parent commit"][0][name]:
                mine = [rd[name][key] for rd in rounds["this tree, whole-batch legs only"]]
                theirs = [rd[name][key] for rd in rounds["parent commit"]]
                mid = statistics.median(mine)
                print("  %s, %s: this %.3f .. %.3f (median %.3f), parent %.3f .. %.3f (median %.3f): %s; slowest round %+.2f %%"
                      % (name, key.strip(), min(mine), max(mine), mid, min(theirs), max(theirs), statistics.median(theirs),
                         "inside" if min(theirs) <= mid <= max(theirs) else "below" if mid < min(theirs) else "ABOVE",
                         100.0 * (max(mine) / max(theirs) - 1.0)))


if __name__ == "__main__":
    main()
