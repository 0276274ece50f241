"""Time of a member-subset session on the common-K engine with its shared KKT pieces: B = 1024, n = 300, m = 600 (the
problem of tools/batch_common_time.py), |S| = 1, 16, 64 members spread evenly over the batch.  Per round the members of S
get a new q, then
  this tree     update(members=S) -> solve(members=S) -> polish(members=S) -> adjoint(members=S)
  parent tree   update (whole)    -> solve(members=S) -> solve(members=rest) -> polish -> adjoint
-- the only sequence the parent commit offers: its update clears every member's solved flag, so the rest has to be
solved again before polish and adjoint are served, and both then work on all B members.  Also timed on both trees, to
show that the whole-batch calls have not moved: update (whole) and, after a whole solve, polish.
Every timed call returns with the handle's stream synchronised (host clock around it).  Two legs, one process each,
alternating repetition by repetition on the same device; a process sets the handle up, solves everybody, runs one
untimed round per |S| (code objects, staging buffers) and then --rounds timed rounds per |S|.  Reported per step: the range
over all timed rounds of all repetitions of a leg.  The S rows of x after the last round are written to --out-dir and
compared between the trees: with the default settings the batch's one adaptive rho sees other columns in the two
sequences, so the two agree to the solve's tolerance, not to the bit.
usage: python tools/batch_members_time.py [--parent-tree DIR] [--S 1,16,64] [--reps 3] [--rounds 5] [--out FILE]
       python tools/batch_members_time.py --rehearse        (no GPU: builds the problem and prints the plan)"""
import argparse
import ast
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, M = 1024, 300, 600
STEPS = dict(this=("update_members", "solve_members", "polish_members", "adjoint_members"),
             parent=("update", "solve_members", "solve_rest", "polish", "adjoint"))


def subset(k):
    return np.arange(k) * (B // k) + (B // k) // 2


def timed(out, name, call):
    t0 = time.perf_counter()
    r = call()
    out.setdefault(name, []).append(time.perf_counter() - t0)
    return r


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    sys.path.insert(0, ROOT)
    from tools.batch_common_time import problem
    P, A, Q, L, U = problem(N, M, B, seed=N)
    rng = np.random.default_rng(12)
    gx, gy = rng.standard_normal((B, N)), rng.standard_normal((B, M))
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", shared_kkt=True)
    h.solve(fetch=False)
    res = dict(leg=a.leg, S={})
    # the whole-batch calls, on either tree: update of q, and polish after a whole solve
    whole = {}
    for r in range(a.rounds + 1):
        keep = whole if r else {}
        Qr = Q * (1.0 + 0.01 * (r + 1))
        assert timed(keep, "update", lambda: h.update(Q=Qr)) == 0
        h.solve(fetch=False)
        timed(keep, "polish", lambda: h.polish(fetch=False))
    res["whole"] = whole
    cur = Q * (1.0 + 0.01 * (a.rounds + 1))
    for k in a.S:
        S = subset(k)
        rest = np.setdiff1d(np.arange(B), S)
        t = {}
        for r in range(a.rounds + 1):
            keep = t if r else {}                          # round 0 warms up
            rows = Q[S] * (1.0 + 0.02 * (r + 1) * (-1) ** r)
            if a.leg == "this":
                assert timed(keep, "update_members", lambda: h.update(Q=rows, members=S)) == 0
                timed(keep, "solve_members", lambda: h.solve(fetch=False, members=S))
                timed(keep, "polish_members", lambda: h.polish(fetch=False, members=S))
                timed(keep, "adjoint_members", lambda: h.adjoint(gx[S], gy[S], members=S))
                x = h.results(members=S).x
            else:
                cur = cur.copy(); cur[S] = rows
                full = cur
                assert timed(keep, "update", lambda: h.update(Q=full)) == 0
                timed(keep, "solve_members", lambda: h.solve(fetch=False, members=S))
                timed(keep, "solve_rest", lambda: h.solve(fetch=False, members=rest))
                timed(keep, "polish", lambda: h.polish(fetch=False))
                timed(keep, "adjoint", lambda: h.adjoint(gx, gy))
                x = h.results().x[S]
        np.save(os.path.join(a.out_dir, "members_time_%s_%d.npy" % (a.leg, k)), x)
        res["S"][k] = t
    print(repr(res))
    h.cleanup()


def fmt(v):
    return "%8.3f .. %8.3f ms" % (1e3 * min(v), 1e3 * max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", default="1,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the parent leg)")
    ap.add_argument("--out-dir", default="/tmp")
    ap.add_argument("--out", help="write the table here too")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--leg", choices=("this", "parent"))
    ap.add_argument("--tree")
    a = ap.parse_args()
    a.S = [int(v) for v in a.S.split(",")]
    if a.rehearse:
        sys.path.insert(0, ROOT)
        from tools.batch_common_time import problem
        P, A, Q, L, U = problem(N, M, B, seed=N)
        print("problem", P.shape, A.shape, Q.shape, "subsets", {k: subset(k)[[0, -1]].tolist() for k in a.S}, "steps", STEPS)
        return
    if a.leg:
        return leg(a)
    legs = [("this", None)] + ([("parent", a.parent_tree)] if a.parent_tree else [])
    runs = {name: [] for name, _ in legs}
    for rep in range(a.reps):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--S", ",".join(map(str, a.S)),
                   "--rounds", str(a.rounds), "--out-dir", a.out_dir] + (["--tree", tree] if tree else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode:
                sys.exit("leg %s failed (%d):\n%s" % (name, p.returncode, p.stderr[-2000:]))
            runs[name].append(ast.literal_eval(p.stdout.strip().splitlines()[-1]))
    lines = ["member-subset session, common-K engine with shared KKT pieces: B = %d, n = %d, m = %d; %d repetitions x %d rounds"
             % (B, N, M, a.reps, a.rounds), "(range over all timed rounds; every call ends in a stream synchronise)", ""]
    for k in a.S:
        lines.append("|S| = %d" % k)
        for name, _ in legs:
            total = None
            for step in STEPS[name]:
                v = [x for r in runs[name] for x in r["S"][k][step]]
                lines.append("  %-7s %-16s %s" % (name, step, fmt(v)))
                per = np.array([r["S"][k][step] for r in runs[name]]).ravel()
                total = per if total is None else total + per
            lines.append("  %-7s %-16s %s" % (name, "the sequence", fmt(total)))
        if len(legs) == 2:
            xa = np.load(os.path.join(a.out_dir, "members_time_this_%d.npy" % k))
            xb = np.load(os.path.join(a.out_dir, "members_time_parent_%d.npy" % k))
            lines.append("  x of S after the last round, this tree against the parent: %s (max |diff| %.3g)"
                         % ("bit-equal" if np.array_equal(xa.view(np.int64), xb.view(np.int64)) else "differs",
                            float(np.abs(xa - xb).max())))
        lines.append("")
    lines.append("whole-batch calls (all %d members)" % B)
    for name, _ in legs:
        for step in ("update", "polish"):
            v = [x for r in runs[name] for x in r["whole"][step]]
            lines.append("  %-7s %-16s %s" % (name, step, fmt(v)))
            per_run = ["%.3f" % (1e3 * np.median(r["whole"][step])) for r in runs[name]]
            lines.append("  %-7s %-16s medians of the repetitions: %s ms" % ("", "", ", ".join(per_run)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
