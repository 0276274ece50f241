"""Time of the batch solve with and without the per-call limits (BatchOSQP.solve(max_iter=, time_limit=)): config 4
(1024 x n = 120, m = 240, tiled engine) and the streamed and common-K engines at n = 300, m = 600, B = 1024.  Two legs, one
process each, one after the other on the same device:
  parent   --parent-tree DIR, a built checkout of the parent commit: the plain solve(), cold (warm_start = 0: zero
           iterates in every solve) and warm (from the last iterates), --rounds solves each after one warm-up solve;
  this     this tree: the same plain solves, then on the cold handle a solve with time_limit = 1e3 (the CLOCK
           instantiations, a clock that cannot bind) over the same rounds, and solves with a time limit of 1/2 and of
           1/4 of its `elapsed`: what solve_report() says of them and the overshoot, elapsed - limit.
A plain solve runs the instantiations the parent runs, with the same resource counts
(profiles/batch_limits_resources.txt), so this tree's median has to lie inside the parent's own min-max range: the
tool prints that verdict per line.  The clocked figures are reported, not judged.
usage: python tools/batch_limits_time.py [--parent-tree DIR] [--rounds 15] [--B 1024]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shapes(B):
    from osqp_amd.problems import mpc_batch
    from tools.batch_common_time import problem as common_problem
    from tools.batch_streamed_time import problem as streamed_problem
    s, Q, L, U = mpc_batch(batch=B)
    return [("tiled, config 4 (n=120, m=240)", "auto", (s["P"], s["A"], Q, L, U)),
            ("streamed (n=300, m=600)", "streamed", tuple(streamed_problem(300, 600, B, seed=300))[:5]),
            ("common-K (n=300, m=600)", "common", tuple(common_problem(300, 600, B, seed=300))[:5])]


def timed(call):
    t0 = time.perf_counter()
    call()                                # returns with the handle's stream synchronised
    return time.perf_counter() - t0


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    out = {}
    for name, engine, pb in shapes(a.B):
        res = out[name] = {}
        hs = {w: osqp_amd.BatchOSQP().setup(*pb, engine=engine, warm_start=int(w == "warm")) for w in ("cold", "warm")}
        for w, h in hs.items():
            h.solve(fetch=False)          # warm-up: code objects, LDS limits
            res["plain " + w] = [timed(lambda: h.solve(fetch=False)) for _ in range(a.rounds)]
        if a.leg == "this":
            h = hs["cold"]
            h.solve(fetch=False, time_limit=1e3)
            res["clocked cold, time_limit=1e3"] = [timed(lambda: h.solve(fetch=False, time_limit=1e3)) for _ in range(a.rounds)]
            full = h.solve_report().elapsed
            res["elapsed of it"] = full
            for frac in (0.5, 0.25):
                rows = []
                for _ in range(a.rounds):
                    r = h.solve(time_limit=frac * full)
                    rep = h.solve_report()
                    rows.append(dict(limit=rep.time_limit, elapsed=rep.elapsed, cut=rep.cut, iter_max=int(r.iter.max()),
                                     cut_status=int((r.status_val == -6).sum())))
                res["time_limit = %g x elapsed" % frac] = rows
        for h in hs.values():
            h.cleanup()
    print("JSON " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the parent leg and the verdict)")
    ap.add_argument("--leg", choices=["this", "parent"], help="run one leg in this process (what the tool starts itself)")
    ap.add_argument("--tree", help="with --leg parent: the tree to import from")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    base = [sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--B", str(a.B)]
    runs = ([("parent", ["--leg", "parent", "--tree", a.parent_tree])] if a.parent_tree else []) + [("this", ["--leg", "this"])]
    got = {}
    for title, args in runs:
        p = subprocess.run(base + args, check=True, timeout=900, stdout=subprocess.PIPE, text=True)
        got[title] = json.loads([l for l in p.stdout.splitlines() if l.startswith("JSON ")][-1][5:])
    ms = lambda v: "median %9.3f ms (min %.3f, max %.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
    print("B=%d, %d rounds after one warm-up solve; wall time of solve(fetch=False)" % (a.B, a.rounds))
    for name, res in got["this"].items():
        print(name + ":")
        for w in ("plain cold", "plain warm"):
            if "parent" in got:
                pv = got["parent"][name][w]
                med = statistics.median(res[w])
                print("  %-30s parent %s" % (w, ms(pv)))
                print("  %-30s this   %s  -> median %s the parent's range"
                      % ("", ms(res[w]), "inside" if min(pv) <= med <= max(pv) else "OUTSIDE"))
            else:
                print("  %-30s this   %s" % (w, ms(res[w])))
        c = res["clocked cold, time_limit=1e3"]
        print("  %-30s this   %s  = %.3f x plain cold" % ("clocked cold, time_limit=1e3", ms(c),
                                                        statistics.median(c) / statistics.median(res["plain cold"])))
        print("  elapsed (device stamps) of a clocked cold solve: %.3f ms" % (1e3 * res["elapsed of it"]))
        for frac in (0.5, 0.25):
            rows = res["time_limit = %g x elapsed" % frac]
            over = [r["elapsed"] - r["limit"] for r in rows]
            print("  time_limit = %.3f ms (%g x): elapsed median %.3f ms; overshoot median %.3f ms (min %.3f, max %.3f); "
                  "cut %d..%d of %d members (status -6: %d..%d); largest iter %d..%d"
                  % (1e3 * rows[0]["limit"], frac, 1e3 * statistics.median(r["elapsed"] for r in rows),
                     1e3 * statistics.median(over), 1e3 * min(over), 1e3 * max(over),
                     min(r["cut"] for r in rows), max(r["cut"] for r in rows), a.B,
                     min(r["cut_status"] for r in rows), max(r["cut_status"] for r in rows),
                     min(r["iter_max"] for r in rows), max(r["iter_max"] for r in rows)))


if __name__ == "__main__":
    main()
