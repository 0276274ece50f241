"""Time of D cotangents per adjoint call and of the KKT inversion kept per solve, on a solved and polished batch: config 4
(1024 x n = 120, m = 240, tiled engine) and the streamed engine at n = 300, m = 600, B = 1024.  Three legs, one process
each, one after the other on the same device:
  sharing on    this tree as it is.  Per repetition: a cold solve and a polish, then adjoint() (it builds the inversion),
                tangent() (it finds it), then adjoint with [B, D, .] cotangents, D = 1, 4, 16, without and with the matrix
                gradients (all on the kept inversion);
  sharing off   this tree under OSQP_AMD_BATCH_KKT_CACHE=0: the same calls, each of which forms and inverts again;
  parent        --parent-tree DIR, a built checkout of the parent commit: adjoint(), tangent(), and D separate adjoint()
                calls for D = 1, 4, 16, without and with the matrix gradients -- what a caller had to do before.
Host arrays in and out: the copies are part of every call.  Medians over --reps after --warmup untimed repetitions.
usage: python tools/batch_adjoint_multi_time.py [--parent-tree DIR] [--reps 3] [--warmup 1] [--B 1024]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = (1, 4, 16)


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    from osqp_amd.problems import mpc_batch
    from tools.batch_streamed_time import problem
    multi = a.leg != "parent"
    s, Q, L, U = mpc_batch(batch=a.B)
    legs = [("tiled, config 4 (n=120, m=240)", "auto", s["P"], s["A"], Q, L, U),
            ("streamed (n=300, m=600)", "streamed") + tuple(problem(300, 600, a.B, seed=300))]
    rng = np.random.default_rng(0)
    for name, engine, P, A, Q, L, U in legs:
        h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, warm_start=0)
        B, n, m = h.B, h.n, h.m
        dX, dY = rng.standard_normal((B, max(DS), n)), rng.standard_normal((B, max(DS), m))
        gx = [np.ascontiguousarray(dX[:, d]) for d in range(max(DS))]
        gy = [np.ascontiguousarray(dY[:, d]) for d in range(max(DS))]
        dQ = rng.standard_normal((B, n))
        keys = ["solve", "polish", "adjoint()", "tangent() after it"]
        keys += ["%s D=%d%s" % ("adjoint [B, D, .]" if multi else "D x adjoint()", D, mat) for mat in ("", " + matrices") for D in DS]
        t = {k: [] for k in keys}
        for k in range(a.warmup + a.reps):
            c = [time.perf_counter()]
            h.solve(fetch=False); c.append(time.perf_counter())
            r = h.polish(); c.append(time.perf_counter())
            g = h.adjoint(gx[0], gy[0]); c.append(time.perf_counter())
            tg = h.tangent(dQ=dQ); c.append(time.perf_counter())
            for mat in (False, True):
                for D in DS:
                    if multi:
                        h.adjoint(np.ascontiguousarray(dX[:, :D]), np.ascontiguousarray(dY[:, :D]), matrices=mat)
                    else:
                        for d in range(D):
                            h.adjoint(gx[d], gy[d], matrices=mat)
                    c.append(time.perf_counter())
            if k >= a.warmup:
                for key, v in zip(keys, np.diff(c)):
                    t[key].append(v)
        med = {k: statistics.median(v) for k, v in t.items()}
        print("  %s, B=%d, %d repetitions after %d warm-up:" % (name, a.B, a.reps, a.warmup))
        for k, v in t.items():
            print("    %-34s: median %9.3f ms (min %.3f, max %.3f)" % (k, 1e3 * med[k], 1e3 * min(v), 1e3 * max(v)))
        st = g.status_adjoint
        line = "    solved %d, polish accepted %d; adjoint computed %d, rejected %d, skipped %d; active rows per member %.1f" \
            % (int(np.sum(r.status_val == 1)), int(np.sum(r.status_polish == 1)), int(np.sum(st == 1)), int(np.sum(st == -1)),
               int(np.sum(st == 0)), np.count_nonzero(g.active, axis=1).mean())
        if multi:
            info = h.kkt_info()
            line += "; builds per repetition %.1f, NPOL %d" % (info.builds / (a.warmup + a.reps), info.npol)
        print(line)
        first = keys[4]
        print("    %s / adjoint() = %.2f; D=16 / (16 x D=1) = %.2f; tangent() after adjoint() / adjoint() = %.2f"
              % (first, med[first] / med["adjoint()"], med[keys[6]] / (16 * med[first]), med["tangent() after it"] / med["adjoint()"]))
        assert np.array_equal(g.active, tg.active)
        sys.stdout.flush()
        h.cleanup()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the parent leg)")
    ap.add_argument("--leg", choices=["on", "off", "parent"], help="run one leg in this process (what the tool starts itself)")
    ap.add_argument("--tree", help="with --leg parent: the tree to import from")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup), "--B", str(a.B)]
    runs = [("sharing on (this tree)", ["--leg", "on"], {}),
            ("sharing off (this tree, OSQP_AMD_BATCH_KKT_CACHE=0)", ["--leg", "off"], {"OSQP_AMD_BATCH_KKT_CACHE": "0"})]
    if a.parent_tree:
        runs.append(("parent commit (D separate adjoint() calls)", ["--leg", "parent", "--tree", a.parent_tree], {}))
    for title, args, env in runs:
        print(title + ":")
        sys.stdout.flush()
        e = dict(os.environ)
        e.pop("OSQP_AMD_BATCH_KKT_CACHE", None)
        e.update(env)
        subprocess.run(base + args, env=e, check=True, timeout=600)


if __name__ == "__main__":
    main()
