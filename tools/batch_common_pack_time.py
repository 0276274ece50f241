"""Time and identity of the common-K engine's packed solve: the problems of tools/batch_common_time.py (B = 1024, m = 2n
capped by the LDS limit, n = 300, 600, 1000, default settings), a cold solve per repetition.  Three legs, one process
each, alternating repetition by repetition on the same device:
  pack on     this tree as it is;
  pack off    this tree under OSQP_AMD_BATCH_COMMON_PACK=0;
  parent      --parent-tree DIR, a built checkout of the parent commit.
Every leg is started --reps times per size (a fresh process, one warm-up solve, then --solves timed cold solves that end
in the stream synchronise of osqp_amd_batch_solve; zero iterates, the rho the handle's previous solve adapted); the range
over all timed solves of a leg is reported, with columns() and the iteration histogram of a process's last solve.  The legs also write x, y and info_raw of the last solve to --out-dir; the parent's and this
tree's are compared bit for bit (the full-solve identity).  A last leg times solve(members=first 64) of the B = 1024
handle against its full solve; the launches of both loops are computed from the iteration count (`loop_launches`).
usage: python tools/batch_common_pack_time.py [--parent-tree DIR] [--n 300,600,1000] [--reps 5] [--solves 3] [--out-dir D]"""
import argparse
import ast
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shape(n):
    NP = (n + 31) // 32 * 32
    return NP, min(2 * n, (160 * 1024 - 8 * (7 * NP + 320)) // 92)


def loop_launches(iters, rounds, packs, n):
    """Launches of bc_solve's loop for a solve of `iters` iterations: k_bc_rhs, k_bc_gemm, k_bc_step per iteration, with
    the refinement on (rounds[1] > 0) k_bc_rows, k_bc_resid and the second k_bc_gemm too; k_bc_check at every 25th
    iteration (the default check_termination; the adaptation points coincide with them: interval 100); n pivot launches,
    k_bc_mark, k_bs_form, k_bc_adopt and k_bc_load_w per inversion; one k_bc_pack per pack.  (The probes of the first
    four iterations after an inversion are left out.)"""
    return iters * (6 if rounds[1] else 3) + iters // 25 + (rounds[0] - 1) * (n + 4) + packs


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    sys.path.insert(0, ROOT)
    from tools.batch_common_time import problem
    n = int(a.n)
    NP, m = shape(n)
    P, A, Q, L, U = problem(n, m, a.B, seed=n)
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", warm_start=0)
    h.solve(fetch=False)                                   # warm-up: code objects, LDS limits
    times = []
    for _ in range(a.solves):
        t0 = time.perf_counter()
        h.solve(fetch=False)                               # returns with the handle's stream synchronised
        times.append(time.perf_counter() - t0)
    r = h.results()
    cols = tuple(h.columns()) if hasattr(h, "columns") else None
    rounds = h.rounds()
    sub = None
    if a.leg == "subset":
        S = np.arange(64)
        sub = []
        for _ in range(a.solves):
            t0 = time.perf_counter()
            h.solve(fetch=False, members=S)
            sub.append(time.perf_counter() - t0)
        rs = h.results()
        sub = (sub, int(rs.iter[S].max()), tuple(h.columns()), h.rounds())
    np.savez(os.path.join(a.out_dir, "%s_n%d.npz" % (a.leg, n)), x=r.x, y=r.y, info=r.info_raw)
    hist = dict(zip(*(v.tolist() for v in np.unique(r.iter, return_counts=True))))
    print(repr(dict(leg=a.leg, n=n, m=m, times=times, cols=cols, hist=hist, rounds=rounds, sub=sub)))
    h.cleanup()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="300,600,1000")
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the parent leg and the identity)")
    ap.add_argument("--out-dir", default="/tmp")
    ap.add_argument("--leg", choices=["on", "off", "parent", "subset"], help="run one leg in this process (what the tool starts itself)")
    ap.add_argument("--tree", help="with --leg parent: the tree to import from")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    os.makedirs(a.out_dir, exist_ok=True)
    legs = [("on", [], {}), ("off", [], {"OSQP_AMD_BATCH_COMMON_PACK": "0"})]
    if a.parent_tree:
        legs.append(("parent", ["--tree", a.parent_tree], {}))

    def run(name, n, extra, env):
        e = dict(os.environ)
        e.pop("OSQP_AMD_BATCH_COMMON_PACK", None)
        e.update(env)
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--n", str(n), "--B", str(a.B), "--solves", str(a.solves),
               "--out-dir", a.out_dir] + extra
        out = subprocess.run(cmd, env=e, check=True, timeout=600, capture_output=True, text=True).stdout
        return ast.literal_eval(out.strip().splitlines()[-1])

    for n in (int(v) for v in a.n.split(",")):
        res = {name: [] for name, _, _ in legs}
        for _ in range(a.reps):
            for name, extra, env in legs:                  # alternating: every leg sees the same drift of the host
                res[name].append(run(name, n, extra, env))
        first = res["on"][0]
        print("n=%d m=%d B=%d: %d processes x %d cold solves per leg; iterations %s; rounds %s"
              % (n, first["m"], a.B, a.reps, a.solves, first["hist"], first["rounds"]))
        for name, _, _ in legs:
            t = 1e3 * np.array([v for d in res[name] for v in d["times"]])
            print("  %-7s cold solve %8.2f .. %8.2f ms (median %8.2f) | columns (started, packs, ended) %s | iterations %s"
                  % (name, t.min(), t.max(), np.median(t), res[name][0]["cols"], "same" if res[name][0]["hist"] == first["hist"] else res[name][0]["hist"]))
        for other in [k for k in ("off", "parent") if k in res]:
            za, zb = (np.load(os.path.join(a.out_dir, "%s_n%d.npz" % (k, n))) for k in ("on", other))
            same = all(np.array_equal(za[k].view(np.int64), zb[k].view(np.int64)) for k in ("x", "y", "info"))
            print("  identity: pack on against %-6s x, y, info_raw of %d members bit-equal: %s" % (other, a.B, same))
        s = run("subset", n, [], {})
        sub, it_s, cols_s, rounds_s = s["sub"]
        full = 1e3 * np.array(s["times"]); part = 1e3 * np.array(sub)
        print("  subset  solve(members=first 64) %8.2f .. %8.2f ms against the full solve %8.2f .. %8.2f ms in the same process; "
              "iterations %d against %d; columns %s against %s; inversions %d against %d; launches of the loop %d against %d"
              % (part.min(), part.max(), full.min(), full.max(), it_s, max(s["hist"]), cols_s, s["cols"], rounds_s[0] - 1,
                 s["rounds"][0] - 1, loop_launches(it_s, rounds_s, cols_s[1], n), loop_launches(max(s["hist"]), s["rounds"], s["cols"][1], n)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
