"""Time of OSQP.verify at the shapes of the benchmark's configs 2, 3 and 5, against what it replaces:
  config 2   osqp_amd.problems.random_sparse_qp(10000, 20000)
  config 3   lasso_qp(): 7.5 M non-zeros, dense columns (the solve is capped at 200 iterations, as bench.py caps it)
  config 5   portfolio_qp(): 400 dense blocks of P and a 50 000-entry row of A
Per shape, after a solve, on the point the handle holds:
  verify, first call    builds the device side: the three patterns, the copies of the raw values
  verify, repeat call   one copy of the point in, four launches, 16 doubles out
  numpy                 what a caller did before: slots 0-9 and 13 from r.x, r.y with scipy sparse products on the host (the
                        certificate tests, comp and the gap are left out, which favours this side)
  residual pass         for orientation, no bar: one hipeng_residuals + hipeng_certificates on the same handle -- the same
                        products on the scaled data, as the solve's own check makes them
  cold solve            the first solve after setup, timed alone -- on this tree and, with --parent-tree, on a built checkout
                        of the parent commit in alternation: verify adds kernels to the library and must leave the solve where
                        it was.
Every timed call returns with the engine's stream synchronised (host clock around it).  One process per leg and repetition;
reported: the range over all timed rounds of all repetitions of a leg, and their median.
usage: python tools/verify_time.py [--parent-tree DIR] [--reps 2] [--rounds 5] [--configs 2,3,5] [--out FILE]"""
import argparse
import ast
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("verify, first call", "verify, repeat call", "numpy", "residual pass", "cold solve")
TITLE = {"2": "config 2: random sparse QP", "3": "config 3: Lasso", "5": "config 5: portfolio"}


def problem(cfg):
    from osqp_amd.problems import lasso_qp, portfolio_qp, random_sparse_qp
    full = {"2": lambda: random_sparse_qp(10000, 20000, seed=1), "3": lasso_qp, "5": portfolio_qp}[cfg]()
    return {k: v for k, v in full.items() if k in "PqAlu"}, (dict(max_iter=200) if cfg == "3" else {})


def in_numpy(Pf, A, At, q, l, u, x, y, eps_abs=1e-3, eps_rel=1e-3):
    """Slots 0-9 and 13 of the record, as a caller writes them on the host."""
    ax, px, aty = A @ x, Pf @ x, At @ y
    z = np.minimum(np.maximum(ax, l), u)
    inf = lambda v: np.abs(v).max() if v.size else 0.0
    obj = 0.5 * (x @ px) + q @ x
    pri, dua = inf(ax - z), inf(px + q + aty)
    eps_pri = eps_abs + eps_rel * max(inf(ax), inf(z))
    eps_dua = eps_abs + eps_rel * max(inf(px), inf(aty), inf(q))
    return obj, pri, dua, eps_pri, eps_dua, pri < eps_pri and dua < eps_dua


def timed(out, name, call):
    t0 = time.perf_counter()
    r = call()
    out.setdefault(name, []).append(time.perf_counter() - t0)
    return r


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    res = {}
    for cfg in a.configs.split(","):
        pb, kw = problem(cfg)
        t = {}

        h = osqp_amd.OSQP().setup(**pb, **kw)
        r = timed(t, "cold solve", h.solve)
        t["shape"] = [int(h.n), int(h.m), int(h.nnzP), int(h.nnzA), str(r.info.status), int(r.info.iter)]
        if a.leg == "this":
            v = timed(t, "verify, first call", h.verify)
            for _ in range(a.rounds):
                v = timed(t, "verify, repeat call", h.verify)
            Pf = sparse.csr_matrix(sparse.triu(pb["P"]) + sparse.triu(pb["P"], 1).T)
            A, At = sparse.csr_matrix(pb["A"]), sparse.csr_matrix(pb["A"].T)
            l, u = np.maximum(pb["l"], -1e30), np.minimum(pb["u"], 1e30)
            for k in range(a.rounds + 1):
                o = timed(t if k else {}, "numpy", lambda: in_numpy(Pf, A, At, pb["q"], l, u, r.x, r.y))
            t["agree"] = [float(abs(v.obj - o[0])), float(abs(v.pri_res - o[1])), float(abs(v.dua_res - o[2])), int(v.optimal != o[5]), int(v.optimal)]
            sys.path.insert(0, ROOT)
            from tests import _hipeng as HE
            L, sc = HE._lib(), HE.HipengScalars()

            def residual_pass():
                assert L.hipeng_residuals(h.engine(), C.byref(sc)) == 0
                assert L.hipeng_certificates(h.engine(), 1e-4 * sc.dx_norm_u, 1, C.byref(sc)) == 0
            for k in range(a.rounds + 1):
                timed(t if k else {}, "residual pass", residual_pass)
        h.cleanup()
        res[cfg] = t
    print(repr(res))


def fmt(v):
    return "%10.3f .. %10.3f ms (median %.3f)" % (1e3 * min(v), 1e3 * max(v), 1e3 * float(np.median(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the parent's cold solve)")
    ap.add_argument("--out", help="write the table here too")
    ap.add_argument("--leg", choices=("this", "parent"))
    ap.add_argument("--tree")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    legs = [("this", None)] + ([("parent", a.parent_tree)] if a.parent_tree else [])
    runs = {name: [] for name, _ in legs}
    for rep in range(a.reps):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--rounds", str(a.rounds), "--configs", a.configs] + (["--tree", tree] if tree else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
            if p.returncode:
                sys.exit("leg %s failed (%d):\n%s" % (name, p.returncode, p.stderr[-2000:]))
            runs[name].append(ast.literal_eval(p.stdout.strip().splitlines()[-1]))
            print("repetition %d, leg %s done" % (rep, name), file=sys.stderr, flush=True)
    lines = ["OSQP.verify after a solve, on the point the handle holds; %d repetitions (one process each) x %d rounds" % (a.reps, a.rounds),
             "(range over all timed rounds; every call ends in a stream synchronise; first call and cold solve: one per repetition)", ""]
    for cfg in a.configs.split(","):
        s = runs["this"][-1][cfg]["shape"]
        lines.append("%s (n = %d, m = %d, nnz triu(P) = %d, nnz A = %d; the solve ends `%s` after %d iterations)" % ((TITLE[cfg],) + tuple(s)))
        for call in CALLS[:4]:
            lines.append("  this    %-20s %s" % (call, fmt([x for r in runs["this"] for x in r[cfg][call]])))
        for name, _ in legs:
            lines.append("  %-7s %-20s %s" % (name, "cold solve", fmt([x for r in runs[name] for x in r[cfg]["cold solve"]])))
        g = runs["this"][-1][cfg]["agree"]
        lines.append("  verify against the numpy side: |obj| diff %.3g, |pri_res| %.3g, |dua_res| %.3g, optimal verdicts differ: %d (optimal: %d)" % tuple(g))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
