"""Time of BatchOSQP.verify at B = 1024 on the three batch engines, against what it replaces:
  tiled      config 4's shape (osqp_amd.problems.mpc_batch: n = 120, m = 240)
  streamed   n = 300, m = 600 (the problem of tools/batch_common_time.py)
  common     the same problem on the common-K engine
Per shape, after a solve, on the point the handle holds:
  verify            the host form: the records [B, 16] arrive on the host
  verify_into       the device form: the records stay on the device
  results + numpy   what a caller did before: results() copies X, Y and the certificates to the host, then obj, pri_res,
                    dua_res, the five norms, the two tolerances and the optimal verdict in numpy (scipy sparse products;
                    the certificate tests, comp and the gap are left out, which favours this side)
  cold solve        setup, then the first solve, timed alone -- on this tree and, with --parent-tree, on a built checkout
                    of the parent commit: verify adds a kernel to the library and must leave the solve where it was.
Every timed call returns with the handle's stream synchronised (host clock around it), as tools/batch_members_time.py
times its calls.  Two legs, one process each, alternating repetition by repetition on the same device; a process runs
one untimed round per call (code objects, staging buffers), then --rounds timed ones.  Reported: the range over all timed
rounds of all repetitions of a leg, and their median.
usage: python tools/batch_verify_time.py [--parent-tree DIR] [--reps 3] [--rounds 5] [--out FILE]
       python tools/batch_verify_time.py --rehearse        (no GPU: builds the problems, runs the numpy side, prints the plan)"""
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
B = 1024
SHAPES = ("tiled", "streamed", "common")
CALLS = ("verify", "verify_into", "results + numpy", "cold solve")


def shape(name):
    """engine, P, A, Q, L, U"""
    if name == "tiled":
        from osqp_amd.problems import mpc_batch
        s, Q, L, U = mpc_batch(B)
        return "auto", s["P"], s["A"], Q, L, U
    sys.path.insert(0, ROOT)
    from tools.batch_common_time import problem
    return ("streamed" if name == "streamed" else "common",) + tuple(problem(300, 600, B, seed=300))


def in_numpy(P, A, Q, L, U, X, Y, eps_abs=1e-3, eps_rel=1e-3):
    """Slots 0-9 and 13 of the record for every member, as a caller writes them on the host."""
    Pf = sparse.csr_matrix(sparse.triu(P) + sparse.triu(P, 1).T)
    A = sparse.csr_matrix(A)
    AX, PX, ATY = (A @ X.T).T, (Pf @ X.T).T, (A.T @ Y.T).T
    Z = np.minimum(np.maximum(AX, L), U)
    inf = lambda M: np.abs(M).max(axis=1) if M.shape[1] else np.zeros(M.shape[0])
    obj = 0.5 * np.einsum("bj,bj->b", X, PX) + np.einsum("bj,bj->b", Q, X)
    pri, dua = inf(AX - Z), inf(PX + Q + ATY)
    eps_pri = eps_abs + eps_rel * np.maximum(inf(AX), inf(Z))
    eps_dua = eps_abs + eps_rel * np.maximum(np.maximum(inf(PX), inf(ATY)), inf(Q))
    return obj, pri, dua, eps_pri, eps_dua, (pri < eps_pri) & (dua < eps_dua)


class DeviceBuffer:
    """[rows, cols] float64 of HBM with `__cuda_array_interface__`."""

    def __init__(self, rows, cols):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), rows * cols * 8) == 0
        self.ptr = p.value
        self.__cuda_array_interface__ = dict(shape=(rows, cols), typestr="<f8", data=(self.ptr, False), version=2, strides=None)

    def free(self):
        self.hip.hipFree(self.ptr)


def timed(out, name, call):
    t0 = time.perf_counter()
    r = call()
    out.setdefault(name, []).append(time.perf_counter() - t0)
    return r


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    res = {}
    for name in SHAPES:
        engine, P, A, Q, L, U = shape(name)
        t = {}
        h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)
        timed(t, "cold solve", lambda: h.solve(fetch=False))
        if a.leg == "this":
            V = DeviceBuffer(B, 16)
            Lc, Uc = np.maximum(L, -1e30), np.minimum(U, 1e30)
            def before():
                rr = h.results()
                return in_numpy(P, A, Q, Lc, Uc, rr.x, rr.y)
            # The numpy side has a loop of its own, after the two forms: a device call that follows its multi-threaded
            # host work was measured 10 - 30 ms late (in steps of about 11 ms, whichever call it was), which is the host's
            # scheduling and not the call.
            for r in range(a.rounds + 1):
                keep = t if r else {}                      # round 0 warms up
                v = timed(keep, "verify", lambda: h.verify())
                timed(keep, "verify_into", lambda: h.verify_into(V))
            for r in range(a.rounds + 1):
                o = timed(t if r else {}, "results + numpy", before)
            ok = v.V[:, 0] != float(0x7FC00000)            # (OSQP_NAN: a member without a solution)
            t["agree"] = [float(np.abs(v.obj - o[0])[ok].max()), float(np.abs(v.pri_res - o[1])[ok].max()),
                          float(np.abs(v.dua_res - o[2])[ok].max()), int(np.sum(v.optimal != o[5]))]
            V.free()
        h.cleanup()
        res[name] = t
    print(repr(res))


def fmt(v):
    return "%9.3f .. %9.3f ms (median %.3f)" % (1e3 * min(v), 1e3 * max(v), 1e3 * float(np.median(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the parent's cold solve)")
    ap.add_argument("--out", help="write the table here too")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--leg", choices=("this", "parent"))
    ap.add_argument("--tree")
    a = ap.parse_args()
    if a.rehearse:
        sys.path.insert(0, ROOT)
        for name in SHAPES:
            engine, P, A, Q, L, U = shape(name)
            rng = np.random.default_rng(1)
            t0 = time.perf_counter()
            o = in_numpy(P, A, Q, np.maximum(L, -1e30), np.minimum(U, 1e30), rng.standard_normal(Q.shape), rng.standard_normal(L.shape))
            print(name, engine, P.shape, A.shape, Q.shape, "numpy side alone: %.1f ms, %d optimal" % (1e3 * (time.perf_counter() - t0), o[5].sum()))
        print("calls", CALLS)
        return
    if a.leg:
        return leg(a)
    legs = [("this", None)] + ([("parent", a.parent_tree)] if a.parent_tree else [])
    runs = {name: [] for name, _ in legs}
    for rep in range(a.reps):
        for name, tree in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--rounds", str(a.rounds)] + (["--tree", tree] if tree else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode:
                sys.exit("leg %s failed (%d):\n%s" % (name, p.returncode, p.stderr[-2000:]))
            runs[name].append(ast.literal_eval(p.stdout.strip().splitlines()[-1]))
            print("repetition %d, leg %s: %s" % (rep, name, {k: ["%.3f" % (1e3 * x) for x in v.get("verify", [])]
                                                          for k, v in runs[name][-1].items()}), file=sys.stderr, flush=True)
    lines = ["BatchOSQP.verify at B = %d after a solve, on the point the handle holds; %d repetitions x %d rounds" % (B, a.reps, a.rounds),
             "(range over all timed rounds; every call ends in a stream synchronise; cold solve: one per repetition)", ""]
    for s in SHAPES:
        lines.append({"tiled": "tiled engine, config 4 (n = 120, m = 240)", "streamed": "streamed engine, n = 300, m = 600",
                      "common": "common-K engine, n = 300, m = 600"}[s])
        for call in CALLS[:3]:
            lines.append("  this    %-16s %s" % (call, fmt([x for r in runs["this"] for x in r[s][call]])))
        for name, _ in legs:
            lines.append("  %-7s %-16s %s" % (name, "cold solve", fmt([x for r in runs[name] for x in r[s]["cold solve"]])))
        g = runs["this"][-1][s]["agree"]
        lines.append("  verify against the numpy side, members with a solution: max |obj| diff %.3g, |pri_res| %.3g, |dua_res| %.3g, "
                     "%d optimal verdicts differ" % tuple(g))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
