"""Polish of the single-QP engine, bit for bit, between two builds of the library (the refactoring of run_polish into the
helpers it shares with osqp_amd_adjoint / osqp_amd_tangent must not move a bit): every member of the planted cases
(tests/_planted_qp.py: one, pad, pad_exact, scan, lp, rows, lds64k) and the random sparse QP n = 200, m = 400 solved
with polish = 1 on the default linear solver and on the PCG paths; polished x, y, obj_val, status_polish, iter, pri_res
and dua_res are recorded.
  python tools/single_sens_identity.py --lib PATH/libosqp_amd.so --dump a.npz     (one process per library)
  python tools/single_sens_identity.py --compare a.npz b.npz"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CASES = ("one", "pad", "pad_exact", "scan", "lp", "rows", "lds64k")


def dump(lib_path, out):
    import _planted_qp as pq
    from _single_sens_reference import member_qp
    from osqp_amd.interface import SolverHandle
    from osqp_amd.problems import random_sparse_qp
    lib = C.CDLL(os.path.abspath(lib_path))
    problems = [("%s[%d]" % (name, b), member_qp(pq.case(name), b)) for name in CASES for b in range(pq.case(name).B)]
    problems.append(("random200", random_sparse_qp(200, 400, seed=3)))
    rec = {}
    for path in ("default", "pcg"):
        if path == "pcg":
            os.environ["OSQP_AMD_DENSE_SMALL"] = "0"
        for tag, pb in problems:
            h = SolverHandle(lib).setup(**pb, polish=1)
            r = h.solve()
            h.cleanup()
            key = "%s %s" % (path, tag)
            rec[key + " x"], rec[key + " y"] = r.x, r.y
            rec[key + " info"] = np.array([r.info.obj_val, r.info.pri_res, r.info.dua_res, r.info.status_polish, r.info.iter, r.info.status_val])
    np.savez(out, **rec)
    print("wrote %d arrays of %d solves to %s" % (len(rec), len(rec) // 3, out))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files)
    diff = [k for k in A.files if not np.array_equal(A[k], B[k], equal_nan=True)]
    solves = sorted({k.rsplit(" ", 1)[0] for k in A.files})
    accepted = sum(1 for s in solves if A[s + " info"][3] == 1)
    print("%d solves (%d with status_polish 1), %d arrays: %d differ" % (len(solves), accepted, len(A.files), len(diff)))
    for k in diff:
        print("   ", k, float(np.abs(A[k] - B[k]).max()))
    print("bit-identical" if not diff else "NOT identical")
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else dump(a.lib, a.dump))
