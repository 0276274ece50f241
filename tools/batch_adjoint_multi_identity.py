"""adjoint() and tangent() of the batch engines, bit for bit, between two builds (the kept KKT inversion and the shared
runner around the three derivative kernels must not move a bit of the existing entry points): on the shapes of
tests/test_gpu_batch_adjoint.py (TILED_SHAPES on the tiled engine, STREAMED_SHAPES on the streamed one, M0_SHAPE on both),
solve -> polish -> adjoint(dX, dY, matrices=True) -> tangent(D = 1, all five tangents) -> tangent(D = 3) -> adjoint again ->
adjoint with [B, 3, .] cotangents (matrices=True) -> adjoint with its [B, 1, .] slice 1; the five gradients, dx, dy, active and
the statuses are recorded.
  python tools/batch_adjoint_multi_identity.py --tree DIR --dump a.npz     (one process per built tree; DIR defaults to this one)
  python tools/batch_adjoint_multi_identity.py --compare a.npz b.npz"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(tree, out):
    sys.path[:0] = [os.path.abspath(tree or ROOT), os.path.join(ROOT, "tests")]
    import osqp_amd
    from test_gpu_batch_adjoint import M0_SHAPE, STREAMED_SHAPES, TILED_SHAPES, _family, _incoming
    rec = {}
    for engine, shapes in (("auto", TILED_SHAPES + [M0_SHAPE]), ("streamed", STREAMED_SHAPES + [M0_SHAPE])):
        for shape in shapes:
            n, m, B, seed = shape
            P, A, Q, L, U, _ = _family(shape)
            h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)
            h.solve(fetch=False)
            r = h.polish()
            dX, dY = _incoming(shape)
            rng = np.random.default_rng(31 + seed)
            tan = dict(dQ=rng.standard_normal((B, 3, n)), dL=rng.standard_normal((B, 3, m)), dU=rng.standard_normal((B, 3, m)),
                       dPx=rng.standard_normal((B, 3, h.Pu.nnz)), dAx=rng.standard_normal((B, 3, h.Ah.nnz)))
            tan = {k: v for k, v in tan.items() if v.shape[2]}       # (m = 0: no row tangents, no dAx)
            a = h.adjoint(dX, dY, matrices=True)
            t1 = h.tangent(**{k: np.ascontiguousarray(v[:, 0]) for k, v in tan.items()})
            t3 = h.tangent(**tan)
            a2 = h.adjoint(dX, dY, matrices=True)
            dX3, dY3 = rng.standard_normal((B, 3, n)), rng.standard_normal((B, 3, m))
            a3 = h.adjoint(dX3, dY3, matrices=True)
            a31 = h.adjoint(np.ascontiguousarray(dX3[:, 1:2]), np.ascontiguousarray(dY3[:, 1:2]), matrices=True)
            key = "%s %s" % (engine, shape)
            rec[key + " x"], rec[key + " status_polish"] = r.x, r.status_polish
            for tag, res, names in (("adjoint", a, ("dq", "dl", "du", "dPx", "dAx", "active", "status_adjoint")),
                                    ("tangent1", t1, ("dx", "dy", "active", "status_tangent")),
                                    ("tangent3", t3, ("dx", "dy", "active", "status_tangent")),
                                    ("adjoint again", a2, ("dq", "dl", "du", "dPx", "dAx", "active", "status_adjoint")),
                                    ("adjoint3", a3, ("dq", "dl", "du", "dPx", "dAx", "active", "status_adjoint")),
                                    ("adjoint3 slice", a31, ("dq", "dl", "du", "dPx", "dAx", "active", "status_adjoint"))):
                for k in names:
                    rec["%s %s %s" % (key, tag, k)] = getattr(res, k)
            h.cleanup()
    np.savez(out, **rec)
    print("wrote %d arrays to %s" % (len(rec), out))
    return 0


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files)
    bits = lambda v: np.ascontiguousarray(v).view(np.uint64) if v.dtype == np.float64 else v
    diff = [k for k in A.files if A[k].shape != B[k].shape or not np.array_equal(bits(A[k]), bits(B[k]))]
    handles = sorted({k.split(") ")[0] + ")" for k in A.files})
    computed = sum(int(np.sum(A[k] == 1)) for k in A.files if k.endswith(" adjoint status_adjoint"))
    members = sum(A[k].size for k in A.files if k.endswith(" adjoint status_adjoint"))
    print("%d handles (engine, (n, m, B, seed)): %s" % (len(handles), "; ".join(handles)))
    print("%d members, status_adjoint 1 for %d; %d arrays compared with ==: %d differ" % (members, computed, len(A.files), len(diff)))
    for k in diff:
        print("   ", k)
    print("bit-identical" if not diff else "NOT identical")
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree")
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else dump(a.tree, a.dump))
