"""Time of BatchOSQP.update_model (osqp_amd_batch_common_update_model) -- new values for the shared model of a live
common-K handle -- against what a user had to do before it existed: cleanup() and a new setup(..., shared_kkt=...) on the
new values.  B = 1024, m = 2n capped by the LDS limit, n = 300 / 600 / 1000, the family of tools/batch_common_time.py,
default settings; the new values alternate between two sets tens of per cent apart (the diagonal of P x 1.3 - 1.9, the
rest of P x 0.5 - 1.0, A x 0.5 - 1.8), so every call really moves the scaling.  Legs, one process each, one after the
other on the same device:
  model    this tree: per size, without and with the shared KKT pieces, update_model through host arrays and through
           CUDA tensors (torch is imported first); with the pieces, two handles side by side -- k_bc_pivot2 (K and H in one
           launch per pivot) and OSQP_AMD_BATCH_MODEL_PIVOT2=0 (two pivot sequences) -- in alternating runs; and
           cleanup() + setup() on this tree
  parent   --parent-tree DIR, a built checkout of the parent commit: cleanup() + setup(), without and with the pieces
Every call returns with the handle's stream synchronised; the host clock is read around it.  --warmup untimed calls, then
--reps timed: median (min, max).
usage: python tools/batch_common_model_time.py [--parent-tree DIR] [--n 300,600,1000] [--reps 5] [--warmup 1] [--B 1024]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def moved(P, A, seed):
    from scipy import sparse
    Pu = sparse.triu(sparse.csc_matrix(P), format="csc"); Pu.sort_indices()
    A = sparse.csc_matrix(A); A.sort_indices()
    rng = np.random.default_rng(seed)
    diag = Pu.indices == np.repeat(np.arange(Pu.shape[0]), np.diff(Pu.indptr))
    Px = Pu.data * np.where(diag, rng.uniform(1.3, 1.9, Pu.nnz), rng.uniform(0.5, 1.0, Pu.nnz))
    Ax = A.data * rng.uniform(0.5, 1.8, A.nnz)
    return Pu, A, [(Px, Ax), (Pu.data.copy(), A.data.copy())]


def with_values(M, v):
    from scipy import sparse
    return sparse.csc_matrix((v, M.indices, M.indptr), shape=M.shape)


def report(name, v):
    print("    %-46s: median %9.3f ms (min %.3f, max %.3f)" % (name, 1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)))
    sys.stdout.flush()


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def leg(a):
    model = a.leg == "model"
    if model:
        import torch                         # before the library is first loaded: one HIP runtime for both
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    sys.path.insert(1, ROOT)
    import osqp_amd
    from tools.batch_common_time import problem
    total = a.warmup + a.reps
    for n in (int(v) for v in a.n.split(",")):
        m = min(2 * n, 1129)
        P, A, Q, L, U = problem(n, m, a.B, seed=n)
        Pu, A, sets = moved(P, A, n + 1)
        print("  n=%d m=%d B=%d nnzP=%d nnzA=%d" % (n, m, a.B, Pu.nnz, A.nnz))
        for shared in (False, True):
            tag = "with the shared pieces" if shared else "without the shared pieces"
            make = lambda vals: osqp_amd.BatchOSQP().setup(with_values(Pu, vals[0]), with_values(A, vals[1]), Q, L, U, engine="common",
                                                           shared_kkt=shared, warm_start=0)
            h = make(sets[1])
            t = []
            for k in range(total):               # what a user must do without the call
                def again():
                    h.cleanup()
                    return make(sets[k % 2])
                h, dt = clock(again)
                t.append(dt)
            report("cleanup + setup, " + tag, t[a.warmup:])
            h.cleanup()
            if not model:
                continue
            handles = {"": make(sets[1])}
            if shared:
                os.environ["OSQP_AMD_BATCH_MODEL_PIVOT2"] = "0"
                handles[" (two pivot sequences)"] = make(sets[1])
                del os.environ["OSQP_AMD_BATCH_MODEL_PIVOT2"]
            dev = [tuple(torch.as_tensor(v, device="cuda") for v in s) for s in sets]
            torch.cuda.synchronize()
            for route, vals in (("host", sets), ("device", dev)):
                t = {k: [] for k in handles}
                for k in range(total):           # alternating runs of the two handles
                    for key, hh in handles.items():
                        rc, dt = clock(lambda: hh.update_model(Px=vals[k % 2][0], Ax=vals[k % 2][1]))
                        assert rc == 0, rc
                        t[key].append(dt)
                for key, v in t.items():
                    report("update_model, %s route, %s%s" % (route, tag, key), v[a.warmup:])
            r = [hh.solve() for hh in handles.values()]
            same = all(np.array_equal(r[0].x, o.x) and np.array_equal(r[0].info_raw, o.info_raw) for o in r[1:])
            print("    a solve after the calls: %d of %d solved%s" % (int(np.sum(r[0].status_val == 1)), a.B,
                                                                        ", the two handles agree to the bit: %s" % same if shared else ""))
            for hh in handles.values():
                hh.cleanup()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="300,600,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the parent leg)")
    ap.add_argument("--leg", choices=["model", "parent"], help="run one leg in this process (what the tool starts itself)")
    ap.add_argument("--tree", help="with --leg parent: the tree to import from")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup), "--B", str(a.B), "--n", a.n]
    runs = [("this tree", ["--leg", "model"])]
    if a.parent_tree:
        runs.append(("parent commit", ["--leg", "parent", "--tree", a.parent_tree]))
    for title, args in runs:
        print(title + ":")
        sys.stdout.flush()
        subprocess.run(base + args, check=True, timeout=900)


if __name__ == "__main__":
    main()
