"""The two collectives that the infeasibility tests of the row-partitioned solve add to a termination check, through the built-in RCCL
provider (osqp_amd_rp_use_rccl, stream-ordered ncclAllReduce) on a one-rank communicator, in a process WITHOUT torch like
tools/rccl_world1_probe.py.  A primal-infeasible and a feasible problem, each with the callback-free one-rank loop and with RCCL: status,
iteration count, solution and certificates must agree bit for bit, and RCCL must have carried more collectives than the same iterations
with the tests off, at most two per check more (exactly that on the feasible problem; the infeasible solve leaves the loop at its last
check, before the rho update that the run with the tests off still makes at that iteration).   usage: python tools/rccl_world1_infeasible_probe.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy import sparse
from osqp_amd import rowpart
assert "torch" not in sys.modules
rng = np.random.RandomState(7)
n, m = 20, 30
A = sparse.lil_matrix((m, n))
for i in range(m):
    A[i, i % n] = 1.0
    A[i, (3 * i + 1) % n] = 0.5
A[0, :] = 0; A[1, :] = 0; A[0, 0] = 1.0; A[1, 0] = 1.0
P = sparse.csc_matrix(sparse.diags(1.0 + rng.rand(n)))
l, u = -np.ones(m), np.ones(m)
ok = True
for label, (l0, u0, l1, u1) in (("infeasible", (1.0, 1e30, -1e30, 0.0)), ("feasible", (-1.0, 1e30, -1e30, 0.0))):       # x0 >= 1 (or >= -1) and x0 <= 0
    l[0], u[0], l[1], u[1] = l0, u0, l1, u1
    scaled = dict(P=sparse.triu(P, format="csc"), q=rng.randn(n), A=sparse.csc_matrix(A), l=l.copy(), u=u.copy(), D=np.ones(n), E=np.ones(m), c=1.0)
    kw = dict(eps_abs=1e-5, eps_rel=1e-5, eps_prim_inf=1e-4, eps_dual_inf=1e-4)
    a = rowpart.NativeRowPartitionedOSQP(world=1).setup(scaled, device=0, **kw)
    ra = a.solve()
    b = rowpart.NativeRowPartitionedOSQP(world=1).setup(scaled, device=0, **kw)
    rc = b.use_rccl_world1()
    print("use_rccl ->", rc, flush=True)
    rb = b.solve()
    c = rowpart.NativeRowPartitionedOSQP(world=1).setup(scaled, device=0, **{k: v for k, v in kw.items() if "inf" not in k}, max_iter=rb.info.iter)
    rc2 = c.use_rccl_world1()
    ro = c.solve()
    checks = -(-rb.info.iter // 25)
    print("%s plain: %s iter %d collectives %d" % (label, ra.info.status, ra.info.iter, ra.info.collectives))
    print("%s rccl : %s iter %d collectives %d (tests off, same iterations: %d; %d checks)" % (label, rb.info.status, rb.info.iter, rb.info.collectives, ro.info.collectives, checks))
    same = all(np.array_equal(getattr(ra, k), getattr(rb, k), equal_nan=True) for k in ("x", "y", "prim_inf_cert", "dual_inf_cert"))
    same = same and (ra.info.status, ra.info.iter, ra.info.obj_val) == (rb.info.status, rb.info.iter, rb.info.obj_val)
    print("%s identical:" % label, same, "torch loaded:", "torch" in sys.modules)
    ok = ok and rc == 0 and rc2 == 0 and same and ra.info.status == ("primal infeasible" if label == "infeasible" else "solved")
    ok = ok and ro.info.collectives < rb.info.collectives <= ro.info.collectives + 2 * checks and ro.info.iter == rb.info.iter
    ok = ok and (label == "infeasible" or rb.info.collectives == ro.info.collectives + 2 * checks)
    for h in (a, b, c):
        h.cleanup()
print("probe ok:", ok)
sys.exit(0 if ok else 1)
