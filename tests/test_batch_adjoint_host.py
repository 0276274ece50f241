"""Host-side contract of the adjoint call on the batch engines (no GPU needed), and the yardstick of the numpy
reference the GPU tests compare against (tests/_adjoint_reference.py): its gradients against central differences of
the CPU oracle."""
import numpy as np
import pytest
from scipy import sparse

from _adjoint_reference import adjoint_reference


def test_library_exports_adjoint():
    import osqp_amd
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    assert hasattr(lib, "osqp_amd_batch_adjoint")
    assert lib.osqp_amd_batch_adjoint.argtypes is not None and len(lib.osqp_amd_batch_adjoint.argtypes) == 10


def test_python_entry_points_exist():
    import osqp_amd
    assert callable(getattr(osqp_amd.BatchOSQP, "adjoint", None))
    assert callable(getattr(osqp_amd, "BatchQPLayer", None))
    assert "BatchQPLayer" in osqp_amd.__all__


B, N, M = 3, 5, 7
MALFORMED = [dict(dX=np.ones((B, N + 1))), dict(dX=np.ones((B + 1, N))), dict(dX=np.ones(N)), dict(dX=np.ones((B, N, 1))),
             dict(dX=np.ones((B, N)), dY=np.ones((B, M + 1))), dict(dX=np.ones((B, N)), dY=np.ones((B - 1, M))),
             dict(dX=np.ones((B, N)), dY=np.ones(M))]


@pytest.mark.parametrize("kwargs", MALFORMED, ids=[str(k) for k in range(len(MALFORMED))])
def test_shape_errors_raise(kwargs):
    from osqp_amd.batch import check_adjoint
    with pytest.raises(ValueError):
        check_adjoint(B, N, M, **kwargs)


def test_well_formed_shapes_pass():
    from osqp_amd.batch import check_adjoint
    dX, dY = check_adjoint(B, N, M, [[1.0] * N] * B)
    assert dX.shape == (B, N) and dX.dtype == np.float64 and dX.flags.c_contiguous and dY is None
    dX, dY = check_adjoint(B, N, M, np.ones((B, N), np.float32), np.ones((B, M)))
    assert dX.dtype == np.float64 and dY.shape == (B, M)


def test_null_handle_is_refused():
    import ctypes as C
    import osqp_amd
    from osqp_amd import abi
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    v = np.ones(4); k = np.zeros(4, np.int64)
    nf = C.cast(None, abi.c_float_p)
    assert lib.osqp_amd_batch_adjoint(None, abi.fptr(v), nf, abi.fptr(v), abi.fptr(v), abi.fptr(v), nf, nf,
                                      abi.iptr(k), abi.iptr(k)) == 7          # OSQP_WORKSPACE_NOT_INIT_ERROR


def _qp(seed=0):
    """n = 5, m = 7, P with a sparse upper triangle, A half full, every row two-sided.  At seed 0 the solution has
    one row active at its lower bound and three at their upper bound, a complementarity margin of 0.1 and
    sigma_min / sigma_max of the active rows = 0.29."""
    rng = np.random.default_rng(seed); n, m = 5, 7
    G = rng.standard_normal((n, n)); Pf = G @ G.T + np.eye(n); Pf[np.abs(Pf) < 0.8] = 0; Pf = (Pf + Pf.T) / 2 + 2 * np.eye(n)
    P = sparse.triu(sparse.csc_matrix(Pf), format="csc")
    A = sparse.random(m, n, density=0.5, random_state=rng, format="csc"); A.data = rng.standard_normal(A.nnz)
    x0 = rng.standard_normal(n); ax = A @ x0
    q = rng.standard_normal(n) * 3
    return P, A, q, ax - rng.uniform(0.1, 0.5, m), ax + rng.uniform(0.1, 0.5, m)


def test_reference_against_central_differences(oracle_mod):
    """The helper's five gradients of loss = gx . x + gy . y against central differences of the oracle (eps 1e-10,
    polish on), error relative to max(1, |gradient|_inf).  Measured on the CPU, worst of the five gradients:
    step 1e-4: 1.8e-8 (truncation, in dAx); step 1e-5: 2.0e-10; step 1e-6: 1.4e-9 (round-off of the polished
    solution over the step).  The bar is 10 x the best of them: 2.0e-9 at step 1e-5."""
    P, A, q, l, u = _qp()
    rng = np.random.default_rng(1000)
    gx, gy = rng.standard_normal(5), rng.standard_normal(7)

    def solve(P, A, q, l, u):
        r = oracle_mod.OracleOSQP().setup(P=P, q=q, A=A, l=l, u=u, eps_abs=1e-10, eps_rel=1e-10, polish=1, max_iter=20000).solve()
        assert r.info.status_val == 1 and r.info.status_polish == 1
        return np.array(r.x), np.array(r.y)

    def shifted(which, k, d):
        P2, A2, v = P.copy(), A.copy(), dict(q=q.copy(), l=l.copy(), u=u.copy())
        if which == "Px":
            P2.data = P.data.copy(); P2.data[k] += d
        elif which == "Ax":
            A2.data = A.data.copy(); A2.data[k] += d
        else:
            v[which][k] += d
        return P2, A2, v["q"], v["l"], v["u"]

    x, y = solve(P, A, q, l, u)
    ref = adjoint_reference(P, A, l, u, x, y, gx, gy)
    assert sorted(ref.active) == [-1, 0, 0, 0, 1, 1, 1] and ref.margin > 1e-2 and ref.sv_ratio > 0.1 and ref.route_err < 1e-12
    want = dict(q=ref.dq, l=ref.dl, u=ref.du, Px=ref.dPx, Ax=ref.dAx)
    worst = {}
    for h in (1e-4, 1e-5, 1e-6):
        errs = []
        for which, g in want.items():
            fd = np.zeros(g.size)
            for k in range(g.size):
                xp, yp = solve(*shifted(which, k, h)); xm, ym = solve(*shifted(which, k, -h))
                fd[k] = ((gx @ xp + gy @ yp) - (gx @ xm + gy @ ym)) / (2 * h)
            errs.append(np.abs(fd - g).max() / max(1.0, np.abs(g).max()))
        worst[h] = max(errs)
        print("step %g:" % h, " ".join("d%s %.2e" % (w, e) for w, e in zip(want, errs)))
    assert worst[1e-5] < 2.0e-9, worst
