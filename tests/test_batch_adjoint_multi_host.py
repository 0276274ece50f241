"""Host-side contract of the multi-cotangent adjoint call and of the kept KKT inversion's read-only view on the batch
engines (no GPU needed), and the property of the numpy reference (tests/_adjoint_reference.py) that makes the
per-cotangent comparison of test_gpu_batch_adjoint_multi.py meaningful: it is linear in the cotangent."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

from _adjoint_reference import adjoint_reference
from _batch_parity import oracle, shape_family

B, N, M = 3, 5, 7


def test_library_exports_adjoint_multi_and_kkt_info():
    import osqp_amd
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    for name, nargs in (("osqp_amd_batch_adjoint_multi", 11), ("osqp_amd_batch_adjoint_multi_dev", 11),
                        ("osqp_amd_batch_kkt_info", 2)):
        f = getattr(lib, name, None)
        assert f is not None, name
        assert f.argtypes is not None and len(f.argtypes) == nargs, (name, f.argtypes)
    assert callable(getattr(osqp_amd.BatchOSQP, "kkt_info", None))


def test_null_handle_is_refused():
    import osqp_amd
    from osqp_amd import abi
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    v = np.ones(4); k = np.zeros(4, np.int64)
    nf = C.cast(None, abi.c_float_p)
    assert lib.osqp_amd_batch_adjoint_multi(None, 2, abi.fptr(v), nf, abi.fptr(v), abi.fptr(v), abi.fptr(v), nf, nf,
                                            abi.iptr(k), abi.iptr(k)) == 7     # OSQP_WORKSPACE_NOT_INIT_ERROR
    assert lib.osqp_amd_batch_adjoint_multi_dev(None, 2, *([None] * 9)) == 7
    assert lib.osqp_amd_batch_kkt_info(None, abi.iptr(k)) == 7


def test_well_formed_shapes_pass():
    from osqp_amd.batch import check_adjoint_multi
    dX, dY, D = check_adjoint_multi(B, N, M, [[[1.0] * N] * 4] * B)
    assert dX.shape == (B, 4, N) and dX.dtype == np.float64 and dX.flags.c_contiguous and dY is None and D == 4
    dX, dY, D = check_adjoint_multi(B, N, M, np.ones((B, 1, N), np.float32), np.ones((B, 1, M)))
    assert dX.dtype == np.float64 and dY.shape == (B, 1, M) and D == 1
    dX, dY, D = check_adjoint_multi(1, 1, M, np.ones((1, 65535, 1)))
    assert D == 65535


MALFORMED = [dict(dX=np.ones((B + 1, 2, N))), dict(dX=np.ones((B, 2, N + 1))), dict(dX=np.ones((B, N))), dict(dX=np.ones(N)),
             dict(dX=np.ones((B, 0, N))), dict(dX=None, dY=np.ones((B, 2, M))),
             dict(dX=np.ones((B, 2, N)), dY=np.ones((B, 2, M + 1))), dict(dX=np.ones((B, 2, N)), dY=np.ones((B - 1, 2, M))),
             dict(dX=np.ones((B, 2, N)), dY=np.ones((B, 3, M))), dict(dX=np.ones((B, 2, N)), dY=np.ones((B, M))),
             dict(dX=np.ones((1, 65536, 1)))]


@pytest.mark.parametrize("kwargs", MALFORMED, ids=[str(k) for k in range(len(MALFORMED))])
def test_shape_errors_raise(kwargs):
    from osqp_amd.batch import check_adjoint_multi
    b, n = (1, 1) if kwargs["dX"] is not None and kwargs["dX"].shape[:2] == (1, 65536) else (B, N)
    with pytest.raises(ValueError):
        check_adjoint_multi(b, n, M, **kwargs)


def test_check_adjoint_keeps_its_refusal():
    """The single-cotangent check is not widened: a 3-D array is still malformed there."""
    from osqp_amd.batch import check_adjoint
    with pytest.raises(ValueError):
        check_adjoint(B, N, M, dX=np.ones((B, N, 1)))


def test_reference_is_linear_in_the_cotangent(oracle_mod):
    """ref(a g1 + g2) = a ref(g1) + ref(g2) for the five gradients, per member of shape_family(5, 7, 3, seed 11) at the
    oracle's polished x, y.  The reference solves M r = g by LU with partial pivoting, whose computed r is the exact
    solution of a system perturbed by O(eps) relative: each of the three solves is off by at most c eps cond(M) |r|, so
    the two sides differ by at most c eps cond(M) (|a| |r1| + |r2| + |r3|) in r, and the gradients are r times entries of
    x, y (or r itself): the bar is that with c = 100 and the factor 2 max(1, |x|, |y|) of the bilinear terms."""
    P, A, Q, L, U, _ = shape_family(N, M, B, seed=11)
    rng = np.random.default_rng(12)
    a = -1.75
    Pf = (P + sparse.triu(P, 1).T).toarray(); Ad = A.toarray()
    for b in range(B):
        ro = oracle(oracle_mod, P, Q[b], A, L[b], U[b], polish=1).solve()
        assert ro.info.status_val == 1
        x, y = np.array(ro.x), np.array(ro.y)
        g1, g2 = (rng.standard_normal(N), rng.standard_normal(M)), (rng.standard_normal(N), rng.standard_normal(M))
        ref = lambda gx, gy: adjoint_reference(P, A, L[b], U[b], x, y, gx, gy)
        r1, r2, r3 = ref(*g1), ref(*g2), ref(a * g1[0] + g2[0], a * g1[1] + g2[1])
        Ar = Ad[r1.rows]; k = r1.rows.size
        Mk = np.zeros((N + k, N + k)); Mk[:N, :N] = Pf; Mk[:N, N:] = Ar.T; Mk[N:, :N] = Ar
        size = lambda r: max(np.abs(r.rx).max(), np.abs(r.rnu).max() if k else 0.0)
        bar = 100 * np.finfo(float).eps * np.linalg.cond(Mk) * (abs(a) * size(r1) + size(r2) + size(r3)) \
            * 2 * max(1.0, np.abs(x).max(), np.abs(y).max())
        assert np.array_equal(r1.active, r3.active) and np.array_equal(r2.active, r3.active)
        for g in ("dq", "dl", "du", "dPx", "dAx"):
            err = np.abs(getattr(r3, g) - (a * getattr(r1, g) + getattr(r2, g))).max()
            print(b, g, "%.2e (bar %.2e)" % (err, bar))
            assert err <= bar, (b, g, err, bar)
