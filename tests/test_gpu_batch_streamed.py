"""GPU tests of the streamed-inverse batch engine (osqp_amd/csrc/batch_streamed.h, BatchOSQP(engine="streamed")):
n from 1 to 1024 around the padding steps of 32 and the tiled engine's 128, m = 0, 1 and about 2n, the shape the
tiled engine refuses for LDS, per-member values with explicit zeros, class-changing updates, mixed statuses, the
setup contracts, K^-1 through the member hook, the device arrays, dispatch order and interleaved batches.

Every parity test runs with a short adaptive-rho interval and asserts that some member's rho moved, so the
rebuild rounds of the host driver (leave the loop, re-form and re-invert K, resume) are exercised."""
import numpy as np
import pytest
from scipy import sparse

from _batch_parity import assert_parity, check_member_kinv, oracle, rel, shape_family

pytestmark = pytest.mark.gpu

KW = dict(adaptive_rho_interval=10)
SHAPES_N = [1, 17, 64, 128, 129, 150, 255, 256, 257, 511, 512, 700, 1024]


def _max_m(n):
    NP = (n + 31) // 32 * 32
    return (160 * 1024 - 8 * (7 * NP + 320)) // 92


def _ms(n):
    return sorted({0, 1, min(2 * n + 3, _max_m(n))})


def _streamed(P, A, Q, L, U, **kw):
    import osqp_amd
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="streamed", **kw)


def _check_batch(bs, r, orc, P, A, Q, L, U, what, kw=KW, Px_all=None, Ax_all=None):
    """Parity of every member against its own oracle run; returns the oracles."""
    out = []
    for b in range(Q.shape[0]):
        Pb, Ab = P, A
        if Px_all is not None:
            Pb = sparse.triu(P, format="csc"); Pb.sort_indices(); Pb = Pb.copy(); Pb.data = Px_all[b].copy()
        if Ax_all is not None:
            Ab = A.copy(); Ab.sort_indices(); Ab.data = Ax_all[b].copy()
        so = oracle(orc, Pb, Q[b], Ab, L[b], U[b], **kw)
        ro = so.solve()
        assert_parity(r, b, ro, what)
        out.append((so, ro))
    return out


def _assert_rebuild_ran(bs, r):
    assert np.any(r.rho_updates > 0), "no member's rho moved: the rebuild round was not exercised"
    assert bs.rounds()[0] >= 2


@pytest.mark.parametrize("n", SHAPES_N)
def test_parity_shapes(gpu_lib, oracle_mod, n):
    for m in _ms(n):
        P, A, Q, L, U, _ = shape_family(n, m, 3, seed=1000 + n + m)
        bs = _streamed(P, A, Q, L, U, **KW)
        assert bs.shape() == (1, (n + 31) // 32 * 32)
        r = bs.solve()
        _check_batch(bs, r, oracle_mod, P, A, Q, L, U, "n=%d m=%d" % (n, m))
        if m > 1:
            _assert_rebuild_ran(bs, r)
        bs.cleanup()


def test_shape_the_tiled_engine_refuses(gpu_lib, oracle_mod, capfd):
    import osqp_amd
    P, A, Q, L, U, _ = shape_family(128, 600, 3, seed=7, per_row=10)
    with pytest.raises(ValueError, match="error 4"):
        osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **KW)
    assert "160 KiB" in capfd.readouterr().err
    bs = _streamed(P, A, Q, L, U, **KW)
    r = bs.solve()
    _check_batch(bs, r, oracle_mod, P, A, Q, L, U, "128x600")
    _assert_rebuild_ran(bs, r)


@pytest.mark.parametrize("n", [17, 64, 128])
def test_both_engines_small(gpu_lib, oracle_mod, n):
    import osqp_amd
    P, A, Q, L, U, _ = shape_family(n, 2 * n, 4, seed=300 + n)
    rt = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **KW).solve()
    bs = _streamed(P, A, Q, L, U, **KW)
    r = bs.solve()
    _check_batch(bs, r, oracle_mod, P, A, Q, L, U, "streamed")
    for b in range(Q.shape[0]):
        so = oracle(oracle_mod, P, Q[b], A, L[b], U[b], **KW)
        assert_parity(rt, b, so.solve(), "tiled")
    _assert_rebuild_ran(bs, r)


@pytest.mark.parametrize("n", [150, 400])
def test_per_member_values_with_explicit_zeros(gpu_lib, oracle_mod, n):
    m, B = 2 * n, 3
    P, A, Q, L, U, _ = shape_family(n, m, B, seed=500 + n)
    Pu = sparse.triu(P, format="csc"); Pu.sort_indices()
    As = A.copy(); As.sort_indices()
    rng = np.random.default_rng(n)
    Px = np.tile(Pu.data, (B, 1)); Ax = np.tile(As.data, (B, 1))
    rows = Pu.indices; cols = np.repeat(np.arange(n), np.diff(Pu.indptr))
    off = np.flatnonzero(rows != cols)
    for b in range(B):
        Px[b] *= rng.uniform(0.8, 1.2, Px.shape[1])
        Ax[b] *= rng.uniform(0.5, 2.0, Ax.shape[1])
        Px[b, rng.choice(off, len(off) // 4, replace=False)] = 0.0      # explicit zeros off the diagonal
        Ax[b, rng.choice(Ax.shape[1], Ax.shape[1] // 5, replace=False)] = 0.0
    bs = _streamed(Pu, As, Q, L, U, Px_all=Px, Ax_all=Ax, **KW)
    r = bs.solve()
    _check_batch(bs, r, oracle_mod, Pu, As, Q, L, U, "zeros", Px_all=Px, Ax_all=Ax)
    _assert_rebuild_ran(bs, r)


@pytest.mark.parametrize("warm", [True, False])
def test_updates_change_classes(gpu_lib, oracle_mod, warm):
    n, m, B = 150, 300, 4
    kw = dict(KW, warm_start=warm)
    P, A, Q, L, U, x0 = shape_family(n, m, B, seed=77)
    bs = _streamed(P, A, Q, L, U, **kw)
    sos = [oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw) for b in range(B)]
    rng = np.random.default_rng(4)
    r = bs.solve()
    for b in range(B):
        assert_parity(r, b, sos[b].solve(), "solve 0")
    moved = np.any(r.rho_updates > 0)
    ax = A @ x0
    for step in range(3):
        L2, U2 = L.copy(), U.copy()
        flip = rng.random((B, m)) < 0.2
        if step == 0:                                    # rows become equality rows
            L2[flip] = U2[flip] = np.broadcast_to(ax, (B, m))[flip]
        elif step == 2:                                  # rows become free
            L2[flip] = -np.inf; U2[flip] = np.inf
        Q2 = Q * (1 + 0.1 * step)                        # step 1: back to the original classes
        assert bs.update(Q=Q2, L=L2, U=U2) == 0
        r = bs.solve()
        for b in range(B):
            sos[b].update(q=Q2[b], l=L2[b], u=U2[b])
            assert_parity(r, b, sos[b].solve(), "update %d" % step)
        moved |= np.any(r.rho_updates > 0)
    assert moved


def test_member_statuses_in_one_batch(gpu_lib, oracle_mod):
    """Primal infeasible, dual infeasible, max-iteration and solved members at n = 150; certificates within 1e-5."""
    from osqp_amd import abi
    n, m, B = 150, 200, 6
    P, A, Q, L, U, x0 = shape_family(n, m, B, seed=55)
    Pd = P.tolil(); Pd[5, :] = 0.0; Pd[:, 5] = 0.0
    P = sparse.triu(Pd.tocsc(), format="csc"); P.eliminate_zeros()
    A = A.tolil(); A[:, 5] = 0.0; A[1, :] = A[0, :]
    if A[0, :].nnz == 0:
        A[0, 0] = A[1, 0] = 1.0
    A = A.tocsc(); A.eliminate_zeros()
    ax = A @ x0
    L = np.tile(ax - 0.5, (B, 1)); U = np.tile(ax + 0.5, (B, 1))
    Q[:, 5] = 0.0
    Q[1, 5] = 1.5; Q[4, 5] = -0.7                                            # dual infeasible
    L[3, 0], U[3, 0] = ax[0] + 5.0, ax[0] + 6.0; L[3, 1], U[3, 1] = ax[0] - 6.0, ax[0] - 5.0   # primal infeasible
    Q[5] *= 1e4                                                              # slow: meets max_iter
    kw = dict(KW, max_iter=300)
    bs = _streamed(P, A, Q, L, U, **kw)
    r = bs.solve()
    res = _check_batch(bs, r, oracle_mod, P, A, Q, L, U, "statuses", kw=kw)
    stats = {b: ro.info.status_val for b, (_, ro) in enumerate(res)}
    assert stats[1] == stats[4] == abi.OSQP_DUAL_INFEASIBLE and stats[3] == abi.OSQP_PRIMAL_INFEASIBLE, stats
    assert abi.OSQP_SOLVED in stats.values(), stats
    for b, (_, ro) in enumerate(res):
        if b in (1, 4):
            assert np.all(np.isnan(r.x[b]) | (r.x[b] == abi.OSQP_NAN))
            assert rel(r.dual_inf_cert[b], ro.dual_inf_cert) < 1e-5, b
        if b == 3:
            assert rel(r.prim_inf_cert[b], ro.prim_inf_cert) < 1e-5
    r2 = _streamed(P, A, Q, L, U, **dict(KW, max_iter=40)).solve()
    for b in range(B):
        ro = oracle(oracle_mod, P, Q[b], A, L[b], U[b], **dict(KW, max_iter=40)).solve()
        assert_parity(r2, b, ro, "max_iter")
    assert np.any(r2.status_val == abi.OSQP_MAX_ITER_REACHED)


def test_nonconvex_member_rejected(gpu_lib, capfd):
    n, B, bad, m = 300, 3, 1, 10
    rng = np.random.default_rng(9)
    Pu = sparse.triu(np.ones((n, n)), format="csc"); Pu.sort_indices()
    r_, c_ = Pu.indices, np.repeat(np.arange(n), np.diff(Pu.indptr))
    Px = np.empty((B, Pu.nnz))
    for b in range(B):
        Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
        ev = rng.uniform(0.5, 2.0, n)
        if b == bad:
            ev[0] = -rng.uniform(0.5, 1.0)
        M = Qm @ np.diag(ev) @ Qm.T
        Px[b] = (0.5 * (M + M.T))[r_, c_]
    A = sparse.hstack([sparse.eye(m, format="csc"), sparse.csc_matrix((m, n - m))], format="csc")
    Q = rng.standard_normal((B, n))
    with pytest.raises(ValueError, match="error 5"):
        _streamed(Pu, A, Q, -np.ones((B, m)), np.ones((B, m)), Px_all=Px, sigma=1e-6)
    assert "QP %d of the batch is non-convex" % bad in capfd.readouterr().err


@pytest.mark.parametrize("n", [129, 300, 700])
def test_member_kinv(gpu_lib, oracle_mod, n):
    P, A, Q, L, U, _ = shape_family(n, n, 3, seed=900 + n)
    kw = dict(KW, eps_abs=1e-5, eps_rel=1e-5)
    bs = _streamed(P, A, Q, L, U, **kw)
    NP = (n + 31) // 32 * 32
    ran = 0
    for b in range(3):                                   # as set up
        ran += check_member_kinv(bs, b, oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw), "setup", NP)
    r = bs.solve()
    for b in range(3):                                   # after rebuilds with the moved rho
        ran += check_member_kinv(bs, b, oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw), "solve", NP)
    assert ran >= 1
    _assert_rebuild_ran(bs, r)


def test_device_arrays_match_results(gpu_lib):
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    P, A, Q, L, U, _ = shape_family(200, 300, 5, seed=3)
    bs = _streamed(P, A, Q, L, U, **KW)
    r = bs.solve()
    got = []
    for a in bs.device_arrays():
        ai = a.__cuda_array_interface__
        h = np.empty(ai["shape"])
        assert hip.hipMemcpy(h.ctypes.data, ai["data"][0], h.nbytes, 2) == 0       # hipMemcpyDeviceToHost
        got.append(h)
    X, Y, I = got
    assert np.array_equal(X, r.x) and np.array_equal(Y[:, :300], r.y) and np.array_equal(I, r.info_raw)


def test_dispatch_order_bit_identical(gpu_lib, monkeypatch):
    import osqp_amd
    P, A, Q, L, U, _ = shape_family(150, 300, 1025, seed=12)
    outs = []
    for lpt in ("0", "1"):
        monkeypatch.setenv("OSQP_AMD_BATCH_LPT", lpt)
        bs = _streamed(P, A, Q, L, U, **KW)
        rs = [bs.solve() for _ in range(3)]
        outs.append(rs)
        bs.cleanup()
    for a, b in zip(*outs):
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y) and np.array_equal(a.info_raw, b.info_raw)
    assert np.any(outs[0][0].rho_updates > 0)


def test_two_streamed_batches_and_a_tiled_one(gpu_lib, oracle_mod):
    import osqp_amd
    p1 = shape_family(150, 300, 3, seed=21)[:5]          # LDS below 64 KiB
    p2 = shape_family(300, 1000, 2, seed=22)[:5]         # LDS above 64 KiB
    pt = shape_family(64, 130, 3, seed=23)[:5]
    s1, s2 = _streamed(*p1, **KW), _streamed(*p2, **KW)
    st = osqp_amd.BatchOSQP().setup(*pt, **KW)
    r2 = s2.solve(); rt = st.solve(); r1 = s1.solve()
    for (P, A, Q, L, U), r in ((p1, r1), (p2, r2), (pt, rt)):
        for b in range(Q.shape[0]):
            assert_parity(r, b, oracle(oracle_mod, P, Q[b], A, L[b], U[b], **KW).solve(), "interleaved")
    r1b = s1.solve(); r2b = s2.solve()                   # warm starts, both alive
    assert np.all(r1b.iter <= r1.iter + 25) and np.all(r2b.iter <= r2.iter + 25)


def test_refusals(gpu_lib, capfd):
    P, A, Q, L, U, _ = shape_family(1025, 10, 2, seed=1)
    with pytest.raises(ValueError, match="error 4"):
        _streamed(P, A, Q, L, U)
    assert "1024" in capfd.readouterr().err
    P, A, Q, L, U, _ = shape_family(1024, 1200, 2, seed=1)
    with pytest.raises(ValueError, match="error 4"):
        _streamed(P, A, Q, L, U)
    assert "160 KiB" in capfd.readouterr().err
    for k in ("polish", "time_limit"):
        with pytest.raises(ValueError, match="error 2"):
            _streamed(P, A, Q, L, U, **{k: 1})
