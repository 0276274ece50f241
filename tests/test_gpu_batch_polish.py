"""Polish on the batch engines (BatchOSQP.polish, osqp_amd_batch_polish) against the CPU oracle run with polish=1.

Bar, per member: status_polish identical to the oracle's; for an accepted member x and y within 1e-6 relative
(_batch_parity.rel, the project's parity bar), the objective within 1e-8 relative, pri_res and dua_res below 1e-8
 and below the residuals the ADMM solve left; for a rejected or skipped member x, y and the info
record bit-equal to what solve() returned.  No member is excused.

With fewer refinement steps or another delta (test_settings) the reference's own polished residuals are above 1e-8
-- the regularisation error is not refined away: its 0-step residuals are 1e-6 .. 1e-4 -- so there the residual bar
is the larger of 1e-8 and twice the oracle's own residual of that member (the factor covers a different summation
order; what dominates such a residual is the deterministic regularisation error)."""
import numpy as np
import pytest

from _batch_parity import oracle, rel, shape_family, assert_parity

pytestmark = pytest.mark.gpu

TILED_SHAPES = [(1, 5, 4, 1), (17, 37, 6, 2), (33, 69, 6, 3), (64, 131, 6, 4), (65, 40, 6, 5), (128, 259, 4, 6), (40, 40, 6, 3)]
STREAMED_SHAPES = TILED_SHAPES + [(150, 303, 4, 7)]
_cache = {}


def _family(shape):
    if shape not in _cache:
        _cache[shape] = shape_family(*shape)
    return _cache[shape]


def _oracle_polished(orc, shape, **kw):
    """Per member: the oracle's result with polish=1 (computed once per shape and settings, never modified)."""
    key = (shape, tuple(sorted(kw.items())))
    if key not in _cache:
        P, A, Q, L, U, _ = _family(shape)
        _cache[key] = [oracle(orc, P, Q[b], A, L[b], U[b], polish=1, **kw).solve() for b in range(Q.shape[0])]
    return _cache[key]


def _run(shape, engine, **kw):
    import osqp_amd
    P, A, Q, L, U, _ = _family(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **kw)
    r0 = bs.solve()
    assert np.all(r0.status_polish == 0)
    return bs, r0, bs.polish()


def _unchanged(r0, r1, b, tag):
    assert np.array_equal(r0.x[b], r1.x[b], equal_nan=True) and np.array_equal(r0.y[b], r1.y[b], equal_nan=True), tag
    assert np.array_equal(r0.info_raw[b], r1.info_raw[b], equal_nan=True), tag
    assert np.array_equal(r0.prim_inf_cert[b], r1.prim_inf_cert[b], equal_nan=True), tag


def _check(r0, r1, refs, what, res_bar=None):
    sp = [int(ro.info.status_polish) for ro in refs]
    for b, ro in enumerate(refs):
        print(what, b, "status_polish", int(r1.status_polish[b]), sp[b], "relx %.2e rely %.2e" % (rel(r1.x[b], ro.x), rel(r1.y[b], ro.y)),
              "obj %.3e" % abs(r1.obj_val[b] - ro.info.obj_val), "res %.2e %.2e" % (r1.pri_res[b], r1.dua_res[b]),
              "oracle %.2e %.2e" % (ro.info.pri_res, ro.info.dua_res), "admm %.2e %.2e" % (r0.pri_res[b], r0.dua_res[b]))
    for b, ro in enumerate(refs):
        tag = (what, b)
        assert ro.info.status_val == 1 and r0.status_val[b] == 1, tag
        assert r1.status_polish[b] == sp[b], tag + (int(r1.status_polish[b]), sp[b])
        if sp[b] == 1:
            assert rel(r1.x[b], ro.x) < 1e-6 and rel(r1.y[b], ro.y) < 1e-6, tag + (rel(r1.x[b], ro.x), rel(r1.y[b], ro.y))
            assert abs(r1.obj_val[b] - ro.info.obj_val) <= 1e-8 * max(1.0, abs(ro.info.obj_val)), tag
            bar_p = 1e-8 if res_bar is None else max(1e-8, res_bar * ro.info.pri_res)
            bar_d = 1e-8 if res_bar is None else max(1e-8, res_bar * ro.info.dua_res)
            assert r1.pri_res[b] < bar_p and r1.dua_res[b] < bar_d, tag + (r1.pri_res[b], r1.dua_res[b])
            assert r1.pri_res[b] <= r0.pri_res[b] and r1.dua_res[b] <= r0.dua_res[b], tag
            assert r1.iter[b] == r0.iter[b] and r1.rho_updates[b] == r0.rho_updates[b] and r1.rho[b] == r0.rho[b], tag
        else:
            _unchanged(r0, r1, b, tag)
    return sp


@pytest.mark.parametrize("shape", TILED_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
def test_parity_tiled(gpu_lib, oracle_mod, shape):
    bs, r0, r1 = _run(shape, "auto")
    assert bs.shape()[0] == 0
    _check(r0, r1, _oracle_polished(oracle_mod, shape), "tiled %s" % (shape,))


@pytest.mark.parametrize("shape", STREAMED_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
def test_parity_streamed(gpu_lib, oracle_mod, shape):
    bs, r0, r1 = _run(shape, "streamed")
    assert bs.shape()[0] == 1
    sp = _check(r0, r1, _oracle_polished(oracle_mod, shape), "streamed %s" % (shape,))
    if shape[0] in (17, 65, 128, 150):
        assert -1 in sp and 1 in sp, sp          # these shapes exercise the rejection path


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_no_constraints(gpu_lib, oracle_mod, engine):
    shape = (20, 0, 3, 8)
    bs, r0, r1 = _run(shape, engine)
    assert r1.y.shape == (3, 0)
    refs = _oracle_polished(oracle_mod, shape)
    for b, ro in enumerate(refs):
        print("m0", engine, b, int(r1.status_polish[b]), ro.info.status_polish, rel(r1.x[b], ro.x), r1.dua_res[b])
        assert r1.status_polish[b] == ro.info.status_polish, (b, int(r1.status_polish[b]), ro.info.status_polish)
        if ro.info.status_polish == 1:
            assert rel(r1.x[b], ro.x) < 1e-6 and r1.pri_res[b] == 0.0 and r1.dua_res[b] < 1e-8
            assert abs(r1.obj_val[b] - ro.info.obj_val) <= 1e-8 * max(1.0, abs(ro.info.obj_val))
        else:
            _unchanged(r0, r1, b, ("m0", b))


@pytest.mark.parametrize("engine", ["auto", "streamed"])
@pytest.mark.parametrize("sc", [{}, dict(scaling=0)], ids=["default", "scaling0"])
@pytest.mark.parametrize("kw", [dict(polish_refine_iter=0), dict(polish_refine_iter=1), dict(delta=1e-5)],
                         ids=["refine0", "refine1", "delta1e-5"])
def test_settings(gpu_lib, oracle_mod, kw, sc, engine):
    shape = (33, 69, 6, 3)
    bs, r0, r1 = _run(shape, engine, **kw, **sc)
    _check(r0, r1, _oracle_polished(oracle_mod, shape, **kw, **sc), "%s %s %s" % (engine, kw, sc), res_bar=2.0)


def _mixed():
    """One member that solves (loose rows), one primal infeasible (two contradictory copies of row 0, as
    test_gpu_batch_edges builds it), one that ends solved-inaccurate and one that reaches max_iter.  max_iter is a
    setting of the whole batch: at 5 no member of this family solves, so it is 40 with a check every iteration."""
    from scipy import sparse  # noqa: F401
    n, m, B = 20, 30, 4
    P, A, Q, L, U, x0 = shape_family(n, m, B, seed=55)
    A = A.tolil(); A[1, :] = A[0, :]; A = A.tocsc(); A.eliminate_zeros()
    ax = A @ x0
    L[0] = ax - 1e3; U[0] = ax + 1e3
    L[1] = ax - 0.5; U[1] = ax + 0.5
    L[1, 0], U[1, 0] = ax[0] + 5.0, ax[0] + 6.0; L[1, 1], U[1, 1] = ax[0] - 6.0, ax[0] - 5.0
    L[2] = ax - 0.05; U[2] = ax + 0.05
    L[3] = ax - 0.05; U[3] = ax + 0.05; Q[3] *= 300
    return P, A, Q, L, U, dict(max_iter=40, check_termination=1)


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_skips(gpu_lib, oracle_mod, engine):
    import osqp_amd
    P, A, Q, L, U, kw = _mixed()
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **kw)
    r0 = bs.solve()
    r1 = bs.polish()
    refs = [oracle(oracle_mod, P, Q[b], A, L[b], U[b], polish=1, **kw).solve() for b in range(4)]
    assert [ro.info.status_val for ro in refs] == [1, -3, 2, -2]
    assert list(r0.status_val) == [1, -3, 2, -2]
    assert r1.status_polish[0] in (1, -1) and r1.status_polish[0] == refs[0].info.status_polish
    assert list(r1.status_polish[1:]) == [0, 0, 0]
    for b in (1, 2, 3):
        _unchanged(r0, r1, b, ("skip", b))
    assert rel(r1.x[0], refs[0].x) < 1e-6 and rel(r1.y[0], refs[0].y) < 1e-6


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_state(gpu_lib, oracle_mod, engine):
    import osqp_amd
    shape = (33, 69, 6, 3)
    P, A, Q, L, U, _ = _family(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)
    with pytest.raises(RuntimeError, match="7"):
        bs.polish()                                      # no solve yet
    bs.solve()
    before = [bs.member_workspace(b) for b in range(Q.shape[0])]
    r1 = bs.polish()
    assert np.any(r1.status_polish == 1)
    for b, w0 in enumerate(before):
        w1 = bs.member_workspace(b)
        for k in ("D", "E", "ctype", "Kinv", "Pv", "Av"):
            assert np.array_equal(w0[k], w1[k]), (b, k)
        assert w0["rho"] == w1["rho"] and w0["c"] == w1["c"], b
    r1b = bs.polish()                                    # twice in a row: the same arrays bit for bit
    for k in ("x", "y", "info_raw", "status_polish"):
        assert np.array_equal(getattr(r1, k), getattr(r1b, k)), k
    # the next warm-started solve begins at the polished point, like the reference's (polish.c copies pol->x, z, y)
    r2 = bs.solve()
    assert np.all(r2.status_polish == 0)
    for b in range(Q.shape[0]):
        so = oracle(oracle_mod, P, Q[b], A, L[b], U[b], polish=1)
        so.solve()
        so.update_settings(polish=0)
        assert_parity(r2, b, so.solve(), "solve after polish")
    assert bs.update(Q=Q * 1.01) == 0
    with pytest.raises(RuntimeError, match="7"):
        bs.polish()                                      # the data moved and no solve has run on it


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_chunks(gpu_lib, monkeypatch, engine):
    """OSQP_AMD_BATCH_POLISH_CAP_BYTES (read at setup) caps the KKT buffer: one member per chunk here."""
    shape = (33, 69, 6, 3)
    _, _, one = _run(shape, engine)
    monkeypatch.setenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES", "1")
    _, _, many = _run(shape, engine)
    for k in ("x", "y", "info_raw", "status_polish"):
        assert np.array_equal(getattr(one, k), getattr(many, k)), k
    assert np.any(one.status_polish == 1)


def test_one_engine_per_member_refuses(gpu_lib):
    import osqp_amd
    P, A, Q, L, U, _ = _family((150, 303, 4, 7))
    bs = osqp_amd.BatchOSQP().setup(P, A, Q[:2], L[:2], U[:2])
    with pytest.raises(RuntimeError, match='engine="streamed"'):
        bs.polish()
