"""CPU checks of tests/_rowpart_reference.py -- the model the row-partitioned kernels are held against in
tests/test_gpu_rowpart_kernels.py -- and of the sharding functions the two-rank cases of tests/test_rowpart.py rely on.

  * the model's whole loop (exact dense solve in place of PCG) against the oracle: status, iter, rho_updates, x and y to 1e-6, on the two
    small problems of test_rowpart.py and on a second solve with kept iterates and rho;
  * every generated case inside the model's conditions: K positive definite (except the one non-convex case), no row's projection
    argument near a bound, class thresholds hit exactly where claimed, planted maxima where claimed;
  * shard_rows / shard_triu: contiguous, disjoint, covering; sum_g sym(P_g) == P bit for bit; the edge shapes as facts."""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import linalg as spla

import _rowpart_reference as R
from osqp_amd import rowpart
from osqp_amd.problems import portfolio_qp, random_sparse_qp

LD = R.LD


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _small(which):
    if which == "portfolio_small":
        return portfolio_qp(8, 25, sector_rows=5, seed=3), dict(eps_abs=1e-5, eps_rel=1e-5)
    return random_sparse_qp(300, 600, seed=5), {}


@pytest.mark.parametrize("which", ["portfolio_small", "random"])
def test_reference_loop_matches_oracle(oracle_mod, which):
    pb, kw = _small(which)
    so = oracle_mod.OracleOSQP().setup(**pb, **kw)
    scaled = rowpart.scaled_problem_from_handle(so)
    ro = so.solve()
    r = R.Model(scaled, **kw).solve()
    assert r.info.status == ro.info.status == "solved" and r.info.iter == ro.info.iter and r.info.rho_updates == ro.info.rho_updates
    assert _rel(r.x, ro.x) < 1e-6 and _rel(r.y, ro.y) < 1e-6
    assert abs(r.info.obj_val - ro.info.obj_val) <= 1e-8 * max(1.0, abs(ro.info.obj_val))
    assert abs(r.info.pri_res - ro.info.pri_res) <= 1e-6 * max(1e-3, ro.info.pri_res) and abs(r.info.dua_res - ro.info.dua_res) <= 1e-6 * max(1e-3, ro.info.dua_res)


def test_reference_second_solve_keeps_rho_like_the_oracle(oracle_mod):
    """The contract of a second solve on one handle: kept iterates, the adapted rho, rho_updates counting on.  The oracle: 110
    iterations and one rho update, then 25 iterations and still one."""
    pb = random_sparse_qp(300, 600, seed=5)
    so = oracle_mod.OracleOSQP().setup(**pb, max_iter=110)
    M = R.Model(rowpart.scaled_problem_from_handle(so), max_iter=110)
    state = None
    for want in ((110, 1), (25, 1)):
        ro, r = so.solve(), M.solve(state)
        state = r.state
        assert (ro.info.iter, ro.info.rho_updates) == want and ro.info.status == r.info.status == "solved"
        assert r.info.iter == ro.info.iter and r.info.rho_updates == ro.info.rho_updates
        assert _rel(r.x, ro.x) < 1e-6 and _rel(r.y, ro.y) < 1e-6


# ---- the generated cases ---------------------------------------------------------------------------------------------------
def _K_sparse(M, rv):
    P = sparse.csc_matrix((M.pv.astype(float), (M.pr, M.pc)), shape=(M.n, M.n))
    A = sparse.csc_matrix((M.av.astype(float), (M.ar, M.ac)), shape=(M.m, M.n))
    return (P + M.st["sigma"] * sparse.eye(M.n) + A.T @ sparse.diags(rv) @ A).tocsc()


def _first_step(scaled, **st):
    """x~ of the first iteration from a float64 sparse factor (close enough to say where rows land), and the model's step on it."""
    M = R.Model(scaled, **st)
    rv = R.rho_vec(M.l, M.u, M.st["rho"])
    z0, x0 = np.zeros(M.m), np.zeros(M.n)
    b, _ = M.rhs(x0, z0, z0, rv)
    xt = spla.splu(_K_sparse(M, rv)).solve(b.astype(float))
    return M, rv, xt, M.step(xt, x0, z0, z0, rv)


def _assert_clear_of_bounds(M, step):
    arg, bound = step["arg"]
    fin_l, fin_u = np.abs(M.l) < 1e20, np.abs(M.u) < 1e20
    # 1e-6: far above both the rounding bound and what the PCG's stopping tolerance leaves of x~
    assert bound.max(initial=0) < 1e-9
    assert np.all(np.abs(arg - M.l)[fin_l] > 1e-6) and np.all(np.abs(arg - M.u)[fin_u] > 1e-6)


@pytest.mark.parametrize("n,m", R.SIZES)
@pytest.mark.parametrize("scaled", [False, True])
def test_banded_cases_stay_inside_the_conditions(n, m, scaled):
    sc = R.banded(n, m, seed=n + m, scaled=scaled)
    M, rv, xt, st = _first_step(sc)
    assert R.dominant(M)
    if n <= 300:
        R.cholesky(M.K_dense(rv))
    _assert_clear_of_bounds(M, st)
    if m >= 255 and n >= 255:            # rows of every kind, and of every landing place
        z = st["z"][0]
        assert {-1, 0, 1} == set(M.cls.tolist())
        assert (z == M.l)[M.cls == 0].any() and (z == M.u)[M.cls == 0].any() and ((z > M.l) & (z < M.u))[M.cls == 0].any()
    assert M.scaled_data == scaled


def test_class_case_sits_on_the_thresholds():
    sc, claimed = R.class_case()
    l, u = sc["l"], sc["u"]
    assert np.array_equal(R.row_class(l, u), claimed)
    assert l[0] == -1e26 and u[1] == 1e26 and l[2] < -1e26 and u[2] > 1e26 and np.nextafter(l[2], 0) == -1e26 and np.nextafter(u[2], 0) == 1e26
    assert u[4] - l[4] == 1e-4 and u[6] - l[6] == 1e-4 and u[5] - l[5] < 1e-4 and np.nextafter(u[5] - l[5], 1) == 1e-4
    for rho, want in ((0.1, 0.1), (1e-7, 1e-6), (1e7, 1e6)):
        rv = R.rho_vec(l, u, rho)
        assert np.array_equal(rv, np.where(claimed == -1, 1e-6, np.where(claimed == 1, 1e3 * want, want)))
        M = R.Model(sc, rho=rho)
        R.cholesky(M.K_dense(rv))
        mi, _ = M.minv(rv)
        assert mi[4] == 1 / LD(M.st["sigma"])                              # the empty column
        assert mi[3] == 1 / (LD(0.75) + LD(M.st["sigma"]))                 # diagonal of P only
    # columns as claimed
    P, A = sparse.csc_matrix(sc["P"]), sparse.csc_matrix(sc["A"])
    assert P[2, 2] == 0 and A[:, 2].nnz > 0 and P[:, 4].nnz == 0 and A[:, 4].nnz == 0 and A[:, 3].nnz == 0


@pytest.mark.parametrize("k", [8191, 8192, 8193])
def test_dense_column_cases(k):
    sc = R.dense_column_case(k)
    M, rv, xt, st = _first_step(sc)
    A, P = sparse.csc_matrix(sc["A"]), sparse.csc_matrix(sc["P"])
    assert A[:, 0].nnz == k and P[:, 0].nnz == 0 and P[0, :].nnz == 0          # row 0 of [P | A'] holds exactly k entries
    R.cholesky(M.K_dense(rv))
    _assert_clear_of_bounds(M, st)


@pytest.mark.parametrize("at", R.PLANT_AT)
@pytest.mark.parametrize("scaled", [False, True])
def test_planted_maxima_sit_where_claimed(at, scaled):
    n = m = 300
    sc = R.planted(n, m, at, seed=40 + at, scaled=scaled)
    M, rv, xt, st = _first_step(sc)
    R.cholesky(M.K_dense(rv))
    _assert_clear_of_bounds(M, st)
    x, z, y = st["x"][0], st["z"][0], st["y"][0]
    i = at % m
    assert z[i] == -1000.0 and sc["q"][i] < 0
    ax, _ = M.A_mul(x)
    for v in (np.abs(z), np.abs(M.Einv * z), np.abs(ax - z), np.abs(M.Einv * (ax - z)), np.abs(M.q), np.abs(M.Dinv * M.q)):
        assert int(np.argmax(v)) == i and np.sort(v)[-2] < 0.9 * v[i]


def test_bookkeeping_cases():
    # q = 0 with 0 strictly inside the bounds
    sc = R.zero_q_case()
    assert not sc["q"].any() and np.all(sc["l"] < 0) and np.all(sc["u"] > 0)
    M = R.Model(sc)
    R.cholesky(M.K_dense(R.rho_vec(M.l, M.u, 0.1)))
    # the slow case: positive definite, and a float64 Jacobi-PCG needs far more than 4 (and than 3) iterations
    sc = R.slow_pcg_case()
    M = R.Model(sc)
    rv = R.rho_vec(M.l, M.u, 0.1)
    R.cholesky(M.K_dense(rv))
    assert R.dominant(M)
    K = _K_sparse(M, rv)
    b = -sc["q"]
    x, r = np.zeros(M.n), b.copy()
    mi = 1.0 / K.diagonal()
    zz = mi * r; p = zz.copy(); rz = r @ zz; it = 0
    while r @ r > (M.eps_pcg ** 2) * (b @ b):
        Kp = K @ p; a = rz / (p @ Kp); x += a * p; r -= a * Kp; zz = mi * r; rz2 = r @ zz; p = zz + (rz2 / rz) * p; rz = rz2; it += 1
    assert it > 20
    # the diagonal case: K is diagonal
    sc = R.diagonal_K_case()
    M = R.Model(sc)
    K = _K_sparse(M, R.rho_vec(M.l, M.u, 0.1))
    assert (K - sparse.diags(K.diagonal())).nnz == 0 and K.diagonal().min() > 0
    # the non-convex case: no Cholesky factor, and the first p'Kp is negative
    sc = R.nonconvex_case()
    M = R.Model(sc)
    with pytest.raises(np.linalg.LinAlgError):
        R.cholesky(M.K_dense(np.zeros(0)))
    d = sc["P"].diagonal() + M.st["sigma"]
    assert ((sc["q"] / d) ** 2 * d).sum() < 0


def test_m0_case():
    sc = R.m0_case()
    M = R.Model(sc)
    assert M.m == 0 and R.dominant(M)
    val, _ = M.scalars(np.ones(M.n), np.zeros(0), np.zeros(0))
    assert not val[:6].any() and M.info(val, 0.1)["pri_res"] == 0


# ---- sharding --------------------------------------------------------------------------------------------------------------
def _shard_cases():
    rng = np.random.RandomState(2)
    n = 12
    B = sparse.random(n, n, density=0.3, random_state=rng)
    P = sparse.triu(B.T @ B + sparse.eye(n), format="csc")
    first = sparse.csc_matrix(np.vstack([np.ones((1, n)), np.zeros((5, n))]))
    last = sparse.csc_matrix(np.vstack([np.zeros((5, n)), np.ones((1, n))]))
    return dict(random=(P, sparse.random(20, n, density=0.3, random_state=rng, format="csc")),
                empty_A=(P, sparse.csc_matrix((0, n))), zero_A=(P, sparse.csc_matrix((7, n))),
                empty_P=(sparse.csc_matrix((n, n)), sparse.random(20, n, density=0.3, random_state=rng, format="csc")),
                tiny=(sparse.csc_matrix(sparse.diags([1.0, 2.0])), sparse.csc_matrix(np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]))),
                first_row=(P, first), last_row=(P, last))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["random", "empty_A", "zero_A", "empty_P", "tiny", "first_row", "last_row"])
def test_shards_are_contiguous_disjoint_covering_and_sum_to_P(name, world):
    P, A = _shard_cases()[name]
    rows = rowpart.shard_rows(A, world)
    assert len(rows) == world and rows[0][0] == 0 and rows[-1][1] == A.shape[0]
    assert all(a <= b for a, b in rows) and all(rows[g][1] == rows[g + 1][0] for g in range(world - 1))
    parts = rowpart.shard_triu(P, world)
    assert len(parts) == world
    tot = sparse.csc_matrix(P.shape)
    for Pg in parts:
        assert Pg.shape == P.shape and sparse.tril(Pg, -1).nnz == 0
        tot = tot + Pg + sparse.triu(Pg, 1).T
    full = sparse.csc_matrix(P + sparse.triu(P, 1).T)
    assert sum(Pg.nnz for Pg in parts) == sparse.csc_matrix(P).nnz
    assert np.array_equal(tot.toarray(), full.toarray())


def test_shard_edge_shapes_as_facts():
    """What the two- and three-rank cases of test_rowpart.py rely on."""
    pb = R.edge_problem("dense_last_row")
    assert rowpart.shard_rows(pb["A"], 2) == [(0, 4), (4, 4)]
    assert [p.nnz for p in rowpart.shard_triu(sparse.csc_matrix(sparse.diags([1.0, 2.0])), 3)] == [1, 1, 0]
    assert [p.nnz for p in rowpart.shard_triu(R.edge_problem("n2_diag")["P"], 3)] == [1, 1, 0]
    P, A = _shard_cases()["first_row"]
    assert rowpart.shard_rows(A, 2) == [(0, 1), (1, 6)] and rowpart.shard_rows(A, 3) == [(0, 1), (1, 1), (1, 6)]
    P, A = _shard_cases()["last_row"]
    assert rowpart.shard_rows(A, 2) == [(0, 6), (6, 6)]
    assert rowpart.shard_rows(sparse.csc_matrix((0, 5)), 3) == [(0, 0)] * 3
    pb = R.edge_problem("eq_on_rank1")
    (a0, b0), (a1, b1) = rowpart.shard_rows(pb["A"], 2)
    eq = pb["u"] - pb["l"] < 1e-4
    assert not eq[a0:b0].any() and eq[a1:b1].any() and b0 - a0 > 0
    assert R.edge_problem("m0")["A"].shape[0] == 0


@pytest.mark.parametrize("name", R.EDGE_WORLD2 + R.EDGE_WORLD3)
def test_edge_problems_are_solved_by_the_oracle(oracle_mod, name):
    ro = oracle_mod.OracleOSQP().setup(**R.edge_problem(name), **R.EDGE_SETTINGS).solve()
    assert ro.info.status == "solved" and ro.info.iter >= 25
