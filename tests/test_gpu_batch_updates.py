"""GPU tests of the batch engines' update family -- `BatchOSQP.update_matrices`, `update_rho`, `warm_start`
(include/osqp_amd_batch.h) -- for both engines: the register-tiled one (engine="auto", n <= 128) and the streamed one.

Parity bar (tests/_batch_parity.assert_parity): status, iteration count and rho updates identical to the member's
oracle run; x, y within 1e-6 relative; objective within 1e-8 relative.  A member's oracle run is OracleOSQP.setup
followed by the same call sequence (update(Px=, Ax=), update_rho, warm_start, update(q, l, u), solve).

No member is let off.  The seeds were chosen on the CPU with the oracle alone (this file's problem generators are
module-level functions so that such a check runs the same data): for every member of every case of
test_matrix_updates_follow_the_oracle (216 member runs) and of test_sequence_of_updates_and_warm_starts (16 member
sequences of ten steps), the oracle's call sequence replayed with the new matrix values moved by 1e-15 relative (three
draws) ends every solve on the same iteration count, count of rho updates and status as without the change, and in
every matrix-update case some member's rho moves in the first solve.

Workspace yardstick of test_workspace_after_matrix_update: a FRESH oracle setup on the new data, because the oracle's
own update path unscales and rescales (its D, E, c, Pv, Av after update(Px, Ax) against a fresh setup on the same
data, over this test's problems: worst relative gap 9.9e-16); where a member's gap is below 1e-14 the updated oracle's
workspace is compared as well."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

from _batch_parity import assert_parity, check_member_kinv, close, oracle, oracle_ws, rel, shape_family

pytestmark = pytest.mark.gpu

KW = dict(adaptive_rho_interval=10)
B = 4
# (engine, kind, n): both tiles and off the tile for the tiled engine, below / above 128 for the streamed one, the MPC shape for both
CASES = [("auto", "family", 12), ("auto", "family", 64), ("auto", "family", 65), ("auto", "family", 120), ("auto", "mpc", 120),
         ("streamed", "family", 40), ("streamed", "family", 150), ("streamed", "family", 300), ("streamed", "mpc", 120)]
IDS = ["%s-%s-%d" % c for c in CASES]
SEED1 = {65: 171}       # test 1's seed is 100 + n; at n = 65 that one leaves every member's rho where it was in the first solve
# (which matrices, full arrays or an index subset, how values are shared, scaling, warm_start): every value of every
# option with each engine and size.  sharing: "shared" (1-D values), "member" (shared at setup, [B, k] at the update),
# "setup_member" (Px_all / Ax_all at setup, then a shared update that writes every member)
COMBOS = [("PA", "full", "member", 10, 1), ("P", "idx", "shared", 10, 0), ("A", "full", "shared", 0, 1),
          ("A", "idx", "member", 10, 1), ("PA", "idx", "setup_member", 0, 0), ("P", "full", "member", 10, 0)]


def problem(kind, n, seed, nB=B):
    """triu(P) and A with sorted indices, Q, L, U and a point x0 every row holds (family) / None (MPC)."""
    if kind == "mpc":
        from osqp_amd.problems import mpc_batch
        s, Q, L, U = mpc_batch(batch=nB, seed0=seed)
        Q = Q + 0.05 * np.random.default_rng(seed).standard_normal(Q.shape)
        P, A, x0 = s["P"], s["A"], None
    else:
        P, A, Q, L, U, x0 = shape_family(n, 2 * n, nB, seed=seed)
    Pu = sparse.triu(P, format="csc"); Pu.sort_indices()
    A = sparse.csc_matrix(A); A.sort_indices()
    return Pu, A, Q, L, U, x0


def new_values(Pu, A, seed, per_member, nB=B):
    """New values tens of per cent away from the old: the diagonal of P grows by 1.3 - 1.9, the rest of P shrinks to
    0.5 - 1.0 (P stays diagonally dominant), A moves by 0.5 - 1.8."""
    rng = np.random.default_rng(seed)
    diag = Pu.indices == np.repeat(np.arange(Pu.shape[0]), np.diff(Pu.indptr))
    shp = (nB,) if per_member else ()
    fP = np.where(diag, rng.uniform(1.3, 1.9, shp + (Pu.nnz,)), rng.uniform(0.5, 1.0, shp + (Pu.nnz,)))
    fA = rng.uniform(0.5, 1.8, shp + (A.nnz,))
    return Pu.data * fP, A.data * fA


def with_values(M, v):
    return M if v is None else sparse.csc_matrix((v, M.indices, M.indptr), shape=M.shape)


def matrix_update_case(case, combo, seed):
    """Everything test_matrix_updates_follow_the_oracle (and the CPU check of its seeds) needs: setup arguments, the
    arguments of update_matrices, and per member those of the oracle's update."""
    (engine, kind, n), (which, form, sharing, scaling, warm) = case, combo
    Pu, A, Q, L, U, _ = problem(kind, n, seed)
    setup = dict(Px_all=None, Ax_all=None)
    if sharing == "setup_member":
        Px0, Ax0 = new_values(Pu, A, seed + 1, True)
        setup = dict(Px_all=Px0, Ax_all=Ax0)
    Pn, An = new_values(Pu, A, seed + 2, sharing == "member")
    rng = np.random.default_rng(seed + 3)
    upd = {}
    for nm, V, nnz in (("P", Pn, Pu.nnz), ("A", An, A.nnz)):
        if nm not in which:
            continue
        if form == "idx":
            idx = np.sort(rng.choice(nnz, max(1, nnz // 2), replace=False))
            if nm == "P":                                   # the whole diagonal moves, so that D does
                idx = np.union1d(idx, np.flatnonzero(Pu.indices == np.repeat(np.arange(Pu.shape[0]), np.diff(Pu.indptr))))
            upd[nm + "x"], upd[nm + "x_idx"] = np.ascontiguousarray(V[..., idx]), idx
        else:
            upd[nm + "x"] = V
    kw = dict(KW, scaling=scaling, warm_start=warm)

    def member_update(b):
        return {k: (v[b] if k in ("Px", "Ax") and v.ndim == 2 else v) for k, v in upd.items()}
    return Pu, A, Q, L, U, setup, upd, member_update, kw


def member_matrices(Pu, A, setup, b):
    return (with_values(Pu, None if setup["Px_all"] is None else setup["Px_all"][b]),
            with_values(A, None if setup["Ax_all"] is None else setup["Ax_all"][b]))


def oracle_update_gap(ou, of):
    """Largest relative distance (to the largest entry, as `close` measures) between two oracle workspaces."""
    return max([float(np.abs(ou[k] - of[k]).max() / np.abs(of[k]).max()) for k in ("D", "E", "Pv", "Av")] +
               [abs(ou["c"] - of["c"]) / abs(of["c"])])


def moved(a, b):
    """Largest relative change of an entry (D and E are positive)."""
    return float((np.abs(a - b) / np.abs(b)).max())


def _batch(engine, Pu, A, Q, L, U, **kw):
    import osqp_amd
    return osqp_amd.BatchOSQP().setup(Pu, A, Q, L, U, engine=engine, **kw)


def _np_of(engine, n):
    return (n + 31) // 32 * 32 if engine == "streamed" else (64 if n <= 64 else 128)


# ---------------------------------------------------------------------------------------------------------------
# 1. matrix updates follow the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", COMBOS, ids=["-".join(str(v) for v in c) for c in COMBOS])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matrix_updates_follow_the_oracle(gpu_lib, oracle_mod, case, combo):
    engine, kind, n = case
    Pu, A, Q, L, U, setup, upd, member_update, kw = matrix_update_case(case, combo, seed=SEED1.get(n, 100 + n))
    bs = _batch(engine, Pu, A, Q, L, U, **setup, **kw)
    sos = [oracle(oracle_mod, Pb, Q[b], Ab, L[b], U[b], **kw) for b, (Pb, Ab) in
           enumerate(member_matrices(Pu, A, setup, b) for b in range(B))]
    r = bs.solve()
    for b in range(B):
        assert_parity(r, b, sos[b].solve(), "first solve")
    assert np.any(r.rho_updates > 0), "no member's rho moved: keeping rho cannot be told from a new setup"
    w0 = [bs.member_workspace(b) for b in range(B)]
    assert bs.update_matrices(**upd) == 0
    w1 = [bs.member_workspace(b) for b in range(B)]
    for b in range(B):
        assert w1[b]["rho"] == w0[b]["rho"] and np.array_equal(w1[b]["ctype"], w0[b]["ctype"])
        if kw["scaling"]:                                   # the new values move the equilibration visibly
            assert moved(w1[b]["D"], w0[b]["D"]) > 0.02, (b, moved(w1[b]["D"], w0[b]["D"]))
            if "Ax" in upd:
                assert moved(w1[b]["E"], w0[b]["E"]) > 0.02, (b, moved(w1[b]["E"], w0[b]["E"]))
    if kw["scaling"]:       # (a single member's c can stay to the bit: it is 1 / |D q|_inf where q's scale beats P's, and that column's D need not move)
        assert any(w1[b]["c"] != w0[b]["c"] for b in range(B))
    r2 = bs.solve()
    for b in range(B):
        assert sos[b].update(**member_update(b)) == 0
        assert_parity(r2, b, sos[b].solve(), "after update_matrices %r" % (combo,))
    bs.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 2. the workspace after a matrix update
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[1] == "family" and c[2] != 64], ids=lambda c: "%s-%s-%d" % c)
def test_workspace_after_matrix_update(gpu_lib, oracle_mod, case):
    engine, kind, n = case
    Pu, A, Q, L, U, _ = problem(kind, n, seed=200 + n)
    Pn, An = new_values(Pu, A, 201 + n, True)
    bs = _batch(engine, Pu, A, Q, L, U, **KW)
    r = bs.solve()
    assert np.any(r.rho_updates > 0)
    w0 = [bs.member_workspace(b) for b in range(B)]
    assert bs.update_matrices(Px=Pn, Ax=An) == 0
    ran = 0
    for b in range(B):
        fresh = oracle(oracle_mod, with_values(Pu, Pn[b]), Q[b], with_values(A, An[b]), L[b], U[b], **KW)
        ran += check_member_kinv(bs, b, fresh, "after update_matrices", _np_of(engine, n))
        g = bs.member_workspace(b)
        assert g["rho"] == w0[b]["rho"], b
        assert np.array_equal(g["ctype"], w0[b]["ctype"]), b
        upd = oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **KW)
        upd.solve(); assert upd.update(Px=Pn[b], Ax=An[b]) == 0
        of, ou = oracle_ws(fresh), oracle_ws(upd)
        gap = oracle_update_gap(ou, of)
        print("member %d: oracle update-vs-fresh gap %.3g" % (b, gap))
        if gap < 1e-14:
            for k in ("D", "E", "Pv", "Av"):
                assert close(g[k], ou[k], 1e-14), (b, k)
            assert abs(g["c"] - ou["c"]) <= 1e-14 * abs(ou["c"]), b
    assert ran >= 1, "the K^-1 accuracy check ran for no member (cond(K) > 1e5 everywhere)"
    bs.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 3. a sequence, as an MPC loop issues it
# ---------------------------------------------------------------------------------------------------------------
# eps 1e-9: two runs that end `solved` then agree far below the 1e-6 the last comparison asks.  Adaptive rho is off in
# this test alone: at such an eps the adaptation acts on residual ratios at roundoff level, and over ten warm-started
# steps the oracle by itself then ends on different iteration counts when the new A values move by 1e-15 (measured
# with intervals of 10, 25 and 50: 12 to 40 of 48 replayed member sequences differ; with adaptive_rho = 0: none).
SEQ_KW = dict(adaptive_rho=0, eps_abs=1e-9, eps_rel=1e-9, max_iter=100000)
SEQ_CASES = [("auto", "mpc", 120), ("streamed", "mpc", 120), ("auto", "family", 64), ("streamed", "family", 150)]


def sequence_step(kind, Pu, A, Q, L, U, x0, step, seed):
    """Per-member A values, q, l, u of one step: A moves by +-20 %; the family's bounds move with A x0 (x0 stays
    feasible), the MPC's come from a drifting initial state."""
    rng = np.random.default_rng(1000 * seed + step)
    Ax = A.data * rng.uniform(0.8, 1.2, (B, A.nnz))
    Qs = Q * (1.0 + 0.1 * np.sin(step + np.arange(B))[:, None])
    if kind == "mpc":
        from osqp_amd.problems import mpc_batch
        _, _, Ls, Us = mpc_batch(batch=B, seed0=seed)
        drift = 1.0 + 0.03 * step
        nx = 6
        Ls = Ls.copy(); Us = Us.copy()
        Ls[:, :nx] *= drift; Us[:, :nx] *= drift
    else:
        Ls = np.empty_like(L); Us = np.empty_like(U)
        for b in range(B):
            d = with_values(A, Ax[b]) @ x0 - A @ x0
            Ls[b], Us[b] = L[b] + d, U[b] + d
    return Ax, Qs, Ls, Us


def shifted(x, y, kind):
    """The previous solution moved on by one stage (MPC: ten variables, six dynamics rows) / one entry."""
    return (np.roll(x, -10 if kind == "mpc" else -1), np.roll(y, -6 if kind == "mpc" else -1))


@pytest.mark.parametrize("case", SEQ_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_sequence_of_updates_and_warm_starts(gpu_lib, oracle_mod, case):
    engine, kind, n = case
    seed = 300 + n
    Pu, A, Q, L, U, x0 = problem(kind, n, seed)
    bs = _batch(engine, Pu, A, Q, L, U, **SEQ_KW)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **SEQ_KW) for b in range(B)]
    r = bs.solve()
    ros = [so.solve() for so in sos]
    for b in range(B):
        assert_parity(r, b, ros[b], "start")
    for step in range(10):
        Ax, Qs, Ls, Us = sequence_step(kind, Pu, A, Q, L, U, x0, step, seed)
        XY = [shifted(ro.x, ro.y, kind) for ro in ros]            # both sides start from the same point
        assert bs.update_matrices(Ax=Ax) == 0
        assert bs.update(Q=Qs, L=Ls, U=Us) == 0
        assert bs.warm_start(X=np.array([x for x, _ in XY]), Y=np.array([y for _, y in XY])) == 0
        r = bs.solve()
        for b, so in enumerate(sos):
            assert so.update(Ax=Ax[b]) == 0 and so.update(q=Qs[b], l=Ls[b], u=Us[b]) == 0
            assert so.warm_start(x=XY[b][0], y=XY[b][1]) == 0
            ros[b] = so.solve()
            assert_parity(r, b, ros[b], "step %d" % step)
            assert ros[b].info.status_val == 1, (step, b, ros[b].info.status)
    fresh = _batch(engine, Pu, A, Qs, Ls, Us, Ax_all=Ax, **SEQ_KW).solve()
    assert np.all(fresh.status_val == 1) and np.all(r.status_val == 1)
    for b in range(B):                                            # updating does not drift
        assert rel(r.x[b], fresh.x[b]) < 1e-6 and rel(r.y[b], fresh.y[b]) < 1e-6, (b, rel(r.x[b], fresh.x[b]), rel(r.y[b], fresh.y[b]))
    bs.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 4. update_rho
# ---------------------------------------------------------------------------------------------------------------
RHO_CASES = [("auto", "family", 65), ("auto", "mpc", 120), ("streamed", "family", 150)]


@pytest.mark.parametrize("case", RHO_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_update_rho(gpu_lib, oracle_mod, case):
    engine, kind, n = case
    Pu, A, Q, L, U, _ = problem(kind, n, seed=400 + n)
    bs = _batch(engine, Pu, A, Q, L, U, **KW)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **KW) for b in range(B)]
    r = bs.solve()
    for b in range(B):
        assert_parity(r, b, sos[b].solve(), "first solve")
    # a non-positive entry: 1, and nothing moves
    before = [bs.member_workspace(b)["rho"] for b in range(B)]
    assert bs.update_rho(np.array([0.5, -1.0, 0.5, 0.5])) == 1 and bs.update_rho(0.0) == 1
    assert [bs.member_workspace(b)["rho"] for b in range(B)] == before
    ran = 0
    for what, rho in (("scalar", 0.7), ("per member, clipped at both ends", np.array([1e-9, 5e7, 0.03, 2.5]))):
        assert bs.update_rho(rho) == 0
        want = np.clip(np.broadcast_to(rho, (B,)), 1e-6, 1e6)
        assert [bs.member_workspace(b)["rho"] for b in range(B)] == list(want), what
        r2 = bs.solve()
        for b in range(B):
            assert sos[b].update_rho(float(np.broadcast_to(rho, (B,))[b])) == 0
            ro = sos[b].solve()
            print(what, b, "iter", int(r2.iter[b]), ro.info.iter, "rho updates", int(r2.rho_updates[b]), ro.info.rho_updates,
                  "x", rel(r2.x[b], ro.x), "y", rel(r2.y[b], ro.y))
            assert_parity(r2, b, ro, what)
            assert r2.rho_updates[b] >= r.rho_updates[b]          # update_rho does not reset the count
            ran += check_member_kinv(bs, b, sos[b], what, _np_of(engine, n))
        r = r2
    assert ran >= 1
    bs.cleanup()


def test_update_rho_needs_one_round_streamed(gpu_lib, oracle_mod):
    kw = dict(adaptive_rho=0)
    Pu, A, Q, L, U, _ = problem("family", 150, seed=450)
    bs = _batch("streamed", Pu, A, Q, L, U, **kw)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **kw) for b in range(B)]
    bs.solve()
    assert bs.update_rho(0.5) == 0
    r = bs.solve()
    assert bs.rounds()[0] == 1
    for b in range(B):
        sos[b].solve(); sos[b].update_rho(0.5)
        assert_parity(r, b, sos[b].solve(), "rho 0.5")


# ---------------------------------------------------------------------------------------------------------------
# 5. warm_start
# ---------------------------------------------------------------------------------------------------------------
WS_CASES = [("auto", "family", 64), ("auto", "mpc", 120), ("streamed", "family", 150), ("streamed", "mpc", 120)]


@pytest.mark.parametrize("case", WS_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_warm_start(gpu_lib, oracle_mod, case):
    engine, kind, n = case
    kw = dict(KW, warm_start=0)
    Pu, A, Q, L, U, _ = problem(kind, n, seed=500 + n)
    bs = _batch(engine, Pu, A, Q, L, U, **kw)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **kw) for b in range(B)]
    r = bs.solve()
    ros = [so.solve() for so in sos]
    for b in range(B):
        assert_parity(r, b, ros[b], "cold")
        assert ros[b].info.status_val == 1
    Xo = np.array([ro.x for ro in ros]); Yo = np.array([ro.y for ro in ros])
    # from the oracle's optimum (the setting turns on), then x only and y only from another member's solution
    for what, X, Y in (("x and y", Xo, Yo), ("x only", Xo[::-1].copy(), None), ("y only", None, Yo[::-1].copy())):
        assert bs.warm_start(X=X, Y=Y) == 0
        r2 = bs.solve()
        for b, so in enumerate(sos):
            assert so.warm_start(x=None if X is None else X[b], y=None if Y is None else Y[b]) == 0
            ro = so.solve()
            assert_parity(r2, b, ro, what)
            if what == "x and y":
                assert ro.info.iter <= ros[b].info.iter, (b, ro.info.iter, ros[b].info.iter)      # the start helps the oracle itself
    # a handle that has not solved yet, started from another member's solution
    cold = _batch(engine, Pu, A, Q, L, U, **kw)
    assert cold.warm_start(X=Xo[::-1].copy(), Y=Yo[::-1].copy()) == 0
    rc = cold.solve()
    for b in range(B):
        so = oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **kw)
        so.warm_start(x=Xo[B - 1 - b], y=Yo[B - 1 - b])
        assert_parity(rc, b, so.solve(), "cold handle")
    with pytest.raises(ValueError):
        bs.warm_start(X=Xo[:, :-1])
    bs.cleanup(); cold.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------
def _c_update(bs, Px, Pi, Pn, Ax, Ai, An):
    """osqp_amd_batch_update_matrices called directly (no Python-side checks), shared values."""
    from osqp_amd import abi
    from osqp_amd.batch import _p
    ip = lambda a: C.cast(None, abi.c_int_p) if a is None else abi.iptr(a)
    return int(bs._lib.osqp_amd_batch_update_matrices(bs._h, _p(Px), ip(Pi), Pn, 0, _p(Ax), ip(Ai), An, 0))


@pytest.mark.parametrize("case", [("auto", "family", 65), ("streamed", "family", 150)], ids=lambda c: "%s-%s-%d" % c)
def test_refusals_write_nothing(gpu_lib, oracle_mod, case):
    engine, kind, n = case
    Pu, A, Q, L, U, _ = problem(kind, n, seed=600 + n)
    bs = _batch(engine, Pu, A, Q, L, U, **KW)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **KW) for b in range(B)]
    r = bs.solve()
    for b in range(B):
        assert_parity(r, b, sos[b].solve(), "first solve")
    nP, nA = Pu.nnz, A.nnz
    bigP, bigA = 7.0 * np.ones(nP + 1), 7.0 * np.ones(nA + 1)
    zP, zA = np.zeros(nP + 1, np.int64), np.zeros(nA + 1, np.int64)
    assert _c_update(bs, bigP, zP, nP + 1, None, None, 0) == 1                       # P_n > nnzP
    assert _c_update(bs, None, None, 0, bigA, zA, nA + 1) == 2                       # A_n > nnzA
    assert _c_update(bs, bigP, zP, 2, bigA, zA, nA + 1) == 2                         # a good P part is not written either
    for bad in (np.array([0, nP], np.int64), np.array([-1, 0], np.int64)):           # OSQP_DATA_VALIDATION_ERROR
        assert _c_update(bs, bigP, bad, 2, None, None, 0) == 1
    for bad in (np.array([0, nA], np.int64), np.array([-1, 0], np.int64)):
        assert _c_update(bs, bigP, zP, 2, bigA, bad, 2) == 1
    for kwargs in (dict(Px=np.ones(nP + 1)), dict(Ax=np.ones((B + 1, nA))), dict(Ax=np.ones((B, nA - 1))),
                   dict(Px=np.ones(3), Px_idx=[0, 1]), dict(Ax=np.ones(2), Ax_idx=[0, nA]), dict(Px=np.ones(2), Px_idx=[-1, 0]),
                   dict(Px=np.ones((2, 2, 2))), dict(Ax_idx=[0]), dict(Ax=np.ones((B, 2)), Ax_idx=[[0, 1]] * B)):
        with pytest.raises(ValueError):
            bs.update_matrices(**kwargs)
    for v in (np.ones(B + 1), np.ones((B, 1))):
        with pytest.raises(ValueError):
            bs.update_rho(v)
    r2 = bs.solve()
    for b in range(B):
        assert_parity(r2, b, sos[b].solve(), "after refused updates")
    bs.cleanup()


@pytest.mark.parametrize("case", [("auto", "family", 65), ("streamed", "family", 150)], ids=lambda c: "%s-%s-%d" % c)
def test_nonconvex_update_is_refused_and_heals(gpu_lib, oracle_mod, capfd, case):
    engine, kind, n = case
    bad = 2
    Pu, A, Q, L, U, _ = problem(kind, n, seed=650 + n)
    bs = _batch(engine, Pu, A, Q, L, U, **KW)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **KW) for b in range(B)]
    r = bs.solve()
    for b in range(B):
        assert_parity(r, b, sos[b].solve(), "first solve")
    good, _ = new_values(Pu, A, 651 + n, True)
    diag = Pu.indices == np.repeat(np.arange(n), np.diff(Pu.indptr))
    Px = good.copy()
    # far below -(sigma + A' rho A): rho <= 1e6 and |A| <= ~1e2 in this family bound A' rho A's diagonal by 3e10 per row entry
    Px[bad, diag] = -1e13
    capfd.readouterr()
    assert bs.update_matrices(Px=Px) == 5                                            # OSQP_NONCVX_ERROR
    assert "QP %d of the batch" % bad in capfd.readouterr().err
    with pytest.raises(RuntimeError, match=r"\(5\)"):
        bs.solve()
    assert bs.update_matrices(Px=good) == 0
    r2 = bs.solve()
    for b in range(B):
        assert sos[b].update(Px=good[b]) == 0
        assert_parity(r2, b, sos[b].solve(), "healed")
    bs.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 7. n > 128 with engine="auto": one single-QP engine per member
# ---------------------------------------------------------------------------------------------------------------
def test_per_member_path_above_128(gpu_lib, oracle_mod):
    n = 150
    Pu, A, Q, L, U, _ = problem("family", n, seed=700)
    bs = _batch("auto", Pu, A, Q, L, U, **KW)
    assert bs._many is not None
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **KW) for b in range(B)]
    r = bs.solve()
    ros = [so.solve() for so in sos]
    for b in range(B):
        assert_parity(r, b, ros[b], "first solve")
    Pn, An = new_values(Pu, A, 701, True)
    rho = np.array([0.4, 0.05, 1.5, 0.2])
    X = np.array([ro.x for ro in ros])[::-1].copy(); Y = np.array([ro.y for ro in ros])[::-1].copy()
    assert bs.update_matrices(Px=Pn[0], Ax=An) == 0 and bs.update_rho(rho) == 0 and bs.warm_start(X=X, Y=Y) == 0
    r2 = bs.solve()
    for b, so in enumerate(sos):
        assert so.update(Px=Pn[0], Ax=An[b]) == 0 and so.update_rho(rho[b]) == 0 and so.warm_start(x=X[b], y=Y[b]) == 0
        assert_parity(r2, b, so.solve(), "after the update round")
    assert bs.update_rho(-1.0) == 1
    with pytest.raises(ValueError):
        bs.update_matrices(Ax=An[:, :-1])
    bs.cleanup()
