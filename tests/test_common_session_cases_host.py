"""tests/_common_session_cases.py and the handle's-life methods of tests/_common_reference.py on the CPU: `solve(members=)`,
`update` and `warm_start` of the long-double loop are anchored on the oracle at B = 1, and every case of
tests/test_gpu_batch_common_sessions.py is shown to hold what that file takes for granted -- decisions far from their
thresholds in every call of a session, a double-precision run that decides alike, the probe ratios of the verdict case, a
check point inside the probed iterations, the shape of each first pack."""
import numpy as np
import pytest

from _batch_parity import oracle, rel
from _common_cases import ADAPTIVE_CASES, adaptive_family, qhat, row_classes
from _common_members_cases import GROUP, MIN_ITER, PACK_CHUNK, packs_of
from _common_reference import (ANCHOR_BAR, MARGIN_ADAPT, MARGIN_CHECK, RHO_BAR, RHO_DIFF_MEASURED, loop_case, margins,
                               reference_for)
from _common_session_cases import (CUT_B, CUT_COLD_OUT, GENERAL_S1, GENERAL_S2, GEOMETRY, GEOMETRY_PROVED, PROBING_B,
                                   PROBING_EASY, PROBING_REFINE_TOL, PROBING_RHO0, REFINE_TOL, VERDICT_B, VERDICT_N1, VERDICT_S, VERDICT_SETTINGS,
                                   first_pack_src, geometry_case, geometry_reference, probe_ratios, probe_replay, session_case,
                                   session_reference, verdict_case, verdict_reference)

FIELDS = ("x", "y", "status_val", "iter", "rho_updates", "rho", "obj_val")


# ---- the reference's new methods -------------------------------------------------------------------------------------------
def test_all_members_listed_is_the_full_solve(oracle_mod):
    """members=None and members=np.arange(B) give the bits of the plain solve, call after call (case A1, then
    update_rho(0.3) and a warm second solve): same results, same moves, same log of decisions."""
    P, A, Q, L, U, kw = loop_case("A1")
    a, b = (reference_for(oracle_mod, P, A, Q, L, U, **kw) for _ in range(2))
    for call in range(2):
        ra, rb = a.solve(), b.solve(members=np.arange(Q.shape[0]))
        for k in FIELDS:
            assert np.array_equal(getattr(ra, k), getattr(rb, k)), (call, k)
        assert ra.moves == rb.moves and ra.final_rho == rb.final_rho and np.array_equal(rb.listed, np.arange(Q.shape[0]))
        assert ra.moves
        a.update_rho(0.3); b.update_rho(0.3)
    assert a.decisions == b.decisions


def test_unlisted_members_stay(oracle_mod):
    """A subset solve leaves x, z, y, status, iter, rho, rho_updates and the stored result of every other member alone,
    and its rho estimate is taken over the listed members only: it equals the run of a reference that holds only them
    when the scaling is given (the same `ws`)."""
    from _common_reference import CommonReference
    P, A, Q, L, U, kw = loop_case("A1")
    S, rest = np.array([1, 3]), np.array([0, 2, 4])
    ref = reference_for(oracle_mod, P, A, Q, L, U, **kw)
    first = ref.solve(members=rest)
    state = [v.copy() for v in (ref.x, ref.z, ref.y)]
    ref.update_rho(0.1)
    r = ref.solve(members=S)
    for k in FIELDS:
        assert np.array_equal(getattr(r, k)[rest], getattr(first, k)[rest]), k
    for v, w in zip(state, (ref.x, ref.z, ref.y)):
        assert np.array_equal(v[rest], w[rest])
    assert np.all(r.iter[S] > 0) and np.all(r.status_val[S] == 1) and np.array_equal(r.listed, S)
    alone = CommonReference(ref.ws, Q[S], L[S], U[S], **kw).solve()
    for k in FIELDS:
        assert np.array_equal(getattr(r, k)[S], getattr(alone, k)), k
    assert r.moves == alone.moves and r.moves


def _assert_anchor(ro, rr, orho, tag):
    got = (int(rr.status_val[0]), int(rr.iter[0]), int(rr.rho_updates[0]))
    assert got == (ro.info.status_val, ro.info.iter, ro.info.rho_updates), tag + (got, ro.info.status_val, ro.info.iter)
    dx, dy = rel(rr.x[0], ro.x), rel(rr.y[0], ro.y)
    dobj = abs(rr.obj_val[0] - ro.info.obj_val) / max(1.0, abs(ro.info.obj_val))
    drho = abs(rr.final_rho - orho) / orho
    print(tag, "x %.1e y %.1e obj %.1e rho %.1e" % (dx, dy, dobj, drho))
    assert dx <= ANCHOR_BAR and dy <= ANCHOR_BAR and dobj <= ANCHOR_BAR, tag + (dx, dy, dobj)
    assert drho <= RHO_DIFF_MEASURED, tag + (drho,)


@pytest.mark.parametrize("warm", [False, True], ids=["update", "update-warm_start"])
@pytest.mark.parametrize("scaled_termination", [0, 1])
@pytest.mark.parametrize("n,m,qscale", ADAPTIVE_CASES)
def test_update_and_warm_start_are_the_oracles(oracle_mod, n, m, qscale, scaled_termination, warm):
    """B = 1, where the common scaling is the member's own: a solve cut at max_iter = 20, `update` of q, l, u (member
    b + 1's data on member b's classes: the bounds move with the feasible point), then a solve to the end (max_iter
    back at 4000); the same with warm_start(x, y) between the update and the solve.  Status, iter and rho_updates
    identical (rho_updates restarts at the update), x, y and the objective under ANCHOR_BAR."""
    kw = dict(adaptive_rho_interval=10, scaled_termination=scaled_termination, max_iter=20)
    P, A, Q, L, U, X0 = adaptive_family(n, m, 5, qscale)
    rng = np.random.default_rng(n + 10 * scaled_termination + warm)
    moved = reset = 0
    for b in range(3):
        own = oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw)
        ref = reference_for(oracle_mod, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1], keep_status=True, **kw)
        ro, rr = own.solve(), ref.solve()
        _assert_anchor(ro, rr, float(own.settings().rho), ("cut", n, scaled_termination, b))
        assert ro.info.status_val == -2
        reset += ro.info.rho_updates
        shift = A @ (X0[b + 1] - X0[b])
        q2, l2, u2 = 0.8 * Q[b + 1], L[b] + shift, U[b] + shift
        assert own.update(q=q2, l=l2, u=u2) == 0
        ref.update(Q=q2[None], L=l2[None], U=u2[None])
        assert ref.rho_updates[0] == 0 and ref.status[0] == 0
        if warm:
            x, y = X0[b + 1] + 0.05 * rng.standard_normal(n), 0.1 * rng.standard_normal(m)
            assert own.warm_start(x=x, y=y) == 0
            ref.warm_start(X=x[None], Y=y[None])
        own.update_settings(max_iter=4000)
        ref.st["max_iter"] = 4000
        ro, rr = own.solve(), ref.solve()
        _assert_anchor(ro, rr, float(own.settings().rho), ("after the update", n, scaled_termination, b, warm))
        assert ro.info.status_val == 1
        moved += ro.info.rho_updates
    assert moved >= 1 and reset >= 1                     # rho_updates had something to restart from, and counts again


@pytest.mark.parametrize("n,m,qscale", ADAPTIVE_CASES)
def test_warm_start_turns_the_setting_on(oracle_mod, n, m, qscale):
    """B = 1 with the setting warm_start = 0 and max_iter = 20: a second solve repeats the first from zero; warm_start(x, y)
    turns the setting on (osqp_warm_start does), so the solve after it starts from x, y and the one after that continues.
    Every solve against the oracle's."""
    kw = dict(adaptive_rho_interval=10, scaled_termination=1, max_iter=20, warm_start=0)
    P, A, Q, L, U, X0 = adaptive_family(n, m, 5, qscale)
    rng = np.random.default_rng(n)
    own = oracle(oracle_mod, P, Q[0], A, L[0], U[0], **kw)
    ref = reference_for(oracle_mod, P, A, Q[:1], L[:1], U[:1], keep_status=True, **kw)
    out = []
    for call in range(4):
        if call == 2:
            x, y = X0[0] + 0.05 * rng.standard_normal(n), 0.1 * rng.standard_normal(m)
            assert own.warm_start(x=x, y=y) == 0
            ref.warm_start(X=x[None], Y=y[None])
            assert own.settings().warm_start == 1 and ref.st["warm_start"] == 1
        ro, rr = own.solve(), ref.solve()
        _assert_anchor(ro, rr, float(own.settings().rho), ("warm_start = 0, solve %d" % call, n))
        out.append(rr)
    # (rho has moved, so the second cold run is not the first; both start from zero -- the oracle agrees above)
    assert not np.array_equal(out[2].x, out[1].x) and not np.array_equal(out[3].x, out[2].x)


def test_update_reforms_k_when_the_common_class_moves(oracle_mod):
    """An inequality row of every member closed to an equality: the reference re-forms K with the rho it holds; rows whose
    class differs between members are refused."""
    P, A, Q, L, U, kw = loop_case("A1")
    ref = reference_for(oracle_mod, P, A, Q, L, U, **kw)
    ref.solve()
    i = int(np.flatnonzero(ref.ctype == 0)[0])
    K0, rho = ref.K.copy(), ref.rho
    L2 = L.copy(); L2[:, i] = U[:, i]
    ref.update(L=L2)
    assert ref.ctype[i] == 1 and ref.rho == rho and not np.array_equal(ref.K, K0) and len(ref.conds) >= 2
    a = ref.A[i].astype(np.float64)
    assert np.allclose((ref.K - K0).astype(np.float64), float(rho) * 999.0 * np.outer(a, a), rtol=1e-12, atol=0)
    L3 = L2.copy(); L3[0, i] = L[0, i]
    with pytest.raises(AssertionError, match="classes not common"):
        ref.update(L=L3)


def _assert_decides_alike(r, d, listed, tag):
    """The plain-double run d against the long-double run r on the listed members: the same decisions, and results within
    the bars the GPU tests set."""
    for f in ("status_val", "iter", "rho_updates"):
        assert np.array_equal(getattr(r, f), getattr(d, f)), tag + (f,)
    assert r.moves == d.moves
    drho = (np.abs(d.rho[listed] - r.rho[listed]) / r.rho[listed]).max()
    dx = max(rel(d.x[b], r.x[b]) for b in listed); dy = max(rel(d.y[b], r.y[b]) for b in listed)
    dobj = (np.abs(d.obj_val - r.obj_val) / np.maximum(1.0, np.abs(r.obj_val)))[listed].max()
    print(*tag, "double against long double: rho %.1e x %.1e y %.1e obj %.1e" % (drho, dx, dy, dobj))
    assert drho <= RHO_BAR and dx <= 1e-6 and dy <= 1e-6 and dobj <= 1e-8, tag + (drho, dx, dy, dobj)


# ---- B1, B2: the sessions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general", "cut", "cut-cold", "probing"])
def test_session_decisions_and_conditioning(oracle_mod, name):
    """In every call of the session: adaptation decisions at least MARGIN_ADAPT and termination decisions at least
    MARGIN_CHECK from their thresholds; the same loop in plain double decides alike and ends within the bars of the GPU
    tests on the listed members."""
    ref, runs = session_reference(oracle_mod, name)
    _, runs64 = session_reference(oracle_mod, name, np.float64)
    for call, ((k, r), (_, d)) in enumerate(zip(runs, runs64), 1):
        ma, mc = margins(ref, call)
        S = r.listed
        print(name, "step", k, "listed", S.size, "margins %.3g %.3g" % (ma, mc), "moves", r.moves, "iter",
              sorted(set(r.iter[S].tolist())), "status", sorted(set(r.status_val[S].tolist())))
        assert ma >= MARGIN_ADAPT and mc >= MARGIN_CHECK, (name, k, ma, mc)
        _assert_decides_alike(r, d, S, (name, "step", k))
    assert len(ref.conds) == 1 + sum(len(r.moves) for _, r in runs) + (name == "general")     # (+ update_rho)


def test_general_session(oracle_mod):
    """q^ of the batch is q^ of neither listed set; S2 overlaps S1 (warm for the overlap, cold for the rest); the update
    keeps every row's class; rho moves in a subset solve and binds the members solved next; every member ends solved."""
    (P, A, Q, L, U), kw, steps = session_case("general")
    assert np.any(qhat(Q) != qhat(Q[GENERAL_S1])) and np.any(qhat(Q) != qhat(Q[GENERAL_S2]))
    over = np.intersect1d(GENERAL_S1, GENERAL_S2)
    assert 0 < over.size < GENERAL_S1.size
    ref, runs = session_reference(oracle_mod, "general")
    new = steps[2][1]
    assert np.array_equal(new["Q"], Q * 1.25) and np.any(new["L"] != L)
    for b in range(Q.shape[0]):
        assert np.array_equal(row_classes(new["L"][b], new["U"][b], ref.ws["E"]), ref.ws["ctype"]), b
    by_step = dict(runs)
    assert sorted(by_step) == [0, 1, 3, 5, 6]
    for k, r in runs:
        assert np.all(r.status_val[r.listed] == 1), k
    assert by_step[0].moves and by_step[1].moves and by_step[3].moves and by_step[5].moves
    # the overlap starts step 1 warm: solved members need fewer iterations than the cold ones beside them
    r0, r1 = by_step[0], by_step[1]
    assert np.median(r1.iter[over]) <= MIN_ITER < np.median(r1.iter[np.setdiff1d(GENERAL_S2, over)])
    # rho_updates: step 1 counts on for the overlap, restarts nowhere; the update sets all to 0
    assert np.all(r1.rho_updates[over] >= r0.rho_updates[over])
    assert np.all(by_step[3].rho_updates[np.setdiff1d(np.arange(Q.shape[0]), GENERAL_S1)] == 0)
    first = [e for e in ref.decisions if e["kind"] == "adapt" and e["call"] == 4][0]
    assert first["rho"] == 0.3                           # step 5 starts from update_rho's value


def test_cut_session(oracle_mod):
    """Members stop unsolved at max_iter = 40 and later subsets continue them; the warm_start in the middle changes what
    follows; in the cold twin the listed members repeat their first solve to the bit."""
    _, runs = session_reference(oracle_mod, "cut")
    by_step = dict(runs)
    r0, r1 = by_step[0], by_step[1]
    unsolved0 = r0.listed[r0.status_val[r0.listed] != 1]
    assert unsolved0.size >= 5 and np.intersect1d(unsolved0, r1.listed).size >= 3
    cont = np.intersect1d(unsolved0, r1.listed)
    assert np.any(r1.status_val[cont] == 1)              # somebody unsolved at 40 is solved by the continuation
    for k, r in runs:
        assert set(r.status_val[r.listed].tolist()) <= {1, 2, -2}, k
        assert np.all((r.iter[r.listed] == MIN_ITER) | (r.iter[r.listed] == 40)), k
    assert (by_step[3].status_val[by_step[3].listed] != 1).any()       # the given start is no solution
    (P, A, Q, L, U), kw, steps = session_case("cut")
    assert steps[2][0] == "warm_start" and np.any(steps[2][2] != 0)
    # the twin
    refc, (c0, c1, c3, c4) = session_reference(oracle_mod, "cut-cold")
    c0, c1, c3, c4 = c0[1], c1[1], c3[1], c4[1]
    S = c1.listed
    assert session_case("cut-cold")[1]["warm_start"] == 0 and not np.intersect1d(S, CUT_COLD_OUT).size
    # after warm_start(X, Y) the setting is on: the last solve continues the evens, it does not repeat their cold run
    assert refc.st["warm_start"] == 1 and np.array_equal(c4.listed, S)
    both = np.intersect1d(c3.listed, S)
    assert not np.array_equal(c4.x[S], c1.x[S]) and (c4.status_val[both] == 1).sum() > (c3.status_val[both] == 1).sum()
    for f in FIELDS:
        assert np.array_equal(getattr(c1, f)[S], getattr(c0, f)[S]), f
        rest = np.setdiff1d(np.arange(CUT_B), S)
        assert np.array_equal(getattr(c1, f)[rest], getattr(c0, f)[rest]), f
    assert (c0.status_val[S] != 1).any()                 # a warm continuation would have gone further
    assert np.all(c1.iter[list(CUT_COLD_OUT)] == 0)


# ---- B3: the verdict case --------------------------------------------------------------------------------------------------
def test_verdict_case(oracle_mod):
    """The float64 replay of the first four probes (Gauss-Jordan without pivoting): every ratio of a member of S at most
    refine_tol / 10, every other member at least 10 refine_tol at some probe -- with the engine's default refine_tol.
    K^-1 keeps the blocks apart exactly, the members of S keep block 2 at exactly zero, and the full reference run
    solves every member with its decisions clear of the thresholds."""
    P, A, Q, L, U = verdict_case()
    rest = np.setdiff1d(np.arange(VERDICT_B), VERDICT_S)
    ratios, cond, kept = probe_ratios(P, A, Q, L, U)
    print("cond(K) %.2e" % cond, "ratios of S at most %.2e" % ratios[:, VERDICT_S].max(), "of the others, per member, at most",
          ["%.2e" % v for v in ratios[:, rest].max(axis=0)], "at least %.2e" % ratios[:, rest].min())
    assert kept and cond >= 1e4
    assert ratios.shape == (4, VERDICT_B)
    assert np.all(ratios[:, VERDICT_S] <= REFINE_TOL / 10)
    assert np.all(ratios[:, rest].max(axis=0) >= 10 * REFINE_TOL)
    assert VERDICT_SETTINGS["scaling"] == 0 and not VERDICT_SETTINGS["adaptive_rho"]
    ref, r = verdict_reference(oracle_mod)
    assert np.all(ref.D == 1) and np.all(ref.E == 1) and ref.c == 1 and float(ref.rho) == 0.1
    assert np.all(r.status_val == 1) and margins(ref)[1] >= MARGIN_CHECK, margins(ref)
    assert not r.x[VERDICT_S, VERDICT_N1:].any() and np.all(np.abs(r.x[rest, VERDICT_N1:]).max(axis=1) > 0)
    for b in range(VERDICT_B):
        assert np.array_equal(row_classes(L[b], U[b], np.ones(L.shape[1])), ref.ctype), b
    print("iter", r.iter.tolist(), "termination margin %.3g" % margins(ref)[1])
    _assert_decides_alike(r, verdict_reference(oracle_mod, np.float64)[1], np.arange(VERDICT_B), ("verdict case",))


# ---- B4: a pack inside the probed iterations ---------------------------------------------------------------------------------
def test_probing_case(oracle_mod):
    """rho moves at iteration 24 and nowhere else before max_iter = 45, so the probed iterations are 1 to 4 and 25 to 28.
    The float64 replay (Gauss-Jordan without pivoting): every ratio of iterations 1 to 4 is at most refine_tol / 10 -- the
    verdict is still off when K is inverted at 24 --, and in iteration 25, where every member still runs, as in 25 to 28
    among the members that run on, some ratio is at least 10 refine_tol: the verdict turns on in that window and nowhere
    else.  Enough members end at the check point 25 for the rule to pack there, with that verdict open."""
    (P, A, Q, L, U), kw, _ = session_case("probing")
    tol = PROBING_REFINE_TOL
    assert kw["adaptive_rho_interval"] == 24 and kw["max_iter"] < 48 and Q.shape[0] == PROBING_B >= GROUP + 1
    ref, ((_, r),) = session_reference(oracle_mod, "probing")
    assert r.moves == [24]
    it0, src = first_pack_src(r.iter)
    assert it0 == 25 and 24 < it0 <= 24 + 4
    assert np.all(r.iter[PROBING_EASY] == 25) and np.all(r.iter[src] == kw["max_iter"]) and set(r.status_val.tolist()) == {1, -2}
    assert packs_of(r.iter)[0] >= 1
    at24 = [e for e in ref.decisions if e["kind"] == "adapt" and e["iter"] == 24][0]
    assert at24["moved"] and at24["rho"] == PROBING_RHO0
    f = lambda v: np.asarray(v, dtype=np.float64)
    ratios, conds, _ = probe_replay(f(ref.P), f(ref.A), f(ref.q), f(ref.l), f(ref.u), ref.ctype, PROBING_RHO0, iters=28,
                                    windows=((1, 4), (25, 28)), moves={24: at24["value"]})
    later = ratios[24:28][:, src]
    print("rho %.3g -> %.3g" % (at24["rho"], at24["value"]), "cond(K) %.2e -> %.2e" % tuple(conds), "ratios of iterations 1-4 at most "
          "%.2e" % ratios[:4].max(), "iteration 25 at most %.2e" % ratios[24].max(), "25-28, members that run on, per iteration at most",
          ["%.2e" % v for v in later.max(axis=1)], "ending at 25:", int((r.iter == 25).sum()), "packs", packs_of(r.iter))
    assert ratios[:4].max() <= tol / 10
    assert ratios[24].max() >= 10 * tol and later.max() >= 10 * tol


# ---- B5: pack geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_geometry_case(oracle_mod, name):
    from _batch_parity import oracle_ws
    from _common_cases import FIXED, common_oracle
    P, A, Q, L, U, hard = geometry_case(name)
    B = Q.shape[0]
    easy = np.setdiff1d(np.arange(B), hard)
    assert np.array_equal(qhat(Q), qhat(Q[hard]))
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **FIXED))
    for b in range(B):
        assert np.array_equal(row_classes(L[b], U[b], ws["E"]), ws["ctype"]), (name, b)
    ref, r = geometry_reference(oracle_mod, name)
    assert np.all(r.status_val == 1) and np.all(r.iter[easy] == MIN_ITER)
    assert margins(ref)[1] >= MARGIN_CHECK, margins(ref)
    _assert_decides_alike(r, geometry_reference(oracle_mod, name, np.float64)[1], np.arange(B), (name,))
    it0, src = first_pack_src(r.iter)
    packs, ended = packs_of(r.iter)
    print(name, "first pack at", it0, "leaves", src.size, "src[0]", src[0], "packs", packs, "ended", ended, "margin %.3g" % margins(ref)[1])
    assert it0 == MIN_ITER and (src.size, packs, ended) == GEOMETRY_PROVED[name]
    if name.startswith("shift-1"):
        assert np.array_equal(src, np.arange(src.size) + 1) and src.size == B - 1          # src[c] = c + 1 over a whole row
    if name == "shift-1":
        assert B == GROUP + 1
    if name == "shift-1-chunk":
        assert src.size > PACK_CHUNK                                                    # the shift crosses the chunk boundary
    if name == "back":
        assert B >= 600 and src[0] >= PACK_CHUNK
    if name == "to-256":
        assert src.size == PACK_CHUNK
    if name == "to-257":
        assert src.size == PACK_CHUNK + 1
