"""GPU tests of the common-K engine's columns (batch_common.h, `bc_solve` in batch.hip): the solve packs its running
columns to the front once a whole group of 64 has finished (k_bc_pack), and `solve(members=...)` solves chosen members
as the columns of a shorter solve, leaving every other member as it was.

Every comparison is an identity: the header promises that a member's bits do not depend on its position in the batch
or on the batch's size, so a packed run equals an unpacked one (OSQP_AMD_BATCH_COMMON_PACK=0, read at setup), a chosen
member equals itself in a handle of the chosen members alone (same scaling: tests/_common_members_cases.py), and an
unlisted member equals what it was.  `_same` compares the bits of x, y, info_raw and both certificates (the fills of an
infeasible member included).  tests/test_common_members_cases_host.py proves on the CPU where the members of the wave
cases end and how many packs that makes."""
import numpy as np
import pytest
from scipy import sparse

from _common_cases import ADAPTIVE, FIXED, MIXED, common_family, mixed_family, qhat
from _common_members_cases import (ADAPTIVE_SUBSET_B, WAVE_M, WAVE_N, WAVE_PROVED, WAVE_SEED, WAVES, adaptive_subset_case,
                                   packs_of, subsets, wave_case, wave_reference)
from _common_reference import loop_case

pytestmark = pytest.mark.gpu

ARRAYS = ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert")


def _common(P, A, Q, L, U, **kw):
    import osqp_amd
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **kw)


def _unpacked(monkeypatch, *args, **kw):
    """A handle set up with packing switched off."""
    monkeypatch.setenv("OSQP_AMD_BATCH_COMMON_PACK", "0")
    try:
        return _common(*args, **kw)
    finally:
        monkeypatch.delenv("OSQP_AMD_BATCH_COMMON_PACK")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(r1, r2, i1=slice(None), i2=slice(None), what=""):
    for k in ARRAYS:
        assert np.array_equal(_bits(getattr(r1, k)[i1]), _bits(getattr(r2, k)[i2])), (what, k)


# ---- packing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WAVES))
def test_identity_across_packing(gpu_lib, oracle_mod, monkeypatch, name):
    """One pack ("one"), packs composed ("two"), more running columns than a chunk of k_bc_pack ("chunk") and packs to
    exactly 64, 65 and 17 columns: the packed solve equals the unpacked one and, on the hard members, a handle of the hard
    members alone; packs, the columns at the end and every member's iteration count are the proved ones."""
    B, h, drop = WAVES[name]
    P, A, Q, L, U, hard = wave_case(B, h, drop)
    _, rr = wave_reference(oracle_mod, B, h, drop)
    bs = _common(P, A, Q, L, U, **FIXED)
    r = bs.solve()
    cols = bs.columns()
    print(name, cols, "iterations", dict(zip(*np.unique(r.iter, return_counts=True))))
    assert np.array_equal(r.iter, rr.iter) and np.array_equal(r.status_val, rr.status_val)
    packs, ended = packs_of(rr.iter)
    assert cols == (B, packs, ended) and packs == WAVE_PROVED[name][1] >= 1
    off = _unpacked(monkeypatch, P, A, Q, L, U, **FIXED)
    _same(r, off.solve(), what=name + " against the unpacked solve")
    assert off.columns() == (B, 0, B)
    alone = _common(P, A, Q[hard], L[hard], U[hard], **FIXED)
    _same(r, alone.solve(), i1=hard, what=name + " against the hard members alone")
    for s in (bs, off, alone):
        s.cleanup()


@pytest.mark.parametrize("name", ["A2-scaled", "A2-default"])
def test_adaptive_rho_across_packing(gpu_lib, monkeypatch, name):
    """B = 65 packs as soon as one member ends; the estimate is taken over the same members in the same order, so rho,
    rho_updates (both in info_raw), iter and the inversions are those of the unpacked run."""
    P, A, Q, L, U, kw = loop_case(name)
    bs, off = _common(P, A, Q, L, U, **kw), _unpacked(monkeypatch, P, A, Q, L, U, **kw)
    r, ro = bs.solve(), off.solve()
    print(name, bs.columns(), bs.rounds(), "rho_updates", r.rho_updates.max())
    _same(r, ro, what=name)
    assert bs.rounds() == off.rounds() and bs.rounds()[0] >= 2
    assert bs.columns().packs >= 1 and bs.columns().ended < 65 and off.columns() == (65, 0, 65)
    assert bs.member_workspace(0)["rho"] == off.member_workspace(0)["rho"]
    bs.cleanup(); off.cleanup()


def _mixed_among_easy():
    """mixed_family()'s six members at scattered places of a batch of 70 whose other members are easy: q = 0 and bounds of
    member 0's kinds around 0 (an equality row 0 = 0, a finite bound at -1 / +1), so they end at iteration 25 and the
    batch's q^ is that of the six."""
    P, A, Q6, L6, U6 = mixed_family()
    B, at = 70, np.array([3, 17, 29, 41, 55, 68])
    eq = L6[0] == U6[0]
    lo = np.where(eq, 0.0, np.where(np.isfinite(L6[0]), -1.0, -np.inf))
    hi = np.where(eq, 0.0, np.where(np.isfinite(U6[0]), 1.0, np.inf))
    Q = np.zeros((B, Q6.shape[1])); L = np.tile(lo, (B, 1)); U = np.tile(hi, (B, 1))
    Q[at], L[at], U[at] = Q6, L6, U6
    assert np.array_equal(qhat(Q), qhat(Q6))
    return P, A, Q, L, U, Q6, L6, U6, at


def test_statuses_land_on_their_member_after_a_pack(gpu_lib, monkeypatch):
    from osqp_amd import abi
    P, A, Q, L, U, Q6, L6, U6, at = _mixed_among_easy()
    kw = dict(FIXED, max_iter=2000)
    bs, off, six = _common(P, A, Q, L, U, **kw), _unpacked(monkeypatch, P, A, Q, L, U, **kw), _common(P, A, Q6, L6, U6, **kw)
    r, ro, r6 = bs.solve(), off.solve(), six.solve()
    print(bs.columns(), "status", r.status_val[at], "iter", r.iter[at])
    easy = np.setdiff1d(np.arange(70), at)
    assert np.all(r.status_val[easy] == 1) and np.all(r.iter[easy] == 25)
    assert bs.columns().packs >= 1 and bs.columns().ended <= 6
    assert r.status_val[at[MIXED["pinf"]]] == -3 and r.status_val[at[MIXED["dinf"]]] == -4
    assert np.all(np.delete(r.status_val[at], [MIXED["pinf"], MIXED["dinf"]]) == 1)
    assert r.iter[at].max() > 25                     # somebody was moved by the pack and went on
    for b in (at[MIXED["pinf"]], at[MIXED["dinf"]]):
        assert np.all(np.isnan(r.x[b]) | (r.x[b] == abi.OSQP_NAN)) and np.all(np.isnan(r.y[b]) | (r.y[b] == abi.OSQP_NAN))
    assert r.obj_val[at[MIXED["pinf"]]] == abi.OSQP_INFTY and r.obj_val[at[MIXED["dinf"]]] == -abi.OSQP_INFTY
    assert np.abs(r.prim_inf_cert[at[MIXED["pinf"]]]).max() > 0 and np.abs(r.dual_inf_cert[at[MIXED["dinf"]]]).max() > 0
    assert not r.prim_inf_cert[easy].any() and not r.dual_inf_cert[easy].any()
    _same(r, ro, what="mixed against the unpacked solve")
    _same(r, r6, i1=at, what="mixed against the six alone")
    for s in (bs, off, six):
        s.cleanup()


def test_warm_solve_after_a_packed_solve(gpu_lib, monkeypatch):
    """max_iter = 40: the easy members end at 25 (a pack), some hard ones stop unsolved at 40; the second solve starts from
    every member's stored iterates, which the packed solve stored by member."""
    B, h, drop = WAVES["one"]
    P, A, Q, L, U, hard = wave_case(B, h, drop)
    kw = dict(FIXED, max_iter=40)
    bs, off = _common(P, A, Q, L, U, **kw), _unpacked(monkeypatch, P, A, Q, L, U, **kw)
    for k in range(2):
        r, ro = bs.solve(), off.solve()
        print("solve", k, bs.columns(), "status", dict(zip(*np.unique(r.status_val, return_counts=True))))
        assert bs.columns().packs >= 1
        _same(r, ro, what="solve %d" % k)
        if k == 0:
            assert (r.status_val[hard] != 1).any() and (r.status_val[hard] == 1).any()
    bs.cleanup(); off.cleanup()


# ---- chosen members ----------------------------------------------------------------------------------------------------
def _plain(B=130):
    return common_family(WAVE_N, WAVE_M, B, WAVE_SEED)[:5]


@pytest.mark.parametrize("mode", ["fixed-unscaled", "adaptive"])
@pytest.mark.parametrize("label,S", subsets(ADAPTIVE_SUBSET_B))
def test_cold_subset(gpu_lib, label, S, mode):
    """The listed members equal a fresh handle set up on them alone; the others are what results() gave before."""
    if mode == "adaptive":
        P, A, Q, L, U = adaptive_subset_case(S)
        kw = dict(ADAPTIVE)
    else:
        P, A, Q, L, U = _plain()
        kw = dict(FIXED, scaling=0, max_iter=300)
    B = Q.shape[0]
    rest = np.setdiff1d(np.arange(B), S)
    bs, alone = _common(P, A, Q, L, U, **kw), _common(P, A, Q[S], L[S], U[S], **kw)
    before = bs.results()
    r, ra = bs.solve(members=S), alone.solve()
    assert bs.columns().started == len(S) and bs.columns()[1:] == alone.columns()[1:]
    _same(r, ra, i1=S, what=label + " listed")
    _same(r, before, i1=rest, i2=rest, what=label + " unlisted")
    assert np.all(r.iter[S] > 0)
    if mode == "adaptive":
        # (inversions + 1, and the one refinement verdict: rounds()[1] reports it as the batch's size or 0)
        assert bs.rounds()[0] == alone.rounds()[0] >= 2 and bool(bs.rounds()[1]) == bool(alone.rounds()[1])
        assert r.rho_updates[S].max() >= 1
        assert bs.member_workspace(0)["rho"] == alone.member_workspace(0)["rho"]
    bs.cleanup(); alone.cleanup()


def test_mask_and_list_agree(gpu_lib):
    P, A, Q, L, U = _plain(40)
    S = np.array([1, 5, 6, 39])
    mask = np.zeros(40, bool); mask[S] = True
    a, b = _common(P, A, Q, L, U, **FIXED), _common(P, A, Q, L, U, **FIXED)
    _same(a.solve(members=S), b.solve(members=mask))
    _same(a.solve(members=list(S)), b.solve(members=tuple(int(v) for v in S)), what="warm repeat")
    a.cleanup(); b.cleanup()


def test_unlisted_iterates_are_untouched(gpu_lib):
    """max_iter = 20, so every solve stops mid-way and the next continues from the stored iterates: solving S and then
    the rest continues every member exactly as a second full solve does."""
    P, A, Q, L, U = _plain()
    kw = dict(FIXED, max_iter=20)
    S = np.arange(17) * 2
    rest = np.setdiff1d(np.arange(130), S)
    h1, h2 = _common(P, A, Q, L, U, **kw), _common(P, A, Q, L, U, **kw)
    _same(h1.solve(), h2.solve(), what="first solve")
    mid = h1.solve(members=S)
    r1 = h1.solve(members=rest)
    r2 = h2.solve()
    _same(mid, r2, i1=S, i2=S, what="S after its solve")
    _same(r1, r2, what="after both parts")
    assert (r2.status_val != 1).any() and h1.columns().started == len(rest)
    h1.cleanup(); h2.cleanup()


def test_all_members_is_the_full_solve(gpu_lib):
    P, A, Q, L, U, _ = wave_case(*WAVES["one"])
    a, b = _common(P, A, Q, L, U, **FIXED), _common(P, A, Q, L, U, **FIXED)
    _same(a.solve(), b.solve(members=np.arange(130)))
    assert a.columns() == b.columns()
    _same(a.solve(), b.solve(members=np.ones(130, bool)), what="warm")
    a.cleanup(); b.cleanup()


def _gamma(k):
    u = 2.0 ** -53
    return k * u / (1 - k * u)


def _assert_definitions(r, b, P, A, q, l, u):
    """obj_val, dua_res and pri_res of member b against their definitions in long double: the bounds of
    test_gpu_batch_common.py::test_adaptive_differing_members, the same formulas."""
    ld = np.longdouble
    n, m = P.shape[0], A.shape[0]
    Pf = (P + sparse.triu(P, 1).T).toarray().astype(ld); Ad = A.toarray().astype(ld)
    k = int(max((Pf[j] != 0).sum() + (Ad[:, j] != 0).sum() for j in range(n))) + 1 + 64
    krow = int(max((Ad[i] != 0).sum() for i in range(m))) + 64
    x, y, q = r.x[b].astype(ld), r.y[b].astype(ld), q.astype(ld)
    terms = np.abs(Pf * x[None, :]).sum(axis=1) + np.abs(q) + (np.abs(Ad) * np.abs(y)[:, None]).sum(axis=0)
    dua = np.abs(Pf @ x + q + Ad.T @ y)
    assert abs(ld(r.dua_res[b]) - dua.max()) <= _gamma(k) * terms.max(), b
    obj = 0.5 * x @ (Pf @ x) + q @ x
    oterms = 0.5 * (np.abs(x)[:, None] * np.abs(Pf) * np.abs(x)[None, :]).sum() + (np.abs(q) * np.abs(x)).sum()
    assert abs(ld(r.obj_val[b]) - obj) <= _gamma(k + n) * oterms, b
    slack = ld(r.pri_res[b]) + _gamma(krow) * (np.abs(Ad) @ np.abs(x))
    lo, hi = np.maximum(l, -1e30).astype(ld), np.minimum(u, 1e30).astype(ld)
    assert np.all(Ad @ x >= lo - slack) and np.all(Ad @ x <= hi + slack), b


def test_rho_adopted_on_a_subset(gpu_lib):
    S = np.arange(17) * 2
    P, A, Q, L, U = adaptive_subset_case(S)
    B = Q.shape[0]
    rest = np.setdiff1d(np.arange(B), S)
    bs = _common(P, A, Q, L, U, **ADAPTIVE)
    before = bs.results()
    r = bs.solve(members=S)
    rho = bs.member_workspace(0)["rho"]
    print("rho", rho, "rho_updates", r.rho_updates[S], "iter", r.iter[S])
    assert rho != 0.1 and np.all(r.rho_updates[S] >= 1) and np.all(r.status_val[S] == 1)
    assert r.rho[S[int(np.argmax(r.iter[S]))]] == rho          # no move follows the last finish
    assert np.array_equal(_bits(r.info_raw[rest]), _bits(before.info_raw[rest]))
    r2 = bs.solve(members=rest)
    _same(r2, r, i1=S, i2=S, what="S after the rest was solved")
    assert np.all(r2.status_val == 1), r2.status_val
    for b in rest[:: max(1, len(rest) // 8)]:
        _assert_definitions(r2, b, P, A, Q[b], L[b], U[b])
    bs.cleanup()


def test_solved_flags_gate_polish_and_derivatives(gpu_lib):
    """update -> solve(members=S) leaves the members outside S unsolved on the new problem: polish is refused (code 7) and
    nothing is kept; after solve(members=rest) polish, adjoint and tangent are those of update -> solve()."""
    P, A, Q, L, U = _plain(40)
    S = np.arange(0, 40, 3)
    rest = np.setdiff1d(np.arange(40), S)
    Q2 = Q * 1.25
    h1, h2 = (_common(P, A, Q, L, U, shared_kkt=True, **FIXED) for _ in range(2))
    _same(h1.solve(), h2.solve())
    h1.adjoint(np.ones_like(Q), np.ones_like(L))
    assert h1.kkt_info().kept == 1
    assert h1.update(Q=Q2) == 0 and h2.update(Q=Q2) == 0
    h1.solve(members=S)
    assert h1.kkt_info().kept == 0
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h1.polish()
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h1.adjoint(np.ones_like(Q), np.ones_like(L))
    h1.solve(members=rest)
    h2.solve()
    p1, p2 = h1.polish(), h2.polish()
    _same(p1, p2, what="polished")
    assert np.array_equal(p1.status_polish, p2.status_polish) and (p1.status_polish == 1).any()
    a1, a2 = (h.adjoint(np.ones_like(Q), np.ones_like(L), matrices=True) for h in (h1, h2))
    for k in ("dq", "dl", "du", "dPx", "dAx", "active", "status_adjoint"):
        assert np.array_equal(getattr(a1, k), getattr(a2, k)), k
    t1, t2 = (h.tangent(dQ=np.ones_like(Q), dL=np.ones_like(L), dU=np.ones_like(L)) for h in (h1, h2))
    for k in ("dx", "dy", "active", "status_tangent"):
        assert np.array_equal(getattr(t1, k), getattr(t2, k)), k
    # on a handle every member of which is solved, a subset solve leaves it solved: polish is served
    h1.solve(members=S)
    h1.polish()
    h1.cleanup(); h2.cleanup()


def test_refusals_change_nothing(gpu_lib):
    import ctypes as C
    from osqp_amd import abi
    P, A, Q, L, U = _plain(40)
    bs, ref = _common(P, A, Q, L, U, **FIXED), _common(P, A, Q, L, U, **FIXED)
    bs.solve(members=[2, 3, 30]); ref.solve(members=[2, 3, 30])
    before, cols = bs.results(), bs.columns()
    for bad in ([3, 2], [1, 1], [0, 40], [-1, 0], [], np.ones(39, bool), np.zeros(40, bool)):
        with pytest.raises(ValueError):
            bs.solve(members=bad)
    call = bs._lib.osqp_amd_batch_solve_members
    for lst, count in (([3, 2], 2), ([1, 1], 2), ([0, 40], 2), ([-1, 0], 2), ([0], 0), ([0], -1), (list(range(41)), 41)):
        assert call(bs._h, abi.iptr(np.array(lst, np.int64)), count) == 1, lst       # OSQP_DATA_VALIDATION_ERROR
    assert call(bs._h, C.cast(None, abi.c_int_p), 1) == 1
    assert bs._lib.osqp_amd_batch_common_columns(bs._h, C.cast(None, abi.c_int_p)) == 1
    _same(bs.results(), before, what="after the refusals")
    assert bs.columns() == cols
    _same(bs.solve(), ref.solve(), what="a full solve after the refusals")
    bs.cleanup(); ref.cleanup()


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_other_engines_refuse(gpu_lib, engine):
    import osqp_amd
    from osqp_amd import abi
    P, A, Q, L, U = _plain(5)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **FIXED)
    before = bs.solve()
    with pytest.raises(RuntimeError, match="not served"):
        bs.solve(members=[0, 1])
    with pytest.raises(RuntimeError):
        bs.columns()
    k = np.array([0, 1], np.int64); out = np.zeros(3, np.int64)
    assert bs._lib.osqp_amd_batch_solve_members(bs._h, abi.iptr(k), 2) == 4        # OSQP_LINSYS_SOLVER_INIT_ERROR
    assert bs._lib.osqp_amd_batch_common_columns(bs._h, abi.iptr(out)) == 4
    _same(bs.results(), before)
    bs.cleanup()
