"""GPU tests of the member-list forms of the matrix and rho updates -- `BatchOSQP.update_matrices(members=)`,
`update_rho(members=)`; osqp_amd_batch_update_matrices_members[_dev], osqp_amd_batch_update_rho_members
(include/osqp_amd_batch.h, "Chosen members") -- on the tiled and the streamed engine.

What is compared with what:
  * a listed member with the whole-batch twin given [B, k] arrays that repeat the unlisted members' current values:
    `member_workspace` and the next solve, to the bit;
  * an unlisted member with itself before the call, and after the next solve with a handle that received nothing: to the bit;
  * every member with its own oracle sequence (tests/_batch_parity.assert_parity): evidence that does not rest on the
    twin, whose code the member form shares.
Cases, lists and seeds: tests/_update_members_cases.py; tests/test_update_members_cases_host.py proves on the CPU that no
member of them is let off."""
import numpy as np
import pytest

import _update_members_cases as uc
from _batch_parity import assert_parity, oracle
from _members_cases import Device, same, same_workspace
from _update_members_cases import B, CASES, IDS, KW, LISTS, members_of
from test_gpu_batch_updates import new_values

pytestmark = pytest.mark.gpu

NAMES = list(LISTS)
SHORT = [NAMES[k] for k in (0, 2, 3, 5)]      # first, two, but_one, mask
ENGINE_CASES = [CASES[0], CASES[3]]           # one shape per engine where the engine is what matters, not the size


def setup_values(case):
    """[B, nnz] values of a handle set up with Px_all / Ax_all."""
    Pu, A = uc.case_data(case)[:2]
    return new_values(Pu, A, uc.SEEDS[case] + 1, True, nB=B)


def handle(case, setup_all=False, **kw):
    import osqp_amd
    Pu, A, Q, L, U = uc.case_data(case)[:5]
    extra = {}
    if setup_all:
        Px0, Ax0 = setup_values(case)
        extra = dict(Px_all=Px0, Ax_all=Ax0)
    return osqp_amd.BatchOSQP().setup(Pu, A, Q, L, U, engine=case[0], **extra, **{**KW, **kw})


def update_args(case, S, which="PA", form="full", per=1, setup_all=False):
    """(the arguments of update_matrices(members=S), those of the whole-batch twin): per = 1 gives every listed member
    its own new values (compact rows), per = 0 the first listed member's to all of them; form "idx": a sorted half of
    the slots, P's diagonal among them."""
    Pu, A, _, _, _, Pn, An = uc.case_data(case)
    mem = members_of(S)
    cur = setup_values(case) if setup_all else (Pu.data, A.data)
    rng = np.random.default_rng(uc.SEEDS[case] + 3)
    mine, twin = {}, {}
    for nm, M, new, have in (("P", Pu, Pn, cur[0]), ("A", A, An, cur[1])):
        if nm not in which:
            continue
        idx = None
        if form == "idx":
            idx = np.sort(rng.choice(M.nnz, max(1, M.nnz // 2), replace=False))
            if nm == "P":
                idx = np.union1d(idx, np.flatnonzero(Pu.indices == np.repeat(np.arange(Pu.shape[0]), np.diff(Pu.indptr))))
            mine[nm + "x_idx"] = twin[nm + "x_idx"] = idx
        v = new[mem] if per else new[mem[0]]
        v = np.ascontiguousarray(v if idx is None else v[..., idx])
        mine[nm + "x"] = v
        twin[nm + "x"] = uc.twin_arrays(have, S, v, idx)
    return mine, twin


def snapshot(h):
    return dict(r=h.results(), ws=[h.member_workspace(b) for b in range(B)], solved=h.solved_members())


def same_snapshot(s1, s2, members, what):
    members = list(members)
    same(s1["r"], s2["r"], members, members, what=what)
    for b in members:
        same_workspace(s1["ws"][b], s2["ws"][b], (what, b))
    assert np.array_equal(s1["solved"][members], s2["solved"][members]), what


def others(S):
    return np.setdiff1d(np.arange(B), members_of(S))


# ---------------------------------------------------------------------------------------------------------------
# 1. the whole update for the listed members: bit-equal to the twin
# ---------------------------------------------------------------------------------------------------------------
# (which matrices, full arrays or an index subset, per_member, storage at setup, scaling)
COMBOS = [("PA", "full", 1, "shared", 10), ("P", "idx", 0, "shared", 10), ("A", "full", 0, "setup_all", 0),
          ("A", "idx", 1, "shared", 10), ("PA", "idx", 1, "setup_all", 0), ("P", "full", 1, "setup_all", 10),
          ("PA", "full", 0, "shared", 0)]


@pytest.mark.parametrize("combo", COMBOS, ids=["-".join(str(v) for v in c) for c in COMBOS])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_listed_members_get_the_twins_bits(gpu_lib, case, combo):
    which, form, per, storage, scaling = combo
    setup_all = storage == "setup_all"
    for name, S in LISTS.items():
        mem = members_of(S)
        a, b = handle(case, setup_all, scaling=scaling), handle(case, setup_all, scaling=scaling)
        same(a.solve(), b.solve(), what=(name, "first solve"))
        mine, twin = update_args(case, S, which, form, per, setup_all)
        assert a.update_matrices(members=S, **mine) == 0 and b.update_matrices(**twin) == 0, name
        for q in mem:
            same_workspace(a.member_workspace(q), b.member_workspace(q), (name, int(q)))
        assert not a.solved_members()[mem].any()
        same(a.solve(), b.solve(), mem, mem, what=(name, "second solve"))
        a.cleanup(); b.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 2. unlisted members keep their bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHORT)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unlisted_members_keep_their_bits(gpu_lib, case, name):
    S = LISTS[name]
    mem, rest = members_of(S), others(S)
    a, c = handle(case), handle(case)
    a.solve(); c.solve()
    sp = a.polish().status_polish
    c.polish()
    before = snapshot(a)
    builds = a.kkt_info().builds
    mine, _ = update_args(case, S)
    assert a.update_matrices(members=S, **mine) == 0
    after = snapshot(a)
    same_snapshot(before, after, rest, name)
    assert after["solved"][rest].all() and not after["solved"][mem].any()
    # the unlisted members are still polished: a repeat does no work and reports what the whole-batch polish reported
    assert np.array_equal(a.polish(members=rest).status_polish, sp[rest]) and a.kkt_info().builds == builds
    for q in mem:                                            # (the listed members' scaling did move)
        assert not np.array_equal(after["ws"][q]["D"], before["ws"][q]["D"]), q
    ra, rc = a.solve(), c.solve()
    same(ra, rc, rest, rest, what=(name, "the next solve"))
    a.cleanup(); c.cleanup()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unlisted_members_keep_their_scaling_after_a_new_q(gpu_lib, case):
    """Every member gets a new q through update() first.  The twin would recompute the unlisted members' D, E, c from it;
    the member call leaves them."""
    S = LISTS["two"]
    mem, rest = members_of(S), others(S)
    Q = uc.case_data(case)[2]
    Qn = Q * np.random.default_rng(5).uniform(20.0, 50.0, Q.shape)     # (q's scale enters c, and D through it)
    a, t = handle(case), handle(case)
    for h in (a, t):
        h.solve()
        assert h.update(Q=Qn) == 0
    before = snapshot(a)
    mine, twin = update_args(case, S)
    assert a.update_matrices(members=S, **mine) == 0 and t.update_matrices(**twin) == 0
    after, moved = snapshot(a), snapshot(t)
    same_snapshot(before, after, rest, "unlisted")
    assert any(moved["ws"][b]["c"] != before["ws"][b]["c"] or not np.array_equal(moved["ws"][b]["D"], before["ws"][b]["D"])
               for b in rest), "the twin leaves the unlisted members' scaling too: the case shows nothing"
    for q in mem:
        same_workspace(after["ws"][q], moved["ws"][q], ("listed", int(q)))
    same(a.solve(), t.solve(), mem, mem, what="listed, the next solve")
    a.cleanup(); t.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 3. against the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_member_follows_its_oracle(gpu_lib, oracle_mod, case, name):
    S = LISTS[name]
    mem = members_of(S)
    Pu, A, Q, L, U, Pn, An = uc.case_data(case)
    a = handle(case)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **KW) for b in range(B)]
    r1 = a.solve()
    for b in range(B):
        assert_parity(r1, b, sos[b].solve(), "first solve")
    assert np.any(r1.rho_updates[mem] > 0), "no listed member's rho moved: keeping rho cannot be told from a new setup"
    rho = [a.member_workspace(b)["rho"] for b in range(B)]
    assert a.update_matrices(Px=Pn[mem], Ax=An[mem], members=S) == 0
    assert [a.member_workspace(b)["rho"] for b in range(B)] == rho
    r2 = a.solve()
    for b in range(B):
        if b in mem:
            assert sos[b].update(Px=Pn[b], Ax=An[b]) == 0
        assert_parity(r2, b, sos[b].solve(), "second solve, %s" % ("listed" if b in mem else "unlisted"))
    a.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 4. state edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_listed_member_with_a_rebuild_pending(gpu_lib, case):
    """A class-changing update(members=) directly before: the listed member's K^-1 is due when the matrix update comes."""
    S = LISTS["two"]
    mem = members_of(S)
    L, U = uc.case_data(case)[3:5]
    q = int(mem[0])
    rows = np.flatnonzero(np.isfinite(L[q]) & np.isfinite(U[q]) & (L[q] < U[q]))[:2]
    assert rows.size == 2
    Un = U[q].copy(); Un[rows] = L[q][rows]                  # two inequality rows become equalities
    a, b = handle(case), handle(case)
    mine, twin = update_args(case, S)
    for h in (a, b):
        h.solve()
        ct = h.member_workspace(q)["ctype"]
        assert h.update(U=Un[None], members=[q]) == 0
        assert np.array_equal(h.member_workspace(q)["ctype"][rows], [1, 1]) and not np.array_equal(ct[rows], [1, 1])
    assert a.update_matrices(members=S, **mine) == 0 and b.update_matrices(**twin) == 0
    for k in mem:
        same_workspace(a.member_workspace(k), b.member_workspace(k), int(k))
    same(a.solve(), b.solve(), mem, mem, what="the next solve")
    a.cleanup(); b.cleanup()


@pytest.mark.parametrize("form", ["full", "idx"])
@pytest.mark.parametrize("per", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_route_is_the_host_route(gpu_lib, case, per, form):
    S = LISTS["mask"]
    a, d = handle(case), handle(case)
    dev = Device()
    try:
        mine, _ = update_args(case, S, "PA", form, per)
        there = {k: (dev.put(v) if k in ("Px", "Ax") else v) for k, v in mine.items()}
        for h, args in ((a, mine), (d, there)):
            h.solve()
            assert h.update_matrices(members=S, **args) == 0
        same_snapshot(snapshot(a), snapshot(d), range(B), "after the call")
        same(a.solve(), d.solve(), what="the next solve")
    finally:
        dev.close()
        a.cleanup(); d.cleanup()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_storage_switch_then_a_shared_index_update(gpu_lib, case):
    """A handle with shared values takes a member call (one row per member from then on), then a whole-batch update of
    shared values on an index list, which writes every member's row."""
    S = LISTS["but_one"]
    Pu = uc.case_data(case)[0]
    a, b = handle(case), handle(case)
    mine, twin = update_args(case, S)
    diag = np.flatnonzero(Pu.indices == np.repeat(np.arange(Pu.shape[0]), np.diff(Pu.indptr)))
    for h, args, kw in ((a, mine, dict(members=S)), (b, twin, {})):
        h.solve()
        assert h.update_matrices(**args, **kw) == 0
        assert h.update_matrices(Px=Pu.data[diag] * 1.25, Px_idx=diag) == 0
    same_snapshot(snapshot(a), snapshot(b), range(B), "after both calls")
    same(a.solve(), b.solve(), what="the next solve")
    a.cleanup(); b.cleanup()


@pytest.mark.parametrize("case", ENGINE_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_a_kept_kkt_inversion_is_dropped(gpu_lib, case):
    a = handle(case)
    a.solve()
    a.adjoint(np.ones((B, a.n)))
    assert a.kkt_info().kept
    mine, _ = update_args(case, [0])
    assert a.update_matrices(members=[0], **mine) == 0
    assert not a.kkt_info().kept
    a.solve()
    a.adjoint(np.ones((B, a.n)))
    assert a.kkt_info().kept
    assert a.update_rho(0.5, members=[B - 1]) == 0
    assert not a.kkt_info().kept
    a.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 5. non-convex members
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ENGINE_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_non_convex_member(gpu_lib, oracle_mod, capfd, case):
    Pu, A, Q, L, U, Pn, An = uc.case_data(case)
    diag = Pu.indices == np.repeat(np.arange(Pu.shape[0]), np.diff(Pu.indptr))
    bad = Pn[1].copy()
    bad[diag] = -1e13                   # far below -(sigma + A' rho A), as tests/test_gpu_batch_updates.py plants it
    a = handle(case)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **KW) for b in range(B)]
    r1 = a.solve()
    for b in range(B):
        assert_parity(r1, b, sos[b].solve(), "first solve")
    capfd.readouterr()
    assert a.update_matrices(Px=bad, members=[1]) == 5                      # OSQP_NONCVX_ERROR
    assert "QP 1 of the batch" in capfd.readouterr().err
    with pytest.raises(RuntimeError, match=r"\(5\)"):
        a.solve()
    # another member's good values: member 1 is still bad, and the call says so
    assert a.update_matrices(Px=Pn[3], Ax=An[3], members=[3]) == 5
    assert "QP 1 of the batch" in capfd.readouterr().err
    with pytest.raises(RuntimeError, match=r"\(5\)"):
        a.solve()
    # the repair
    assert a.update_matrices(Px=Pn[1], members=[1]) == 0
    r2 = a.solve()
    assert sos[1].update(Px=Pn[1]) == 0 and sos[3].update(Px=Pn[3], Ax=An[3]) == 0
    for b in range(B):
        assert_parity(r2, b, sos[b].solve(), "after the repair")
    a.cleanup()


@pytest.mark.parametrize("case", ENGINE_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_non_convex_verdict_survives_other_updates(gpu_lib, capfd, case):
    """update_rho and a class-changing update store the bad member's flag word anew.  Its K is as indefinite as before:
    a member call on another member still returns 5 and solve still refuses, until a matrix update repairs the member."""
    Pu, A, Q, L, U, Pn, An = uc.case_data(case)
    diag = Pu.indices == np.repeat(np.arange(Pu.shape[0]), np.diff(Pu.indptr))
    bad = Pn[1].copy()
    bad[diag] = -1e13
    rows = np.flatnonzero(np.isfinite(L[1]) & np.isfinite(U[1]) & (L[1] < U[1]))[:2]
    Un = U[1].copy(); Un[rows] = L[1][rows]
    a = handle(case)
    a.solve()
    assert a.update_matrices(Px=bad, members=[1]) == 5
    for what, call in (("update_rho", lambda: a.update_rho(0.5)),
                       ("update_rho(members=)", lambda: a.update_rho(0.3, members=[1])),
                       ("a class-changing update(members=)", lambda: a.update(U=Un[None], members=[1])),
                       ("a warm start", lambda: a.warm_start(X=np.zeros((1, a.n)), members=[1]))):
        assert call() == 0, what
        capfd.readouterr()
        assert a.update_matrices(Px=Pn[3], Ax=An[3], members=[3]) == 5, what
        assert "QP 1 of the batch" in capfd.readouterr().err, what
        with pytest.raises(RuntimeError, match=r"\(5\)"):
            a.solve()
    assert np.array_equal(a.member_workspace(1)["ctype"][rows], [1, 1])
    # bad values for members 0 and 1; the repair of one leaves the other bad (5), the repair of both is 0
    assert a.update_matrices(Px=bad, members=[0, 1]) == 5
    assert a.update_matrices(Px=Pn[1], members=[1]) == 5
    assert a.update_matrices(Px=Pn[0], members=[0]) == 0
    r = a.solve()
    assert np.all(np.isfinite(r.x)) and a.solved_members().all()
    assert a.update_matrices(Px=bad[None].repeat(B, 0)) == 5 and a.update_matrices(Px=Pn[:1], members=[0]) == 5
    assert a.update_matrices(Px=Pn) == 0
    a.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 6. update_rho(members=)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["first", "two", "mask", "all"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_update_rho_members(gpu_lib, oracle_mod, case, name):
    S = LISTS[name]
    mem, rest = members_of(S), others(S)
    Pu, A, Q, L, U = uc.case_data(case)[:5]
    a, c = handle(case), handle(case)
    sos = [oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **KW) for b in range(B)]
    r1 = a.solve(); c.solve()
    for b in range(B):
        assert_parity(r1, b, sos[b].solve(), "first solve")
    before = snapshot(a)
    # a value <= 0: 1, and nothing moves
    bad = uc.RHO[mem].copy(); bad[-1] = 0.0
    assert a.update_rho(bad, members=S) == 1 and a.update_rho(-1.0, members=S) == 1
    same_snapshot(before, snapshot(a), range(B), "after a refused rho")
    assert a.update_rho(uc.RHO[mem], members=S) == 0
    after = snapshot(a)
    same_snapshot(before, after, rest, "unlisted")
    for b in mem:
        assert after["ws"][b]["rho"] == uc.RHO[b] and not after["solved"][b]
        assert after["r"].rho_updates[b] == before["r"].rho_updates[b]           # update_rho does not reset the count
    r2, rc = a.solve(), c.solve()
    same(r2, rc, rest, rest, what="unlisted, the next solve")
    for b in range(B):
        if b in mem:
            assert sos[b].update_rho(float(uc.RHO[b])) == 0
        ro = sos[b].solve()
        assert_parity(r2, b, ro, "after update_rho, %s" % ("listed" if b in mem else "unlisted"))
        assert r2.rho_updates[b] >= r1.rho_updates[b]
    a.cleanup(); c.cleanup()


def test_update_rho_members_clips_and_takes_a_scalar(gpu_lib):
    a = handle(CASES[0])
    a.solve()
    rho = [a.member_workspace(b)["rho"] for b in range(B)]
    assert a.update_rho(np.array([1e-9, 5e7]), members=[1, 3]) == 0
    assert [a.member_workspace(b)["rho"] for b in range(B)] == [rho[0], 1e-6, rho[2], 1e6, rho[4]]
    assert a.update_rho(0.25, members=[0, 4]) == 0
    assert [a.member_workspace(b)["rho"] for b in range(B)] == [0.25, 1e-6, rho[2], 1e6, 0.25]
    a.cleanup()


def test_update_rho_members_on_the_common_engine(gpu_lib, capfd):
    import osqp_amd
    from _common_cases import FIXED, common_family
    P, A, Q, L, U = common_family(33, 66, B, 533)[:5]
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **FIXED)
    h.solve()
    r, solved = h.results(), h.solved_members()
    capfd.readouterr()
    assert h.update_rho(0.5, members=[1, 3]) == 1
    assert "one rho for the batch" in capfd.readouterr().err
    same(r, h.results(), what="after the refusal")
    assert np.array_equal(solved, h.solved_members())
    assert h.update_rho(0.5, members=list(range(B))) == 0            # all B members: the twin
    assert not h.solved_members().any()
    with pytest.raises(RuntimeError, match="update_matrices is not served by the common-K engine"):
        h.update_matrices(Px=np.zeros(h.Pu.nnz), members=[1])
    h.cleanup()


def test_common_engine_refuses_at_the_abi(gpu_lib, capfd):
    """The C entries on a common-K handle, which the Python layer never reaches there: the list's refusal comes first, then
    the engine's (the twin's words, naming the call); update_rho_members with count < B returns 1.  Nothing changes."""
    import ctypes as C
    import osqp_amd
    from osqp_amd import abi
    from _common_cases import FIXED, common_family
    P, A, Q, L, U = common_family(33, 66, B, 533)[:5]
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **FIXED)
    h.solve()
    before = (h.results(), h.solved_members())
    Lb = h._lib
    vP = np.ones(h.Pu.nnz)
    ok, desc = np.array([1, 3], np.int64), np.array([3, 1], np.int64)
    for name, ptr in (("osqp_amd_batch_update_matrices_members", abi.fptr(vP)),
                      ("osqp_amd_batch_update_matrices_members_dev", C.c_void_p(vP.ctypes.data))):
        f = getattr(Lb, name)
        capfd.readouterr()
        for mem, cnt in ((None, 2), (abi.iptr(desc), 2), (abi.iptr(ok), 0), (abi.iptr(ok), B + 1)):
            assert f(h._h, mem, cnt, ptr, None, 0, 0, None, None, 0, 0) == 1           # OSQP_DATA_VALIDATION_ERROR: the list
        assert capfd.readouterr().err == ""
        # a good list: the engine's refusal, before the twin's own (P_n > nnzP would be 1, both NULL would be 0)
        for args in ((ptr, abi.iptr(ok), h.Pu.nnz + 1, 0, None, None, 0, 0), (None, None, 0, 0, None, None, 0, 0),
                     (ptr, None, 0, 1, None, None, 0, 0)):
            assert f(h._h, abi.iptr(ok), 2, *args) == 4                                # OSQP_LINSYS_SOLVER_INIT_ERROR
            err = capfd.readouterr().err
            assert name + " is not served by the common-K engine" in err, err
        assert f(h._h, abi.iptr(np.arange(B, dtype=np.int64)), B, ptr, None, 0, 0, None, None, 0, 0) == 4   # all B members too
        capfd.readouterr()
        same(before[0], h.results(), what=name)
        assert np.array_equal(before[1], h.solved_members()) and before[1].all()
    fr = Lb.osqp_amd_batch_update_rho_members
    assert fr(h._h, abi.iptr(desc), 2, abi.fptr(np.array([0.5])), 0) == 1 and capfd.readouterr().err == ""
    assert fr(h._h, abi.iptr(ok), 2, abi.fptr(np.array([0.5])), 0) == 1
    assert "one rho for the batch" in capfd.readouterr().err
    same(before[0], h.results(), what="update_rho_members")
    assert np.array_equal(before[1], h.solved_members())
    h.cleanup()


# ---------------------------------------------------------------------------------------------------------------
# 7. refusals change nothing
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ENGINE_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_refusals_change_nothing(gpu_lib, case):
    """Every refusal of the C entries, in the header's order, straight at the ABI (the Python layer would stop most of
    them first), with the whole handle compared after each."""
    import ctypes as C
    from osqp_amd import abi
    Pu, A = uc.case_data(case)[:2]
    a = handle(case)
    a.solve()
    before = snapshot(a)
    Lb, h = a._lib, a._h
    fm, fd, fr = (Lb.osqp_amd_batch_update_matrices_members, Lb.osqp_amd_batch_update_matrices_members_dev,
                  Lb.osqp_amd_batch_update_rho_members)
    null_i = C.cast(None, abi.c_int_p)
    ok = np.array([1, 3], np.int64)
    vP, vA = np.ones(Pu.nnz), np.ones(A.nnz)
    i2 = np.array([0, 1], np.int64)
    mat = lambda f, mem, cnt, Px=None, Pi=None, Pn=0, Ax=None, Ai=None, An=0: f(h, mem, cnt, Px, Pi, Pn, 0, Ax, Ai, An, 0)
    lists = [(null_i, 2), (abi.iptr(ok), 0), (abi.iptr(ok), B + 1), (abi.iptr(np.array([3, 1], np.int64)), 2),
             (abi.iptr(np.array([1, 1], np.int64)), 2), (abi.iptr(np.array([0, B], np.int64)), 2),
             (abi.iptr(np.array([-1, 0], np.int64)), 2)]
    BAD = 1                                  # OSQP_DATA_VALIDATION_ERROR; the reference's code for P_n > nnzP is 1 too, so
    for f in (fm, fd):                       # the order of the refusals is shown on A_n > nnzA, which is 2
        ptr = (lambda v: abi.fptr(v)) if f is fm else (lambda v: C.c_void_p(v.ctypes.data))
        for mem, cnt in lists:               # the list comes before the twin's own refusals
            assert mat(f, mem, cnt, Ax=ptr(vA), Ai=abi.iptr(i2), An=A.nnz + 1) == BAD
        assert mat(f, abi.iptr(ok), 2, ptr(vP), abi.iptr(i2), Pu.nnz + 1, ptr(vA), abi.iptr(i2), A.nnz + 1) == 1
        assert mat(f, abi.iptr(ok), 2, ptr(vP), abi.iptr(i2), 2, ptr(vA), abi.iptr(i2), A.nnz + 1) == 2
        assert mat(f, abi.iptr(ok), 2, ptr(vP), abi.iptr(np.array([0, Pu.nnz], np.int64)), 2) == BAD
        assert mat(f, abi.iptr(ok), 2, Ax=ptr(vA), Ai=abi.iptr(np.array([-1, 0], np.int64)), An=2) == BAD
        assert mat(f, abi.iptr(ok), 2) == 0                                                 # both NULL: nothing to do
        same_snapshot(before, snapshot(a), range(B), f.__name__)
    # the device form: host arrays are no device memory of the handle's device; a bad index list comes first (2, not 1)
    assert mat(fd, abi.iptr(ok), 2, C.c_void_p(vP.ctypes.data)) == BAD
    assert mat(fd, abi.iptr(ok), 2, Ax=C.c_void_p(vA.ctypes.data), Ai=abi.iptr(i2), An=A.nnz + 1) == 2
    for mem, cnt in lists:
        assert fr(h, mem, cnt, abi.fptr(np.ones(2)), 1) == BAD
    assert fr(h, abi.iptr(ok), 2, None, 0) == BAD
    assert fr(h, abi.iptr(ok), 2, abi.fptr(np.array([0.5, 0.0])), 1) == 1
    assert fr(h, abi.iptr(ok), 2, abi.fptr(np.array([-0.5])), 0) == 1
    same_snapshot(before, snapshot(a), range(B), "update_rho_members")
    assert a.solved_members().all() and a.kkt_info() is not None
    a.cleanup()
