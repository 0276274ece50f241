"""GPU tests of the member-list forms of the batch calls (batch_members.h): update, warm_start, polish, adjoint, tangent
and results with `members=` on the tiled, the streamed and the common-K engine.

Identities first: a member call equals its whole-batch twin given the same data (the unlisted rows repeated from what the
handle holds), to the bit and in every result; of an unlisted member nothing changes; all B members listed is the twin.
Then the oracle at the bars of tests/_batch_parity.py, the planted truths of tests/_planted_qp.py and
tests/_common_planted.py at the bars of test_gpu_batch_planted.py (with subsets whose padded KKT orders NPOL / NS are
smaller than the whole batch's: a member's bits must not depend on them), chunks, the gathers and the refusals."""
from types import SimpleNamespace

import ctypes as C
import numpy as np
import pytest

import _common_kkt_reference as kr
import _common_planted as cp
import _planted_qp as pq
from _batch_parity import assert_parity, oracle
from _members_cases import (ARRAYS, B, ENGINES, FIXED_RHO, LISTS, SHAPES, Device, bits, handle, new_rows, problem, same,
                            same_workspace, whole)

pytestmark = pytest.mark.gpu

ADJ = pq.ADJOINT + ("active", "status_adjoint")
TAN = pq.TANGENT + ("active", "status_tangent")
ENGINE_LISTS = [(e, k) for e in ENGINES for k in LISTS]


@pytest.fixture
def dev(gpu_lib):
    d = Device()
    yield d
    d.close()


def _rest(S):
    return np.setdiff1d(np.arange(B), S)


def _snapshot(h):
    return SimpleNamespace(r=h.results(), ws=[h.member_workspace(q) for q in range(B)], solved=h.solved_members())


def _unlisted_unchanged(h, before, S, what):
    """Results, workspace and solved flag of every member outside S carry the bits of `before`."""
    rest = _rest(S)
    now = _snapshot(h)
    same(now.r, before.r, rest, rest, what=what + ": an unlisted member's results")
    for q in rest:
        same_workspace(now.ws[q], before.ws[q], what + ": workspace of unlisted member %d" % q)
    assert np.array_equal(now.solved[rest], before.solved[rest]), what
    return now


# ---- 1. twin equality --------------------------------------------------------------------------------------------------
def _twin_updates(engine, pb, S, whiches, kw=None, adaptive=False):
    P, A, Q, L, U = pb
    a, b = handle(engine, pb, **(kw or {})), handle(engine, pb, **(kw or {}))
    same(a.solve(), b.solve(), what="first solve")
    assert a.solved_members().all()
    cur = dict(Q=Q.copy(), L=L.copy(), U=U.copy())
    rest = _rest(S)
    # Setup scales q, l, u pass by pass through the equilibration, an update in one product with the final D, E, c: the
    # same raw row gives other last bits.  So that "the unlisted rows repeated" is a no-op on `b`, both handles first take
    # a whole update with the data they hold; from there on every scaled row is an update's.
    first = dict(cur) if L.shape[1] else dict(Q=cur["Q"])
    assert a.update(**first) == 0 and b.update(**first) == 0
    same(a.solve(), b.solve(), what="the solve after the levelling update")
    for k, which in enumerate(whiches):
        what = "%s %s %s" % (engine, S, which)
        rows = new_rows(engine, cur, S, which, 77 + k)
        full = whole(cur, S, rows)
        before = _snapshot(a)
        assert a.update(members=S, **rows) == 0, what
        assert b.update(**full) == 0, what
        cur.update(full)
        _unlisted_unchanged(a, before, S, what)
        want = np.zeros(B, bool); want[rest] = True
        assert np.array_equal(a.solved_members(), want), what
        if len(S) == B:
            assert np.array_equal(a.solved_members(), b.solved_members()) and not b.solved_members().any()
        ra, rb = a.solve(), b.solve()
        if adaptive:
            # rho_updates counts on from the previous solve until an update resets it (batch_admm.h): the whole update
            # has reset every member's, the member update the listed members' alone.  So an unlisted member of `a` holds
            # what it had before plus what this solve added, which is what `b` reports; everything else is the twin's.
            col = 5
            assert np.array_equal(ra.info_raw[rest, col], before.r.info_raw[rest, col] + rb.info_raw[rest, col]), what
            print(what, "rho_updates before", before.r.info_raw[:, col], "this solve", rb.info_raw[:, col])
            ia, ib = ra.info_raw.copy(), rb.info_raw.copy()
            ia[:, col] = ib[:, col] = 0
            ra.info_raw, rb.info_raw = ia, ib
        same(ra, rb, what=what + ": the solve after the update")
        assert a.solved_members().all()
    a.cleanup(); b.cleanup()


@pytest.mark.parametrize("engine,lst", ENGINE_LISTS, ids=["%s-%s" % el for el in ENGINE_LISTS])
def test_update_members_is_the_whole_update(gpu_lib, engine, lst):
    """Q only, L only, U only and all three, one after the other on a live pair of handles: `a` is told the rows of S,
    `b` the whole batch with the unlisted rows repeated.  Before the solve nothing of an unlisted member of `a` has
    changed; after it every result equals."""
    _twin_updates(engine, problem(engine), LISTS[lst], ("Q", "L", "U", "QLU"))


@pytest.mark.parametrize("engine", ENGINES)
def test_update_members_keeps_unlisted_rho_updates(gpu_lib, engine):
    """With adaptive rho and a q large enough to move it, an unlisted member's rho_updates is not reset by a member
    update (it is by the whole update, as the reference's reset_info): the one figure in which the twins differ."""
    kw = dict(adaptive_rho=1, adaptive_rho_interval=10)
    _twin_updates(engine, problem(engine, qscale=100.0), LISTS["three"], ("Q", "QLU"), kw=kw, adaptive=True)


@pytest.mark.parametrize("engine", ENGINES)
def test_update_members_without_constraints(gpu_lib, engine):
    _twin_updates(engine, problem(engine, m0=True), LISTS["three"], ("Q",))


@pytest.mark.parametrize("engine,lst", ENGINE_LISTS, ids=["%s-%s" % el for el in ENGINE_LISTS])
def test_warm_start_members_is_the_whole_warm_start(gpu_lib, engine, lst):
    """X only, Y only and both, on three handles in step: `a` is told the rows of S, `b` the whole batch, `c` nothing.
    A whole warm start cannot hand an unlisted member its own stored point back (x = D^-1 (D xs) rounds, and z becomes
    A x), so the whole-batch twin vouches for the listed members and `c` for the unlisted ones: rho is fixed, so a
    member's solve depends on its own data and iterates alone.  max_iter = 15: every solve stops mid-way and the next one
    shows what the stored iterates were.  All members listed: `a` is `b` in everything."""
    pb, S = problem(engine), np.asarray(LISTS[lst])
    kw = dict(max_iter=15)
    a, b, c = (handle(engine, pb, **kw) for _ in range(3))
    r0 = a.solve(); same(r0, b.solve()); same(r0, c.solve())
    rest = _rest(S)
    for k, (useX, useY) in enumerate(((True, False), (False, True), (True, True))):
        what = "%s %s X=%s Y=%s" % (engine, S, useX, useY)
        r = b.results()
        assert np.isfinite(r.x).all() and np.isfinite(r.y).all()
        X, Y = r.x + 0.01 * (k + 1), r.y * 0.5
        before = _snapshot(a)
        assert a.warm_start(X=X[S] if useX else None, Y=Y[S] if useY else None, members=S) == 0, what
        _unlisted_unchanged(a, before, S, what)
        want = np.zeros(B, bool); want[rest] = True
        assert np.array_equal(a.solved_members(), want), what
        assert b.warm_start(X=X if useX else None, Y=Y if useY else None) == 0
        if len(S) == B:
            assert np.array_equal(a.solved_members(), b.solved_members())
        ra, rb, rc = a.solve(), b.solve(), c.solve()
        same(ra, rb, S, S, what=what + ": the listed members")
        same(ra, rc, rest, rest, what=what + ": the unlisted members")
        assert a.solved_members().all()
    # both NULL: the setting, and nothing else
    before = _snapshot(a)
    assert a.warm_start(members=S) == 0
    _unlisted_unchanged(a, before, [], "warm_start(members=S) without arrays")
    a.cleanup(); b.cleanup(); c.cleanup()


# ---- 2. the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_subset_session_against_the_oracle(gpu_lib, oracle_mod, engine):
    """setup -> solve -> update(members=S) -> solve (of S on the common-K engine, of everyone elsewhere), every member
    against its own oracle run of the same session at the parity bar.  The common-K engine shares one scaling over the
    batch, which a per-member oracle run does not have: it is compared without scaling, as test_gpu_batch_common.py's
    direct parity is."""
    pb, S = problem(engine, shape=(17, 34) if engine == "common" else None), np.asarray(LISTS["three"])
    P, A, Q, L, U = pb
    kw = dict(FIXED_RHO[engine], **(dict(scaling=0, max_iter=300) if engine == "common" else {}))
    h = handle(engine, pb, **kw)
    sos = [oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw) for b in range(B)]
    r = h.solve()
    ros = [so.solve() for so in sos]
    for b in range(B):
        assert_parity(r, b, ros[b], "%s first solve" % engine)
    rows = new_rows(engine, dict(Q=Q, L=L, U=U), S, "QLU", 5)
    assert h.update(members=S, **rows) == 0
    r = h.solve(members=S) if engine == "common" else h.solve()
    for k, b in enumerate(S):
        sos[b].update(q=rows["Q"][k], l=rows["L"][k], u=rows["U"][k])
        ros[b] = sos[b].solve()
    if engine != "common":
        for b in _rest(S):
            ros[b] = sos[b].solve()
    for b in range(B):
        assert_parity(r, b, ros[b], "%s after update(members=%s)" % (engine, S))
    assert h.solved_members().all()
    h.cleanup()


# ---- 3. the common-K class rule ----------------------------------------------------------------------------------------
def test_common_class_rule(gpu_lib, capfd, dev):
    pb, S = problem("common"), np.asarray(LISTS["three"])
    P, A, Q, L, U = pb
    h, twin = handle("common", pb), handle("common", pb)
    same(h.solve(), twin.solve())
    row = int(np.flatnonzero(h.member_workspace(0)["ctype"] == 0)[0])
    assert np.isfinite(U[:, row]).all()
    L2, U2 = L[S].copy(), U[S].copy()
    L2[1, row] = U2[1, row]                                    # an inequality row becomes an equality in member S[1] alone
    before = _snapshot(h)
    capfd.readouterr()
    assert h.update(members=S, L=L2, U=U2) == 1
    err = capfd.readouterr().err
    assert "member %d" % S[1] in err and "row %d" % row in err and "update_members" in err, err
    _unlisted_unchanged(h, before, [], "a refused class change")
    # the same bounds for every member, all B listed: the twin's rule, a class change common to the batch
    Lall, Uall = L.copy(), U.copy()
    Lall[:, row] = Uall[:, row]
    assert h.update(members=np.arange(B), L=Lall, U=Uall) == 0 and twin.update(L=Lall, U=Uall) == 0
    assert not h.solved_members().any()
    same(h.solve(), twin.solve(), what="a common class change through all members listed")
    assert h.update(members=np.arange(B), L=L, U=U) == 0 and twin.update(L=L, U=U) == 0
    same(h.solve(), twin.solve())
    # l > u in one listed row: 1 from the C entry (batch.py raises before it), host and device arrays, nothing written
    L3, U3 = L[S].copy(), U[S].copy()
    L3[2, row] = U3[2, row] + 1.0
    before = _snapshot(h)
    from osqp_amd import abi
    mem = np.ascontiguousarray(S, np.int64)
    with pytest.raises(ValueError, match="lower bound greater"):
        h.update(members=S, L=L3, U=U3)
    assert h._lib.osqp_amd_batch_update_members(h._h, abi.iptr(mem), 3, None, abi.fptr(L3), abi.fptr(U3)) == 1
    assert h.update(members=S, L=dev.put(L3), U=dev.put(U3)) == 1
    _unlisted_unchanged(h, before, [], "l > u in a listed row")
    same(h.solve(), twin.solve(), what="after the refusals")
    h.cleanup(); twin.cleanup()


def test_update_members_device_route(gpu_lib, dev):
    """Device arrays with bounds past +-OSQP_INFTY: clamped as the host route clamps, the same bits afterwards."""
    for engine in ENGINES:
        pb, S = problem(engine), np.asarray(LISTS["three"])
        P, A, Q, L, U = pb
        a, b = handle(engine, pb), handle(engine, pb)
        same(a.solve(), b.solve())
        rows = new_rows(engine, dict(Q=Q, L=L, U=U), S, "QLU", 9)
        big = dict(rows)
        big["L"] = np.where(big["L"] == -np.inf, -1e40, big["L"]); big["U"] = np.where(big["U"] == np.inf, 1e40, big["U"])
        assert a.update(members=S, **rows) == 0
        assert b.update(members=S, **{k: dev.put(v) for k, v in big.items()}) == 0
        assert np.array_equal(a.solved_members(), b.solved_members())
        same(a.solve(), b.solve(), what=engine + ": device route")
        a.cleanup(); b.cleanup()


# ---- 4. the event session ----------------------------------------------------------------------------------------------
def test_event_session_common(gpu_lib):
    pb, S = problem("common"), np.asarray(LISTS["three"])
    P, A, Q, L, U = pb
    n, m = SHAPES["common"]
    rest = _rest(S)
    rng = np.random.default_rng(3)
    gx, gy = rng.standard_normal((B, 2, n)), rng.standard_normal((B, 2, m))
    tq, tl = rng.standard_normal((B, 2, n)), rng.standard_normal((B, 2, m))
    h, twin = handle("common", pb), handle("common", pb)
    same(h.solve(), twin.solve())
    cur = dict(Q=Q, L=L, U=U)
    rows = {k: v for w in "QLU" for k, v in new_rows("common", cur, S, w, 11).items()}      # new q, wider bounds: feasible
    assert h.update(members=S, **rows) == 0
    assert twin.update(**whole(cur, S, rows)) == 0
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.polish()
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.polish(members=S)
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.adjoint(gx[S], gy[S], members=S)
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.tangent(dQ=tq[S], members=S)
    served = h.polish(members=rest)                              # the others kept their right to be polished
    assert served.status_polish.shape == (len(rest),) and (served.status_polish == 1).any()
    again = h.polish(members=rest)
    same(again, served, what="a repeat does no work")
    assert np.array_equal(again.status_polish, served.status_polish)
    builds = h.kkt_info().builds
    assert np.all(h.solve(members=S).status_val[S] == 1)
    twin.solve(members=S); twin.solve(members=rest)
    assert h.solved_members().all()
    ph, pt = h.polish(members=S), twin.polish()
    same(ph, pt, i2=S, what="polish(members=S) against the S rows of polish()")
    assert np.array_equal(ph.status_polish, pt.status_polish[S])
    assert h.kkt_info().builds == builds + 1 and h.kkt_info().kept == 0
    ah, at = h.adjoint(gx[S], gy[S], matrices=True, members=S), twin.adjoint(gx, gy, matrices=True)
    same(ah, at, i2=S, fields=ADJ, what="adjoint(members=S)")
    info = h.kkt_info()
    assert info.builds == builds + 2 and info.kept == 1 and info.members == int((ah.status_adjoint != 0).sum()) == 3, info
    th, tt = h.tangent(dQ=tq[S], dL=tl[S], dU=tl[S], members=S), twin.tangent(dQ=tq, dL=tl, dU=tl)
    same(th, tt, i2=S, fields=TAN, what="tangent(members=S)")
    assert h.kkt_info() == info                                  # one build shared by the two calls
    other = S[:2]
    ao = h.adjoint(gx[other], gy[other], matrices=True, members=other)
    same(ao, at, i2=other, fields=ADJ, what="adjoint of another list")
    assert h.kkt_info().builds == builds + 3 and h.kkt_info().members == 2
    h.adjoint(gx, gy)                                            # a whole-batch call reuses only a whole-batch build
    assert h.kkt_info().builds == builds + 4 and h.kkt_info().members == B
    assert h.warm_start(X=np.zeros((1, n)), members=[0]) == 0    # any member update or warm start drops what is kept
    assert h.kkt_info().kept == 0
    h.cleanup(); twin.cleanup()


# ---- 5. planted truths -------------------------------------------------------------------------------------------------
def _planted_handle(c, engine, **kw):
    import osqp_amd
    if engine == "common":
        return osqp_amd.BatchOSQP().setup(c.P, c.A, c.Q, c.L, c.U, engine="common", shared_kkt=True, **{**c.settings, **kw})
    return osqp_amd.BatchOSQP().setup(c.P, c.A, c.Q, c.L, c.U, Px_all=c.Px_all if c.P.nnz else None, Ax_all=c.Ax_all,
                                      engine=engine, **{**c.settings, **kw})


def _planted_calls(h, c, S):
    """polish, adjoint with one and with three cotangents (the member's, twice the member's, zero) and tangent with
    pq.NDIR directions: for the members S (compact arrays) or, S = None, for the batch."""
    i = c.inc
    cut = (lambda a: a) if S is None else (lambda a: a[S])
    kw = {} if S is None else dict(members=S)
    gx3 = np.stack([i.gx, 2.0 * i.gx, np.zeros_like(i.gx)], axis=1)
    gy3 = np.stack([i.gy, 2.0 * i.gy, np.zeros_like(i.gy)], axis=1)
    p = h.polish(**kw)
    a1 = h.adjoint(cut(i.gx), cut(i.gy), matrices=True, **kw)
    a3 = h.adjoint(cut(gx3), cut(gy3), matrices=True, **kw)
    t = h.tangent(cut(i.dQ), cut(i.dL), cut(i.dU), cut(i.dPx) if c.P.nnz else None, cut(i.dAx), **kw)
    return p, a1, a3, t


# (case, engine, S, the padded order of S, that of the batch)
PLANTED = [("pad", "auto", [0, 1], 64, 96), ("pad", "streamed", [0, 1], 64, 96), ("rows", "common", [1], 32, 128),
           ("ns_exact", "common", [0, 2], 32, 32)]


@pytest.mark.parametrize("name,engine,S,order,whole_order", PLANTED, ids=["%s-%s" % p[:2] for p in PLANTED])
def test_planted_subsets(gpu_lib, name, engine, S, order, whole_order):
    """Subsets whose padded order (NPOL of the whole matrix; NS of the Schur complement on the common-K engine) is
    smaller than the batch's: the listed members against their truth at the bars of test_gpu_batch_planted.py, and to the
    bit against the S rows of the whole-batch calls on a twin."""
    c = cp.case(name) if engine == "common" else pq.case(name)
    S = np.asarray(S)
    h, w = _planted_handle(c, engine), _planted_handle(c, engine)
    r0 = h.solve(); same(r0, w.solve())
    ph, a1h, a3h, th = _planted_calls(h, c, S)
    info = h.kkt_info()
    pw, a1w, a3w, tw = _planted_calls(w, c, None)
    assert info.kept == 1 and info.npol == order and info.members == len(S), info
    assert w.kkt_info().npol == whole_order, w.kkt_info()
    same(ph, pw, i2=S, what="polish"); assert np.array_equal(ph.status_polish, pw.status_polish[S])
    same(a1h, a1w, i2=S, fields=ADJ, what="adjoint"); same(a3h, a3w, i2=S, fields=ADJ, what="adjoint, three cotangents")
    same(th, tw, i2=S, fields=TAN, what="tangent")
    assert a3h.dq.shape == (len(S), 3, c.n) and th.dx.shape == (len(S), pq.NDIR, c.n) and a1h.dAx.shape == (len(S), c.A.nnz)
    worst = {}
    ws0 = h.member_workspace(0)
    for k, b in enumerate(S):
        tag = (name, engine, int(b))
        assert r0.status_val[b] == 1 and ph.status_polish[k] == 1, tag
        tr = pq.truth(c, b)
        mo = kr.block_model(c, b, 3, ws=ws0) if engine == "common" else pq.model(c, b, 3, 1e-6, h.member_workspace(b))
        assert pq.accepts(mo.pri, mo.dua, r0.pri_res[b], r0.dua_res[b]), tag
        pq.check(tag, SimpleNamespace(x=ph.x[k], y=ph.y[k], obj=np.array([ph.obj_val[k]])), tr, mo, pq.POLISH, worst=worst)
        assert a1h.status_adjoint[k] == 1 and a3h.status_adjoint[k] == 1 and th.status_tangent[k] == 1, tag
        assert np.array_equal(a1h.active[k], c.act[b]) and np.array_equal(th.active[k], c.act[b]), tag
        pq.check(tag, SimpleNamespace(**{g: getattr(a1h, g)[k] for g in pq.ADJOINT}), tr, mo, pq.ADJOINT, worst=worst)
        pq.check(tag, SimpleNamespace(**{g: getattr(a3h, g)[k, 0] for g in pq.ADJOINT}), tr, mo, pq.ADJOINT, worst=worst)
        pq.check(tag, SimpleNamespace(**{g: 0.5 * getattr(a3h, g)[k, 1] for g in pq.ADJOINT}), tr, mo, pq.ADJOINT, worst=worst)
        assert all(not getattr(a3h, g)[k, 2].any() for g in pq.ADJOINT), tag
        pq.check(tag, SimpleNamespace(dx=th.dx[k], dy=th.dy[k]), tr, mo, pq.TANGENT, worst=worst)
    print(name, engine, "worst err / bar:", " ".join("%s %.3f" % kv for kv in worst.items()))
    h.cleanup(); w.cleanup()


@pytest.mark.parametrize("name,engine,S", [p[:3] for p in PLANTED[1:3]], ids=["%s-%s" % p[:2] for p in PLANTED[1:3]])
def test_members_that_did_not_end_solved(gpu_lib, name, engine, S):
    """max_iter = 1: nobody ends OSQP_SOLVED.  Status 0, outputs 0, nothing polished -- as the whole-batch calls say."""
    c = cp.case(name) if engine == "common" else pq.case(name)
    S = np.asarray(S)
    h, w = _planted_handle(c, engine, max_iter=1), _planted_handle(c, engine, max_iter=1)
    r0 = h.solve(); same(r0, w.solve())
    assert np.all(r0.status_val != 1)
    outs_h, outs_w = _planted_calls(h, c, S), _planted_calls(w, c, None)
    for oh, ow, fields in zip(outs_h, outs_w, (ARRAYS + ("status_polish",), ADJ, ADJ, TAN)):
        same(oh, ow, i2=S, fields=fields, what=name)
    p, a1, a3, t = outs_h
    same(p, r0, i2=S, what="nothing polished")
    assert not p.status_polish.any() and not a1.status_adjoint.any() and not a3.status_adjoint.any() and not t.status_tangent.any()
    for o, fields in ((a1, ADJ), (a3, ADJ), (t, TAN)):
        assert all(not getattr(o, f).any() for f in fields)
    assert h.kkt_info().kept == 0
    h.cleanup(); w.cleanup()


# ---- 6. chunks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["streamed", "common"])
def test_chunks(gpu_lib, monkeypatch, engine):
    """OSQP_AMD_BATCH_POLISH_CAP_BYTES (read at setup) at two members' matrices and five listed members: chunks of 2, 2
    and 1.  Bit-equal to the call in one chunk, and nothing is kept."""
    pb, S = problem(engine), np.array([0, 2, 3, 5, 8])
    n, m = SHAPES[engine]
    rng = np.random.default_rng(4)
    gx, gy, tq = rng.standard_normal((5, n)), rng.standard_normal((5, m)), rng.standard_normal((5, n))

    def calls(h):
        r = h.solve()
        assert (r.status_val[S] == 1).all()
        return h.polish(members=S), h.adjoint(gx, gy, matrices=True, members=S), h.tangent(dQ=tq, members=S)
    one = handle(engine, pb)
    outs1 = calls(one)
    info = one.kkt_info()
    assert info.kept == 1 and info.members == 5
    monkeypatch.setenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES", str(2 * info.npol * info.npol * 8))
    two = handle(engine, pb)
    monkeypatch.delenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES")
    outs2 = calls(two)
    assert two.kkt_info().kept == 0 and two.kkt_info().builds == 3
    for o1, o2, fields in zip(outs1, outs2, (ARRAYS + ("status_polish",), ADJ, TAN)):
        same(o1, o2, fields=fields, what="%s in chunks" % engine)
    one.cleanup(); two.cleanup()


# ---- 7. the gathers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_results_of_members(gpu_lib, dev, engine):
    pb = problem(engine)
    n, m = SHAPES[engine]
    h = handle(engine, pb)
    r = h.solve()
    for S in (LISTS["first"], LISTS["last"], LISTS["three"], LISTS["all"]):
        S = np.asarray(S)
        mask = np.zeros(B, bool); mask[S] = True
        for members in (S, mask, list(S)):
            rs = h.results(members=members)
            same(rs, r, i2=S, what="results(members=%s)" % (S,))
            for f in ("iter", "status_val", "obj_val", "pri_res", "dua_res", "rho_updates", "rho_estimate", "rho", "status_polish"):
                assert np.array_equal(getattr(rs, f), getattr(r, f)[S]), f
        R = len(S)
        guard = lambda cols: dev.put(np.full((R + 1, cols), 7.0), rows=R)
        X, Y, info, DX, DY = guard(n), guard(m), guard(8), guard(n), guard(m)
        h.results_into(X=X, Y=Y, info=info, DX=DX, DY=DY, members=S)
        for got, want in ((X, r.x), (Y, r.y), (info, r.info_raw), (DX, r.dual_inf_cert), (DY, r.prim_inf_cert)):
            g = got.get()
            assert np.array_equal(bits(g[:R]), bits(want[S])) and np.all(g[R] == 7.0), "exactly count rows are written"
    host = np.zeros((3, n))
    fake = SimpleNamespace(__cuda_array_interface__=dict(shape=(3, n), typestr="<f8", data=(host.ctypes.data, False),
                                                         version=2, strides=None))
    with pytest.raises(RuntimeError, match="not device memory"):
        h.results_into(X=fake, members=LISTS["three"])
    from osqp_amd import abi
    mem = np.array(LISTS["three"], np.int64)
    f = h._lib.osqp_amd_batch_get_members_dev
    assert f(h._h, abi.iptr(mem), 3, host.ctypes.data, None, None, None, None) == 1       # OSQP_DATA_VALIDATION_ERROR
    same(h.results(), r, what="after the refusals")
    h.cleanup()


def test_derivatives_into_device_arrays(gpu_lib, dev):
    """adjoint_into / tangent_into with members=: the bits of adjoint / tangent with members=, exactly count rows."""
    engine = "streamed"
    pb, S = problem(engine), np.asarray(LISTS["three"])
    n, m = SHAPES[engine]
    h = handle(engine, pb)
    h.solve()
    rng = np.random.default_rng(6)
    gx, gy, tq = rng.standard_normal((3, 2, n)), rng.standard_normal((3, 2, m)), rng.standard_normal((3, 2, n))
    a, t = h.adjoint(gx, gy, members=S), h.tangent(dQ=tq, members=S)
    guard = lambda *shape: dev.put(np.full((4,) + shape, 7.0), rows=3)
    dq, dl, du, dx, dy = guard(2, n), guard(2, m), guard(2, m), guard(2, n), guard(2, m)
    act, st = dev.put(np.full((4, m), 7), np.int32, rows=3), dev.put(np.full(4, 7), np.int32, rows=3)
    h.adjoint_into(dev.put(gx), dev.put(gy), dq, dl, du, active=act, status_adjoint=st, members=S)
    for got, want in ((dq, a.dq), (dl, a.dl), (du, a.du), (act, a.active), (st, a.status_adjoint)):
        g = got.get()
        assert np.array_equal(bits(g[:3].astype(want.dtype)), bits(want)) and np.all(g[3] == 7), "adjoint_into"
    h.tangent_into(dx, dy, dQ=dev.put(tq), members=S)
    for got, want in ((dx, t.dx), (dy, t.dy)):
        g = got.get()
        assert np.array_equal(bits(g[:3]), bits(want)) and np.all(g[3] == 7.0), "tangent_into"
    h.cleanup()


# ---- 8. refusals change nothing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_refusals_change_nothing(gpu_lib, engine):
    from osqp_amd import abi
    from osqp_amd.batch import MEMBER_CALLS
    pb = problem(engine)
    n, m = SHAPES[engine]
    h, ref = handle(engine, pb), handle(engine, pb)
    same(h.solve(), ref.solve())
    before = _snapshot(h)
    buf = np.zeros(4 * B * (n + 2 * m) + 64)                 # room for any compact argument, should a call get that far
    ibuf = np.zeros(B * (m + 1), np.int64)
    bad = (([3, 2], 2), ([1, 1], 2), ([0, B], 2), ([-1, 0], 2), ([0], 0), ([0], -1), (list(range(B + 1)), B + 1))
    for name, args in MEMBER_CALLS.items():
        if name.endswith("_dev"):
            rest = [1 if k == "n" else None for k in args]     # (no device pointer is looked at before the list)
        else:
            rest = [1 if k == "n" else abi.iptr(ibuf) if k == "i" else abi.fptr(buf) for k in args]
        f = getattr(h._lib, "osqp_amd_batch_" + name)
        for lst, count in bad:
            assert f(h._h, abi.iptr(np.array(lst, np.int64)), count, *rest) == 1, (name, lst)   # OSQP_DATA_VALIDATION_ERROR
        assert f(h._h, C.cast(None, abi.c_int_p), 1, *rest) == 1, name
    assert h._lib.osqp_amd_batch_solved_members(h._h, C.cast(None, abi.c_int_p)) == 1
    for lst in ([3, 2], [1, 1], [0, B], [-1, 0], [], np.ones(B - 1, bool), np.zeros(B, bool)):
        for call in (lambda: h.update(Q=np.zeros((2, n)), members=lst), lambda: h.warm_start(X=np.zeros((2, n)), members=lst),
                     lambda: h.polish(members=lst), lambda: h.results(members=lst)):
            with pytest.raises(ValueError):
                call()
    _unlisted_unchanged(h, before, [], "after the refusals")
    assert h.solved_members().all()
    same(h.solve(), ref.solve(), what="a whole solve after the refusals")
    h.cleanup(); ref.cleanup()


def test_common_without_shared_pieces_refuses(gpu_lib, capfd):
    """The polish, adjoint and tangent forms on a common-K handle without its shared KKT pieces: the twin's code and
    the twin's line on stderr, naming the call; update, warm_start and results with members= are served."""
    import osqp_amd
    from osqp_amd import abi
    P, A, Q, L, U = problem("common")
    n, m = SHAPES["common"]
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **FIXED_RHO["common"])
    r = h.solve()
    mem = np.array([1, 2], np.int64)
    z = np.zeros((2, n + m + 8))
    i2 = np.zeros(2 * (m + 1), np.int64)
    for name, args in (("polish_members", [abi.iptr(i2)]),
                       ("adjoint_members", [1] + [abi.fptr(z)] * 7 + [abi.iptr(i2)] * 2),
                       ("tangent_members", [1] + [abi.fptr(z)] * 7 + [abi.iptr(i2)] * 2)):
        capfd.readouterr()
        assert getattr(h._lib, "osqp_amd_batch_" + name)(h._h, abi.iptr(mem), 2, *args) == 4     # OSQP_LINSYS_SOLVER_INIT_ERROR
        err = capfd.readouterr().err
        assert "osqp_amd_batch_" + name in err and "shared KKT pieces" in err, err
    with pytest.raises(RuntimeError, match="shared KKT pieces"):
        h.polish(members=[1, 2])
    same(h.results(members=[1, 2]), r, i2=[1, 2])
    assert h.update(Q=Q[[1, 2]] * 1.5, members=[1, 2]) == 0 and h.warm_start(X=np.zeros((2, n)), members=[1, 2]) == 0
    assert np.array_equal(h.solved_members(), np.array([True, False, False] + [True] * (B - 3)))
    h.cleanup()
