"""Polish, adjoint and tangent of the common-K engine on its shared KKT pieces (osqp_amd_batch_common_kkt,
osqp_amd/csrc/batch_common_kkt.h): H = (P~ + delta I)^-1 and Wt = A~ H once per handle, S = Ar H Ar' + delta I per member.

References, none of them the device's own: the long-double truth of the pieces (_common_kkt_reference.pieces_truth) on
the handle's scaled values; the pre-scaled CPU oracle with polish = 1 and _adjoint_reference / _tangent_reference at its
point on the family cases, at the project's parity bar (1e-6 relative, objective 1e-8), with test_gpu_batch_adjoint.py's
excuse rule (test_common_kkt_reference_host.py shows who is excused at these seeds); the planted truth of
_common_planted.py under _planted_qp.bar with the float64 model of the block route.  The family shapes and the planted
cases, and why each is there, are listed in _common_kkt_reference.FAMILY and _common_planted._build."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _common_kkt_reference as kr
import _common_planted as cp
import _planted_qp as pq
from _batch_parity import rel
from _common_cases import MIXED

pytestmark = pytest.mark.gpu

GRADS = ("dq", "dl", "du", "dPx", "dAx")
RESULT = ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert")


def _handle(P, A, Q, L, U, shared=True, engine="common", **kw):
    import osqp_amd
    extra = dict(shared_kkt=shared) if engine == "common" else {}
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **extra, **kw)


def _same(a, b, fields=RESULT):
    return all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) for k in fields)


def _rows(active):
    return np.concatenate([np.flatnonzero(active < 0), np.flatnonzero(active > 0)]).astype(np.int64)


# ---- 1. the gate ---------------------------------------------------------------------------------------------------
def test_gate(gpu_lib, capfd):
    P, A, Q, L, U = kr.family(kr.FAMILY[2])
    h, twin = _handle(P, A, Q, L, U, shared=False, **kr.FAMILY_KW), _handle(P, A, Q, L, U, shared=False, **kr.FAMILY_KW)
    assert _same(h.solve(), twin.solve())
    with pytest.raises(RuntimeError, match="common-K"):
        h.polish()
    h.shared_kkt(True)
    H0 = h.shared_kkt_peek()
    h.shared_kkt(True)                                    # a second enable is a no-op
    H1 = h.shared_kkt_peek()
    assert np.array_equal(H0["H"], H1["H"]) and np.array_equal(H0["Wt"], H1["Wt"]) and h.kkt_info().builds == 0
    assert _same(h.solve(), twin.solve())
    a = h.adjoint(np.ones_like(Q), np.ones_like(L))
    assert np.all(a.status_adjoint == 1) and h.kkt_info().kept == 1
    h.shared_kkt(False)
    for call in (h.polish, lambda: h.adjoint(np.zeros_like(Q)), h.tangent, h.kkt_info, h.shared_kkt_peek):
        with pytest.raises(RuntimeError):
            call()
    capfd.readouterr()
    assert h._lib.osqp_amd_batch_polish(h._h, None) == 4
    err = capfd.readouterr().err
    assert "osqp_amd_batch_polish " in err and "common-K" in err and "osqp_amd_batch_common_kkt" in err, err
    assert _same(h.solve(), twin.solve())
    h.shared_kkt(True)                                    # and on again, on a solved handle
    with pytest.raises(RuntimeError, match="common-K"):
        h.update_matrices(Px=np.ones(h.Pu.nnz))            # never served
    assert h._lib.osqp_amd_batch_update_matrices(h._h, None, None, 0, 0, None, None, 0, 0) == 4
    assert np.all(h.polish().status_polish == 1)
    hs = _handle(P, A, Q, L, U, engine="streamed", **kr.FAMILY_KW)
    capfd.readouterr()
    assert hs._lib.osqp_amd_batch_common_kkt(hs._h, 1) == 4
    assert "common-K" in capfd.readouterr().err
    with pytest.raises(RuntimeError, match=r"\(4\)"):
        hs.shared_kkt()


# ---- 2. the pieces -------------------------------------------------------------------------------------------------
def _check_pieces(h, P, A, what, sinv=True):
    """H, Wt and, of every member with active rows, S^-1 (sinv=False: its shape and padding alone).  Returns how many
    S^-1 were held to the accuracy bar; the callers assert that count."""
    ws = h.member_workspace(0)
    Ps, As = kr.scaled_dense(kr.sparse_triu(P), A.tocsc(), ws)
    n, m = h.n, h.m
    pk = h.shared_kkt_peek()
    NP = pk["NP"]
    assert NP == (n + 31) // 32 * 32
    pad = np.eye(NP); pad[:n, :n] = pk["H"][:n, :n]
    assert np.array_equal(pk["H"], pad), (what, "H: padding is not the identity")
    assert not pk["Wt"][:, n:].any(), (what, "Wt: padding is not zero")
    tr = kr.pieces_truth(Ps, As, None)
    for name, got in (("H", pk["H"][:n, :n]), ("Wt", pk["Wt"][:, :n])):
        e, bar = pq.err(got, tr[name][0]), kr.piece_bar(*tr[name])
        print(what, name, "err %.2e bar %.2e" % (e, bar))
        assert e <= bar, (what, name, e, bar)
    a = h.adjoint(np.ones((h.B, n)), np.ones((h.B, m)))
    checked = 0
    assert np.all(a.status_adjoint == 1), (what, a.status_adjoint)
    for b in range(h.B):
        pm = h.shared_kkt_peek(b)
        rows = _rows(a.active[b])
        mred, NS = pm["mred"], pm["NS"]
        assert mred == rows.size and NS == max(32, (max(int(np.count_nonzero(x)) for x in a.active) + 31) // 32 * 32)
        pad = np.eye(NS); pad[:mred, :mred] = pm["Sinv"][:mred, :mred]
        assert np.array_equal(pm["Sinv"], pad), (what, b, "S^-1: padding is not the identity")
        if not mred or not sinv:
            continue
        t = kr.pieces_truth(Ps, As, rows)["Sinv"]
        cond = np.linalg.cond(np.linalg.inv(t[0]))
        if cond > 1e5:                                     # as check_member_kinv: numpy's own inverse is no yardstick there
            print(what, "S^-1 of member", b, "not held to the bar: cond(S) = %.1e" % cond)
            continue
        e, bar = pq.err(pm["Sinv"][:mred, :mred], t[0]), kr.piece_bar(*t)
        print(what, "S^-1 of member", b, "mred", mred, "err %.2e bar %.2e" % (e, bar))
        assert e <= bar, (what, b, e, bar)
        checked += 1
    return checked


@pytest.mark.parametrize("shape", kr.FAMILY, ids=str)
def test_pieces_family(gpu_lib, shape):
    P, A, Q, L, U = kr.family(shape)
    h = _handle(P, A, Q, L, U, **kr.FAMILY_KW)
    assert np.all(h.solve().status_val == 1)
    checked = _check_pieces(h, P, A, str(shape))
    assert checked >= (min(2, h.B) if shape[:2] != (1, 1) else 1) if h.m else checked == 0, (shape, checked)


@pytest.mark.parametrize("name", ["ns_exact", "lp", "rows"])
def test_pieces_planted(gpu_lib, name):
    c = cp.case(name)
    h = _handle(c.P, c.A, c.Q, c.L, c.U)
    assert np.all(h.solve().status_val == 1)
    # rows: variables without P entries put 1 / delta into H and cond(S) is past 1e5 in both members, where numpy's own
    # inverse is no yardstick (check_member_kinv's rule): there H, Wt, the shapes and the paddings are checked here and S^-1
    # through the outputs of test_planted[rows]
    checked = _check_pieces(h, c.P, c.A, name, sinv=name != "rows")
    assert checked == (0 if name == "rows" else c.B), (name, checked)


# ---- 3. polish, 4. adjoint and tangent: the family against the oracle ------------------------------------------------
def _duality(tag, dr, b, a, t):
    lhs = [dr.gx[b] @ t.dx[b], dr.gy[b] @ t.dy[b]]
    rhs = [a.dq[b] @ dr.dq[b], a.dl[b] @ dr.dl[b], a.du[b] @ dr.du[b], a.dPx[b] @ dr.dPx[b], a.dAx[b] @ dr.dAx[b]]
    gap, size = abs(sum(lhs) - sum(rhs)), max(1.0, sum(abs(v) for v in lhs + rhs))
    assert gap <= 1e-9 * size, tag + ("duality", gap, size)
    return gap / size


@pytest.mark.parametrize("shape", kr.FAMILY, ids=str)
def test_family(gpu_lib, oracle_mod, shape):
    P, A, Q, L, U = kr.family(shape)
    ws, dr, refs = kr.family_references(oracle_mod, shape)
    h = _handle(P, A, Q, L, U, **kr.FAMILY_KW)
    r0 = h.solve()
    r = h.polish()
    a = h.adjoint(dr.gx, dr.gy, matrices=True)
    t = h.tangent(dr.dq, dr.dl, dr.du, dr.dPx if h.Pu.nnz else None, dr.dAx if h.Ah.nnz else None)
    compared = 0
    for b, ref in enumerate(refs):
        tag = (shape, b)
        assert r0.status_val[b] == ref.status_val == 1, tag + (int(r0.status_val[b]), ref.status_val)
        assert r.status_polish[b] == ref.status_polish, tag + (int(r.status_polish[b]), ref.status_polish)
        assert a.status_adjoint[b] == 1 and t.status_tangent[b] == 1, tag
        if ref.status_polish != 1:
            continue
        assert rel(r.x[b], ref.x) < 1e-6 and rel(r.y[b], ref.y) < 1e-6, tag + (rel(r.x[b], ref.x), rel(r.y[b], ref.y))
        assert abs(r.obj_val[b] - ref.obj) <= 1e-8 * max(1.0, abs(ref.obj)), tag + (r.obj_val[b], ref.obj)
        why = kr.excuse(ref.adj) or ("tangent route %.1e" % ref.tan.route_err if ref.tan.route_err > 1e-7 else "")
        if why:
            print(shape, b, "excused:", why)
            continue
        assert np.array_equal(a.active[b], ref.adj.active) and np.array_equal(t.active[b], ref.tan.active), tag
        errs = {g: rel(getattr(a, g)[b], getattr(ref.adj, g)) for g in GRADS}
        errs.update(dx=rel(t.dx[b], ref.tan.dx), dy=rel(t.dy[b], ref.tan.dy))
        d = _duality(tag, dr, b, a, t)
        print(shape, b, " ".join("%s %.1e" % kv for kv in errs.items()), "duality %.1e" % d)
        assert all(e < 1e-6 for e in errs.values()), tag + (errs,)
        compared += 1
    assert compared >= min(2, len(refs)), (shape, compared)
    # a warm solve after an accepted polish starts from the polished point: one check interval and it is done
    rw = h.solve()
    ok = r.status_polish == 1
    assert np.all(rw.iter <= r0.iter) and np.all(rw.iter[ok] == 25), (shape, rw.iter, r0.iter)


def test_mixed_family(gpu_lib, oracle_mod):
    """A primal- and a dual-infeasible member: not tried, outputs zero, the neighbours as without them."""
    P, A, Q, L, U = kr.family("mixed")
    ws, dr, refs = kr.family_references(oracle_mod, "mixed")
    pinf, dinf = MIXED["pinf"], MIXED["dinf"]
    h = _handle(P, A, Q, L, U, **kr.FAMILY_KW)
    r0 = h.solve()
    assert [int(v) for v in r0.status_val] == [rf.status_val for rf in refs]
    r = h.polish()
    a = h.adjoint(dr.gx, dr.gy, matrices=True)
    t = h.tangent(dr.dq, dr.dl, dr.du, dr.dPx, dr.dAx)
    for b, ref in enumerate(refs):
        if b in (pinf, dinf):
            assert r.status_polish[b] == 0 and a.status_adjoint[b] == 0 and t.status_tangent[b] == 0, b
            assert all(not getattr(a, g)[b].any() for g in GRADS + ("active",)) and not t.dx[b].any() and not t.dy[b].any(), b
            assert _same(SimpleNamespace(**{k: getattr(r, k)[b] for k in RESULT}), SimpleNamespace(**{k: getattr(r0, k)[b] for k in RESULT}))
            continue
        assert r.status_polish[b] == ref.status_polish and a.status_adjoint[b] in (1, -1), b
        if ref.status_polish == 1:                       # (x is unique; the two equal equality rows leave y free)
            assert rel(r.x[b], ref.x) < 1e-6 and abs(r.obj_val[b] - ref.obj) <= 1e-8 * max(1.0, abs(ref.obj)), b
    keep = [b for b in range(Q.shape[0]) if b not in (pinf, dinf)]
    h2 = _handle(P, A, Q[keep], L[keep], U[keep], **kr.FAMILY_KW)
    h2.solve(fetch=False)
    r2 = h2.polish()
    a2 = h2.adjoint(dr.gx[keep], dr.gy[keep], matrices=True)
    # (the common scaling is that of the batch without the two, _common_cases.mixed_family: the neighbours' bits stay)
    assert np.array_equal(r2.x, r.x[keep]) and np.array_equal(r2.y, r.y[keep])
    assert all(np.array_equal(getattr(a2, g), getattr(a, g)[keep]) for g in GRADS)


# ---- the planted cases against the truth -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cp.CASES)
def test_planted(gpu_lib, name):
    c = cp.case(name)
    i = c.inc
    h = _handle(c.P, c.A, c.Q, c.L, c.U, **c.settings)
    r0 = h.solve()
    r = h.polish()
    a = h.adjoint(i.gx, i.gy, matrices=True)
    t = h.tangent(i.dQ, i.dL, i.dU, i.dPx if c.P.nnz else None, i.dAx)
    ws = h.member_workspace(0)
    info = h.kkt_info()
    mmax = max(int(np.count_nonzero(x)) for x in c.act)
    assert info.kept == 1 and info.npol == max(32, (mmax + 31) // 32 * 32) and info.members == c.B, info
    worst = {}
    for b in range(c.B):
        tag = (name, b)
        assert r0.status_val[b] == 1 and r.status_polish[b] == 1, tag + (int(r0.status_val[b]), int(r.status_polish[b]))
        tr, mo = pq.truth(c, b), kr.block_model(c, b, 3, ws=ws)
        assert pq.accepts(mo.pri, mo.dua, r0.pri_res[b], r0.dua_res[b]), tag
        pq.check(tag, SimpleNamespace(x=r.x[b], y=r.y[b], obj=np.array([r.obj_val[b]])), tr, mo, pq.POLISH, worst=worst)
        assert a.status_adjoint[b] == 1 and t.status_tangent[b] == 1, tag
        assert np.array_equal(a.active[b], c.act[b]) and np.array_equal(t.active[b], c.act[b]), tag
        pq.check(tag, SimpleNamespace(**{g: getattr(a, g)[b] for g in pq.ADJOINT}), tr, mo, pq.ADJOINT, worst=worst)
        pq.check(tag, SimpleNamespace(dx=t.dx[b], dy=t.dy[b]), tr, mo, pq.TANGENT, worst=worst)
    print(name, "worst err / bar:", " ".join("%s %.3f" % kv for kv in worst.items()))


@pytest.mark.parametrize("k", [0, 1])
def test_refinement_steps(gpu_lib, k):
    """Exactly polish_refine_iter steps with delta in both H and S: at 0 and 1 steps the error of the adjoint and the
    tangent is the regularisation error and must be the block model's within 10x either way (the two-sided bar of
    test_gpu_batch_planted.py; test_common_kkt_reference_host.py shows that a missing delta or a step too few or too many
    misses it).  No polish: at so few steps its acceptance rule turns points down; the point is the ADMM iterate."""
    c = cp.case("ns_exact")
    i = c.inc
    h = _handle(c.P, c.A, c.Q, c.L, c.U, polish_refine_iter=k, **c.settings)
    r0 = h.solve()
    a = h.adjoint(i.gx, i.gy, matrices=True)
    t = h.tangent(i.dQ, i.dL, i.dU, i.dPx, i.dAx)
    ws = h.member_workspace(0)
    worst = {}
    for b in range(c.B):
        tag = ("ns_exact k=%d" % k, b)
        assert r0.status_val[b] == 1 and a.status_adjoint[b] == 1 and t.status_tangent[b] == 1, tag
        assert np.array_equal(a.active[b], c.act[b]), tag
        mo = kr.block_model(c, b, k, ws=ws, point=(r0.x[b], r0.y[b]))
        ta = pq.truth_at(c, b, r0.x[b], r0.y[b])
        pq.check(tag, SimpleNamespace(**{g: getattr(a, g)[b] for g in pq.ADJOINT}), ta, mo, pq.ADJOINT, True, worst)
        pq.check(tag, SimpleNamespace(dx=t.dx[b], dy=t.dy[b]), ta, mo, pq.TANGENT, True, worst)
    print("ns_exact k =", k, "worst err / bar:", " ".join("%s %.3f" % kv for kv in worst.items()))


# ---- 5. bits -------------------------------------------------------------------------------------------------------
def _calls(h, dr):
    """adjoint and tangent with the draws"""
    return h.adjoint(dr.gx, dr.gy, matrices=True), h.tangent(dr.dq, dr.dl, dr.du, dr.dPx, dr.dAx)


def _wide(dr, D):
    """The draws as [B, D, .] arrays: slice 0 the draws themselves, the others random, each slice different."""
    rng = np.random.default_rng(99)
    wide = lambda v: np.concatenate([v[:, None, :], rng.standard_normal((v.shape[0], D - 1, v.shape[1]))], axis=1)
    return SimpleNamespace(**{k: wide(getattr(dr, k)) for k in ("gx", "gy", "dq", "dl", "du", "dPx", "dAx")})


def test_slices_and_chunks(gpu_lib, oracle_mod, monkeypatch):
    shape = kr.FAMILY[2]
    P, A, Q, L, U = kr.family(shape)
    _, dr, _ = kr.family_references(oracle_mod, shape)
    h = _handle(P, A, Q, L, U, **kr.FAMILY_KW)
    h.solve(fetch=False)
    a1, t1 = _calls(h, dr)
    # D = 3 in one call equals three D = 1 calls, slice by slice, every gradient and dx / dy
    w = _wide(dr, 3)
    a3, t3 = _calls(h, w)
    assert a3.dq.shape == (h.B, 3, h.n) and t3.dx.shape == (h.B, 3, h.n)
    for d in range(3):
        one = SimpleNamespace(**{k: np.ascontiguousarray(v[:, d]) for k, v in vars(w).items()})
        ad, td = _calls(h, one)
        for g in GRADS:
            assert np.array_equal(getattr(a3, g)[:, d], getattr(ad, g)), (g, d)
        assert np.array_equal(t3.dx[:, d], td.dx) and np.array_equal(t3.dy[:, d], td.dy), d
        assert np.array_equal(a3.active, ad.active) and np.array_equal(t3.active, td.active), d
        assert np.array_equal(a3.status_adjoint, ad.status_adjoint) and np.array_equal(t3.status_tangent, td.status_tangent), d
        assert np.any(ad.dq != a1.dq) == (d > 0)                  # (the slices are different problems: slice 0 is the draws)
    assert h.kkt_info().builds == 1
    rp = h.polish()
    NS = 32
    assert max(int(np.count_nonzero(x)) for x in a1.active) <= NS
    monkeypatch.setenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES", str(NS * NS * 8))      # one member's S per chunk
    hc = _handle(P, A, Q, L, U, **kr.FAMILY_KW)
    hc.solve(fetch=False)
    ac, tc = _calls(hc, dr)
    info = hc.kkt_info()
    assert info.kept == 0 and info.builds == 2, info      # with more than one chunk nothing is kept
    assert _same(ac, a1, GRADS + ("active", "status_adjoint")) and _same(tc, t1, ("dx", "dy", "active", "status_tangent"))
    assert _same(hc.polish(), rp, RESULT + ("status_polish",))


def test_position_in_the_batch(gpu_lib, oracle_mod):
    """Member 3 of 5 and the same member alone, without scaling (the common scaling depends on the batch) and with a
    fixed rho: every bit of polish, adjoint and tangent."""
    shape = kr.FAMILY[2]
    P, A, Q, L, U = kr.family(shape)
    _, dr, _ = kr.family_references(oracle_mod, shape)
    kw = dict(kr.FAMILY_KW, scaling=0, eps_abs=1e-3, eps_rel=1e-3)
    one = SimpleNamespace(**{k: getattr(dr, k)[3:4] for k in ("gx", "gy", "dq", "dl", "du", "dPx", "dAx")})
    outs = []
    for sl, d in ((slice(None), dr), (slice(3, 4), one)):
        h = _handle(P, A, Q[sl], L[sl], U[sl], **kw)
        r0 = h.solve()
        a, t = _calls(h, d)
        outs.append((r0, a, t, h.polish()))
    (r5, a5, t5, p5), (r1, a1, t1, p1) = outs
    assert r5.status_val[3] == 1 and r1.status_val[0] == 1
    pick = lambda o, k, b: getattr(o, k)[b]
    for k in RESULT:
        assert np.array_equal(pick(r5, k, 3), pick(r1, k, 0)) and np.array_equal(pick(p5, k, 3), pick(p1, k, 0)), k
    assert all(np.array_equal(pick(a5, g, 3), pick(a1, g, 0)) for g in GRADS + ("active",))
    assert np.array_equal(t5.dx[3], t1.dx[0]) and np.array_equal(t5.dy[3], t1.dy[0])


# ---- 6. state ------------------------------------------------------------------------------------------------------
def test_state(gpu_lib, oracle_mod):
    shape = kr.FAMILY[2]
    P, A, Q, L, U = kr.family(shape)
    _, dr, _ = kr.family_references(oracle_mod, shape)
    h, twin = _handle(P, A, Q, L, U, **kr.FAMILY_KW), _handle(P, A, Q, L, U, **kr.FAMILY_KW)
    pk0 = h.shared_kkt_peek()
    same_pieces = lambda: all(np.array_equal(pk0[k], h.shared_kkt_peek()[k]) for k in ("H", "Wt"))
    h.solve(fetch=False); twin.solve(fetch=False)
    assert h.kkt_info() == (0, 0, 0, 0)
    _calls(h, dr); h.adjoint(dr.gx, dr.gy)
    info = h.kkt_info()
    assert info.builds == 1 and info.kept == 1 and info.npol == 32 and info.members == h.B, info
    assert _same(h.results(), twin.results())
    for b in (0, h.B - 1):
        w, wt = h.member_workspace(b), twin.member_workspace(b)
        assert all(np.array_equal(w[k], wt[k]) for k in w), b
    assert _same(h.polish(), twin.polish(), RESULT + ("status_polish",))      # a working polish: on the same bits, and it drops
    assert h.kkt_info().kept == 0 and h.kkt_info().builds == 2
    h.adjoint(dr.gx, dr.gy)
    assert h.kkt_info().kept == 1
    assert _same(h.polish(), twin.polish(), RESULT + ("status_polish",)) and h.kkt_info().kept == 1     # a repeated polish drops nothing
    # what drops the kept inversion, and what leaves H and Wt alone
    h.solve(fetch=False)
    assert h.kkt_info().kept == 0
    h.adjoint(dr.gx, dr.gy)
    assert h.kkt_info().kept == 1 and h.update(Q=Q * 1.5) == 0 and h.kkt_info().kept == 0 and same_pieces()
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.adjoint(dr.gx, dr.gy)
    h.solve(fetch=False); h.adjoint(dr.gx, dr.gy)
    assert h.kkt_info().kept == 1 and h.warm_start(X=np.zeros_like(Q)) == 0 and h.kkt_info().kept == 0
    assert h.update_rho(0.3) == 0 and same_pieces()
    h.solve(fetch=False)
    ct = h.member_workspace(0)["ctype"]
    row = int(np.flatnonzero(ct == 0)[0])
    Lm, Um = L.copy(), U.copy()
    Um[:, row] = Lm[:, row] = np.where(np.isfinite(L[:, row]), L[:, row], U[:, row])      # an inequality row becomes an equality row in every member
    assert h.update(L=Lm, U=Um) == 0
    r = h.solve()
    assert h.member_workspace(0)["ctype"][row] == 1 and same_pieces()
    a = h.adjoint(dr.gx, dr.gy)
    assert np.all(np.isin(a.status_adjoint[r.status_val == 1], (1, -1))) and not a.status_adjoint[r.status_val != 1].any()
    assert h.kkt_info().builds == 6


# ---- 7. the layer and the device route (torch: a process of its own) -----------------------------------------------
_worker_out = {}


def _worker(tmp_path_factory, route):
    if route not in _worker_out:
        from _common_kkt_layer_worker import SHAPE
        n, m, B, _ = SHAPE
        rng = np.random.default_rng(4242)
        d = dict(W=rng.standard_normal((B, n)), dq=rng.standard_normal((B, n)), dl=rng.standard_normal((B, m)),
                 du=rng.standard_normal((B, m)))
        tmp = tmp_path_factory.mktemp("common_kkt_layer_" + route)
        np.savez(tmp / "in.npz", **d)
        worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_common_kkt_layer_worker.py")
        p = subprocess.run([sys.executable, worker, route, str(tmp / "in.npz"), str(tmp / "out.npz")], capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        _worker_out[route] = (d, SimpleNamespace(**np.load(tmp / "out.npz")))
    return _worker_out[route]


@pytest.mark.parametrize("route", ["host", "dev"])
def test_layer(gpu_lib, oracle_mod, tmp_path_factory, route):
    """BatchQPLayer(engine="common", shared_kkt=True) against BatchQPLayer(engine="streamed") on the same inputs, at
    eps 1e-8 with polish: X, the gradients of sum(W X) with respect to Q, L, U and the forward_ad tangent of X within 1e-6
    on the members that _adjoint_reference, at either layer's point, does not excuse."""
    from _adjoint_reference import adjoint_reference
    from _common_kkt_layer_worker import SHAPE
    d, o = _worker(tmp_path_factory, route)
    P, A, Q, L, U = kr.family(SHAPE)
    g = lambda e, k: getattr(o, "%s_%s_%s" % (route, e, k))
    assert g("common", "route")[0] == g("streamed", "route")[0] == ("host" if route == "host" else "device")
    assert np.all(g("common", "status_polish") == 1) and np.all(g("streamed", "status_polish") == 1)
    compared = 0
    for b in range(Q.shape[0]):
        assert g("common", "status_adjoint")[b] == 1
        # (the layer returns no y here: the reference takes that of a CPU oracle run of the member's own problem)
        ref = adjoint_reference(P, A, L[b], U[b], g("streamed", "X")[b], _y_of(oracle_mod, P, A, Q, L, U, b), d["W"][b])
        why = kr.excuse(ref)
        if why:
            print(route, b, "excused:", why)
            continue
        errs = {k: rel(g("common", k)[b], g("streamed", k)[b]) for k in ("X", "gQ", "gL", "gU", "tX")}
        print(route, b, errs)
        assert all(v < 1e-6 for v in errs.values()), (route, b, errs)
        assert rel(g("common", "gQ")[b], ref.dq) < 1e-6, (route, b)
        compared += 1
    assert compared >= 2
    assert "takes no Px / Ax" in str(getattr(o, route + "_px_error")[0])
    msg, row = str(getattr(o, route + "_class_error")[0]), int(getattr(o, route + "_class_row")[0])
    assert "member 2" in msg and "row %d" % row in msg, msg


def _y_of(orc, P, A, Q, L, U, b):
    """y of member b from a CPU oracle run of its own problem at the layer's tolerances, polished."""
    from _batch_parity import oracle
    key = ("y", b)
    if key not in _worker_out:
        _worker_out[key] = oracle(orc, P, Q[b], A, L[b], U[b], eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, polish=1).solve().y
    return _worker_out[key]


def test_device_route(gpu_lib, oracle_mod, tmp_path_factory):
    """adjoint_into (D = 3), tangent_into and results_into(status_polish=) with torch CUDA tensors return the bits of the
    host calls."""
    _, o = _worker(tmp_path_factory, "dev")
    assert bool(o.routes_same)
    assert np.array_equal(o.status_polish_dev, o.status_polish_host) and np.all(o.status_polish_host == 1)
