"""The wrong-pivot verdict (-1) of polish, adjoint and tangent on the tiled and the streamed batch engine, through every
layer that has to step round the member whose slot of the KKT buffer is full of inf / NaN: k_bp_polish's early return,
bd_open's report, the zeroed staging, the verdict copy of a kept inversion (bd_run), the compact rows of a members=
call (pl.pos), the chunks that reuse the poisoned slot, the device-array routes and BatchQPLayer.

The batch is the case "wrongpivot" of tests/_planted_qp.py: four members on one pattern, one of which holds
[[1, 1], [1, 1]] on a decoupled pair of variables of P; with scaling = 0 and delta = 2^-60 the device's sweep meets the
pivot 0.0 there.  tests/test_planted_verdict_host.py proves on the CPU that it must (a float64 model of the sweep), that
the recipe needs both settings, and that every other member is inside the conditions of the planted cases.

Contract of the member with the wrong pivot: status_polish, status_adjoint, status_tangent -1; x, y, info_raw keep
solve()'s bits; every row of dq, dl, du, dPx, dAx, dx, dy and `active` is exactly 0.  Every other member: status 1,
active == the planted set, and its outputs against the truth of _planted_qp.py under pq.bar, with the model of the
device route (3 refinement steps, delta = 2^-60) evaluated on member_workspace -- the helpers and bars of
tests/test_gpu_batch_planted.py.  Everything else asserted here is an exact equality, and every float array any call
returns is finite everywhere."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _planted_qp as pq
from _members_cases import ARRAYS, Device, bits, same, same_workspace

pytestmark = pytest.mark.gpu

ENGINES = list(pq.ENGINES["wrongpivot"])
DELTA = pq.VERDICT_DELTA
ADJ = pq.ADJOINT + ("active", "status_adjoint")
TAN = pq.TANGENT + ("active", "status_tangent")
NPOL = 96
CAP = "OSQP_AMD_BATCH_POLISH_CAP_BYTES"


@pytest.fixture
def dev(gpu_lib):
    d = Device()
    yield d
    d.close()


def _handle(c, engine):
    import osqp_amd
    h = osqp_amd.BatchOSQP().setup(c.P, c.A, c.Q, c.L, c.U, Px_all=c.Px_all, Ax_all=c.Ax_all, engine=engine, **c.settings)
    assert h.shape()[0] == (1 if engine == "streamed" else 0)
    return h


def _finite(what, *outs):
    for o in outs:
        for k, v in vars(o).items():
            if isinstance(v, np.ndarray) and v.dtype == np.float64:
                assert np.isfinite(v).all(), (what, k, np.argwhere(~np.isfinite(v))[:4])


def _solve(h, c):
    r0 = h.solve()
    _finite("solve", r0)
    assert np.all(r0.status_val == 1) and np.all(r0.status_polish == 0), (r0.status_val, r0.status_polish)
    ws = h.member_workspace(c.singular)               # the device holds the very bits of the recipe
    assert np.array_equal(bits(ws["Pv"]), bits(c.Px_all[c.singular])) and np.all(ws["D"] == 1.0) and ws["c"] == 1.0
    return r0


def _cot3(c):
    """Three cotangents per member: the case's, twice the case's, zero."""
    i = c.inc
    return (np.stack([i.gx, 2.0 * i.gx, np.zeros_like(i.gx)], axis=1), np.stack([i.gy, 2.0 * i.gy, np.zeros_like(i.gy)], axis=1))


def _calls(h, c, S=None):
    """polish, adjoint with one and with three cotangents and the matrices, tangent with all five tangents and pq.NDIR
    directions: of the batch, or (compact arrays) of the members S."""
    i = c.inc
    cut = (lambda a: a) if S is None else (lambda a: a[np.asarray(S)])
    kw = {} if S is None else dict(members=S)
    gx3, gy3 = _cot3(c)
    p = h.polish(**kw)
    a1 = h.adjoint(cut(i.gx), cut(i.gy), matrices=True, **kw)
    a3 = h.adjoint(cut(gx3), cut(gy3), matrices=True, **kw)
    t = h.tangent(cut(i.dQ), cut(i.dL), cut(i.dU), cut(i.dPx), cut(i.dAx), **kw)
    out = SimpleNamespace(p=p, a1=a1, a3=a3, t=t)
    _finite("calls", p, a1, a3, t)
    return out


def _same_calls(x, y, what, rows=slice(None)):
    """The four results of _calls bit for bit; rows: the rows of y that x's rows are."""
    same(x.p, y.p, i2=rows, fields=ARRAYS + ("status_polish",), what=what + ": polish")
    same(x.a1, y.a1, i2=rows, fields=ADJ, what=what + ": adjoint")
    same(x.a3, y.a3, i2=rows, fields=ADJ, what=what + ": adjoint, three cotangents")
    same(x.t, y.t, i2=rows, fields=TAN, what=what + ": tangent")


def _contract(what, h, c, r0, out, S=None):
    """The module's contract on the results `out` of _calls after the solve r0: row k is member S[k] (None: the batch)."""
    members = list(range(c.B)) if S is None else [int(b) for b in S]
    R = len(members)
    p, a1, a3, t = out.p, out.a1, out.a3, out.t
    _finite(what, p, a1, a3, t)
    assert a1.dq.shape == (R, c.n) and a1.dPx.shape == (R, c.P.nnz) and a1.dAx.shape == (R, c.A.nnz) and a1.active.shape == (R, c.m)
    assert a3.dq.shape == (R, 3, c.n) and a3.dl.shape == (R, 3, c.m) and a3.dAx.shape == (R, 3, c.A.nnz)
    assert t.dx.shape == (R, pq.NDIR, c.n) and t.dy.shape == (R, pq.NDIR, c.m) and t.active.shape == (R, c.m)
    assert p.status_polish.shape == a1.status_adjoint.shape == a3.status_adjoint.shape == t.status_tangent.shape == (R,)
    worst = {}
    for k, b in enumerate(members):
        tag = (what, b)
        if b == c.singular:
            assert p.status_polish[k] == -1, tag + (int(p.status_polish[k]),)
            for f in ("x", "y", "info_raw"):
                assert np.array_equal(bits(getattr(p, f)[k]), bits(getattr(r0, f)[b])), tag + (f, "polish moved a rejected member")
            assert a1.status_adjoint[k] == -1 and a3.status_adjoint[k] == -1 and t.status_tangent[k] == -1, \
                tag + (int(a1.status_adjoint[k]), int(a3.status_adjoint[k]), int(t.status_tangent[k]))
            for o, fields in ((a1, pq.ADJOINT + ("active",)), (a3, pq.ADJOINT + ("active",)), (t, pq.TANGENT + ("active",))):
                for f in fields:
                    assert not getattr(o, f)[k].any(), tag + (f, "not zero")
            continue
        assert p.status_polish[k] == 1 and a1.status_adjoint[k] == 1 and a3.status_adjoint[k] == 1 and t.status_tangent[k] == 1, \
            tag + (int(p.status_polish[k]), int(a1.status_adjoint[k]), int(a3.status_adjoint[k]), int(t.status_tangent[k]))
        for o in (a1, a3, t):
            assert np.array_equal(o.active[k], c.act[b]), tag + (np.flatnonzero(o.active[k] != c.act[b]),)
        tr = pq.truth(c, b)
        mo = pq.model(c, b, 3, DELTA, h.member_workspace(b))
        assert pq.accepts(mo.pri, mo.dua, r0.pri_res[b], r0.dua_res[b]), tag + (mo.pri, mo.dua, r0.pri_res[b], r0.dua_res[b])
        pq.check(tag, SimpleNamespace(x=p.x[k], y=p.y[k], obj=np.array([p.obj_val[k]])), tr, mo, pq.POLISH, worst=worst)
        bp, bd = pq.residual_bars(tr, mo)
        assert p.pri_res[k] <= bp and p.dua_res[k] <= bd, tag + (p.pri_res[k], bp, p.dua_res[k], bd)
        pq.check(tag, SimpleNamespace(**{g: getattr(a1, g)[k] for g in pq.ADJOINT}), tr, mo, pq.ADJOINT, worst=worst)
        pq.check(tag, SimpleNamespace(**{g: getattr(a3, g)[k, 0] for g in pq.ADJOINT}), tr, mo, pq.ADJOINT, worst=worst)
        pq.check(tag, SimpleNamespace(**{g: 0.5 * getattr(a3, g)[k, 1] for g in pq.ADJOINT}), tr, mo, pq.ADJOINT, worst=worst)
        assert all(not getattr(a3, g)[k, 2].any() for g in pq.ADJOINT), tag + ("the zero cotangent",)
        pq.check(tag, SimpleNamespace(dx=t.dx[k], dy=t.dy[k]), tr, mo, pq.TANGENT, worst=worst)
    print(what, "worst err / bar:", " ".join("%s %.3f" % kv for kv in worst.items()))
    want = np.array([-1 if b == c.singular else 1 for b in members])
    for got in (p.status_polish, a1.status_adjoint, a3.status_adjoint, t.status_tangent):
        assert np.array_equal(got, want), (what, got, want)


# ---- (a) the whole batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_whole_batch(gpu_lib, engine):
    c = pq.case("wrongpivot")
    h = _handle(c, engine)
    r0 = _solve(h, c)
    out = _calls(h, c)
    _contract("whole batch %s" % engine, h, c, r0, out)
    again = h.polish()                                   # finds the work done and reports it again
    _finite("second polish", again)
    same(again, out.p, fields=ARRAYS + ("status_polish",), what="a second polish")
    r = h.results()
    _finite("results", r)
    assert np.array_equal(r.status_polish, [-1 if b == c.singular else 1 for b in range(c.B)])
    same(r, out.p, what="results after polish")
    h.cleanup()


# ---- (b) the kept inversion --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_kept_inversion(gpu_lib, monkeypatch, engine):
    """adjoint builds; tangent, adjoint [B, 3, .] and adjoint again run on the kept inversion, whose verdicts bd_run
    copies from kkt_piv into the call's own array.  A twin set up under OSQP_AMD_BATCH_KKT_CACHE=0 builds every time:
    the same statuses, the same bits."""
    c = pq.case("wrongpivot")
    i = c.inc
    gx3, gy3 = _cot3(c)
    h = _handle(c, engine)
    monkeypatch.setenv("OSQP_AMD_BATCH_KKT_CACHE", "0")
    tw = _handle(c, engine)
    monkeypatch.delenv("OSQP_AMD_BATCH_KKT_CACHE")
    outs = []
    for b in (h, tw):
        kept = b is h
        r0 = _solve(b, c)
        p = b.polish()
        builds = b.kkt_info().builds
        assert tuple(b.kkt_info())[1:] == (0, 0, 0)
        first = b.adjoint(i.gx, i.gy, matrices=True)
        assert tuple(b.kkt_info()) == ((builds + 1, 1, NPOL, c.B) if kept else (builds + 1, 0, 0, 0))
        t = b.tangent(i.dQ, i.dL, i.dU, i.dPx, i.dAx)
        a3 = b.adjoint(gx3, gy3, matrices=True)
        a1 = b.adjoint(i.gx, i.gy, matrices=True)
        assert tuple(b.kkt_info()) == ((builds + 1, 1, NPOL, c.B) if kept else (builds + 4, 0, 0, 0))
        _finite("kept" if kept else "twin", first)
        same(first, a1, fields=ADJ, what="the call that built against a call on what it kept")
        outs.append((r0, SimpleNamespace(p=p, a1=a1, a3=a3, t=t)))
    same(outs[0][0], outs[1][0], what="solve")
    _same_calls(outs[0][1], outs[1][1], "kept inversion against OSQP_AMD_BATCH_KKT_CACHE=0")
    _contract("kept inversion %s" % engine, h, c, *outs[0])
    h.cleanup(); tw.cleanup()


# ---- (c) chunks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_chunks(gpu_lib, monkeypatch, engine):
    """OSQP_AMD_BATCH_POLISH_CAP_BYTES (read at setup) at two members' matrices: chunks {0, 1} and {2, 3}, so member 3's
    matrix is formed in the slot member 1 left full of inf / NaN.  Bit-equal to the handle with one chunk; nothing kept."""
    c = pq.case("wrongpivot")
    assert c.singular == 1
    one = _handle(c, engine)
    r1 = _solve(one, c)
    out1 = _calls(one, c)
    assert tuple(one.kkt_info())[1:] == (1, NPOL, c.B)
    monkeypatch.setenv(CAP, str(2 * NPOL * NPOL * 8))
    two = _handle(c, engine)
    monkeypatch.delenv(CAP)
    r2 = _solve(two, c)
    out2 = _calls(two, c)
    assert tuple(two.kkt_info()) == (4, 0, 0, 0)          # polish and the three derivative calls each built, in two chunks
    same(r1, r2, what="solve")
    _same_calls(out2, out1, "two chunks against one")
    _contract("chunks %s" % engine, two, c, r2, out2)
    one.cleanup(); two.cleanup()


# ---- (d) member lists --------------------------------------------------------------------------------------------------
def _snapshot(h, B):
    return SimpleNamespace(r=h.results(), ws=[h.member_workspace(q) for q in range(B)], solved=h.solved_members())


@pytest.mark.parametrize("engine", ENGINES)
def test_member_lists(gpu_lib, engine):
    """members = S with the -1 member at compact row 0, at compact row 1, and not listed: the compact rows are the S rows
    of the whole-batch calls on a twin, the status sits in the member's compact row and nowhere else, and of the unlisted
    members nothing changes."""
    c = pq.case("wrongpivot")
    w = _handle(c, engine)
    rw = _solve(w, c)
    outw = _calls(w, c)
    counts = [int(np.count_nonzero(a)) for a in c.act]
    for S in ([1, 3], [0, 1], [0, 2]):
        what = "%s members=%s" % (engine, S)
        S = np.asarray(S)
        rest = np.setdiff1d(np.arange(c.B), S)
        h = _handle(c, engine)
        r0 = _solve(h, c)
        same(r0, rw, what=what + ": solve")
        before = _snapshot(h, c.B)
        out = _calls(h, c, S)
        info = h.kkt_info()
        assert (info.kept, info.npol, info.members) == (1, (c.n + max(counts[b] for b in S) + 31) & ~31, len(S)), info
        _same_calls(out, outw, what, rows=S)
        _contract(what, h, c, r0, out, S)
        now = _snapshot(h, c.B)
        same(now.r, before.r, rest, rest, what=what + ": an unlisted member's results")
        for q in rest:
            same_workspace(now.ws[q], before.ws[q], what + ": workspace of unlisted member %d" % q)
        assert np.array_equal(now.solved, before.solved) and now.solved.all(), what
        same(now.r, outw.p, S, S, what=what + ": the listed members' results")
        h.cleanup()
    w.cleanup()


# ---- (e) device arrays -------------------------------------------------------------------------------------------------
def _rows_equal(what, got, want, R, fill):
    """The first R rows of the device array carry want's bits; the guard row keeps its fill."""
    g = got.get()
    assert np.array_equal(bits(g[:R].astype(want.dtype)), bits(np.ascontiguousarray(want))), what
    assert np.all(g[R] == fill), what + ": more than count rows written"
    if g.dtype == np.float64:
        assert np.isfinite(g).all(), what


@pytest.mark.parametrize("engine", ENGINES)
def test_device_arrays(gpu_lib, dev, engine):
    """adjoint_into / tangent_into, whole batch ([B, 3, .] / [B, NDIR, .]) and members= (flat / [count, NDIR, .]), into
    arrays prefilled with 7.0 and 9: afterwards the -1 member's rows are 0, its status -1, its `active` 0, and everything
    is what the host-array call returns."""
    c = pq.case("wrongpivot")
    i, n, m, nP, nA, bad = c.inc, c.n, c.m, c.P.nnz, c.A.nnz, c.singular
    h = _handle(c, engine)
    _solve(h, c)
    h.polish()
    gx3, gy3 = _cot3(c)
    for S in (None, [1, 3], [0, 1]):
        what = "%s device arrays members=%s" % (engine, S)
        kw = {} if S is None else dict(members=S)
        rows = np.arange(c.B) if S is None else np.asarray(S)
        R = len(rows)
        lead = (3,) if S is None else ()                      # three cotangents for the batch, one (flat) for a list
        fl = lambda *shape: dev.put(np.full((R + 1,) + shape, 7.0), rows=R)
        it = lambda *shape: dev.put(np.full((R + 1,) + shape, 9), np.int32, rows=R)
        gx, gy = (gx3, gy3) if S is None else (i.gx[rows], i.gy[rows])
        a = h.adjoint(gx, gy, matrices=True, **kw)
        t = h.tangent(i.dQ[rows], i.dL[rows], i.dU[rows], i.dPx[rows], i.dAx[rows], **kw)
        _finite(what, a, t)
        g = dict(dq=fl(*lead, n), dl=fl(*lead, m), du=fl(*lead, m), dPx=fl(*lead, nP), dAx=fl(*lead, nA))
        act, st = it(m), it()
        h.adjoint_into(dev.put(gx), dev.put(gy), active=act, status_adjoint=st, **g, **kw)
        for k, v in g.items():
            _rows_equal(what + " " + k, v, getattr(a, k), R, 7.0)
        _rows_equal(what + " active", act, a.active, R, 9)
        _rows_equal(what + " status_adjoint", st, a.status_adjoint, R, 9)
        dx, dy, tact, tst = fl(pq.NDIR, n), fl(pq.NDIR, m), it(m), it()
        h.tangent_into(dx, dy, dQ=dev.put(i.dQ[rows]), dL=dev.put(i.dL[rows]), dU=dev.put(i.dU[rows]), dPx=dev.put(i.dPx[rows]),
                       dAx=dev.put(i.dAx[rows]), active=tact, status_tangent=tst, **kw)
        _rows_equal(what + " dx", dx, t.dx, R, 7.0)
        _rows_equal(what + " dy", dy, t.dy, R, 7.0)
        _rows_equal(what + " active (tangent)", tact, t.active, R, 9)
        _rows_equal(what + " status_tangent", tst, t.status_tangent, R, 9)
        k = int(np.flatnonzero(rows == bad)[0])
        want = np.ones(R, np.int32); want[k] = -1
        assert np.array_equal(st.get()[:R], want) and np.array_equal(tst.get()[:R], want), what
        for v in list(g.values()) + [dx, dy, act, tact]:
            got = v.get()
            assert not got[k].any(), what + ": the -1 member's row is not zero"
        for v in (g["dq"], dx, act):                           # (and the others' rows are not: the prefill was overwritten by results)
            got = v.get()
            assert all(got[r].any() and not np.all(got[r] == (9 if got.dtype == np.int32 else 7.0)) for r in range(R) if r != k), what
    h.cleanup()


# ---- (f) the verdict is not sticky -------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 1], ids=["0to1", "1to0"])
@pytest.mark.parametrize("engine", ENGINES)
def test_verdict_is_not_sticky(gpu_lib, engine, first):
    """update_matrices and update to the other variant, which carries the singular pair in another member: until the new
    solve the three calls refuse (7); after it the member that was -1 is served and compared with its truth, and the
    other one is -1."""
    ca, cb = pq.case("wrongpivot", first), pq.case("wrongpivot", 1 - first)
    assert ca.singular != cb.singular
    h = _handle(ca, engine)
    _contract("%s variant %d" % (engine, first), h, ca, _solve(h, ca), _calls(h, ca))
    assert h.update_matrices(Px=cb.Px_all, Ax=cb.Ax_all) == 0
    assert h.update(Q=cb.Q, L=cb.L, U=cb.U) == 0
    i = cb.inc
    for call in (h.polish, lambda: h.adjoint(i.gx, i.gy, matrices=True), lambda: h.tangent(i.dQ, i.dL, i.dU, i.dPx, i.dAx)):
        with pytest.raises(RuntimeError, match=r"\(7\)"):
            call()
    _contract("%s variant %d after variant %d" % (engine, 1 - first, first), h, cb, _solve(h, cb), _calls(h, cb))
    h.cleanup()


# ---- (g) BatchQPLayer --------------------------------------------------------------------------------------------------
def test_layer(gpu_lib, tmp_path):
    """One backward pass through BatchQPLayer on CPU tensors, per engine, in a child process
    (tests/_pivot_verdict_layer_worker.py): the -1 member's gradient rows are zero and finite and last_status_adjoint
    says -1; the others carry the bits of adjoint() on a handle that went the same way, which are held to their truth."""
    c = pq.case("wrongpivot")
    i, bad = c.inc, c.singular
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_pivot_verdict_layer_worker.py")
    p = subprocess.run([sys.executable, worker, str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = dict(np.load(tmp_path / "out.npz"))
    want_status = np.array([-1 if b == bad else 1 for b in range(c.B)])
    for engine in ENGINES:
        g = SimpleNamespace(**{k[len(engine) + 1:]: v for k, v in got.items() if k.startswith(engine + "_")})
        _finite("layer " + engine, g)
        h = _handle(c, engine)
        r0 = _solve(h, c)
        out = _calls(h, c)
        _contract("layer's twin %s" % engine, h, c, r0, out)
        assert np.all(g.status_val == 1)
        assert np.array_equal(g.status_polish, want_status) and np.array_equal(g.status_adjoint, want_status), engine
        assert np.array_equal(bits(g.X), bits(out.p.x)) and np.array_equal(bits(g.Y), bits(out.p.y)), engine
        for k in pq.ADJOINT:
            assert np.array_equal(bits(getattr(g, k)), bits(getattr(out.a1, k))), (engine, k)
            assert not getattr(g, k)[bad].any(), (engine, k)
        assert np.array_equal(bits(g.X[bad]), bits(r0.x[bad]))
        h.cleanup()
