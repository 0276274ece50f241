"""The polish / adjoint / tangent route of the batch engines (k_bp_active, k_bp_form, k_bp_invert, kkt_solve_refined,
then k_bp_polish, k_ba_adjoint or k_bt_tangent) on QPs whose solution and active set are planted
(tests/_planted_qp.py; tests/test_planted_qp_host.py proves on the CPU that every case stays inside its conditions and
that the oracle attains the bar).

Reference: the truth of _planted_qp.py -- a refined solve of the unregularised KKT system on the planted rows --
never the oracle's point.  Yardstick: its float64 model of the device route, evaluated on the scaled data the handle
returns through member_workspace (D, E, c, Pv, Av), then unscaled.  Bar, per output array:
err <= 10 err_model + 1e-14 max|truth| (pq.bar); with 0 or 1 refinement steps also err >= err_model / 10.  Every
member has its own P and A values (Px_all, Ax_all), its own active set and is compared: none is excused.

With 0 or 1 refinement steps polish.c's acceptance rule turns some polished points down (their residuals are the
regularisation error, 1e-6 .. 1e-3, next to ADMM's).  The rule is evaluated on the model's residuals and the
residuals solve() returned; the device must decide the same, a rejected member must keep solve()'s x, y and info
bit for bit, and its adjoint and tangent are compared at the point the handle then holds, the ADMM iterate."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import _planted_qp as pq

pytestmark = pytest.mark.gpu

CASE_ENGINES = [(name, e) for name in pq.CASES for e in pq.ENGINES[name]]


def _handle(c, engine, **kw):
    import osqp_amd
    bs = osqp_amd.BatchOSQP().setup(c.P, c.A, c.Q, c.L, c.U, Px_all=c.Px_all if c.P.nnz else None, Ax_all=c.Ax_all,
                                    engine=engine, **{**c.settings, **kw})
    assert bs.shape()[0] == (1 if engine == "streamed" else 0)
    return bs


def _calls(bs, c):
    """solve, polish, adjoint with both incoming gradients and the matrices, tangent with all five tangents and
    pq.NDIR directions (no dPx where P has no stored entry)."""
    i = c.inc
    r0 = bs.solve()
    assert np.all(r0.status_polish == 0)
    r = bs.polish()
    a = bs.adjoint(i.gx, i.gy, matrices=True)
    t = bs.tangent(i.dQ, i.dL, i.dU, i.dPx if c.P.nnz else None, i.dAx)
    return r0, r, a, t


def _check(what, bs, c, out, k=3, delta=1e-6, scaled=False, two_sided=False, must_accept=True):
    """Every member of the batch against its truth.  Returns the worst err / bar per output."""
    r0, r, a, t = out
    worst = {}
    assert a.dq.shape == (c.B, c.n) and a.dPx.shape == (c.B, c.P.nnz) and a.dAx.shape == (c.B, c.A.nnz)
    assert t.dx.shape == (c.B, pq.NDIR, c.n) and t.dy.shape == (c.B, pq.NDIR, c.m)
    for b in range(c.B):
        tag = (what, b)
        assert r0.status_val[b] == 1 and r.status_val[b] == 1, tag + (int(r0.status_val[b]),)
        tr = pq.truth(c, b)
        ws = bs.member_workspace(b)
        mo = pq.model(c, b, k, delta, ws)
        want = pq.accepts(mo.pri_s if scaled else mo.pri, mo.dua_s if scaled else mo.dua, r0.pri_res[b], r0.dua_res[b])
        if must_accept:
            assert want, tag + ("the model's polished point is not accepted", mo.pri, mo.dua, r0.pri_res[b], r0.dua_res[b])
        assert r.status_polish[b] == (1 if want else -1), tag + (int(r.status_polish[b]), want)
        if want:
            got = SimpleNamespace(x=r.x[b], y=r.y[b], obj=np.array([r.obj_val[b]]))
            pq.check(tag, got, tr, mo, pq.POLISH, two_sided, worst)
            bp, bd = pq.residual_bars(tr, mo, scaled)
            assert r.pri_res[b] <= bp and r.dua_res[b] <= bd, tag + (r.pri_res[b], bp, r.dua_res[b], bd)
            worst["pri_res"] = max(worst.get("pri_res", 0.0), r.pri_res[b] / bp if bp > 0 else 0.0)
            worst["dua_res"] = max(worst.get("dua_res", 0.0), r.dua_res[b] / bd)
            ta = tr
        else:
            for f in ("x", "y", "info_raw"):
                assert np.array_equal(getattr(r, f)[b], getattr(r0, f)[b]), tag + (f,)
            mo = pq.model(c, b, k, delta, ws, point=(r0.x[b], r0.y[b]))
            ta = pq.truth_at(c, b, r0.x[b], r0.y[b])
        assert a.status_adjoint[b] == 1 and t.status_tangent[b] == 1, tag + (int(a.status_adjoint[b]), int(t.status_tangent[b]))
        assert np.array_equal(a.active[b], c.act[b]), tag + (np.flatnonzero(a.active[b] != c.act[b]),)
        assert np.array_equal(t.active[b], c.act[b]), tag + (np.flatnonzero(t.active[b] != c.act[b]),)
        pq.check(tag, SimpleNamespace(**{g: getattr(a, g)[b] for g in pq.ADJOINT}), ta, mo, pq.ADJOINT, two_sided, worst)
        pq.check(tag, SimpleNamespace(dx=t.dx[b], dy=t.dy[b]), ta, mo, pq.TANGENT, two_sided, worst)
    print(what, "worst err / bar:", " ".join("%s %.3f" % kv for kv in worst.items()))
    return worst


@pytest.mark.parametrize("name,engine", CASE_ENGINES, ids=["%s-%s" % ce for ce in CASE_ENGINES])
def test_planted(gpu_lib, name, engine):
    c = pq.case(name)
    t0 = time.perf_counter()
    bs = _handle(c, engine)
    out = _calls(bs, c)
    t1 = time.perf_counter()
    _check("%s %s" % (name, engine), bs, c, out)
    print(name, engine, "device calls %.2f s, references %.2f s" % (t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("engine", ["auto", "streamed"])
@pytest.mark.parametrize("delta", [1e-6, 1e-4])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_refinement_steps_and_delta(gpu_lib, k, delta, engine):
    """Exactly polish_refine_iter steps with the handle's delta: at 0 and 1 steps the error is the regularisation
    error and must be the model's within 10x either way."""
    c = pq.case("pad")
    bs = _handle(c, engine, polish_refine_iter=k, delta=delta)
    _check("pad %s k=%d delta=%g" % (engine, k, delta), bs, c, _calls(bs, c), k=k, delta=delta, two_sided=k < 2,
           must_accept=k >= 2)


@pytest.mark.parametrize("engine", ["auto", "streamed"])
@pytest.mark.parametrize("kw", [dict(scaling=0), dict(scaled_termination=1)], ids=["scaling0", "scaled_termination"])
def test_scaling_switches(gpu_lib, kw, engine):
    """The same truth without scaling, and with the residuals of the scaled problem (k_bp_polish's `unscaled` switch)."""
    c = pq.case("pad")
    bs = _handle(c, engine, **kw)
    ws = bs.member_workspace(0)
    assert (np.all(ws["D"] == 1.0) and ws["c"] == 1.0) == ("scaling" in kw)
    _check("pad %s %s" % (engine, kw), bs, c, _calls(bs, c), scaled="scaled_termination" in kw)


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_update_sequence(gpu_lib, engine):
    """update_matrices and update to a second planted problem on the same patterns: other values, so other D and E,
    and other active sets.  Until the new solve the three calls refuse (7); after it everything holds again."""
    c0, c1 = pq.case("pad"), pq.case("pad", 1)
    bs = _handle(c0, engine)
    _check("pad %s before the update" % engine, bs, c0, _calls(bs, c0))
    before = [bs.member_workspace(b) for b in range(c0.B)]
    assert bs.update_matrices(Px=c1.Px_all, Ax=c1.Ax_all) == 0
    assert bs.update(Q=c1.Q, L=c1.L, U=c1.U) == 0
    i = c1.inc
    for call in (bs.polish, lambda: bs.adjoint(i.gx, i.gy, matrices=True), lambda: bs.tangent(i.dQ, i.dL, i.dU, i.dPx, i.dAx)):
        with pytest.raises(RuntimeError, match=r"\(7\)"):
            call()
    for b, w0 in enumerate(before):
        w1 = bs.member_workspace(b)
        assert not np.allclose(w0["D"], w1["D"], rtol=1e-3, atol=0) and not np.allclose(w0["E"], w1["E"], rtol=1e-3, atol=0), b
    _check("pad %s after the update" % engine, bs, c1, _calls(bs, c1))


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_chunks(gpu_lib, monkeypatch, engine):
    """OSQP_AMD_BATCH_POLISH_CAP_BYTES (read at setup) at one member's KKT matrix: one member per chunk, and every
    output of the three calls bit-equal to the run in one chunk."""
    c = pq.case("pad")
    one = _calls(_handle(c, engine), c)
    monkeypatch.setenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES", str(96 * 96 * 8))
    bs = _handle(c, engine)
    many = _calls(bs, c)
    _check("pad %s one member per chunk" % engine, bs, c, many)
    for o, mny, fields in zip(one[1:], many[1:], (("x", "y", "info_raw", "status_polish"),
                                                  pq.ADJOINT + ("active", "status_adjoint"),
                                                  pq.TANGENT + ("active", "status_tangent"))):
        for f in fields:
            assert np.array_equal(getattr(o, f), getattr(mny, f)), f
