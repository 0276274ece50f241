"""Forward sensitivities on the batch engines (BatchOSQP.tangent / tangent_into, osqp_amd_batch_tangent[_dev],
_BatchQPFunction.jvp).

Reference: tests/_tangent_reference.py (numpy; test_batch_tangent_host.py checks it against central differences and,
with the adjoint's reference, on the duality identity) applied to the CPU oracle's x, y -- never to the device's.
Flow: solve() -> polish() -> tangent(all five tangents) with the seeded draws of _tangent_reference.draws.

Bar, per member whose polish was accepted: status_tangent 1, `active` equal to the reference's set, and dx, dy within
1e-6 relative (_batch_parity.rel, the project's parity bar).  A member is excused from the comparison (status and
finiteness are still checked) by the rule of the adjoint tests, judged on the oracle's data alone
(test_batch_tangent_host.cases); at most half of the accepted members of a shape may be excused and two must be
compared (one where the batch has one member)."""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse

from _batch_parity import rel
from _tangent_reference import tangent_matrices, tangent_reference
from test_batch_tangent_host import TANGENTS, cases, compared, duality_sides, shape_draws
from test_gpu_batch_adjoint import M0_SHAPE, STREAMED_SHAPES, TILED_SHAPES, _family, _incoming, _references, excuse
from test_gpu_batch_device_io import same

pytestmark = pytest.mark.gpu

SMALL = (17, 37, 6, 2)
ADMM_KW = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
OUT = ("dx", "dy", "active", "status_tangent")
_runs = {}


def _kwargs(d, names=TANGENTS, rows=slice(None)):
    """The draws as tangent()'s keyword arguments (dq -> dQ, ...)."""
    return {"d" + k[1:].capitalize() if k in ("dq", "dl", "du") else k: getattr(d, k)[rows] for k in names}


def _setup(shape, engine, polish=True, **kw):
    import osqp_amd
    P, A, Q, L, U, _ = _family(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **kw)
    r = bs.solve()
    if polish:
        r = bs.polish()
    return bs, r


def _run(shape, engine, polish=True, **kw):
    """One solve of the shape: results, tangent(all five) and adjoint(gx, gy, matrices=True) of the same handle (host
    arrays, kept for the tests that only read them)."""
    key = (shape, engine, polish, tuple(sorted(kw.items())))
    if key not in _runs:
        bs, r = _setup(shape, engine, polish, **kw)
        d = shape_draws(shape)
        t = bs.tangent(**_kwargs(d))
        a = bs.adjoint(d.gx, d.gy, matrices=True)
        _runs[key] = SimpleNamespace(r=r, t=t, a=a, engine_id=bs.shape()[0])
        bs.cleanup()
    return _runs[key]


def _check_status(t, cs, members, what):
    """status_tangent 1 for every member looked at, excused ones included; only where the reference's own model of the
    route is not finite may the device answer -1."""
    for b in members:
        if np.isfinite(cs[b].t.route_err):
            assert t.status_tangent[b] == 1, (what, b, int(t.status_tangent[b]))
        else:
            print(what, b, "route model not finite; status_tangent", int(t.status_tangent[b]))
            assert t.status_tangent[b] in (1, -1), (what, b)


def _check_polished(orc, shape, engine, **kw):
    run = _run(shape, engine, **kw)
    r, t = run.r, run.t
    n, m, B, _ = shape
    assert t.dx.shape == (B, n) and t.dy.shape == t.active.shape == (B, m) and t.status_tangent.shape == (B,)
    cs = cases(orc, shape, polish=1, **kw)
    sp = np.array([c.ro.info.status_polish for c in cs])
    assert np.array_equal(r.status_polish, sp), (r.status_polish, sp)
    assert np.all(r.status_val == 1) and np.all(np.isin(t.status_tangent, (1, -1)))
    assert np.all(np.isfinite(t.dx)) and np.all(np.isfinite(t.dy))
    what = "%s %s" % (engine, shape)
    print(what, "status_polish", list(sp), "status_tangent", list(t.status_tangent))
    accepted = [b for b in range(B) if sp[b] == 1]
    assert accepted
    _check_status(t, cs, accepted, what)
    for b in compared(cs, accepted, what):
        ex, ey = rel(t.dx[b], cs[b].t.dx), rel(t.dy[b], cs[b].t.dy)
        eq = np.array_equal(t.active[b], cs[b].t.active)
        print(what, b, "active equal", eq, "dx %.2e dy %.2e (bar 1e-6) route %.1e |M^-1| %.1e"
              % (ex, ey, cs[b].t.route_err, cs[b].t.minv_norm))
        assert eq, (what, b, t.active[b], cs[b].t.active)
        assert ex < 1e-6 and ey < 1e-6, (what, b, ex, ey)
    return run


@pytest.mark.parametrize("shape", TILED_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
def test_parity_tiled(gpu_lib, oracle_mod, shape):
    assert _check_polished(oracle_mod, shape, "auto").engine_id == 0


@pytest.mark.parametrize("shape", STREAMED_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
def test_parity_streamed(gpu_lib, oracle_mod, shape):
    assert _check_polished(oracle_mod, shape, "streamed").engine_id == 1


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_scaling_off(gpu_lib, oracle_mod, engine):
    _check_polished(oracle_mod, SMALL, engine, scaling=0)


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_no_constraints(gpu_lib, oracle_mod, engine):
    """m = 0: dx = -P^-1 (dq + dP x) with the oracle's x, and no row arrays."""
    t = _run(M0_SHAPE, engine).t
    P = _family(M0_SHAPE)[0]
    d, cs = shape_draws(M0_SHAPE), cases(oracle_mod, M0_SHAPE, polish=1)
    Pf = (P + sparse.triu(P, 1).T).toarray()
    assert t.dy.shape == t.active.shape == (3, 0) and t.dx.shape == (3, 20)
    for b in range(3):
        assert t.status_tangent[b] == 1
        want = -np.linalg.solve(Pf, d.dq[b] + tangent_matrices(P, sparse.csc_matrix((0, 20)), d.dPx[b], None)[0] @ cs[b].ro.x)
        print("m0", engine, b, rel(t.dx[b], want), rel(t.dx[b], cs[b].t.dx))
        assert rel(t.dx[b], want) < 1e-6 and rel(t.dx[b], cs[b].t.dx) < 1e-6


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_without_polish(gpu_lib, oracle_mod, engine):
    """tangent() at the ADMM point (eps 1e-9, no polish) against the reference on the oracle's unpolished x, y.
    With the vector tangents alone the answer depends on the point only through the active set: the parity bar 1e-6.
    With all five the right-hand side carries dP x, dA' y and dA x, and the batch engines hold the oracle's x, y to
    the parity bar, |dx| <= 1e-6 max(1, |x|), |dy| <= 1e-6 max(1, |y|), so the answer moves by at most |M^-1| times
    that: the bar is 1e-6 + |M^-1|_inf 1e-6 (|dP|_inf max(1, |x|) + |dA'|_inf max(1, |y|) + |dA|_inf max(1, |x|)) /
    max(1, |[dx; dy]|_inf), from the reference's quantities alone, with the error measured against the same
    max(1, |[dx; dy]|_inf).  Every figure is printed beside its bar."""
    shape = SMALL
    P, A = _family(shape)[:2]
    bs, r = _setup(shape, engine, polish=False, **ADMM_KW)
    d = shape_draws(shape)
    t5 = bs.tangent(**_kwargs(d))
    t3 = bs.tangent(**_kwargs(d, ("dq", "dl", "du")))
    bs.cleanup()
    cs = cases(oracle_mod, shape, **ADMM_KW)
    assert [c.ro.info.status_val for c in cs] == list(r.status_val)
    solved = [b for b in range(shape[2]) if r.status_val[b] == 1]
    what = "admm %s" % engine
    _check_status(t5, cs, solved, what)
    _check_status(t3, cs, solved, what)
    assert np.all(np.isfinite(t5.dx)) and np.all(np.isfinite(t5.dy)) and np.all(np.isfinite(t3.dx)) and np.all(np.isfinite(t3.dy))
    mx = lambda v: max(1.0, float(np.abs(v).max()) if np.size(v) else 0.0)
    ninf = lambda M: float(np.abs(M).sum(axis=1).max()) if M.size else 0.0
    fails = []
    for b in compared(cs, solved, what):
        ro, ref = cs[b].ro, cs[b].t
        ref3 = tangent_reference(P, A, ro.x, ro.y, d.dq[b], d.dl[b], d.du[b])
        assert ref3.route_err <= 1e-7, (b, ref3.route_err)
        e3 = max(rel(t3.dx[b], ref3.dx), rel(t3.dy[b], ref3.dy))
        dP, dA = tangent_matrices(P, A, d.dPx[b], d.dAx[b])
        scale = mx(np.concatenate([ref.dx, ref.dy]))
        bar = 1e-6 + ref.minv_norm * 1e-6 * (ninf(dP) * mx(ro.x) + ninf(dA.T) * mx(ro.y) + ninf(dA) * mx(ro.x)) / scale
        e5 = max(np.abs(t5.dx[b] - ref.dx).max(), np.abs(t5.dy[b] - ref.dy).max()) / scale
        eq = np.array_equal(t5.active[b], ref.active) and np.array_equal(t3.active[b], ref.active)
        print(what, b, "active equal", eq, "vector tangents %.2e (bar 1e-6); all five %.2e (bar %.1e)" % (e3, e5, bar))
        if not (eq and e3 < 1e-6 and e5 < bar):
            fails.append((b, eq, e3, e5, bar))
    assert not fails, fails


@pytest.mark.parametrize("engine,shapes", [("auto", TILED_SHAPES), ("streamed", STREAMED_SHAPES)], ids=["tiled", "streamed"])
def test_duality_on_the_device(gpu_lib, oracle_mod, engine, shapes):
    """tangent() and adjoint(gx, gy, matrices=True) of one handle: gx . dx + gy . dy equals the adjoint's gradients
    times the tangents within what the two parity bars imply: 1e-6 |gx|_1 max(1, |dx_ref|_inf) + 1e-6 |gy|_1
    max(1, |dy_ref|_inf) + the sum over the five pairs of 1e-6 |tangent|_1 max(1, |gradient_ref|_inf)."""
    mx = lambda v: max(1.0, float(np.abs(v).max()) if np.size(v) else 0.0)
    fails = []
    for shape in shapes:
        run, d, cs = _run(shape, engine), shape_draws(shape), cases(oracle_mod, shape, polish=1)
        accepted = [b for b, c in enumerate(cs) if c.ro.info.status_polish == 1]
        for b in compared(cs, accepted, "duality %s %s" % (engine, shape)):
            g = SimpleNamespace(**{k: getattr(run.a, k)[b] for k in TANGENTS})
            lhs, rhs = duality_sides(d, b, run.t.dx[b], run.t.dy[b], g)
            bar = 1e-6 * np.abs(d.gx[b]).sum() * mx(cs[b].t.dx) + 1e-6 * np.abs(d.gy[b]).sum() * mx(cs[b].t.dy)
            bar += sum(1e-6 * np.abs(getattr(d, k)[b]).sum() * mx(getattr(cs[b].a, k)) for k in TANGENTS)
            print(engine, shape, b, "lhs %.12e rhs %.12e |lhs - rhs| %.2e (bar %.1e)" % (lhs, rhs, abs(lhs - rhs), bar))
            if not abs(lhs - rhs) <= bar:
                fails.append((shape, b, lhs, rhs, bar))
    assert not fails, fails


def _more_directions(shape, nnzP, nnzA):
    n, m, B, seed = shape
    rng = np.random.default_rng(888 + seed)
    return {k: rng.standard_normal((B, 2, s)) for k, s in zip(("dQ", "dL", "dU", "dPx", "dAx"), (n, m, m, nnzP, nnzA))}


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_directions(gpu_lib, engine):
    """One call with D = 3 equals, bit for bit, three calls with D = 1 of the same slices; [B, k] equals [B, 1, k]."""
    bs, _ = _setup(SMALL, engine)
    first = _kwargs(shape_draws(SMALL))
    more = _more_directions(SMALL, bs.Pu.nnz, bs.Ah.nnz)
    all3 = {k: np.concatenate([first[k][:, None, :], more[k]], axis=1) for k in first}
    t3 = bs.tangent(**all3)
    B, n, m = bs.B, bs.n, bs.m
    assert t3.dx.shape == (B, 3, n) and t3.dy.shape == (B, 3, m) and t3.active.shape == (B, m)
    assert np.all(t3.status_tangent == 1) and np.any(t3.dx[:, 1] != t3.dx[:, 2])
    for k in range(3):
        t1 = bs.tangent(**{name: v[:, k:k + 1] for name, v in all3.items()})
        assert t1.dx.shape == (B, 1, n) and t1.dy.shape == (B, 1, m)
        assert same(t1.dx[:, 0], t3.dx[:, k]) and same(t1.dy[:, 0], t3.dy[:, k]), k
        assert same(t1.active, t3.active) and same(t1.status_tangent, t3.status_tangent), k
    flat = bs.tangent(**first)
    assert flat.dx.shape == (B, n) and flat.dy.shape == (B, m)
    assert same(flat.dx, t3.dx[:, 0]) and same(flat.dy, t3.dy[:, 0])
    # a call with more directions after one with fewer (the staging is the larger one's)
    again = bs.tangent(**all3)
    assert same(again.dx, t3.dx) and same(again.dy, t3.dy)
    bs.cleanup()


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_zero_and_missing_tangents(gpu_lib, engine):
    bs, _ = _setup(SMALL, engine)
    kw = _kwargs(shape_draws(SMALL))
    t0 = bs.tangent()
    assert np.all(t0.dx == 0) and np.all(t0.dy == 0) and np.all(t0.status_tangent == 1)
    assert t0.dx.shape == (bs.B, bs.n) and t0.dy.shape == (bs.B, bs.m)
    full = bs.tangent(**kw)
    for name in kw:                                      # a missing tangent is a tangent of zeros, to the bit
        t_none = bs.tangent(**{k: v for k, v in kw.items() if k != name})
        t_zero = bs.tangent(**{k: (np.zeros_like(v) if k == name else v) for k, v in kw.items()})
        assert same(t_none.dx, t_zero.dx) and same(t_none.dy, t_zero.dy), name
        assert not same(t_none.dx, full.dx), name        # ... and every tangent counts
    bs.cleanup()


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_handle_untouched(gpu_lib, engine):
    bs, r0 = _setup(SMALL, engine)
    d = shape_draws(SMALL)
    B = SMALL[2]
    a0 = bs.adjoint(d.gx, d.gy, matrices=True)
    w0 = [bs.member_workspace(b) for b in range(B)]
    t0 = bs.tangent(**_kwargs(d))
    r1 = bs.results()
    for k in ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert", "status_polish"):
        assert same(getattr(r0, k), getattr(r1, k)), k
    for b in range(B):
        w1 = bs.member_workspace(b)
        for k in ("D", "E", "ctype", "Kinv", "Pv", "Av"):
            assert same(w0[b][k], w1[k]), (b, k)
        assert w0[b]["rho"] == w1["rho"] and w0[b]["c"] == w1["c"], b
    a1 = bs.adjoint(d.gx, d.gy, matrices=True)
    for k in TANGENTS + ("active", "status_adjoint"):
        assert same(getattr(a0, k), getattr(a1, k)), k
    r2 = bs.polish()                                     # polish's own record is still there
    for k in ("x", "y", "info_raw", "status_polish"):
        assert same(getattr(r0, k), getattr(r2, k)), k
    t1 = bs.tangent(**_kwargs(d))
    for k in OUT:
        assert same(getattr(t0, k), getattr(t1, k)), k
    assert same(t0.active, a0.active)                    # `active` as the adjoint reports it
    bs.cleanup()


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_chunks(gpu_lib, monkeypatch, engine):
    """OSQP_AMD_BATCH_POLISH_CAP_BYTES (read at setup) set to two members' matrices: three chunks, same bits."""
    d = shape_draws(SMALL)
    more = None
    got = []
    for capped in (False, True):
        if capped:
            npol = (SMALL[0] + int(np.count_nonzero(got[0][0].active, axis=1).max()) + 31) & ~31
            monkeypatch.setenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES", str(2 * npol * npol * 8))
        bs, _ = _setup(SMALL, engine)
        more = more or _more_directions(SMALL, bs.Pu.nnz, bs.Ah.nnz)
        got.append((bs.tangent(**_kwargs(d)), bs.tangent(**more)))
        bs.cleanup()
    for one, many in zip(*got):
        for k in OUT:
            assert same(getattr(one, k), getattr(many, k)), k
    assert np.all(got[0][0].status_tangent == 1)


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_unsolved_members_get_zeros(gpu_lib, engine):
    """The status-mix batch of the polish tests: solved, primal infeasible, solved inaccurate, max_iter."""
    import osqp_amd
    from test_gpu_batch_polish import _mixed
    P, A, Q, L, U, kw = _mixed()
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **kw)
    r = bs.solve()
    assert list(r.status_val) == [1, -3, 2, -2]
    rng = np.random.default_rng(7)
    t = bs.tangent(dQ=rng.standard_normal((4, 2) + Q.shape[1:]), dL=rng.standard_normal((4, 2) + L.shape[1:]),
                   dU=rng.standard_normal((4, 2) + L.shape[1:]), dPx=rng.standard_normal((4, 2, bs.Pu.nnz)),
                   dAx=rng.standard_normal((4, 2, bs.Ah.nnz)))
    assert list(t.status_tangent) == [1, 0, 0, 0]
    assert np.any(t.dx[0, 0] != 0.0) and np.any(t.dx[0, 1] != 0.0)
    for b in (1, 2, 3):
        for k in ("dx", "dy", "active"):
            assert np.all(getattr(t, k)[b] == 0), (b, k)
    bs.cleanup()


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_needs_a_solve(gpu_lib, engine):
    import osqp_amd
    P, A, Q, L, U, _ = _family(SMALL)
    kw = _kwargs(shape_draws(SMALL))
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)
    with pytest.raises(RuntimeError, match=r"failed \(7\)"):
        bs.tangent(**kw)                                 # no solve yet
    bs.solve()
    assert np.all(bs.tangent(**kw).status_tangent == 1)
    assert bs.update(Q=Q * 1.01) == 0
    with pytest.raises(RuntimeError, match=r"failed \(7\)"):
        bs.tangent(**kw)                                 # the data moved and no solve has run on it
    with pytest.raises(ValueError):
        bs.tangent(dQ=kw["dQ"][:, :-1])
    with pytest.raises(ValueError):
        bs.tangent(dQ=kw["dQ"], dL=kw["dL"][:, None, :])
    bs.cleanup()


def test_one_engine_per_member_refuses(gpu_lib):
    import osqp_amd
    shape = STREAMED_SHAPES[-1]
    P, A, Q, L, U, _ = _family(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q[:2], L[:2], U[:2])
    with pytest.raises(RuntimeError, match='engine="streamed"'):
        bs.tangent(dQ=np.ones((2, shape[0])))
    bs.cleanup()


def _worker(tmp_path, mode):
    import os
    import subprocess
    import sys
    d = shape_draws(SMALL)
    np.savez(tmp_path / "in.npz", W=_incoming(SMALL)[0], **{k: getattr(d, k) for k in TANGENTS})
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_tangent_layer_worker.py")
    p = subprocess.run([sys.executable, worker, mode] + [str(v) for v in SMALL] + [str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return SimpleNamespace(**np.load(tmp_path / "out.npz"))


def test_layer(gpu_lib, oracle_mod, tmp_path):
    """BatchQPLayer under torch.autograd.forward_ad on CPU tensors: Q, L, U, Ax carry the draws' tangents and the tangent
    of X (and Y) equals the reference's; with a tangent on Q alone the others count as zero; a plain backward pass in the
    same process still returns the adjoint test's dq.  The layer runs in a child process (tests/_tangent_layer_worker.py)."""
    got = _worker(tmp_path, "host")
    shape = SMALL
    P, A, Q, L, U, _ = _family(shape)
    d, cs = shape_draws(shape), cases(oracle_mod, shape, polish=1)
    assert np.array_equal(got.status_polish, [c.ro.info.status_polish for c in cs])
    accepted = [b for b, c in enumerate(cs) if c.ro.info.status_polish == 1]
    assert list(got.route) == ["host"] and np.all(got.status_tangent[accepted] == 1)
    W, dY = _incoming(shape)
    backs = _references(oracle_mod, shape, gx=W, gy=np.zeros_like(dY), polish=1)       # the adjoint test's
    for b in compared(cs, accepted, "layer"):
        ro = cs[b].ro
        ref4 = tangent_reference(P, A, ro.x, ro.y, d.dq[b], d.dl[b], d.du[b], None, d.dAx[b])
        ref1 = tangent_reference(P, A, ro.x, ro.y, d.dq[b])
        back = backs[b]
        assert max(ref4.route_err, ref1.route_err) <= 1e-7 and not excuse(back), b
        errs = (rel(got.tX[b], ref4.dx), rel(got.tY[b], ref4.dy), rel(got.tX_q[b], ref1.dx), rel(got.dq[b], back.dq))
        print("layer", b, "tX %.2e tY %.2e tX (Q alone) %.2e backward dq %.2e (bar 1e-6)" % errs)
        assert rel(got.X[b], ro.x) < 1e-6 and max(errs) < 1e-6, (b, errs)


def test_device_route(gpu_lib, tmp_path):
    """tangent_into with torch CUDA tensors is bit-equal to tangent() from host arrays of the same numbers (D = 1 flat
    and D = 3), and the layer on CUDA tensors under forward_ad takes the device route and returns the host route's bits."""
    got = _worker(tmp_path, "device")
    for k in ("dx", "dy", "active", "status_tangent", "dx3", "dy3"):
        assert same(getattr(got, "host_" + k), getattr(got, "dev_" + k)), k
    assert np.all(got.host_status_tangent == 1) and got.host_dx3.shape == (SMALL[2], 3, SMALL[0])
    assert list(got.routes) == ["device", "host"] and bool(got.on_device)
    assert same(got.layer_dev_tX, got.layer_host_tX) and same(got.layer_dev_tY, got.layer_host_tY)
    assert same(got.layer_dev_status_tangent, got.layer_host_status_tangent) and np.any(got.layer_dev_tX != 0)
