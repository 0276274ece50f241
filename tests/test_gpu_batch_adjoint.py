"""Adjoint derivatives on the batch engines (BatchOSQP.adjoint, osqp_amd_batch_adjoint, osqp_amd.BatchQPLayer).

Reference: tests/_adjoint_reference.py (numpy; test_batch_adjoint_host.py checks it against central differences)
applied to the CPU oracle's polished x, y -- never to the device's.  Flow: solve() -> polish() ->
adjoint(dX, dY, matrices=True) with seeded random dX, dY.

Bar, per member whose polish was accepted: status_adjoint 1, `active` equal to the reference's set, and dq, dl, du,
dPx, dAx within 1e-6 relative (_batch_parity.rel, the project's parity bar).  A member is excused from the comparison
(status_adjoint and finiteness are still checked) only when the reference, on the oracle's data alone, reports a
strict-complementarity margin below 1e-6 (not differentiable there), sigma_min / sigma_max of the active rows below
1e-8 (multipliers and their adjoints not unique), or an error of its model of the device route -- explicit inverse
of the delta-regularised matrix, polish_refine_iter refinement steps -- above 1e-7 against the direct solve.  At most
half of the accepted members of a shape may be excused and two must be compared (one where the batch has one
member); each test prints who was excused and why."""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse

from _adjoint_reference import adjoint_reference
from _batch_parity import oracle, rel, shape_family

pytestmark = pytest.mark.gpu

# (n, m, B, seed of shape_family).  Order 1 plus rows; off the 16 tile; NP 128 with fewer rows than variables; the
# tiled limit; beyond it (streamed only).  The last two carry other seeds than the polish tests' (6 and 7): there the
# reference excuses two of three and one of two accepted members (dependent or nearly dependent active rows); at
# these seeds it excuses one of three and none of two.
TILED_SHAPES = [(1, 5, 4, 1), (17, 37, 6, 2), (65, 40, 6, 5), (128, 259, 4, 31)]
STREAMED_SHAPES = TILED_SHAPES + [(150, 303, 4, 14)]
M0_SHAPE = (20, 0, 3, 8)
GRADS = ("dq", "dl", "du", "dPx", "dAx")
_cache = {}


def _family(shape):
    if shape not in _cache:
        _cache[shape] = shape_family(*shape)
    return _cache[shape]


def _incoming(shape):
    """Seeded dl/dx [B, n] and dl/dy [B, m]."""
    n, m, B, seed = shape
    rng = np.random.default_rng(4242 + seed)
    return rng.standard_normal((B, n)), rng.standard_normal((B, m))


def _oracle_runs(orc, shape, **kw):
    """Per member: the oracle's result (computed once per shape and settings, never modified)."""
    key = ("oracle", shape, tuple(sorted(kw.items())))
    if key not in _cache:
        P, A, Q, L, U, _ = _family(shape)
        _cache[key] = [oracle(orc, P, Q[b], A, L[b], U[b], **kw).solve() for b in range(Q.shape[0])]
    return _cache[key]


def _references(orc, shape, gx=None, gy=None, **kw):
    """Per member: the numpy reference on the oracle's x, y, with the handle's delta and polish_refine_iter."""
    key = ("ref", shape, gx is None, gy is None, tuple(sorted(kw.items())))
    if key not in _cache:
        P, A, Q, L, U, _ = _family(shape)
        dX, dY = _incoming(shape)
        gx = dX if gx is None else gx
        gy = dY if gy is None else gy
        runs = _oracle_runs(orc, shape, **kw)
        _cache[key] = [adjoint_reference(P, A, L[b], U[b], ro.x, ro.y, gx[b], gy[b]) for b, ro in enumerate(runs)]
    return _cache[key]


def excuse(ref):
    """Why a member is not compared, from the reference's diagnostics alone ('' = it is compared)."""
    why = []
    if ref.margin < 1e-6:
        why.append("complementarity margin %.1e" % ref.margin)
    if ref.sv_ratio < 1e-8:
        why.append("active rows dependent (%.1e)" % ref.sv_ratio)
    if ref.route_err > 1e-7:
        why.append("route model error %.1e" % ref.route_err)
    return ", ".join(why)


def _compare(a, refs, members, what, bar=1e-6, check_active=True, grads=GRADS):
    """members: those to look at (accepted by polish, or solved).  bar: one number, or a function of the member that
    returns one bar per gradient.  Returns the worst rel() over the compared members.  status_adjoint must be 1 for
    every member looked at, excused ones included; only where the reference's own model of the route breaks down
    (a non-finite route error: the regularised matrix is singular to numpy) may the device answer -1."""
    excused, compared, worst = [], [], 0.0
    for b in members:
        ref, tag = refs[b], (what, b)
        if np.isfinite(ref.route_err):
            assert a.status_adjoint[b] == 1, tag + (int(a.status_adjoint[b]),)
        else:
            print(what, b, "route model not finite; status_adjoint", int(a.status_adjoint[b]))
            assert a.status_adjoint[b] in (1, -1), tag
        for g in grads:
            assert np.all(np.isfinite(getattr(a, g)[b])), tag + (g,)
        why = excuse(ref)
        if why:
            excused.append((b, why, int(a.status_adjoint[b])))
            continue
        errs = [rel(getattr(a, g)[b], getattr(ref, g)) for g in grads]
        bars = bar(b) if callable(bar) else [bar] * len(grads)
        same = np.array_equal(a.active[b], ref.active) if check_active else None
        print(what, b, "status_adjoint", int(a.status_adjoint[b]), "active equal", same,
              " ".join("%s %.2e (bar %.1e)" % (g, e, t) for g, e, t in zip(grads, errs, bars)),
              "margin %.1e sv %.1e route %.1e" % (ref.margin, ref.sv_ratio, ref.route_err))
        compared.append((b, errs, bars, same))
    print(what, "excused (member, why, status_adjoint):", excused)
    for b, errs, bars, same in compared:
        tag = (what, b)
        if check_active:
            assert same, tag + (a.active[b], refs[b].active)
        assert all(e < t for e, t in zip(errs, bars)), tag + tuple(errs) + tuple(bars)
        worst = max(worst, max(errs))
    assert len(excused) <= len(members) // 2, (what, excused)
    assert len(compared) >= min(2, len(members)) and compared, (what, excused)
    return worst


def _run(shape, engine, polish=True, **kw):
    import osqp_amd
    P, A, Q, L, U, _ = _family(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **kw)
    r = bs.solve()
    if polish:
        r = bs.polish()
    dX, dY = _incoming(shape)
    return bs, r, bs.adjoint(dX, dY, matrices=True)


def _check_polished(orc, shape, engine, **kw):
    bs, r, a = _run(shape, engine, **kw)
    n, m, B, _ = shape
    assert a.dq.shape == (B, n) and a.dl.shape == a.du.shape == a.active.shape == (B, m)
    assert a.dPx.shape == (B, bs.Pu.nnz) and a.dAx.shape == (B, bs.Ah.nnz) and a.status_adjoint.shape == (B,)
    runs = _oracle_runs(orc, shape, polish=1, **kw)
    sp = np.array([ro.info.status_polish for ro in runs])
    assert np.array_equal(r.status_polish, sp), (r.status_polish, sp)
    assert np.all(r.status_val == 1) and np.all(np.isin(a.status_adjoint, (1, -1)))
    print(engine, shape, "status_polish", list(sp), "status_adjoint", list(a.status_adjoint))
    accepted = [b for b in range(B) if sp[b] == 1]
    assert accepted
    _compare(a, _references(orc, shape, polish=1, **kw), accepted, "%s %s" % (engine, shape))
    return bs, r, a


@pytest.mark.parametrize("shape", TILED_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
def test_parity_tiled(gpu_lib, oracle_mod, shape):
    bs, _, _ = _check_polished(oracle_mod, shape, "auto")
    assert bs.shape()[0] == 0


@pytest.mark.parametrize("shape", STREAMED_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
def test_parity_streamed(gpu_lib, oracle_mod, shape):
    bs, _, _ = _check_polished(oracle_mod, shape, "streamed")
    assert bs.shape()[0] == 1


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_no_constraints(gpu_lib, oracle_mod, engine):
    """m = 0: dl/dq = -P^-1 dX, and no row arrays."""
    bs, r, a = _run(M0_SHAPE, engine)
    P, A, Q, L, U, _ = _family(M0_SHAPE)
    dX, _ = _incoming(M0_SHAPE)
    Pf = (P + sparse.triu(P, 1).T).toarray()
    assert a.dl.shape == a.du.shape == a.active.shape == (3, 0) and a.dAx.shape == (3, 0)
    refs = _references(oracle_mod, M0_SHAPE, polish=1)
    for b in range(3):
        assert a.status_adjoint[b] == 1
        want = -np.linalg.solve(Pf, dX[b])
        print("m0", engine, b, rel(a.dq[b], want), rel(a.dPx[b], refs[b].dPx))
        assert rel(a.dq[b], want) < 1e-6 and rel(a.dq[b], refs[b].dq) < 1e-6 and rel(a.dPx[b], refs[b].dPx) < 1e-6


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_scaling_off(gpu_lib, oracle_mod, engine):
    _check_polished(oracle_mod, (17, 37, 6, 2), engine, scaling=0)


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
    a = bs.adjoint(rng.standard_normal(Q.shape), rng.standard_normal(L.shape), matrices=True)
    assert a.status_adjoint[0] in (1, -1) and list(a.status_adjoint[1:]) == [0, 0, 0]
    assert np.any(a.dq[0] != 0.0)
    for b in (1, 2, 3):
        for g in GRADS + ("active",):
            assert np.all(getattr(a, g)[b] == 0), (b, g)


# The issue's bar for test_without_polish: ten times the worst member measured on an MI355X.  None = not measured
# yet; the derived bars of _admm_bars then hold (see the test's docstring).
ADMM_BAR = None


def _admm_bars(ref, ro):
    """Bars for the gradients at an ADMM point, from the reference and the oracle's point alone.  The batch engines
    hold the oracle's x, y to the parity bar, |dx| <= 1e-6 max(1, |x|), |dy| <= 1e-6 max(1, |y|), and a compared
    member's solve to the excuse rule, |dr| <= 1e-7 max(1, |r|).  dq, dl, du depend on the active set and the
    matrix only: the parity bar as after polish.  dAx = -(y rx + rnu x) and dPx = -(rx x' + x rx') are bilinear:
        |d dAx| <= |rx| |dy| + |rnu| |dx| + (|x| + |y|) |dr|,    |d dPx| <= 2 |rx| |dx| + 2 |x| |dr|,
    relative to max(1, |gradient|) as rel() measures, on top of the parity bar."""
    x, y = np.asarray(ro.x), np.asarray(ro.y)
    mx = lambda v: float(np.abs(v).max()) if np.size(v) else 0.0
    nx, ny, rx, rnu = mx(x), mx(y), mx(ref.rx), mx(ref.rnu)
    dr = 1e-7 * max(1.0, rx, rnu)
    eA = 1e-6 * (max(1.0, ny) * rx + max(1.0, nx) * rnu) + (nx + ny) * dr
    eP = 2e-6 * max(1.0, nx) * rx + 2 * nx * dr
    return [1e-6, 1e-6, 1e-6, 1e-6 + eP / max(1.0, mx(ref.dPx)), 1e-6 + eA / max(1.0, mx(ref.dAx))]


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_without_polish(gpu_lib, oracle_mod, engine):
    """adjoint() at the ADMM point (eps_abs = eps_rel = 1e-9, no polish) against the reference on the oracle's
    unpolished x, y: status, active set and the five gradients.  The bar the issue sets is ten times the worst
    member measured on the GPU (ADMM_BAR).  Measured: not yet.  Until it is, each compared member is held to the
    bars of _admm_bars, derived from the parity bar of x, y and the reference's own quantities (1e-6 for dq, dl, du;
    1e-6 plus the bilinear terms for dPx, dAx), never from what the device returns; the test prints every figure
    beside its bar."""
    shape = (17, 37, 6, 2)
    kw = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
    bs, r, a = _run(shape, engine, polish=False, **kw)
    runs = _oracle_runs(oracle_mod, shape, **kw)
    assert [ro.info.status_val for ro in runs] == list(r.status_val)
    solved = [b for b in range(shape[2]) if r.status_val[b] == 1]
    refs = _references(oracle_mod, shape, **kw)
    bar = ADMM_BAR if ADMM_BAR is not None else (lambda b: _admm_bars(refs[b], runs[b]))
    worst = _compare(a, refs, solved, "admm %s" % engine, bar=bar)
    print("admm", engine, "worst rel %.3e" % worst)


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_handle_untouched(gpu_lib, engine):
    shape = (17, 37, 6, 2)
    bs, r0, a0 = _run(shape, engine)
    B = shape[2]
    w0 = [bs.member_workspace(b) for b in range(B)]
    dX, dY = _incoming(shape)
    a1 = bs.adjoint(dX, dY, matrices=True)
    r1 = bs.results()
    for k in ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert", "status_polish"):
        assert np.array_equal(getattr(r0, k), getattr(r1, k), equal_nan=True), k
    for k in GRADS + ("active", "status_adjoint"):
        assert np.array_equal(getattr(a0, k), getattr(a1, k)), k
    for b in range(B):
        w1 = bs.member_workspace(b)
        for k in ("D", "E", "ctype", "Kinv", "Pv", "Av"):
            assert np.array_equal(w0[b][k], w1[k]), (b, k)
        assert w0[b]["rho"] == w1["rho"] and w0[b]["c"] == w1["c"], b
    r2 = bs.polish()                                     # polish's own record is still there
    for k in ("x", "y", "info_raw", "status_polish"):
        assert np.array_equal(getattr(r0, k), getattr(r2, k), equal_nan=True), k
    # dY = None is dY = 0, and without matrices=True the matrix gradients are not computed
    a2 = bs.adjoint(dX)
    a3 = bs.adjoint(dX, np.zeros_like(dY), matrices=True)
    assert a2.dPx is None and a2.dAx is None
    for k in ("dq", "dl", "du", "active", "status_adjoint"):
        assert np.array_equal(getattr(a2, k), getattr(a3, k)), k


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_chunks(gpu_lib, monkeypatch, engine):
    """OSQP_AMD_BATCH_POLISH_CAP_BYTES (read at setup) set to two members' matrices: three chunks, same bits."""
    shape = (17, 37, 6, 2)
    _, _, one = _run(shape, engine)
    npol = (shape[0] + int(np.count_nonzero(one.active, axis=1).max()) + 31) & ~31
    monkeypatch.setenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES", str(2 * npol * npol * 8))
    _, _, many = _run(shape, engine)
    for k in GRADS + ("active", "status_adjoint"):
        assert np.array_equal(getattr(one, k), getattr(many, k)), k
    assert np.all(one.status_adjoint == 1)


@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_needs_a_solve(gpu_lib, engine):
    import osqp_amd
    shape = (17, 37, 6, 2)
    P, A, Q, L, U, _ = _family(shape)
    dX, dY = _incoming(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)
    with pytest.raises(RuntimeError, match=r"failed \(7\)"):
        bs.adjoint(dX, dY)                               # no solve yet
    bs.solve()
    assert np.all(bs.adjoint(dX, dY).status_adjoint == 1)
    assert bs.update(Q=Q * 1.01) == 0
    with pytest.raises(RuntimeError, match=r"failed \(7\)"):
        bs.adjoint(dX, dY)                               # the data moved and no solve has run on it
    with pytest.raises(ValueError):
        bs.adjoint(dX[:, :-1], dY)


def test_one_engine_per_member_refuses(gpu_lib):
    import osqp_amd
    shape = STREAMED_SHAPES[-1]
    P, A, Q, L, U, _ = _family(shape)
    dX, dY = _incoming(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q[:2], L[:2], U[:2])
    with pytest.raises(RuntimeError, match='engine="streamed"'):
        bs.adjoint(dX[:2], dY[:2])


def test_layer(gpu_lib, oracle_mod, tmp_path):
    """BatchQPLayer: loss = (X * W).sum() -> Q.grad, L.grad, U.grad, Ax.grad equal the reference's values with
    dX = W, dY = 0; inputs that do not require a gradient get none.  CPU tensors only.  The layer runs in a child process
    (tests/_adjoint_layer_worker.py says why); the comparison is made here."""
    import os
    import subprocess
    import sys
    shape = (17, 37, 6, 2)
    B = shape[2]
    W, dY = _incoming(shape)
    np.save(tmp_path / "w.npy", W)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_adjoint_layer_worker.py")
    p = subprocess.run([sys.executable, worker] + [str(v) for v in shape] + [str(tmp_path / "w.npy"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = SimpleNamespace(**np.load(tmp_path / "out.npz"))
    runs = _oracle_runs(oracle_mod, shape, polish=1)
    assert np.array_equal(got.status_polish, [ro.info.status_polish for ro in runs])
    refs = _references(oracle_mod, shape, gx=W, gy=np.zeros_like(dY), polish=1)
    accepted = [b for b in range(B) if runs[b].info.status_polish == 1]
    _compare(got, refs, accepted, "layer", check_active=False, grads=("dq", "dl", "du", "dAx"))
    assert got.Y2.shape == (B, shape[1]) and bool(got.others_none) and list(got.raised) == [True, True]
    for b in accepted:
        assert rel(got.X[b], runs[b].x) < 1e-6 and rel(got.X2[b], runs[b].x) < 1e-6, b
        if not excuse(refs[b]):
            assert rel(got.dq2[b], refs[b].dq) < 1e-6, b
