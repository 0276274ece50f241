"""Host-side contract of the tangent call on the batch engines (no GPU needed), and the yardsticks of the numpy
reference the GPU tests compare against (tests/_tangent_reference.py): its dx, dy against central differences of the
CPU oracle, and the duality identity between it and the adjoint's reference.

The helpers the GPU tests share live here too: the cases (oracle run, tangent reference, adjoint reference, excuse)
of a shape, computed once and never modified."""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse

from _adjoint_reference import adjoint_reference
from _tangent_reference import draws, tangent_reference
from osqp_amd.batch import check_tangent
from test_batch_adjoint_host import _qp
from test_gpu_batch_adjoint import M0_SHAPE, STREAMED_SHAPES, _family, _oracle_runs, excuse

ALL_SHAPES = STREAMED_SHAPES + [M0_SHAPE]
TANGENTS = ("dq", "dl", "du", "dPx", "dAx")
_cache = {}


def shape_draws(shape):
    if ("draws", shape) not in _cache:
        P, A = _family(shape)[:2]
        _cache["draws", shape] = draws(shape, sparse.triu(P).nnz, sparse.csc_matrix(A).nnz)
    return _cache["draws", shape]


def cases(orc, shape, **kw):
    """Per member of shape_family(*shape): a namespace with the oracle's run `ro` (settings kw), the tangent reference
    `t` and the adjoint reference `a` (for gx, gy of the draws) on the oracle's x, y, and `why`: the excuse rule of the
    adjoint tests on the reference's data alone ('' = compared) -- complementarity margin below 1e-6, sigma_min /
    sigma_max of the active rows below 1e-8, or the tangent's route model more than 1e-7 off the direct solve."""
    key = ("cases", shape, tuple(sorted(kw.items())))
    if key not in _cache:
        P, A, Q, L, U, _ = _family(shape)
        d = shape_draws(shape)
        out = []
        for b, ro in enumerate(_oracle_runs(orc, shape, **kw)):
            t = tangent_reference(P, A, ro.x, ro.y, d.dq[b], d.dl[b], d.du[b], d.dPx[b], d.dAx[b])
            a = adjoint_reference(P, A, L[b], U[b], ro.x, ro.y, d.gx[b], d.gy[b])
            why = excuse(SimpleNamespace(margin=a.margin, sv_ratio=a.sv_ratio, route_err=t.route_err))
            out.append(SimpleNamespace(ro=ro, t=t, a=a, why=why))
        _cache[key] = out
    return _cache[key]


def compared(cs, members, what):
    """The members of `members` that are compared; the cap of the adjoint tests: at most half excused, at least two
    compared (one where there is one member)."""
    excused = [(b, cs[b].why) for b in members if cs[b].why]
    keep = [b for b in members if not cs[b].why]
    print(what, "members", list(members), "excused (member, why):", excused)
    assert len(excused) <= len(members) // 2, (what, excused)
    assert len(keep) >= min(2, len(members)) and keep, (what, excused)
    return keep


def duality_sides(d, b, dx, dy, g):
    """(gx . dx + gy . dy, the five products of the gradients g with the tangents of member b)."""
    lhs = float(d.gx[b] @ dx + d.gy[b] @ dy)
    rhs = float(sum(np.dot(getattr(g, k), getattr(d, k)[b]) for k in TANGENTS))
    return lhs, rhs


def test_library_exports_tangent():
    import osqp_amd
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    for name in ("osqp_amd_batch_tangent", "osqp_amd_batch_tangent_dev"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 11, name


def test_python_entry_points_exist():
    import torch
    import osqp_amd
    from osqp_amd import batch, layer
    assert callable(getattr(osqp_amd.BatchOSQP, "tangent", None))
    assert callable(getattr(osqp_amd.BatchOSQP, "tangent_into", None))
    assert callable(getattr(batch, "check_tangent", None))
    assert layer._BatchQPFunction.jvp is not torch.autograd.Function.jvp
    assert osqp_amd.BatchQPLayer(sparse.eye(2), sparse.eye(2)).last_status_tangent is None


def test_null_handle_is_refused():
    import ctypes as C
    import osqp_amd
    from osqp_amd import abi
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    v = np.ones(4); k = np.zeros(4, np.int64)
    nf = C.cast(None, abi.c_float_p)
    assert lib.osqp_amd_batch_tangent(None, 1, abi.fptr(v), nf, nf, nf, nf, abi.fptr(v), abi.fptr(v),
                                      abi.iptr(k), abi.iptr(k)) == 7          # OSQP_WORKSPACE_NOT_INIT_ERROR
    assert lib.osqp_amd_batch_tangent_dev(None, 1, *([None] * 9)) == 7


B, N, M, NP_, NA = 3, 5, 7, 6, 9
one = lambda *s: np.ones(s)
MALFORMED = [dict(dQ=one(B, N + 1)), dict(dQ=one(B + 1, N)), dict(dQ=one(N)), dict(dQ=one(B, 2, N, 1)),
             dict(dL=one(B, M + 1)), dict(dU=one(B - 1, M)), dict(dPx=one(B, NP_ + 1)), dict(dAx=one(B, 2, NA - 1)),
             dict(dPx=one(NP_)), dict(dQ=one(B, 0, N)),
             dict(dQ=one(B, N), dL=one(B, 1, M)),                 # [B, k] mixed with [B, D, k]
             dict(dQ=one(B, 2, N), dAx=one(B, NA)),
             dict(dQ=one(B, 2, N), dL=one(B, 3, M)),              # disagreeing D
             dict(dL=one(B, 2, M), dU=one(B, 2, M), dPx=one(B, 4, NP_)),
             dict(dQ=one(B, 2, N), dx=one(B, N)),                 # an output of tangent_into in the other form
             dict(dQ=one(B, 2, N), dx=one(B, 2, N), dy=one(B, 3, M))]


@pytest.mark.parametrize("kwargs", MALFORMED, ids=[str(k) for k in range(len(MALFORMED))])
def test_shape_errors_raise(kwargs):
    with pytest.raises(ValueError):
        check_tangent(B, N, M, NP_, NA, **kwargs)


def test_well_formed_shapes_pass():
    assert check_tangent(B, N, M, NP_, NA) == (None,) * 5 + (1, True)
    dQ, dL, dU, dPx, dAx, D, flat = check_tangent(B, N, M, NP_, NA, dQ=[[1.0] * N] * B, dAx=np.ones((B, NA), np.float32))
    assert dQ.shape == (B, N) and dQ.dtype == np.float64 and dQ.flags.c_contiguous and dAx.dtype == np.float64
    assert dL is None and dU is None and dPx is None and (D, flat) == (1, True)
    out = check_tangent(B, N, M, NP_, NA, dQ=one(B, 4, N), dL=one(B, 4, M), dU=one(B, 4, M), dPx=one(B, 4, NP_),
                        dAx=one(B, 4, NA)[:, :, ::-1], dx=one(B, 4, N), dy=one(B, 4, M))
    assert out[5:] == (4, False) and all(a.flags.c_contiguous for a in out[:5])
    assert check_tangent(B, N, M, NP_, NA, dL=one(B, 1, M))[5:] == (1, False)


def test_reference_against_central_differences(oracle_mod):
    """The reference's dx, dy for all five tangents at once against central differences of the oracle along that
    direction (eps 1e-10, polish on), error relative to max(1, |.|_inf).  Measured on the CPU, dx / dy:
    step 1e-4: 4.0e-9 / 4.3e-9 (truncation); step 1e-5: 2.9e-11 / 3.7e-11; step 1e-6: 2.9e-10 / 2.4e-10 (round-off of
    the polished solution over the step).  The bar is 10 x the best of them: 3.7e-10 at step 1e-5."""
    P, A, q, l, u = _qp()
    rng = np.random.default_rng(2000)
    dq, dl, du = rng.standard_normal(5), rng.standard_normal(7), rng.standard_normal(7)
    dPx, dAx = rng.standard_normal(P.nnz), rng.standard_normal(A.nnz)

    def solve(s):
        P2, A2 = P.copy(), A.copy()
        P2.data = P.data + s * dPx; A2.data = A.data + s * dAx
        r = oracle_mod.OracleOSQP().setup(P=P2, q=q + s * dq, A=A2, l=l + s * dl, u=u + s * du, eps_abs=1e-10, eps_rel=1e-10,
                                          polish=1, max_iter=20000).solve()
        assert r.info.status_val == 1 and r.info.status_polish == 1
        return np.array(r.x), np.array(r.y)

    x, y = solve(0.0)
    ref = tangent_reference(P, A, x, y, dq, dl, du, dPx, dAx)
    assert sorted(ref.active) == [-1, 0, 0, 0, 1, 1, 1] and ref.route_err < 1e-12 and np.isfinite(ref.minv_norm)
    worst = {}
    for h in (1e-4, 1e-5, 1e-6):
        (xp, yp), (xm, ym) = solve(h), solve(-h)
        ex = np.abs((xp - xm) / (2 * h) - ref.dx).max() / max(1.0, np.abs(ref.dx).max())
        ey = np.abs((yp - ym) / (2 * h) - ref.dy).max() / max(1.0, np.abs(ref.dy).max())
        worst[h] = max(ex, ey)
        print("step %g: dx %.2e dy %.2e" % (h, ex, ey))
    assert worst[1e-5] < 3.7e-10, worst


def test_duality_of_the_references(oracle_mod):
    """gx . dx + gy . dy of the tangent reference equals the adjoint reference's gradients (for gx, gy) times the
    tangents, on every accepted, non-excused member of the GPU tests' shapes; error relative to max(1, |lhs|, |rhs|).
    Worst measured on the CPU: 9.8e-15; the bar is 1e-12."""
    worst = 0.0
    for shape in ALL_SHAPES:
        cs, d = cases(oracle_mod, shape, polish=1), shape_draws(shape)
        accepted = [b for b, c in enumerate(cs) if c.ro.info.status_polish == 1]
        for b in compared(cs, accepted, "duality %s" % (shape,)):
            lhs, rhs = duality_sides(d, b, cs[b].t.dx, cs[b].t.dy, cs[b].a)
            err = abs(lhs - rhs) / max(1.0, abs(lhs), abs(rhs))
            print(shape, b, "lhs %.15e rhs %.15e err %.2e route %.1e (adjoint's %.1e) |M^-1| %.1e"
                  % (lhs, rhs, err, cs[b].t.route_err, cs[b].a.route_err, cs[b].t.minv_norm))
            assert err < 1e-12, (shape, b, lhs, rhs)
            worst = max(worst, err)
    print("worst %.2e" % worst)


def test_excuses_at_the_admm_point(oracle_mod):
    """The cap of the excuse rule also holds at the ADMM point the GPU test without polish uses."""
    kw = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
    cs = cases(oracle_mod, (17, 37, 6, 2), **kw)
    solved = [b for b, c in enumerate(cs) if c.ro.info.status_val == 1]
    assert len(compared(cs, solved, "admm")) >= 2
