"""CPU side of the single-QP engine's derivatives (OSQP.adjoint / OSQP.tangent, osqp_amd_adjoint / osqp_amd_tangent).

1. The route against the truth.  tests/_single_sens_reference.py models the route -- the reduced solve with
   d = max(delta, 1e-3), run_polish's stop rule, in the scaled space of the oracle's D, E, c -- and this file holds
   every output of it, for every planted member the GPU tests use, to 1e-10 relative to max(1, |truth|_inf) of
   _planted_qp.truth: no member is excused, which is the condition under which the GPU tests may compare every member
   at the parity bar 1e-6.
2. Unscaling.  The scaled-space formulas with an exact solve equal the unscaled-space formulas of _planted_qp.py at
   rounding level: 100 cond(M~) eps relative (the two sides solve differently scaled systems by LU; each is backward
   stable, so their forward errors are a modest multiple of cond eps).
3. The random QP of the GPU tests needs no excuse from the reference alone.
4. Argument checks of the Python methods, without a device."""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse

import _planted_qp as pq
import _single_sens_reference as sr
from _adjoint_reference import adjoint_reference
from _batch_parity import oracle, oracle_ws
from _tangent_reference import tangent_reference

EPS = np.finfo(float).eps


def _scaled(orc, c, b, **kw):
    so = oracle(orc, **sr.member_qp(c, b), **kw)
    ws = oracle_ws(so)
    return np.asarray(ws["D"], float), np.asarray(ws["E"], float).reshape(c.m), float(ws["c"])


def _outputs(c, b, D, E, cs, solve_of):
    """adjoint and tangent of member b by the scaled-space formulas at the truth's point; solve_of(Pfs, Ar) -> solve(g)."""
    tr, mem, inc = pq.truth(c, b), pq.member(c, b), pq.member_inc(c, b)
    Pfs, Ads, rows = sr.scaled_problem(mem.Pu, mem.Ac, mem.act, D, E, cs)
    assert np.array_equal(rows, mem.rows)
    solve = solve_of(Pfs, Ads[rows])
    a = sr.scaled_adjoint(mem.Pu, mem.Ac, mem.act, D, E, cs, tr.x, tr.y, inc.gx, inc.gy, solve)
    t = sr.scaled_tangent(mem.Pu, mem.Ac, mem.act, D, E, cs, tr.x, tr.y, inc.dQ, inc.dL, inc.dU, inc.dPx, inc.dAx, solve)
    return tr, SimpleNamespace(**vars(a), **vars(t)), (Pfs, Ads[rows])


def _relmax(got, tru):
    return {k: float(np.abs(getattr(got, k) - getattr(tru, k)).max() / max(1.0, np.abs(getattr(tru, k)).max()))
            if np.size(getattr(tru, k)) else 0.0 for k in pq.ADJOINT + pq.TANGENT}


@pytest.mark.parametrize("scaling", [10, 0])
def test_route_model_against_truth(oracle_mod, scaling):
    """Every planted member of the GPU tests: the route model within 1e-10 of the truth, none excused."""
    worst, bad = (0.0, None), []
    for name, b in sr.PLANTED_MEMBERS:
        if scaling == 0 and name != "pad":
            continue                                   # (the GPU tests run scaling = 0 on `pad` only)
        c = pq.case(name)
        D, E, cs = _scaled(oracle_mod, c, b, scaling=scaling)
        info = {}

        def solve_of(Pfs, Ar):
            def solve(g):
                s, info["kkt_res"], info["steps"] = sr.route_solve(Pfs, Ar, g)
                return s
            return solve
        tr, got, _ = _outputs(c, b, D, E, cs, solve_of)
        errs = _relmax(got, tr)
        e = max(errs.values())
        print("scaling %d %s[%d] worst %.2e (%s) last solve: %d steps, kkt_res %.1e"
              % (scaling, name, b, e, max(errs, key=errs.get), info["steps"], info["kkt_res"]))
        if e > worst[0]:
            worst = (e, (name, b))
        if not e <= 1e-10:
            bad.append((name, b, errs))
    print("scaling %d: worst route-model error %.2e at %s" % (scaling, worst[0], worst[1]))
    assert not bad, bad


def test_route_model_on_raw_data():
    """The same without any scaling data (D = E = 1, c = 1), every member."""
    worst = 0.0
    for name, b in sr.PLANTED_MEMBERS:
        c = pq.case(name)
        solve_of = lambda Pfs, Ar: (lambda g: sr.route_solve(Pfs, Ar, g)[0])
        tr, got, _ = _outputs(c, b, np.ones(c.n), np.ones(c.m), 1.0, solve_of)
        e = max(_relmax(got, tr).values())
        worst = max(worst, e)
        assert e <= 1e-10, (name, b, e)
    print("raw data: worst route-model error %.2e" % worst)


@pytest.mark.parametrize("name,b", [("pad", 1), ("pad", 3), ("one", 3), ("lp", 0), ("rows", 0)])
def test_unscaling(oracle_mod, name, b):
    c = pq.case(name)
    D, E, cs = _scaled(oracle_mod, c, b)
    assert not np.allclose(D, 1.0) and cs != 1.0

    def solve_of(Pfs, Ar):
        n, k = Pfs.shape[0], Ar.shape[0]
        M = np.zeros((n + k, n + k)); M[:n, :n] = Pfs; M[:n, n:] = Ar.T; M[n:, :n] = Ar
        solve_of.cond = float(np.linalg.cond(M))
        return lambda g: np.linalg.solve(M, g)
    tr, got, _ = _outputs(c, b, D, E, cs, solve_of)
    mem, inc = pq.member(c, b), pq.member_inc(c, b)
    direct = lambda g: np.linalg.solve(tr.route.M, g)
    want = SimpleNamespace(**vars(pq.adjoint_from(mem, tr.x, tr.y, inc.gx, inc.gy, direct)),
                           **vars(pq.tangent_from(mem, tr.x, tr.y, inc, direct)))
    bar = 100.0 * max(solve_of.cond, float(np.linalg.cond(tr.route.M))) * EPS
    errs = _relmax(got, want)
    print(name, b, "cond %.1e bar %.1e" % (solve_of.cond, bar), " ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= bar, errs


def test_random_qp_needs_no_excuse(oracle_mod):
    """The random sparse QP of the GPU tests at the oracle's polished point: margin >= 1e-6, sv_ratio >= 1e-8, route_err <= 1e-7."""
    from osqp_amd.problems import random_sparse_qp
    pb = random_sparse_qp(sr.RANDOM_QP["n"], sr.RANDOM_QP["m"], seed=sr.RANDOM_QP["seed"])
    ro = oracle(oracle_mod, polish=1, **pb).solve()
    assert ro.info.status_val == 1 and ro.info.status_polish == 1
    rng = np.random.default_rng(99)
    a = adjoint_reference(pb["P"], pb["A"], pb["l"], pb["u"], ro.x, ro.y, rng.standard_normal(200), rng.standard_normal(400))
    t = tangent_reference(pb["P"], pb["A"], ro.x, ro.y, rng.standard_normal(200), rng.standard_normal(400), rng.standard_normal(400))
    print("margin %.2e sv_ratio %.2e route_err %.2e / %.2e, active rows %d" % (a.margin, a.sv_ratio, a.route_err, t.route_err, a.rows.size))
    assert a.margin >= 1e-6 and a.sv_ratio >= 1e-8 and a.route_err <= 1e-7 and t.route_err <= 1e-7


# ------------------------------------------------------------------------------------------------ Python arguments
def test_argument_checks():
    from osqp_amd.interface import check_adjoint, check_tangent
    n, m, nnzP, nnzA = 3, 2, 4, 5
    dx, dy = check_adjoint(n, m, [1, 2, 3], None)
    assert dx.dtype == np.float64 and dx.flags.c_contiguous and dy is None
    assert check_adjoint(n, m, np.zeros(3, np.float32), np.zeros(2))[0].dtype == np.float64
    for bad in ((np.zeros(4), None), (np.zeros((1, 3)), None), (np.zeros(3), np.zeros(3)), (np.zeros(3), np.zeros((1, 2)))):
        with pytest.raises(ValueError):
            check_adjoint(n, m, *bad)
    # nothing given: one direction of zeros
    assert check_tangent(n, m, nnzP, nnzA) == (None, None, None, None, None, 1, True)
    out = check_tangent(n, m, nnzP, nnzA, dq=np.zeros(3), dAx=np.zeros(5, np.float32))
    assert out[5:] == (1, True) and out[4].dtype == np.float64 and out[1] is None
    out = check_tangent(n, m, nnzP, nnzA, dq=np.zeros((4, 3)), dl=np.zeros((4, 2)), dPx=np.zeros((4, 4)))
    assert out[5:] == (4, False)
    assert check_tangent(n, m, nnzP, nnzA, du=np.zeros((1, 2)))[5:] == (1, False)
    strided = np.zeros((4, 6))[:, ::2]
    assert check_tangent(n, m, nnzP, nnzA, dq=strided)[0].flags.c_contiguous
    for bad in (dict(dq=np.zeros(4)), dict(dq=np.zeros((2, 4))), dict(dl=np.zeros((2, 1, 2))), dict(dPx=np.zeros((0, 4))),
                dict(dq=np.zeros(3), dl=np.zeros((1, 2))),                   # flat and stacked mixed
                dict(dq=np.zeros((2, 3)), dAx=np.zeros((3, 5))),             # two values of D
                dict(dAx=np.zeros(4)), dict(du=np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            check_tangent(n, m, nnzP, nnzA, **bad)
    # P stored empty: a dPx of no entries is a valid tangent
    assert check_tangent(n, m, 0, nnzA, dPx=np.zeros((2, 0)), dq=np.zeros((2, 3)))[5:] == (2, False)


def test_methods_check_before_the_c_side():
    """A handle that was never set up has no workspace: the shape checks must fire before anything is called."""
    from osqp_amd.interface import SolverHandle

    class _NoLib:
        def __getattr__(self, name):
            raise AssertionError("the C side was reached: %s" % name)
    h = SolverHandle.__new__(SolverHandle)
    h._lib, h._prefix, h._work, h.n, h.m, h.nnzP, h.nnzA = _NoLib(), "", None, 3, 2, 4, 5
    with pytest.raises(ValueError):
        h.adjoint(np.zeros(2))
    with pytest.raises(ValueError):
        h.tangent(dq=np.zeros(3), dl=np.zeros((2, 2)))


def test_layer_argument_checks():
    import torch
    from osqp_amd.layer import QPLayer
    layer = QPLayer(sparse.eye(3, format="csc"), sparse.csc_matrix(np.ones((2, 3))))
    assert layer.settings["polish"] == 1 and QPLayer(sparse.eye(3), sparse.eye(3), polish=0).settings["polish"] == 0
    q, l, u = torch.zeros(3, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    with pytest.raises(TypeError):
        layer(q.float(), l, u)
    with pytest.raises(ValueError):
        layer(q, l[:1], u)
    with pytest.raises(ValueError):
        layer(q, l, u, Ax=torch.zeros(5, dtype=torch.float64))
    assert layer.h is None
