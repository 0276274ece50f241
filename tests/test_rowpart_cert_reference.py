"""The model of tests/_rowpart_cert_reference.py against the oracle, on the CPU.  The oracle's is_primal_infeasible / is_dual_infeasible are
reached through its solve: warm-started at (x0, y0), ONE iteration with a check and residual tolerances that nothing passes, so the status
is the verdict of the two tests (at eps, then at 10 eps: the approximate branch) and the result carries the certificates.  A twin
workspace makes the same iteration through orc_admm_iterate and hands over the iterates before and after; the model works on those.
Every case must stay inside the model's conditions: no comparison within the rounding bounds of its two sides."""
import numpy as np
import pytest

import _rowpart_reference as R
import _rowpart_cert_reference as CR
from osqp_amd import rowpart


def _unscaled(sc):
    return {k: sc[k] for k in "PqAlu"}


def _case(oracle_mod, sc, x0, y0, scaling, stt, expect_at=None):
    pb = _unscaled(sc)
    st = dict(CR.KERNEL_SETTINGS, scaled_termination=stt)
    twin = oracle_mod.OracleOSQP().setup(**pb, scaling=scaling, **st)
    twin.warm_start(x=x0, y=y0)
    xa, _, ya = twin.iterates()
    twin.iterate(1)
    xb, _, yb = twin.iterates()
    M = R.Model(rowpart.scaled_problem_from_handle(twin), **st)
    assert M.scaled_data == bool(scaling)
    dx, dy = CR.deltas(M, xa, ya, xb, yb)
    val, bnd, at = CR.cert_scalars(M, dx, dy)
    if expect_at is not None:
        assert CR.planted_at(at, M.n, M.m, expect_at), at
    seen = set()
    for eps in CR.EPS_SWEEP:
        p0, d0, c0 = CR.tests(M, val, eps, eps, bnd)
        p1, d1, c1 = CR.tests(M, val, 10 * eps, 10 * eps, bnd)
        assert c0 and c1, (eps, dict(zip(CR.SC7_NAMES, val)))
        want = ("primal infeasible" if p0 else "dual infeasible" if d0 else "primal infeasible inaccurate" if p1
                else "dual infeasible inaccurate" if d1 else "maximum iterations reached")
        so = oracle_mod.OracleOSQP().setup(**pb, scaling=scaling, eps_prim_inf=eps, eps_dual_inf=eps, **st)
        so.warm_start(x=x0, y=y0)
        ro = so.solve()
        assert ro.info.status == want, (eps, ro.info.status, want)
        seen.add(want)
        p, d = CR.certificates(M, dx, dy, val)
        if want.startswith("primal"):
            assert np.abs(p - ro.prim_inf_cert).max() < 1e-9
        if want.startswith("dual"):
            assert np.abs(d - ro.dual_inf_cert).max() < 1e-9
    return M, dy, seen


@pytest.mark.parametrize("at", R.PLANT_AT)
def test_model_agrees_with_the_oracle_on_the_planted_cases(oracle_mod, at):
    """Unscaled data, scaled data with the unscaled test, scaled data with scaled_termination; rows with one, both and no infinite bounds
    and dy of both signs on each kind; primal infeasible, dual infeasible and neither along the sweep of tolerances."""
    sc, x0, y0 = CR.planted(300, 300, at, seed=90 + at, scaled=False)
    seen = set()
    for scaling, stt in ((0, 0), (10, 0), (10, 1)):
        # (with the oracle's own Ruiz scaling and scaled_termination the maxima are taken in ITS scaled space, which equilibrates the planted
        # entries away; the places are asserted where the unscaled quantities decide, and on the device for given D, E in all three forms)
        M, dy, s = _case(oracle_mod, sc, x0, y0, scaling, stt, expect_at=None if (scaling and stt) else at)
        seen |= s
        kinds = [(M.u > 1e26) & (M.l < -1e26), (M.u > 1e26) & (M.l > -1e26), (M.u < 1e26) & (M.l < -1e26), (M.u < 1e26) & (M.l > -1e26)]
        assert all(k.any() for k in kinds) and not dy[kinds[0]].any() and (dy[kinds[1]] < 0).any() and (dy[kinds[2]] > 0).any()
        assert (dy[kinds[3]] < 0).any() and (dy[kinds[3]] > 0).any()
    assert {"maximum iterations reached", "primal infeasible"} <= seen or {"maximum iterations reached", "primal infeasible inaccurate"} <= seen, seen


@pytest.mark.parametrize("i", range(len(R.SIZES)))
def test_model_agrees_with_the_oracle_at_the_kernel_sizes(oracle_mod, i):
    n, m = R.SIZES[i]
    sc, x0, y0 = CR.planted(n, m, -1, seed=n + m, scaled=False)
    _case(oracle_mod, sc, x0, y0, 0, 0, expect_at=-1)


def test_model_agrees_with_the_oracle_without_rows_and_without_movement(oracle_mod):
    sc, x0, y0 = CR.m0()
    M, _, seen = _case(oracle_mod, sc, x0, y0, 10, 0)
    assert M.m == 0 and not any(s.startswith("primal") for s in seen)
    sc, x0, y0 = CR.still()
    M = R.Model(sc, **CR.KERNEL_SETTINGS)
    val, bnd, _ = CR.cert_scalars(M, np.zeros(M.n), np.zeros(M.m))
    assert not val.any() and CR.tests(M, val, 1e6, 1e6, bnd)[:2] == (False, False)         # |d.| = 0 is not > OSQP_DIVISION_TOL
    so = oracle_mod.OracleOSQP().setup(**_unscaled(sc), scaling=0, eps_prim_inf=1e6, eps_dual_inf=1e6, **dict(CR.KERNEL_SETTINGS, eps_abs=0.0))
    assert so.solve().info.status == "maximum iterations reached"


def test_thresholds_are_strict_in_the_model():
    """Values exactly on eps |d.|: `<` and `>` as the reference writes them; a norm exactly on OSQP_DIVISION_TOL is too small."""
    M = R.Model(R.banded(4, 5, seed=1))
    base = dict(ndy=4.0, viol=0.0, lhs=-1.0, nAtdy=0.5, ndx=4.0, qdx=-1.0, nPdx=0.5)
    t = lambda **kw: CR.tests(M, [dict(base, **kw)[k] for k in CR.SC7_NAMES], 0.25, 0.25)[:2]
    assert t() == (True, True) and t(lhs=1.0) == (False, True) and t(nAtdy=1.0) == (False, True) and t(ndy=1e-30) == (False, True)
    assert t(qdx=1.0) == (True, False) and t(nPdx=1.0) == (True, False) and t(viol=1.0) == (True, True)
    assert t(viol=np.nextafter(1.0, 2.0)) == (True, False) and t(ndx=1e-30) == (True, False) and t(lhs=np.nextafter(1.0, 0.0)) == (True, True)
