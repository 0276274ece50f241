"""The infeasibility kernels and the live handle of osqp_amd_rp_solve (csrc/rowpart_native.h) on the device, one rank, against the
long-double model of tests/_rowpart_cert_reference.py (checked against the oracle on the CPU in tests/test_rowpart_cert_reference.py).

A kernel case is a fresh handle, warm-started at (x0, y0) through osqp_amd_rp_warm_start, that runs ONE iteration with a check.  Read
through osqp_amd_rp_peek: the scaled warm start against numpy (one or two float64 products: exact), dx and the projected dy against the
peeked iterates (one subtraction, one selection: exact), the seven scalars against the model evaluated on the device's own dx, dy, and the
status and the certificates against the model's verdict on the device's own scalars.  Then the update kernels against numpy, whole solves
and the update sequence against the oracle, and the promise that a handle with the tests off is the handle of before."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _rowpart_reference as R
import _rowpart_cert_reference as CR
from conftest import ROOT
from osqp_amd import rowpart

pytestmark = pytest.mark.gpu
LD, U = R.LD, R.U
NEVER = 1e-300        # a tolerance that switches a test on and lets nothing pass: the raw dx, dy stay to be peeked
OLD_PEEKS = ("x", "xt", "z", "y", "rv", "minv", "b", "r", "sc15", "S")


def _handle(scaled, **st):
    return rowpart.NativeRowPartitionedOSQP(world=1).setup(scaled, device=0, **st)


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if np.size(b) else 0.0


def _within(dev, ref, bound, names):
    err = np.abs(np.asarray(dev, dtype=LD) - ref)
    print("  ".join("%s %.6g (err %.2g, bound %.2g)" % (k, float(d), float(e), float(b)) for k, d, e, b in zip(names, dev, err, bound)))
    assert np.all(err <= bound), [k for k, e, b in zip(names, err, bound) if e > b]


def _kernel_case(scaled, x0, y0, **st):
    """One iteration from the warm start; returns (model, peeked state) after checking dx, dy and the seven scalars."""
    st = dict(CR.KERNEL_SETTINGS, **st)
    M = R.Model(scaled, **st)
    h = _handle(scaled, eps_prim_inf=NEVER, eps_dual_inf=NEVER, **st)
    assert h.warm_start(x=x0, y=y0) == 0
    x0s, y0s = M.Dinv * x0, (M.Einv * y0) * M.c
    assert np.array_equal(h.peek("x"), x0s) and np.array_equal(h.peek("xt"), x0s) and np.array_equal(h.peek("y"), y0s)
    if M.m:
        az, aab = M.A_mul(x0s)
        assert np.all(np.abs(h.peek("z").astype(LD) - az) <= (M.LAr + 4) * U * aab)
    r = h.solve()
    d = {k: h.peek(k) for k in ("x", "y", "dx", "dy", "sc7", "sc15")}
    h.cleanup()
    assert r.info.iter == 1 and r.info.status == "maximum iterations reached"
    dx, dy = CR.deltas(M, x0s, y0s, d["x"], d["y"])
    assert np.array_equal(d["dx"], dx) and np.array_equal(d["dy"], dy)
    val, bnd, at = CR.cert_scalars(M, d["dx"], d["dy"])
    _within(d["sc7"], val, bnd, CR.SC7_NAMES)
    return M, d, at


def _verdicts(M, scaled, x0, y0, d, **st):
    """The status and the certificates along EPS_SWEEP against the model's verdict on the device's own scalars."""
    st = dict(CR.KERNEL_SETTINGS, **st)
    seen = set()
    for eps in CR.EPS_SWEEP:
        prim, dual, _ = CR.tests(M, d["sc7"], 10 * eps, 10 * eps)           # (max_iter = 1 with residuals that never pass: the approximate branch decides)
        prim0, dual0, _ = CR.tests(M, d["sc7"], eps, eps)
        want = ("primal infeasible" if prim0 else "dual infeasible" if dual0 else "primal infeasible inaccurate" if prim
                else "dual infeasible inaccurate" if dual else "maximum iterations reached")
        h = _handle(scaled, eps_prim_inf=eps, eps_dual_inf=eps, **st)
        h.warm_start(x=x0, y=y0)
        r = h.solve()
        after = [h.peek(k) for k in ("x", "xt", "z", "y")]
        h.cleanup()
        assert r.info.status == want, eps
        seen.add(want.replace(" inaccurate", ""))
        p, q = CR.certificates(M, d["dx"], d["dy"], d["sc7"])
        if want.startswith("primal"):
            assert np.array_equal(r.prim_inf_cert, p) and np.isnan(r.dual_inf_cert).all() and r.info.obj_val == 1e30
        elif want.startswith("dual"):
            assert np.array_equal(r.dual_inf_cert, q) and np.isnan(r.prim_inf_cert).all() and r.info.obj_val == -1e30
        if want != "maximum iterations reached":
            assert np.isnan(r.x).all() and np.isnan(r.y).all() and not any(v.any() for v in after)
    return seen


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SIZES)))
def test_cert_kernels_at_the_workgroup_and_grid_boundaries(gpu_lib, i):
    """n and m in {1, 255, 256, 257, 32 768, 32 769}, the four planted maxima in the last row and the last column (beyond the first sweep
    at the two large sizes); scaled data with the unscaled test, scaled data with scaled_termination, and unscaled data by turns."""
    n, m = R.SIZES[i]
    scaled, stt = (True, 0) if i % 3 == 0 else (True, 1) if i % 3 == 1 else (False, 0)
    sc, x0, y0 = CR.planted(n, m, -1, seed=n + m, scaled=scaled)
    M, d, at = _kernel_case(sc, x0, y0, scaled_termination=stt)
    assert CR.planted_at(at, n, m, -1), at
    if m >= 255:
        kinds = [(M.u > 1e26) & (M.l < -1e26), (M.u > 1e26) & (M.l > -1e26), (M.u < 1e26) & (M.l < -1e26), (M.u < 1e26) & (M.l > -1e26)]
        assert all(k.any() for k in kinds) and not d["dy"][kinds[0]].any() and (d["dy"][kinds[1]] <= 0).all() and (d["dy"][kinds[2]] >= 0).all()
        assert (d["dy"][kinds[1]] < 0).any() and (d["dy"][kinds[2]] > 0).any() and (d["dy"][kinds[3]] < 0).any() and (d["dy"][kinds[3]] > 0).any()


@pytest.mark.parametrize("at", R.PLANT_AT)
@pytest.mark.parametrize("scaled,scaled_termination", [(False, 0), (True, 0), (True, 1)])
def test_cert_scalars_with_the_largest_entry_planted(gpu_lib, at, scaled, scaled_termination):
    """The largest |E dy| and the largest row violation at row 0, 63, 64, 255, 256 and the last of 300, the largest |Dinv A'dy| and
    |Dinv P dx| at that column, and the verdicts along the sweep of tolerances."""
    n = m = 300
    sc, x0, y0 = CR.planted(n, m, at, seed=90 + at, scaled=scaled)
    M, d, where = _kernel_case(sc, x0, y0, scaled_termination=scaled_termination)
    assert CR.planted_at(where, n, m, at), where
    seen = _verdicts(M, sc, x0, y0, d, scaled_termination=scaled_termination)
    print(sorted(seen))
    assert len(seen) >= 2


def test_cert_kernels_without_rows_and_without_movement(gpu_lib):
    """m_total = 0: the row scalars stay 0, the primal test is off, the dual one decides alone.  Nothing moves: both norms are 0, at most
    OSQP_DIVISION_TOL, and no tolerance makes that infeasible."""
    sc, x0, y0 = CR.m0()
    M, d, _ = _kernel_case(sc, x0, y0)
    assert not d["sc7"][:4].any() and d["sc7"][4] > 0
    _verdicts(M, sc, x0, y0, d)
    sc, x0, y0 = CR.still()
    h = _handle(sc, eps_prim_inf=1e6, eps_dual_inf=1e6, **dict(CR.KERNEL_SETTINGS, eps_abs=0.0))
    r = h.solve()
    assert not h.peek("sc7").any() and not h.peek("dx").any() and not h.peek("dy").any()
    h.cleanup()
    assert r.info.status == "maximum iterations reached"


# ---- the update kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 255), (255, 256), (256, 257), (257, 1), (32769, 32769)])
def test_update_kernels_against_numpy(gpu_lib, n, m):
    sc = R.banded(n, m, seed=3 * n + m, scaled=True)
    rng = np.random.RandomState(n + m)
    h = _handle(sc)
    D, E, c = sc["D"], sc["E"], sc["c"]
    q = rng.randn(n)
    assert h.update(q=q) == 0 and np.array_equal(h.peek("q"), (D * q) * c)
    l, u = -1.0 - np.abs(rng.randn(m)), 1.0 + np.abs(rng.randn(m))
    l[::5], u[1::5], u[2::5] = -np.inf, 1e40, l[2::5]                 # clamped to +-1e30; equality rows
    assert h.update(l=l, u=u) == 0
    lo, hi = np.maximum(l, -1e30), np.minimum(u, 1e30)
    assert np.array_equal(h.peek("l"), E * lo) and np.array_equal(h.peek("u"), E * hi)
    k = int(np.flatnonzero(hi < 1e30)[-1])                            # the last row with a finite upper bound
    bad_l = l.copy(); bad_l[k] = hi[k] + 1.0
    assert k >= m - 2 and bad_l[k] > hi[k]
    assert h.update(l=bad_l, u=u) == 1 and np.array_equal(h.peek("l"), E * lo) and np.array_equal(h.peek("u"), E * hi)
    assert h.update(q=2 * q, l=bad_l, u=u) == 1 and np.array_equal(h.peek("q"), (D * q) * c)          # refused bounds leave q as it was, too
    x, y = rng.randn(n), rng.randn(m)
    assert h.warm_start(x=x, y=y) == 0
    assert np.array_equal(h.peek("x"), (1.0 / D) * x) and np.array_equal(h.peek("xt"), (1.0 / D) * x) and np.array_equal(h.peek("y"), ((1.0 / E) * y) * c)
    assert h.warm_start(y=2 * y) == 0 and np.array_equal(h.peek("x"), (1.0 / D) * x) and np.array_equal(h.peek("y"), ((1.0 / E) * (2 * y)) * c)
    h.cleanup()


def test_bounds_update_rebuilds_rho_only_on_a_class_change_and_update_rho_at_once(gpu_lib):
    sc = R.banded(257, 255, seed=6, scaled=True)
    h = _handle(sc, max_iter=1, adaptive_rho=0)
    h.solve()
    rv, minv = h.peek("rv"), h.peek("minv")
    l, u = sc["l"] / sc["E"], sc["u"] / sc["E"]
    assert h.update(l=l - 0.5 * (R.row_class(sc["l"], sc["u"]) == 0), u=u) == 0            # inequality rows move, no class changes
    assert np.array_equal(h.peek("rv"), rv) and np.array_equal(h.peek("minv"), minv)
    l2 = l.copy(); l2[0] = u[0]                                                            # row 0 (narrow) becomes an equality row
    assert h.update(l=l2, u=u) == 0
    want = R.rho_vec(h.peek("l"), h.peek("u"), 0.1)
    assert want[0] == 100.0 and np.array_equal(h.peek("rv"), want) and not np.array_equal(h.peek("minv"), minv)
    assert h.update_rho(0.0) == 1 and h.update_rho(-1.0) == 1 and np.array_equal(h.peek("rv"), want)
    assert h.update_rho(1e9) == 0 and np.array_equal(h.peek("rv"), R.rho_vec(h.peek("l"), h.peek("u"), 1e6))
    M = R.Model(dict(sc, l=h.peek("l"), u=h.peek("u")))
    mi, mi_b = M.minv(h.peek("rv"))
    assert np.all(np.abs(h.peek("minv").astype(LD) - mi) <= mi_b)
    h.cleanup()


# ---- whole solves ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.SOLVE_NAMES)
def test_whole_solves_match_the_oracle(gpu_lib, oracle_mod, name):
    pb, kw = CR.solve_problem(name)
    ro = oracle_mod.OracleOSQP().setup(**pb, **kw).solve()
    h = _handle(rowpart.scaled_problem_from_engine(**pb), **kw)
    r = h.solve()
    after = [h.peek(k) for k in ("x", "xt", "z", "y")]
    h.cleanup()
    print(name, ro.info.status, ro.info.iter, "|", r.info.status, r.info.iter)
    assert (r.info.status, r.info.iter) == (ro.info.status, ro.info.iter)
    if ro.info.status in CR.INFEASIBLE:
        prim = ro.info.status.startswith("primal")
        mine, theirs = (r.prim_inf_cert, ro.prim_inf_cert) if prim else (r.dual_inf_cert, ro.dual_inf_cert)
        print("certificate: %.3e" % _rel(mine, theirs))
        assert _rel(mine, theirs) < 1e-5 and r.info.obj_val == ro.info.obj_val == (1e30 if prim else -1e30)
        assert np.isnan(r.x).all() and np.isnan(r.y).all() and not any(v.any() for v in after)
    else:
        assert _rel(r.x, ro.x) < 1e-6 and _rel(r.y, ro.y) < 1e-6


def test_update_sequence_matches_the_oracle(gpu_lib, oracle_mod):
    pb, kw, steps = CR.sequence()
    so = oracle_mod.OracleOSQP().setup(**pb, **kw)
    h = _handle(rowpart.scaled_problem_from_engine(**pb), **kw)
    k = 0
    for call, args in steps:
        a, b = getattr(so, call)(**args), getattr(h, call)(**args)
        if call != "solve":
            assert int(bool(a)) == b, (call, a, b)
            continue
        print("solve %d: oracle %s / %d   native %s / %d" % (k, a.info.status, a.info.iter, b.info.status, b.info.iter))
        assert (b.info.status, b.info.iter, b.info.rho_updates) == (a.info.status, a.info.iter, a.info.rho_updates)
        if k:
            assert _rel(b.x, a.x) < 1e-6 and _rel(b.y, a.y) < 1e-6
        else:
            assert _rel(b.prim_inf_cert, a.prim_inf_cert) < 1e-5
        k += 1
    h.cleanup()
    assert k == 5


# ---- off is the handle of before -------------------------------------------------------------------------------------------------------
def test_tests_off_changes_nothing_and_tests_on_changes_no_iterate(gpu_lib):
    """A feasible solve on a handle that never calls osqp_amd_rp_set_infeasibility, on one that calls it with (0, 0), and on one with the
    tests on: the first two agree bit for bit in all ten peek arrays, info and collectives; the third in x, z, y and the solution."""
    from osqp_amd.problems import random_sparse_qp
    scaled = rowpart.scaled_problem_from_engine(**random_sparse_qp(300, 600, seed=5))
    got = []
    for mode in ("never", "zero", "on"):
        h = _handle(scaled)
        if mode == "zero":
            h.set_infeasibility(0.0, 0.0)
        if mode == "on":
            h.set_infeasibility(1e-4, 1e-4)
        r = h.solve()
        got.append((r, {k: h.peek(k) for k in OLD_PEEKS}))
        h.cleanup()
    (ra, da), (rb, db), (rc, dc) = got
    assert ra.info.status == "solved"
    for k in OLD_PEEKS:
        assert da[k] == db[k] if k == "S" else np.array_equal(da[k], db[k]), k
    assert vars(ra.info) == vars(rb.info) and np.array_equal(ra.x, rb.x) and np.array_equal(ra.y, rb.y)
    for k in ("x", "z", "y"):
        assert np.array_equal(da[k], dc[k]), k
    assert np.array_equal(ra.x, rc.x) and np.array_equal(ra.y, rc.y) and (rc.info.status, rc.info.iter) == (ra.info.status, ra.info.iter)


def test_rccl_provider_carries_the_two_new_collectives(gpu_lib):
    """tools/rccl_world1_infeasible_probe.py in a process of its own without torch (see tests/test_rowpart.py on why): the stream-ordered
    provider on a one-rank communicator with the tests on, bit-equal to the callback-free loop, at most two collectives per check more than off."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_world1_infeasible_probe.py")], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "probe ok: True" in p.stdout and "infeasible identical: True torch loaded: False" in p.stdout
