"""The k_rp_* kernels and the loop of osqp_amd_rp_solve (csrc/rowpart_native.h) at their edges, one rank, against the long-double
model of tests/_rowpart_reference.py (its cases and its bounds are checked on the CPU in tests/test_rowpart_reference.py).

A step is a fresh handle with max_iter = k (a handle starts from zeros); its state is read with osqp_amd_rp_peek.  For one step:
rho per row exactly, the Jacobi inverse, the right-hand side b and b'b, the PCG's result through the true residual of the peeked
x~ (||b - K x~|| <= 2 eps ||b|| + the rounding of K x~: the factor 2 covers the gap between the recursive and the true residual),
update_x / update_z / update_y from the device's own x~, the fifteen scalars of the check from the device's own x, y, z, and the
info fields and the status from the device's own scalars.  Then the PCG's bookkeeping (RpS) and a second solve on one handle."""
import numpy as np
import pytest

import _rowpart_reference as R
from osqp_amd import rowpart

pytestmark = pytest.mark.gpu
LD, U = R.LD, R.U
HIPENG_ERR_ARG = -103


def _handle(scaled, **st):
    return rowpart.NativeRowPartitionedOSQP(world=1).setup(scaled, device=0, **st)


def _peek_all(h):
    return {k: h.peek(k) for k in ("x", "xt", "z", "y", "rv", "minv", "b", "r", "sc15", "S")}


def _within(dev, ref, bound, what):
    err = np.abs(np.asarray(dev, dtype=LD) - ref)
    bad = err > bound
    assert not bad.any(), "%s: %d beyond the bound, worst %.3g against %.3g at %d" % (
        what, int(bad.sum()), float(err[bad].max()), float(np.asarray(bound)[bad][int(np.argmax(err[bad]))]), int(np.flatnonzero(bad)[0]))


def _check_info(M, sc, info, rho):
    """The info record and the status from the device's own fifteen scalars: selections and single float64 operations, so exact."""
    sc = np.asarray(sc, dtype=np.float64)
    want = M.info(sc, np.float64(rho))
    assert info.pri_res == want["pri_res"] and info.dua_res == want["dua_res"] and info.obj_val == want["obj_val"]
    assert abs(info.rho_estimate - want["rho_estimate"]) <= 4 * U * want["rho_estimate"]
    assert info.status == M.status(sc)


def _check_step(scaled, k=1, expect_iters=None, **st):
    """Iteration k of a fresh handle against the model; returns (model, peeked state, info)."""
    st = dict(dict(check_termination=1, adaptive_rho=0), **st)
    M = R.Model(scaled, max_iter=k, **st)
    n, m = M.n, M.m
    prev = dict(x=np.zeros(n), z=np.zeros(m), y=np.zeros(m))
    if k > 1:
        h = _handle(scaled, max_iter=k - 1, **st)
        r0 = h.solve()
        prev = _peek_all(h)
        h.cleanup()
        assert r0.info.iter == k - 1
    h = _handle(scaled, max_iter=k, **st)
    res = h.solve()
    d = _peek_all(h)
    h.cleanup()
    info, S = res.info, d["S"]
    assert info.iter == k
    # classes and preconditioner
    rv = R.rho_vec(M.l, M.u, M.st["rho"])
    assert d["rv"].shape == (m,) and np.array_equal(d["rv"], rv)
    mi, mi_b = M.minv(rv)
    _within(d["minv"], mi, mi_b, "minv")
    # right-hand side from the previous iterates, b'b and the PCG's threshold from the device's b
    b, b_b = M.rhs(prev["x"], prev["z"], prev["y"], rv)
    _within(d["b"], b, b_b, "b")
    bd = d["b"].astype(LD)
    bb = (bd * bd).sum()
    assert abs(S["bb"] - bb) <= (n + 8) * U * bb
    assert S["tol2"] == max(np.float64(M.eps_pcg) * np.float64(M.eps_pcg) * np.float64(S["bb"]), 1e-30)
    # the linear solve: true residual of the peeked x~
    assert S["done"] == 1 and S["bad"] == 0 and S["rr"] <= S["tol2"] and 0 < S["iters"] < S["cap"]
    if expect_iters is not None:
        assert S["iters"] == expect_iters
    assert info.pcg_iters >= S["iters"]
    kx, kx_b = M.K_mul(d["xt"], rv)
    res2 = np.sqrt(((bd - kx) ** 2).sum())
    lim = 2 * M.eps_pcg * np.sqrt(bb) + np.sqrt((kx_b ** 2).sum())
    print("n %d m %d k %d: pcg iters %d  ||b - K xt|| %.3e  limit %.3e (rounding part %.3e)" % (n, m, k, S["iters"], float(res2), float(lim), float(np.sqrt((kx_b ** 2).sum()))))
    assert res2 <= lim
    # update_x / update_z / update_y from the device's own x~
    s = M.step(d["xt"], prev["x"], prev["z"], prev["y"], rv)
    for name in ("x", "z", "y"):
        _within(d[name], s[name][0], s[name][1], name)
    if m:
        arg, arg_b = s["arg"]
        below, above = arg < M.l - arg_b, arg > M.u + arg_b
        assert np.array_equal(d["z"][below], M.l[below]) and np.array_equal(d["z"][above], M.u[above])
        assert np.all(d["z"] >= M.l) and np.all(d["z"] <= M.u)
    # the check's scalars from the device's own x, y, z; info from the device's own scalars
    sc, sc_b = M.scalars(d["x"], d["y"], d["z"])
    _within(d["sc15"], sc, sc_b, "check scalars " + " ".join(R.SC_NAMES))
    _check_info(M, d["sc15"], info, R.clip_rho(M.st["rho"]))
    if m == 0:
        assert info.pri_res == 0.0 and not d["sc15"][:6].any()
    return M, d, info, s


# ---- classes and preconditioner ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.1, 1e-7, 1e7])
def test_classes_on_the_thresholds_and_the_three_kinds_of_column(gpu_lib, rho):
    """Bounds exactly on +-1e26 and one ulp beyond, u - l exactly 1e-4 and one ulp below; rho settings that clip to 1e-6 / 1e6;
    a column with no diagonal of P stored and an entirely empty one (minv = 1 / sigma)."""
    sc, claimed = R.class_case()
    M, d, info, s = _check_step(sc, rho=rho)
    want = R.clip_rho(rho)
    assert want == {0.1: 0.1, 1e-7: 1e-6, 1e7: 1e6}[rho]
    assert np.array_equal(d["rv"], np.where(claimed == -1, 1e-6, np.where(claimed == 1, 1e3 * want, want)))
    assert d["minv"][4] == 1.0 / M.st["sigma"]


@pytest.mark.parametrize("k", [8191, 8192, 8193])
def test_dense_column_of_A(gpu_lib, k):
    """Row 0 of [P | A'] with k entries: below, at and beyond HUGE_ROW = 8192."""
    _check_step(R.dense_column_case(k))


# ---- one iteration at every size ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SIZES)))
def test_one_iteration_at_the_workgroup_and_grid_boundaries(gpu_lib, i):
    """n and m in {1, 255, 256, 257, 32 768, 32 769}: whole workgroups without an element, the first second element of a thread; alpha and
    scaled data by turns."""
    n, m = R.SIZES[i]
    M, d, info, s = _check_step(R.banded(n, m, seed=n + m, scaled=bool(i % 2)), alpha=(1.0, 1.6)[(i // 2) % 2])
    if n >= 255 and m >= 255:
        z, c = d["z"], M.cls
        assert (z == M.l)[c == 0].any() and (z == M.u)[c == 0].any() and ((z > M.l) & (z < M.u))[c == 0].any() and (c == -1).any() and (c == 1).any()


@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("scaled", [False, True])
def test_one_iteration_both_alphas(gpu_lib, alpha, scaled):
    _check_step(R.banded(256, 257, seed=513, scaled=scaled), alpha=alpha)


@pytest.mark.parametrize("n,m,alpha", [(257, 255, 1.6), (257, 255, 1.0), (32769, 32768, 1.6)])
def test_third_iteration_warm_started_with_a_nonzero_y(gpu_lib, n, m, alpha):
    M, d, info, s = _check_step(R.banded(n, m, seed=n + m, scaled=True), k=3, alpha=alpha)
    assert d["y"].any()


# ---- the check's scalars -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", R.PLANT_AT)
@pytest.mark.parametrize("scaled,scaled_termination", [(False, 0), (True, 0), (True, 1)])
def test_check_scalars_with_the_largest_entry_planted(gpu_lib, at, scaled, scaled_termination):
    """The largest |z|, |Ax - z| and |q| (negative) in lane 0 and 63 of the first wavefront, in the second wavefront, in the last thread, in a
    thread's second turn and in the last element; unscaled data, scaled data with the unscaled and with the scaled termination test."""
    n = m = 300
    sc = R.planted(n, m, at, seed=40 + at, scaled=scaled)
    M, d, info, s = _check_step(sc, scaled_termination=scaled_termination)
    i = at % m
    assert d["z"][i] == -1000.0 and d["sc15"][4] == 1000.0 and d["sc15"][9] == -sc["q"][i]
    assert d["sc15"][1] == abs(M.Einv[i] * -1000.0) and d["sc15"][8] == abs(M.Dinv[i] * sc["q"][i])
    assert info.pri_res == (d["sc15"][0] if scaled and not scaled_termination else d["sc15"][3])
    assert info.dua_res == (d["sc15"][6] / M.c if scaled and not scaled_termination else d["sc15"][7])


@pytest.mark.parametrize("eps", [1e-3, 1e4])
def test_status_from_both_termination_tests(gpu_lib, eps):
    """Far from the solution after one iteration: maximum iterations reached at eps = 1e-3, solved at an eps no residual exceeds; scaled
    and unscaled data, scaled_termination 0 and 1 (the status is compared with the model's decision in _check_step)."""
    for scaled, stt in ((False, 0), (False, 1), (True, 0), (True, 1)):
        M, d, info, s = _check_step(R.banded(257, 255, seed=77, scaled=scaled), scaled_termination=stt, eps_abs=eps, eps_rel=eps, pcg_eps_rel=1e-9)
        assert info.status == ("solved" if eps > 1 else "maximum iterations reached")


def test_no_rows_at_all(gpu_lib):
    """m_total = 0: pri_res is 0.0 exactly, and three iterations work."""
    _check_step(R.m0_case())
    _check_step(R.m0_case(), k=3)


# ---- PCG bookkeeping -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_zero_right_hand_side_takes_no_pcg_iteration(gpu_lib, k):
    """q = 0 and 0 inside the bounds: b = 0, no PCG iteration (the first group's kernels all return at once), x stays 0; with
    check_termination = 0 the second iteration is run as well, its first group as long as max(1, 0)."""
    h = _handle(R.zero_q_case(), max_iter=k, check_termination=0, adaptive_rho=0)
    r = h.solve()
    d = _peek_all(h)
    h.cleanup()
    S = d["S"]
    assert S["iters"] == 0 and S["done"] == 1 and S["bad"] == 0 and S["bb"] == 0.0 and S["tol2"] == 1e-30
    assert r.info.pcg_iters == 0 and not d["x"].any() and not d["xt"].any() and not d["z"].any() and not d["y"].any() and not r.x.any()
    assert r.info.status == "solved" and r.info.iter == k and r.info.pri_res == 0.0 and r.info.dua_res == 0.0


def test_pcg_iteration_cap(gpu_lib):
    sc = R.slow_pcg_case()
    h = _handle(sc, max_iter=4, check_termination=1, adaptive_rho=0, pcg_max_iter=3)
    r = h.solve()
    S = h.peek("S")
    h.cleanup()
    assert S["iters"] == 3 and S["cap"] == 3 and S["done"] == 1 and S["bad"] == 0 and S["rr"] > S["tol2"]
    assert r.info.iter == 4 and r.info.pcg_iters == 3 * r.info.iter


def test_iterations_issued_past_convergence_change_nothing(gpu_lib):
    """K diagonal: the Jacobi-PCG ends after one iteration, the other three of the first group of four return at once."""
    _check_step(R.diagonal_K_case(), expect_iters=1)
    M, d, info, s = _check_step(R.diagonal_K_case(), k=2)
    assert d["S"]["iters"] <= 2


def test_slow_first_solve_is_looked_at_in_groups(gpu_lib):
    """More than four PCG iterations: the first group of four and then groups of two, stopped at the iteration that converged."""
    M, d, info, s = _check_step(R.slow_pcg_case())
    assert d["S"]["iters"] > 20


@pytest.mark.parametrize("case", ["slow", "banded"])
def test_two_solves_of_one_iteration_equal_one_solve_of_two(gpu_lib, case):
    """The same two ADMM iterations as one solve and as two solves on one handle: bit-equal x, y and info.  (The second of the two
    solves keeps the iterates and rho per row, and its PCG starts with a first group as long as the first solve's PCG took.)"""
    sc = R.slow_pcg_case() if case == "slow" else R.banded(257, 255, seed=512, scaled=True)
    st = dict(check_termination=1, adaptive_rho=0)
    a = _handle(sc, max_iter=2, **st)
    ra = a.solve()
    da = _peek_all(a)
    a.cleanup()
    b = _handle(sc, max_iter=1, **st)
    r1 = b.solve()
    first = b.peek("S")["iters"]
    rb = b.solve()
    db = _peek_all(b)
    b.cleanup()
    assert first > 4 and ra.info.iter == 2 and rb.info.iter == 1 and r1.info.pcg_iters + rb.info.pcg_iters == ra.info.pcg_iters
    for k in ("x", "xt", "z", "y", "b", "sc15"):
        assert np.array_equal(da[k], db[k]), k
    assert da["S"] == db["S"] and np.array_equal(ra.x, rb.x) and np.array_equal(ra.y, rb.y)
    for k in ("status", "obj_val", "pri_res", "dua_res", "rho_estimate", "rho_updates"):
        assert getattr(ra.info, k) == getattr(rb.info, k), k


def test_nonconvex_problem_is_an_error_return(gpu_lib):
    """p'Kp <= 0 in the first PCG iteration: `bad` on the device, HIPENG_ERR_ARG from osqp_amd_rp_solve, an exception from the wrapper,
    and the handle can still be read and freed."""
    h = _handle(R.nonconvex_case(), max_iter=5)
    with pytest.raises(RuntimeError, match=r"\(%d\)" % HIPENG_ERR_ARG):
        h.solve()
    S = h.peek("S")
    assert S["bad"] == 1 and S["done"] == 1 and S["iters"] == 1
    assert not h.peek("xt").any()                     # the step length of that iteration is zero
    h.cleanup()


# ---- a second solve on the same handle ---------------------------------------------------------------------------------------------
def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.parametrize("which", ["random", "portfolio_small"])
def test_second_solve_on_one_handle_matches_the_oracles_second_solve(gpu_lib, oracle_mod, which):
    """Two solves on one handle against two solves on one oracle workspace, each against the solve of the same ordinal: status, iter,
    rho_updates equal, x and y to 1e-6, objective to 1e-8.  The second starts from the kept iterates with the adapted rho and counts
    rho_updates on.  (With rho put back to the setting, as before this test existed, the second solve of the random problem takes
    other iterations and ends 5.6e-4 (x) and 2.5e-3 (y) away on the CPU variant.)"""
    from osqp_amd.problems import portfolio_qp, random_sparse_qp
    if which == "random":
        pb, kw, want = random_sparse_qp(300, 600, seed=5), dict(max_iter=110), ((110, 1), (25, 1))
    else:
        pb, kw, want = portfolio_qp(8, 25, sector_rows=5, seed=3), dict(eps_abs=1e-5, eps_rel=1e-5), None
    so = oracle_mod.OracleOSQP().setup(**pb, **kw)
    h = _handle(rowpart.scaled_problem_from_engine(**pb), **kw)
    for ordinal in range(2):
        ro, r = so.solve(), h.solve()
        print("%s solve %d: oracle %s / %d / %d   native %s / %d / %d   x %.3e  y %.3e  obj %.3e" % (
            which, ordinal + 1, ro.info.status, ro.info.iter, ro.info.rho_updates, r.info.status, r.info.iter, r.info.rho_updates,
            _rel(r.x, ro.x), _rel(r.y, ro.y), abs(r.info.obj_val - ro.info.obj_val)))
        if want:
            assert (ro.info.iter, ro.info.rho_updates) == want[ordinal]
        assert r.info.status == ro.info.status == "solved" and r.info.iter == ro.info.iter and r.info.rho_updates == ro.info.rho_updates
        assert _rel(r.x, ro.x) < 1e-6 and _rel(r.y, ro.y) < 1e-6
        assert abs(r.info.obj_val - ro.info.obj_val) <= 1e-8 * max(1.0, abs(ro.info.obj_val))
    h.cleanup()
