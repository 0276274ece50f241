"""GPU tests of the fused termination check (OSQP_AMD_FUSED_CHECK, engine.hip hipeng_run_admm_check / osqp_host.c osqp_solve).

A window of ADMM iterations that ends where osqp_solve looks at the residuals (a termination check, a printed line, a rho-interval
check, the last iteration) carries the residual pass directly behind its graphs; scalars and State come back in one copy after one
wait.  With the switch on, the window's prologue, hipeng_cold_start and the reset of the PCG start history are one launch each.
None of it changes an operand: every solve below is run twice, switch on and switch off (the switch is read when the engine is
created), and x, y, both certificates and every field of info except the times must agree in every bit.

The waits are the code's own count (osqp_amd_get_stats, host_syncs).  With the switch on a solve waits once per window and once for
the download; with it off, once more per window that ends in a look.  A certificate pass (hipeng_certificates, taken when a check
finds a candidate for an infeasibility certificate) is a wait of its own under either setting, and how many a solve takes is not
visible from outside: `_waits` takes their number from the run with the switch off, where every other wait is known, and holds the
run with the switch on to exactly windows + download + that number.  `_windows` below replays osqp_solve's window rule."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

PRINT_INTERVAL = 200
INFO = ("iter", "status", "status_val", "obj_val", "pri_res", "dua_res", "rho_updates", "rho_estimate", "status_polish")


def _windows(iters, max_iter, check, rho_interval, verbose, adaptive_rho=True):
    """(windows, windows that end in a look at the residuals) of a solve that stopped after `iters` iterations."""
    if adaptive_rho and not rho_interval:
        rho_interval = 4 * check if check else 100
    it = w = looks = 0
    while it < iters:
        nxt = max_iter
        if check:
            nxt = min(nxt, (it // check + 1) * check)
        if adaptive_rho and rho_interval:
            nxt = min(nxt, (it // rho_interval + 1) * rho_interval)
        if verbose:
            nxt = min(nxt, 1 if it == 0 else (it // PRINT_INTERVAL + 1) * PRINT_INTERVAL)
        nxt = min(nxt, it + 128)
        w += 1
        looks += int(bool(check and nxt % check == 0) or bool(verbose and (nxt % PRINT_INTERVAL == 0 or nxt == 1))
                     or bool(adaptive_rho and rho_interval and nxt % rho_interval == 0) or nxt == max_iter)
        it = nxt
    return w, looks


def _waits(tag, on, off, w, looks):
    """The waits of both runs: off = windows + looks + download + certificate passes; on = windows + download + the same passes."""
    certs = off.syncs - (w + looks + 1)
    assert certs >= 0, (tag, off.syncs, w, looks)
    assert on.syncs == w + 1 + certs, (tag, on.syncs, off.syncs, w, looks, certs)
    return certs


def _solve(monkeypatch, switch, pb, env=None, **kw):
    import osqp_amd
    monkeypatch.setenv("OSQP_AMD_FUSED_CHECK", str(switch))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    s = osqp_amd.OSQP().setup(**pb, **kw)
    s0 = s.stats()
    r = s.solve()
    s1 = s.stats()
    r.syncs = s1["host_syncs"] - s0["host_syncs"]
    r.resident = s1["resident"]
    s.cleanup()
    return r


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _same(tag, a, b):
    for k in ("x", "y", "prim_inf_cert", "dual_inf_cert"):
        assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), (tag, k)
    for k in INFO:
        va, vb = getattr(a.info, k), getattr(b.info, k)
        if isinstance(va, float):
            assert _bits([va])[0] == _bits([vb])[0], (tag, k, va, vb)
        else:
            assert va == vb, (tag, k, va, vb)


def _pair(monkeypatch, tag, pb, env=None, **kw):
    on = _solve(monkeypatch, 1, pb, env, **kw)
    off = _solve(monkeypatch, 0, pb, env, **kw)
    print(tag, "iter", on.info.iter, on.info.status, "waits on/off", on.syncs, off.syncs)
    _same(tag, on, off)
    return on, off


@pytest.mark.parametrize("form", ["resident", "steps"])
@pytest.mark.parametrize("check", [1, 7, 25])
def test_stop_in_the_middle_of_a_window(gpu_lib, monkeypatch, form, check):
    """A QP that stops at an iteration that is no multiple of 128: check_termination = 1, 7, 25 on the resident PCG and on the
    launch-per-step kernels (whose first windows of a solve are two iterations long and may stall: the early scalars of such a
    window are dropped).  On the resident form the waits are exactly one per window plus the download."""
    from osqp_amd.problems import random_sparse_qp
    pb = random_sparse_qp(600, 1200, seed=5)
    env = dict(OSQP_AMD_DENSE_SMALL=0, OSQP_AMD_RESIDENT=int(form == "resident"))
    kw = dict(check_termination=check, max_iter=4000)
    on, off = _pair(monkeypatch, (form, check), pb, env, **kw)
    assert on.info.status == "solved" and on.resident == int(form == "resident")
    assert on.info.iter % 128 != 0
    w, looks = _windows(on.info.iter, 4000, check, 0, False)
    if form == "resident":
        certs = _waits((form, check), on, off, w, looks)
        assert check != 25 or certs == 0, (on.syncs, off.syncs, w, looks)       # (no candidate at iteration 25 and later on this QP)
    else:
        assert w + 1 <= on.syncs <= off.syncs, (on.syncs, off.syncs, w)


def test_verbose_and_rho_interval_off_the_check_cadence(gpu_lib, monkeypatch, capfd):
    """verbose = 1 (a look at iteration 1 and every 200: print and check coincide at 200) with adaptive_rho_interval = 75, no
    multiple of check_termination = 20: windows that end in a print alone, a rho check alone, a check alone, and several at once.
    (tests/test_gpu_statuses.py runs this QP at eps = 1e-6 past iteration 175; at 1e-8 it cannot stop before 200.)"""
    from osqp_amd.problems import random_sparse_qp
    pb = random_sparse_qp(300, 600, seed=5)
    kw = dict(eps_abs=1e-8, eps_rel=1e-8, max_iter=450, adaptive_rho_interval=75, check_termination=20, verbose=1)
    on, off = _pair(monkeypatch, "verbose", pb, dict(OSQP_AMD_DENSE_SMALL=0), **kw)
    capfd.readouterr()
    assert on.info.iter >= 200
    w, looks = _windows(on.info.iter, 450, 20, 75, True)
    _waits("verbose", on, off, w, looks)


def test_max_iter_without_a_check(gpu_lib, monkeypatch):
    """check_termination = 0 and no adaptive rho: the only look is the one behind the last window (200 = 128 + 72)."""
    from osqp_amd.problems import random_sparse_qp
    pb = random_sparse_qp(300, 600, seed=5)
    kw = dict(check_termination=0, adaptive_rho=0, max_iter=200, eps_abs=1e-12, eps_rel=1e-12)
    on, off = _pair(monkeypatch, "max_iter", pb, dict(OSQP_AMD_DENSE_SMALL=0), **kw)
    assert on.info.iter == 200 and on.info.status == "maximum iterations reached"
    _waits("max_iter", on, off, 2, 1)


@pytest.mark.parametrize("A, u, want", [("A12", "u2", "primal infeasible"), ("A34", "u3", "dual infeasible")])
def test_certificate_pass_follows_a_fused_check(gpu_lib, monkeypatch, A, u, want):
    """The small infeasible QPs of tests/golden: the certificate kernel runs right after a check whose scalars came with the window."""
    d = load_golden("primal_dual_infeasibility")
    pb = dict(P=d["P"], q=d["q"], A=d[A], l=d["l"], u=d[u])
    on, off = _pair(monkeypatch, want, pb, None, alpha=1.6, max_iter=50)
    assert on.info.status == want
    w, looks = _windows(on.info.iter, 50, 25, 0, False)
    assert _waits(want, on, off, w, looks) >= 1


def test_second_solve_on_the_same_workspace(gpu_lib, monkeypatch):
    """Cold start and reset of the start history in one launch each: a workspace solved twice (the second solve starts from the
    first's solution, warm_start = 1) and once more after a new q, against the switch off."""
    import osqp_amd
    from osqp_amd.problems import random_sparse_qp
    pb = random_sparse_qp(600, 1200, seed=7)
    out = {}
    for switch in (1, 0):
        monkeypatch.setenv("OSQP_AMD_FUSED_CHECK", str(switch))
        monkeypatch.setenv("OSQP_AMD_DENSE_SMALL", "0")
        s = osqp_amd.OSQP().setup(**pb, warm_start=0)
        r = [s.solve(), s.solve()]
        s.update(q=pb["q"] * 1.5)
        r.append(s.solve())
        s.cleanup()
        out[switch] = r
    for k in range(3):
        _same(("solve", k), out[1][k], out[0][k])
        assert out[1][k].info.status == "solved"
