"""GPU tests of the per-call limits of a batch solve: `BatchOSQP.solve(max_iter=, time_limit=)` and `solve_report()`
(osqp_amd_batch_solve_limited / _solve_report; admm_loop<.., CLOCK>, k_batch_solve<.., 3>, k_bs_loop<true>, bc_solve).

Almost every comparison is an identity.  A call with max_iter = k leaves what a handle set up with max_iter = k leaves
-- results, certificates, the member workspace (rho, K^-1), rounds, columns, and, through the bits of a second solve that
starts from them, the stored iterates.  A clock that cannot bind changes nothing; a clock that has already expired ends
every member at the first clock iteration (tests/test_batch_limits_cases_host.py proves no member ends earlier) with
the record of a max_iter = INTERVAL handle, the status word aside; a clock in between leaves every member in one of
two classes, whichever way the timing falls.  Where the oracle is asked, the bar is the batch parity bar
(tests/_batch_parity.py: assert_parity)."""
from types import SimpleNamespace

import ctypes as C
import numpy as np
import pytest

from _batch_parity import assert_parity
from _limits_cases import (BETWEEN, BUDGET, BUDGET_COMMON_ADAPTIVE, CHECK, EXPIRED, INTERVAL, KS, MAX_ITER, SHAPES,
                           member_oracles, problem)

pytestmark = pytest.mark.gpu

ARRAYS = ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert")
TIME_LIMIT_REACHED, MAX_ITER_REACHED, SOLVED_INACCURATE = -6, -2, 2
# name -> (shape of _limits_cases, extra setup arguments, settings of the budget tests, compared with the oracle)
HANDLES = {
    "tile4": ("tile4", {}, BUDGET["tile4"], True),
    "tile8": ("tile8", {}, BUDGET["tile8"], True),
    "streamed": ("streamed", {}, BUDGET["streamed"], True),
    "common": ("common", {}, BUDGET["common"], True),
    "common-kkt": ("common", dict(shared_kkt=True), BUDGET["common"], True),
    "common-adaptive": ("common", {}, BUDGET_COMMON_ADAPTIVE, False),
}


def _setup(name, kw, **extra):
    import osqp_amd
    engine, P, A, Q, L, U = problem(name)
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **dict(kw, **extra))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _record(r, rows=slice(None), status_aside=False):
    """The bits of the rows' results; status_aside: without the status word of info8."""
    out = {}
    for k in ARRAYS:
        a = np.array(getattr(r, k)[rows], dtype=np.float64)
        if k == "info_raw" and status_aside:
            a[..., 1] = 0.0
        out[k] = _bits(a)
    return out


def _state(bs, r, status_aside=False):
    """Everything a solve leaves that a test can read: the results, rounds, columns and the member workspace (the
    common-K engine has one; the others are read at both ends of the batch)."""
    st = _record(r, status_aside=status_aside)
    st["rounds"] = np.array(bs.rounds())
    if bs.engine == "common":
        st["columns"] = np.array(bs.columns())
    for qp in ((0,) if bs.engine == "common" else (0, bs.B - 1)):
        for k, v in bs.member_workspace(qp).items():
            st["ws%d.%s" % (qp, k)] = _bits(v) if np.asarray(v).dtype.kind == "f" else np.asarray(v)
    return st


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def _oracle_member(unscale, ro):
    x, y, obj = unscale(ro)
    return SimpleNamespace(x=x, y=y, info=SimpleNamespace(status_val=ro.info.status_val, iter=ro.info.iter,
                                                          rho_updates=ro.info.rho_updates, obj_val=obj))


# ---- budget ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS, ids=[str(k) for k in KS])
@pytest.mark.parametrize("name", list(HANDLES))
def test_budget_equals_a_handle_set_up_with_it(gpu_lib, oracle_mod, name, k):
    shape, extra, kw, with_oracle = HANDLES[name]
    lim = _setup(shape, kw, **extra)
    if k is None:                                        # past every member's convergence
        probe = _setup(shape, kw, **extra)
        k = int(probe.solve().iter.max()) + 7
        if shape == "streamed":
            assert probe.rounds()[0] > 1                 # some member left for a rebuild in the unlimited solve
        probe.cleanup()
    ref = _setup(shape, dict(kw, max_iter=k), **extra)
    first = None
    for turn in range(2):                                # the second solve starts from the iterates the first one stored
        r, rr = lim.solve(max_iter=k), ref.solve()
        first = first or r
        print(name, "k", k, "turn", turn, "iter", np.unique(r.iter), "status", np.unique(r.status_val), lim.rounds())
        _assert_same(_state(lim, r), _state(ref, rr), "max_iter=%d, solve %d" % (k, turn))
        assert lim.solve_report() == (k, 0.0, 0.0, 0) and np.all(r.iter <= k)
    r = lim.solve()                                      # the setup's cap is back
    assert lim.solve_report() == (MAX_ITER, 0.0, 0.0, 0)
    if with_oracle:
        some = None if lim.B <= 8 else range(0, lim.B, 9)
        for b, (so, unscale) in member_oracles(oracle_mod, shape, kw, members=some).items():
            so.update_settings(max_iter=k)
            ro = so.solve()
            if k == 10:                                  # the limited solve itself against the oracle's max_iter = k run
                assert_parity(first, b, _oracle_member(unscale, ro), "%s max_iter=%d" % (name, k))
            so.solve()
            so.update_settings(max_iter=MAX_ITER)
            assert_parity(r, b, _oracle_member(unscale, so.solve()), "%s plain solve after max_iter=%d" % (name, k))
    lim.cleanup(); ref.cleanup()


# ---- a clock that cannot bind ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HANDLES))
def test_a_clock_that_cannot_bind_changes_nothing(gpu_lib, name):
    shape, extra, kw, _ = HANDLES[name]
    lim, ref = _setup(shape, kw, **extra), _setup(shape, kw, **extra)
    for turn in range(2):
        r, rr = lim.solve(time_limit=1e3), ref.solve()
        _assert_same(_state(lim, r), _state(ref, rr), "time_limit=1e3, solve %d" % turn)
        rep = lim.solve_report()
        print(name, rep)
        assert rep.max_iter == MAX_ITER and rep.time_limit == 1e3 and rep.cut == 0 and 0.0 < rep.elapsed < 1e3
        assert ref.solve_report() == (MAX_ITER, 0.0, 0.0, 0)
    lim.cleanup(); ref.cleanup()


# ---- a clock that has already expired ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tile4", "tile8", "streamed", "common", "common-kkt"])
def test_a_clock_that_has_expired_stops_every_member_at_the_first_clock_iteration(gpu_lib, oracle_mod, name):
    shape, extra = HANDLES[name][:2]
    kw = EXPIRED[shape]
    lim, ref = _setup(shape, kw, **extra), _setup(shape, dict(kw, max_iter=INTERVAL), **extra)
    r, rr = lim.solve(time_limit=1e-9), ref.solve()
    rep = lim.solve_report()
    print(name, rep, "status", np.unique(r.status_val), "rho_updates", r.rho_updates, lim.rounds())
    assert np.all(r.iter == INTERVAL)
    assert np.all(np.isin(r.status_val, (TIME_LIMIT_REACHED, SOLVED_INACCURATE)))
    assert np.array_equal(r.status_val == TIME_LIMIT_REACHED, rr.status_val == MAX_ITER_REACHED)
    assert np.array_equal(r.status_val == SOLVED_INACCURATE, rr.status_val == SOLVED_INACCURATE)
    _assert_same(_state(lim, r, status_aside=True), _state(ref, rr, status_aside=True), "time_limit=1e-9")
    assert rep.max_iter == kw["max_iter"] and rep.time_limit == 1e-9 and rep.cut == lim.B and rep.elapsed > 0.0
    if shape == "streamed":                              # nobody left for a rebuild, though rho moved in that iteration
        assert lim.rounds()[0] == 1 and np.any(r.rho_updates > 0)
    # polish and adjoint skip a member the clock stopped -- "not tried" -- and leave its bits alone
    if name != "common":
        before = _record(r)
        rp = lim.polish()
        assert not rp.status_polish.any()
        _assert_same(before, _record(rp), "polish")
        ad = lim.adjoint(np.ones((lim.B, lim.n)))
        assert not ad.status_adjoint.any() and not ad.dq.any() and not ad.dl.any() and not ad.du.any()
        _assert_same(before, _record(lim.results()), "adjoint")
    # streamed: the plain solve that follows goes on from the stored iterates with a current K^-1 -- the rebuild was
    # left to the host's last pass -- and ends where the oracle ends (the other engines: the budget test's plain solve)
    if shape == "streamed":
        r2 = lim.solve()
        for b, (so, unscale) in member_oracles(oracle_mod, shape, kw).items():
            so.update_settings(max_iter=INTERVAL)
            so.solve()
            so.update_settings(max_iter=kw["max_iter"])
            assert_parity(r2, b, _oracle_member(unscale, so.solve()), "%s plain solve after the cut" % name)
    lim.cleanup(); ref.cleanup()


# ---- a clock in between ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_clock_in_between_leaves_two_classes_of_member(gpu_lib, name):
    """Nothing is asserted about how many members the clock stops.  Every member is either untouched -- its record is
    that of the unlimited solve -- or stopped: status -6 or 2 at a positive multiple of the check interval, with the record
    (status word aside) of a fresh handle's solve(max_iter=iter)."""
    kw = BETWEEN[name]
    full = _setup(name, kw)
    rf = full.solve(time_limit=1e3)
    half = 0.5 * full.solve_report().elapsed
    lim = _setup(name, kw)
    r = lim.solve(time_limit=half)
    rep = lim.solve_report()
    print(name, "limit", half, rep, "iter", r.iter, "unlimited", rf.iter, "status", r.status_val)
    capped, stopped = {}, 0
    for b in range(lim.B):
        if all(np.array_equal(v, _record(rf, b)[k]) for k, v in _record(r, b).items()):
            continue
        k = int(r.iter[b])
        assert r.status_val[b] in (TIME_LIMIT_REACHED, SOLVED_INACCURATE), (b, r.status_val[b])
        assert k > 0 and k % CHECK == 0 and k <= MAX_ITER, (b, k)
        if k not in capped:
            h = _setup(name, kw)
            capped[k] = h.solve(max_iter=k)
            h.cleanup()
        _assert_same(_record(r, b, status_aside=True), _record(capped[k], b, status_aside=True), "member %d cut at %d" % (b, k))
        stopped += 1
    assert rep.cut >= stopped and rep.time_limit == half      # (a stopped member may equal its unlimited record)
    full.cleanup(); lim.cleanup()


# ---- chosen members with limits (common-K) -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["max_iter", "time_limit"])
def test_members_with_limits(gpu_lib, kind):
    S = [0, 3, 63, 64, 69]
    kw = BUDGET["common"] if kind == "max_iter" else EXPIRED["common"]
    k = 10 if kind == "max_iter" else INTERVAL
    lim, ref = _setup("common", kw), _setup("common", dict(kw, max_iter=k))
    r0 = lim.results()                                   # what setup left in every member's record
    rest = np.setdiff1d(np.arange(lim.B), S)
    r = lim.solve(members=S, **({"max_iter": k} if kind == "max_iter" else {"time_limit": 1e-9}))
    rr = ref.solve(members=S)
    aside = kind == "time_limit"
    _assert_same(_record(r, S, aside), _record(rr, S, aside), "listed")
    _assert_same(_record(r, rest), _record(r0, rest), "unlisted")
    assert lim.columns() == ref.columns() and lim.columns().started == len(S)
    assert np.array_equal(lim.solved_members(), ref.solved_members()) and lim.solved_members()[S].all()
    rep = lim.solve_report()
    if kind == "max_iter":
        assert rep == (k, 0.0, 0.0, 0) and np.all(r.iter[S] <= k)
    else:
        assert np.all(r.iter[S] == INTERVAL) and np.all(np.isin(r.status_val[S], (TIME_LIMIT_REACHED, SOLVED_INACCURATE)))
        assert rep.cut == len(S) and rep.time_limit == 1e-9 and rep.max_iter == kw["max_iter"]
    lim.cleanup(); ref.cleanup()


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tile4", "streamed", "common"])
def test_refusals_leave_the_handle_alone(gpu_lib, name, capfd):
    from osqp_amd import abi
    bs = _setup(name, BUDGET[name])
    r = bs.solve(max_iter=7)
    before, rep = _record(r), bs.solve_report()
    null = C.cast(None, abi.c_int_p)
    f = bs._lib.osqp_amd_batch_solve_limited
    two = np.array([1, 0], np.int64)
    assert f(bs._h, null, 0, -1, 0.0) == 2 and f(bs._h, null, 0, 0, -1.0) == 2       # OSQP_SETTINGS_VALIDATION_ERROR
    assert f(bs._h, null, 0, 3, float("nan")) == 2 and f(bs._h, null, 0, 3, float("inf")) == 2
    assert f(bs._h, abi.iptr(two), 2, -1, 0.0) == 2                                  # ... before the list is looked at
    if name == "common":
        assert f(bs._h, abi.iptr(two), 2, 3, 0.0) == 1                               # OSQP_DATA_VALIDATION_ERROR: not ascending
        assert f(bs._h, abi.iptr(two), 0, 3, 0.0) == 1
    else:
        assert f(bs._h, abi.iptr(two[::-1].copy()), 2, 3, 0.0) == 4                  # OSQP_LINSYS_SOLVER_INIT_ERROR
        assert "osqp_amd_batch_solve_members is a call of the common-K engine" in capfd.readouterr().err
        with pytest.raises(RuntimeError, match="not served by the tiled or the streamed engine"):
            bs.solve(members=[0, 1], max_iter=3)
    for bad in (dict(max_iter=0), dict(max_iter=2.5), dict(time_limit=0.0), dict(time_limit=float("inf"))):
        with pytest.raises(ValueError):
            bs.solve(**bad)
    _assert_same(before, _record(bs.results()), "results after the refusals")
    assert bs.solve_report() == rep == (7, 0.0, 0.0, 0)
    bs.cleanup()
