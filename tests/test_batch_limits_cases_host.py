"""What tests/test_gpu_batch_limits.py takes for granted about its cases (tests/_limits_cases.py), proved on the CPU
oracle.

The tests of a clock that has already expired assert that every member ends at the first clock iteration, INTERVAL.
That is fair only if no member passes the exact termination test before: the oracle, checking in EVERY iteration of
the first INTERVAL (check_termination = 1, max_iter = INTERVAL) on the case's data, eps and cold start, must end no
member before the cap -- neither solved nor with a certificate.  rho is adapted at the same iterations in both runs
(adaptive_rho_interval is set explicitly), so the iterates are those of the check_termination = 0 run on the GPU."""
import pytest

from _limits_cases import BETWEEN, EXPIRED, INTERVAL, SHAPES, member_oracles


@pytest.mark.parametrize("name", list(SHAPES))
def test_no_member_ends_within_the_first_clock_interval(oracle_mod, name):
    kw = dict(EXPIRED[name], check_termination=1, max_iter=INTERVAL)
    moved = 0
    for b, (so, _) in member_oracles(oracle_mod, name, kw).items():
        ro = so.solve()
        print(name, b, ro.info.status_val, ro.info.iter, ro.info.rho_updates)
        assert ro.info.iter == INTERVAL and ro.info.status_val in (-2, 2), (name, b, ro.info.status_val, ro.info.iter)
        moved += ro.info.rho_updates > 0
    if name == "streamed":         # a member's rho moves in iteration INTERVAL: the clock stops it with a rebuild due
        assert moved > 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_in_between_cases_run_many_clock_intervals(oracle_mod, name):
    """The in-between test halves the time of a full solve: some member has to run for many check intervals for that to
    stop anybody (the test itself holds however the timing falls)."""
    kw = BETWEEN[name]
    its = [so.solve().info.iter for so, _ in list(member_oracles(oracle_mod, name, kw, members=range(5)).values())]
    print(name, its)
    assert max(its) >= 20 * kw["check_termination"]
