"""The cases of tests/_common_cases.py on the CPU, with the oracle alone: what the GPU tests of the common-K engine
take for granted about their inputs and their yardstick."""
import numpy as np
import pytest

from _batch_parity import oracle, oracle_ws, rel
from _common_cases import (ADAPTIVE, ADAPTIVE_CASES, CASES, CASES_UNSCALED, FIXED, MIXED, UNSCALED_MAX_ITER, adaptive_family,
                           common_family, common_oracle, mixed_family, prescaled_oracle, qhat, row_classes, unscale)

B = 5


def _case(n, m):
    return common_family(n, m, B, 1000 + n + m)


@pytest.mark.parametrize("n,m", CASES)
def test_classes_agree_and_members_solve(oracle_mod, n, m):
    """One class per row over the batch on the commonly scaled bounds, and every member ends `solved` under the
    common scaling with the fixed rho, well inside max_iter."""
    P, A, Q, L, U, _ = _case(n, m)
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **FIXED))
    cls = [row_classes(L[b], U[b], ws["E"]) for b in range(B)]
    for b in range(B):
        assert np.array_equal(cls[b], cls[0]), (n, m, b)
    assert np.array_equal(cls[0], ws["ctype"])
    if m > 3:
        assert len(set(cls[0])) == 3, "the case should hold loose, inequality and equality rows"
    for b in range(B):
        ro = prescaled_oracle(oracle_mod, ws, Q, L, U, b, **FIXED).solve()
        assert ro.info.status_val == 1 and ro.info.iter <= 400, (n, m, b, ro.info.status_val, ro.info.iter)


@pytest.mark.parametrize("n,m", CASES_UNSCALED)
def test_unscaled_cases(oracle_mod, n, m):
    """scaling = 0: every member solves within the default max_iter, and UNSCALED_MAX_ITER stops some members of the
    largest case and not others (the members that end at max_iter in the GPU test)."""
    P, A, Q, L, U, _ = _case(n, m)
    kw = dict(FIXED, scaling=0)
    its = []
    for b in range(B):
        ro = oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw).solve()
        assert ro.info.status_val == 1, (n, m, b, ro.info.status_val)
        its.append(ro.info.iter)
    if (n, m) == CASES_UNSCALED[-1]:
        assert min(its) <= UNSCALED_MAX_ITER < max(its), its


@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("n,m", [(33, 66), (129, 258)])
def test_prescaled_run_is_the_scaled_run(oracle_mod, n, m, adaptive):
    """The yardstick: the reference with its own scaling and scaled_termination = 1 equals the reference with
    scaling = 0 on the data scaled by hand -- iterations and rho updates equal, obj = obj~ / c, x and y to 1e-10.
    The two runs differ in the rounding of the scaling products: a relative eps = 1.1e-16 per entry of the data, which
    the iterates see through K (condition up to ~1e5 here: equality rows weigh 1e3 rho) -- 1e-11, and a decade for
    the hundreds of iterations.  That is four decades below the 1e-6 the GPU tests ask of the engine against this
    yardstick.  (A one-member batch: q^ = |q| gives the member's own scaling, Ruiz sees norms only.)"""
    P, A, Q, L, U, _ = adaptive_family(n, m, B, 100.0) if adaptive else _case(n, m)   # (rho moves / fixed rho converges)
    kw = dict(scaled_termination=1, adaptive_rho=adaptive, adaptive_rho_interval=10)
    for b in range(2):
        ws = oracle_ws(common_oracle(oracle_mod, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1], **kw))
        own = oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw)
        wo = oracle_ws(own)
        assert np.array_equal(wo["D"], ws["D"]) and np.array_equal(wo["E"], ws["E"]) and wo["c"] == ws["c"]
        r1 = own.solve()
        r2 = prescaled_oracle(oracle_mod, ws, Q, L, U, b, **kw).solve()
        assert (r1.info.status_val, r1.info.iter, r1.info.rho_updates) == (r2.info.status_val, r2.info.iter, r2.info.rho_updates)
        assert r1.info.status_val == 1 and (r1.info.rho_updates > 0) == bool(adaptive)
        x, y, obj = unscale(ws, r2)
        assert rel(x, r1.x) < 1e-10 and rel(y, r1.y) < 1e-10, (rel(x, r1.x), rel(y, r1.y))
        assert abs(obj - r1.info.obj_val) <= 1e-10 * max(1.0, abs(r1.info.obj_val))


@pytest.mark.parametrize("n,m,qscale", ADAPTIVE_CASES)
def test_adaptive_cases_move_rho(oracle_mod, n, m, qscale):
    """The adaptive GPU cases: with the default settings and adaptive_rho_interval = 10 every member's own reference
    run solves and moves rho at least once -- so does a batch of copies of a member -- and the classes agree."""
    P, A, Q, L, U, _ = adaptive_family(n, m, B, qscale)
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **ADAPTIVE))
    for b in range(B):
        assert np.array_equal(row_classes(L[b], U[b], ws["E"]), ws["ctype"])
        ro = oracle(oracle_mod, P, Q[b], A, L[b], U[b], **ADAPTIVE).solve()
        assert ro.info.status_val == 1 and ro.info.rho_updates > 0, (n, m, b, ro.info.rho_updates)


def test_mixed_statuses_case(oracle_mod):
    """The mixed batch: classes agree, the planted members end primal / dual infeasible and the others solved in the
    yardstick run, and the batch without the two has the same q^ (so the same scaling)."""
    P, A, Q, L, U = mixed_family()
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **FIXED))
    keep = [b for b in range(MIXED["B"]) if b not in (MIXED["pinf"], MIXED["dinf"])]
    assert np.array_equal(qhat(Q), qhat(Q[keep])) and keep[0] == 0
    for b in range(MIXED["B"]):
        assert np.array_equal(row_classes(L[b], U[b], ws["E"]), ws["ctype"]), b
        st = prescaled_oracle(oracle_mod, ws, Q, L, U, b, **FIXED).solve().info.status_val
        assert st == (-3 if b == MIXED["pinf"] else -4 if b == MIXED["dinf"] else 1), (b, st)
