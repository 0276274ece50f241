"""tests/_common_reference.py on the CPU, with the oracle alone: the long-double batch loop is anchored on the oracle
where the two must agree (B = 1: the member's own scaling, and the "mean" is its own estimate), and the cases of
tests/test_gpu_batch_common_loop.py are shown to hold what they are meant to hold, with every decision of the loop far
enough from its threshold that the engine cannot honestly decide differently."""
import numpy as np
import pytest

from _batch_parity import oracle, rel
from _common_cases import ADAPTIVE_CASES, adaptive_family
from _common_reference import (ANCHOR_BAR, COND_WIDE, LOOP_CASES, MARGIN_ADAPT, MARGIN_CHECK, RHO_BAR, RHO_DIFF_MEASURED,
                               case_reference, margins, reference_for)


def _anchor(orc, n, m, qscale, b, calls, keep_status=False, **kw):
    """The oracle's own adaptive run of member b next to the reference at B = 1, solve by solve: [(ro, rr, oracle's rho)]."""
    P, A, Q, L, U, _ = adaptive_family(n, m, 5, qscale)
    own = oracle(orc, P, Q[b], A, L[b], U[b], **kw)
    ref = reference_for(orc, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1], keep_status=keep_status, **kw)
    out = []
    for _ in range(calls):
        ro, rr = own.solve(), ref.solve()
        out.append((ro, rr, float(own.settings().rho)))
    return out


def _assert_anchor(ro, rr, orho, tag):
    got = (int(rr.status_val[0]), int(rr.iter[0]), int(rr.rho_updates[0]))
    assert got == (ro.info.status_val, ro.info.iter, ro.info.rho_updates), tag + (got,)
    dx, dy = rel(rr.x[0], ro.x), rel(rr.y[0], ro.y)
    dobj = abs(rr.obj_val[0] - ro.info.obj_val) / max(1.0, abs(ro.info.obj_val))
    drho = abs(rr.final_rho - orho) / orho
    print(tag, "x %.1e y %.1e obj %.1e rho %.1e" % (dx, dy, dobj, drho))
    assert dx <= ANCHOR_BAR and dy <= ANCHOR_BAR and dobj <= ANCHOR_BAR, tag + (dx, dy, dobj)
    assert rr.rho[0] == rr.final_rho                     # one member: it finishes with the batch's last rho
    # the rho bar of the GPU tests is derived from this figure: a larger one must be written into _common_reference.py
    assert drho <= RHO_DIFF_MEASURED, tag + (drho,)


@pytest.mark.parametrize("scaled_termination", [0, 1])
@pytest.mark.parametrize("n,m,qscale", ADAPTIVE_CASES)
def test_one_member_is_the_oracles_adaptive_run(oracle_mod, n, m, qscale, scaled_termination):
    kw = dict(adaptive_rho_interval=10, scaled_termination=scaled_termination)
    moved = 0
    for b in range(3):
        (ro, rr, orho), = _anchor(oracle_mod, n, m, qscale, b, 1, **kw)
        _assert_anchor(ro, rr, orho, ("full run", n, scaled_termination, b))
        assert ro.info.status_val == 1
        moved += ro.info.rho_updates
    assert moved >= 3                                    # the anchor is about runs whose rho moves


@pytest.mark.parametrize("scaled_termination", [0, 1])
@pytest.mark.parametrize("n,m,qscale", ADAPTIVE_CASES)
def test_max_iter_order_and_warm_second_solve(oracle_mod, n, m, qscale, scaled_termination):
    """max_iter = 20 and a second solve(): the order of check, adaptation and final tests at max_iter (20 is an adaptation
    point and no check point), rho_updates counting on, and the warm continuation from x, z, y and the moved rho.
    The oracle keeps the status of the first solve where the second passes no exact test (`keep_status` in
    _common_reference.py); the loop as the engine runs it makes the approximate test again -- same iterates, and a
    status that differs exactly where that test passes."""
    kw = dict(adaptive_rho_interval=10, scaled_termination=scaled_termination, max_iter=20)
    at_20 = kept = 0
    for b in range(3):
        runs = _anchor(oracle_mod, n, m, qscale, b, 2, keep_status=True, **kw)
        plain = _anchor(oracle_mod, n, m, qscale, b, 2, **kw)
        for call, ((ro, rr, orho), (_, rp, _)) in enumerate(zip(runs, plain)):
            _assert_anchor(ro, rr, orho, ("max_iter 20, solve %d" % call, n, scaled_termination, b))
            assert ro.info.status_val == -2 and ro.info.iter == 20
            assert np.array_equal(rp.x, rr.x) and np.array_equal(rp.y, rr.y) and np.array_equal(rp.rho_updates, rr.rho_updates)
            assert rp.status_val[0] == -2 if call == 0 else rp.status_val[0] in (-2, 2)
            kept += int(rp.status_val[0] != rr.status_val[0])
        at_20 += 20 in runs[0][1].moves
    assert at_20 >= 1                                    # some member moves rho at max_iter itself
    if scaled_termination:                               # (the scaled residuals are within 10 eps after 40 iterations)
        assert kept >= 1                                 # the kept status is exercised, not only modelled


def test_rho_bar():
    assert RHO_BAR == min(1e-6, 100.0 * RHO_DIFF_MEASURED) and RHO_BAR <= 1e-6


# ---- the GPU cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_decisions_are_far_from_their_thresholds(oracle_mod, name):
    """Every adaptation decision at least 1e-2 from its threshold in log(value / rho), every termination decision at
    least 1e-3 in relative terms: three decades or more above the 1e-6 parity bar."""
    ref, runs = case_reference(oracle_mod, name)
    ma, mc = margins(ref)
    print(name, "adaptation margin %.3g, termination margin %.3g" % (ma, mc), "moves", [r.moves for r in runs],
          "iter", [sorted(set(r.iter.tolist())) for r in runs])
    assert ma >= MARGIN_ADAPT and mc >= MARGIN_CHECK, (name, ma, mc)
    want = {"C20": {-2, 2}, "C40": {-2, 2}}.get(name, {1})
    for r in runs:
        assert set(r.status_val.tolist()) <= want, (name, r.status_val)
    assert any(r.moves for r in runs), name


@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_cases_are_well_conditioned(oracle_mod, name):
    """The third input condition: the same loop in plain double with numpy's unrefined inverse (dtype=np.float64, the
    crudest honest double arithmetic -- the engine refines its solves) decides as the long-double run does and ends
    within the bars the GPU tests set.  A case that misses this cannot tell a wrong engine from rounding: rho estimated
    from one member's nearly converged residuals is a ratio of small differences, and a move made on it late in a run
    carries the noise of double arithmetic into everything after it."""
    _, runs = case_reference(oracle_mod, name)
    _, runs64 = case_reference(oracle_mod, name, np.float64)
    for call, (r, d) in enumerate(zip(runs, runs64)):
        for k in ("status_val", "iter", "rho_updates"):
            assert np.array_equal(getattr(r, k), getattr(d, k)), (name, call, k)
        assert r.moves == d.moves
        drho = (np.abs(d.rho - r.rho) / r.rho).max()
        dx = max(rel(d.x[b], r.x[b]) for b in range(r.x.shape[0])); dy = max(rel(d.y[b], r.y[b]) for b in range(r.x.shape[0]))
        dobj = (np.abs(d.obj_val - r.obj_val) / np.maximum(1.0, np.abs(r.obj_val))).max()
        print(name, "solve", call, "double against long double: rho %.1e x %.1e y %.1e obj %.1e" % (drho, dx, dy, dobj))
        assert drho <= RHO_BAR and dx <= 1e-6 and dy <= 1e-6 and dobj <= 1e-8, (name, call, drho, dx, dy, dobj)


def test_case_a1_freezes_members(oracle_mod):
    ref, (r, r2) = case_reference(oracle_mod, "A1")
    assert r.moves == [10, 20, 130, 160] and sorted(r.iter.tolist()) == [75, 75, 100, 125, 225]
    assert sorted(r.rho_updates.tolist()) == [2, 2, 2, 2, 4]
    assert len(set(r.rho_updates.tolist())) >= 2 and len(set(r.rho.tolist())) >= 2
    moved_with_done = [e for e in ref.decisions if e["kind"] == "adapt" and e["call"] == 1 and e["moved"] and e["done"] > 0]
    assert len(moved_with_done) >= 1
    # after update_rho(0.3) the warm second solve moves rho again and members finish at different checks
    assert r2.moves and len(set(r2.iter.tolist())) >= 2 and np.all(r2.rho_updates > r.rho_updates)
    first = [e for e in ref.decisions if e["kind"] == "adapt" and e["call"] == 2][0]
    assert first["rho"] == 0.3


@pytest.mark.parametrize("name", ["A2-scaled", "A2-default"])
def test_case_a2_staggers_the_finishes(oracle_mod, name):
    _, (r,) = case_reference(oracle_mod, name)
    assert r.x.shape[0] == 65 and len(set(r.iter.tolist())) >= 10, sorted(set(r.iter.tolist()))
    assert r.iter[64] > 0 and len(r.moves) >= 2
    if name == "A2-default":                             # here rho also moves with members frozen
        assert len(set(r.rho_updates.tolist())) >= 2 and len(set(r.rho.tolist())) >= 2


def test_case_c_moves_rho_at_max_iter(oracle_mod):
    ref, (r, r2) = case_reference(oracle_mod, "C20")
    assert r.moves[-1] == 20 and np.all(r.status_val == -2) and np.all(r.iter == 20)
    at_20 = [e for e in ref.decisions if e["kind"] == "adapt" and e["call"] == 1 and e["iter"] == 20][0]
    assert at_20["moved"] and np.all(r.rho == at_20["value"])          # the rho after the last adaptation, not before
    assert np.all(r.rho_updates == len(r.moves))
    # 20 + 20 warm-started iterations are the 40 of one run: no check point passes in between, and the rebuild that ends
    # the first solve is the rebuild an uninterrupted run makes at iteration 20
    _, (r40,) = case_reference(oracle_mod, "C40")
    assert np.all(r2.iter == 20) and np.all(r40.iter == 40)
    assert r40.moves == r.moves + [20 + k for k in r2.moves]
    for k in ("status_val", "rho_updates", "rho"):
        assert np.array_equal(getattr(r2, k), getattr(r40, k)), k
    assert rel(r2.x, r40.x) <= 1e-15 and rel(r2.y, r40.y) <= 1e-15


def test_case_d_has_no_equality_rows_and_a_tame_k(oracle_mod):
    ref, (r,) = case_reference(oracle_mod, "D-wide")
    assert not np.any(ref.ctype == 1) and np.any(ref.ctype == 0) and np.any(ref.ctype == -1)
    assert len(ref.conds) == 1 + len(r.moves) and max(ref.conds) <= COND_WIDE, ref.conds
    ref1, _ = case_reference(oracle_mod, "A1")
    assert np.any(ref1.ctype == 1) and max(ref1.conds) > COND_WIDE     # what the widening removes
