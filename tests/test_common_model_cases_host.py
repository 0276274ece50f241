"""tests/_common_model_cases.py on the CPU, with the oracle alone: ModelReference's update_model is anchored on the
oracle's own osqp_update_P_A at B = 1, the cases of tests/test_gpu_batch_common_model.py are shown to decide far from
their thresholds and to keep their row classes under the new scaling, and five one-place mistakes of the call are shown
to miss the GPU bars by more than ten times.  Also the host-side contract of the two new entry points."""
import ctypes as C

import numpy as np
import pytest

from _batch_parity import oracle, oracle_ws, rel
from _common_cases import ADAPTIVE, CASES, common_family, common_oracle
from _common_model_cases import (BITS, DEFECT_CASE, DEFECTS, MODEL_CASES, ModelReference, bits_case, certificates_fire, classes_under,
                                 model_case, model_reference, moved_model, qhat_test_q, split_solve_fires)
from _common_reference import ANCHOR_BAR, MARGIN_ADAPT, MARGIN_CHECK, RHO_BAR, RHO_DIFF_MEASURED, margins


# ---- the anchor ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled_termination", [0, 1])
@pytest.mark.parametrize("name", ["M33", "M129"])
def test_one_member_follows_the_oracles_matrix_update(oracle_mod, name, scaled_termination):
    """B = 1, every member of the case's family on its own: setup -> solve (max_iter = 20) -> update(Px, Ax) -> solve on
    the oracle, next to the reference with update_model in place of the update; the new scaled space is that of a fresh
    oracle set-up on the new values."""
    n, m, qscale, B, seed = MODEL_CASES[name][:5]
    P, A, Q, L, U, _ = common_family(n, m, B, seed)
    Q = Q * qscale
    Pu, A, P2, A2, Px, Ax = moved_model(P, A, seed + 1)
    kw = dict(adaptive_rho_interval=10, scaled_termination=scaled_termination, max_iter=20)
    moved = compared = 0
    for b in range(B):
        own = oracle(oracle_mod, Pu, Q[b], A, L[b], U[b], **kw)
        one = (Q[b:b + 1], L[b:b + 1], U[b:b + 1])
        spaces = [oracle_ws(common_oracle(oracle_mod, Pb, Ab, *one, **kw)) for Pb, Ab in ((Pu, A), (P2, A2))]
        ref, split = ModelReference(spaces[0], *one, **kw), ModelReference(spaces[0], *one, **kw)
        ro, rr = own.solve(), ref.solve()
        moved += ro.info.rho_updates
        assert (ro.info.status_val, ro.info.iter) == (-2, 20) and rr.status_val[0] == -2
        assert not split_solve_fires(split, (1.0,)) or not scaled_termination
        assert own.update(Px=Px, Ax=Ax) == 0
        for r in (ref, split):
            r._set_rho(ref.rho)
            r.update_model(spaces[1], *one)
        ro, rr = own.solve(), ref.solve()
        tag = ("after the update", n, scaled_termination, b)
        # The reference models no infeasibility certificate.  Twenty iterations after new matrix values the approximate
        # tests of max_iter can fire on a feasible member: the oracle then reports 3 or 4, and with scaled_termination = 1,
        # which _common_model_cases.split_solve_fires restates, that diagnostic must say so too -- it is what keeps the
        # GPU cases clear of such members (test_no_certificate_fires_in_the_cases).
        fired = ro.info.status_val in (3, 4)
        if scaled_termination:
            assert split_solve_fires(split, (1.0,)) == fired, tag
        if fired:
            print(tag, "the oracle ends with an approximate certificate (%d): not compared" % ro.info.status_val)
            continue
        compared += 1
        got = (int(rr.status_val[0]), int(rr.iter[0]), int(rr.rho_updates[0]))
        assert got == (ro.info.status_val, ro.info.iter, ro.info.rho_updates), tag + (got,)
        dx, dy = rel(rr.x[0], ro.x), rel(rr.y[0], ro.y)
        dobj = abs(rr.obj_val[0] - ro.info.obj_val) / max(1.0, abs(ro.info.obj_val))
        orho = float(own.settings().rho)
        drho = abs(rr.final_rho - orho) / orho
        print(tag, "x %.1e y %.1e obj %.1e rho %.1e" % (dx, dy, dobj, drho))
        assert dx <= ANCHOR_BAR and dy <= ANCHOR_BAR and dobj <= ANCHOR_BAR, tag + (dx, dy, dobj)
        assert drho <= RHO_DIFF_MEASURED, tag + (drho,)
    assert moved >= 3 and compared >= 3                  # rho has moved before the update: "rho stays" is exercised


# ---- the GPU cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_decisions_are_far_from_their_thresholds(oracle_mod, name):
    c, ref, (r1, r2), rho = model_reference(oracle_mod, name)
    ma, mc = margins(ref)
    print(name, "adaptation margin %.3g, termination margin %.3g" % (ma, mc), "moves", r1.moves, r2.moves)
    assert ma >= MARGIN_ADAPT and mc >= MARGIN_CHECK, (name, ma, mc)
    assert r1.moves and np.all(r1.rho_updates == len(r1.moves))         # rho has moved before the call ...
    assert rho != c["ws_old"]["rho"] and np.all(r1.iter == 20) and set(r1.status_val.tolist()) <= {-2, 2}
    assert np.all(r2.rho_updates == len(r2.moves))                      # ... and the count restarts at it
    assert np.abs(c["ws_new"]["D"] / c["ws_old"]["D"] - 1).max() > 0.1 and np.abs(c["ws_new"]["E"] / c["ws_old"]["E"] - 1).max() > 0.1


@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_no_certificate_fires_in_the_cases(oracle_mod, name):
    """Neither solve of a case ends on an approximate infeasibility certificate, which the reference does not model: on the
    step of iteration 20 neither test fires for any member at half, once or twice the approximate eps."""
    assert certificates_fire(oracle_mod, name) == [False, False], name


@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_classes_under_the_old_and_the_new_scaling(oracle_mod, name):
    """A fresh handle on the new values is a bit-yardstick for the updated one only where no member's row changes its class
    under the new E; the crossing case is built so that exactly one row does, in every member."""
    c = model_case(oracle_mod, name)
    old, new = classes_under(c["ws_old"], c["L"], c["U"]), classes_under(c["ws_new"], c["L"], c["U"])
    assert np.all(old == old[0]) and np.all(new == new[0]) and np.array_equal(old[0], c["ws_old"]["ctype"])
    if c["row"] is None:
        assert np.array_equal(old, new)
    else:
        differ = np.flatnonzero(old[0] != new[0])
        assert differ.tolist() == [c["row"]] and old[0][c["row"]] == 1 and new[0][c["row"]] == 0


@pytest.mark.parametrize("shape,mode", [b[:2] for b in BITS], ids=str)
def test_bit_yardstick_cases(oracle_mod, shape, mode):
    """The cases of the fresh-handle comparison: no member's row changes its class between the scaling of the model the
    handle is set up on and that of the moved model (also with the larger Q of test_qhat_follows_update), every shape of
    _common_cases.CASES is among them, and under the moved model every member ends solved -- in the reference's batch
    loop, so polish, adjoint and tangent have every member to work on."""
    c = bits_case(shape, mode)
    Q, L, U = c["Q"], c["L"], c["U"]
    for Qx in (Q, qhat_test_q(Q)):
        w0 = oracle_ws(common_oracle(oracle_mod, c["P0"], c["A0"], Q, L, U, **ADAPTIVE))
        w1 = oracle_ws(common_oracle(oracle_mod, c["P2"], c["A2"], Qx, L, U, **ADAPTIVE))
        assert np.array_equal(classes_under(w0, L, U), classes_under(w1, L, U)), (shape, mode)
        assert shape[0] == 1 or np.abs(w1["D"] / w0["D"] - 1).max() > 0.05
    assert {b[0][:2] for b in BITS} == set(CASES)
    r = ModelReference(oracle_ws(common_oracle(oracle_mod, c["P2"], c["A2"], Q, L, U, **ADAPTIVE)), Q, L, U, **ADAPTIVE).solve()
    assert np.all(r.status_val == 1), (shape, mode, r.status_val)


@pytest.mark.parametrize("defect", DEFECTS)
def test_defects_miss_the_gpu_bars(oracle_mod, defect):
    """Each one-place mistake, planted in the reference, against the reference itself on its named case: an integer of
    the second solve differs, or x / y, the objective or rho is off by more than ten times the GPU bar."""
    name = DEFECT_CASE[defect]
    _, _, (_, good), _ = model_reference(oracle_mod, name)
    _, _, (_, bad), _ = model_reference(oracle_mod, name, defect)
    B = good.x.shape[0]
    ints = all(np.array_equal(getattr(good, k), getattr(bad, k)) for k in ("status_val", "iter", "rho_updates"))
    dx = max(rel(bad.x[b], good.x[b]) for b in range(B)); dy = max(rel(bad.y[b], good.y[b]) for b in range(B))
    dobj = (np.abs(bad.obj_val - good.obj_val) / np.maximum(1.0, np.abs(good.obj_val))).max()
    drho = (np.abs(bad.rho - good.rho) / good.rho).max()
    print(defect, name, "integers equal", ints, "x %.1e y %.1e obj %.1e rho %.1e" % (dx, dy, dobj, drho))
    assert not ints or max(dx, dy) > 10 * 1e-6 or dobj > 10 * 1e-8 or drho > 10 * RHO_BAR, (defect, name)


# ---- the entry points --------------------------------------------------------------------------------------------------
def _lib():
    import osqp_amd
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    return lib


def test_symbols_exported_and_bound():
    lib = _lib()
    assert len(lib.osqp_amd_batch_common_update_model.argtypes) == 7
    assert len(lib.osqp_amd_batch_common_update_model_dev.argtypes) == 7


def test_null_handle():
    from osqp_amd import abi
    lib = _lib()
    no_f, no_i = C.cast(None, abi.c_float_p), C.cast(None, abi.c_int_p)
    v = np.ones(3)
    assert lib.osqp_amd_batch_common_update_model(None, no_f, no_i, 0, no_f, no_i, 0) == 7        # OSQP_WORKSPACE_NOT_INIT_ERROR
    assert lib.osqp_amd_batch_common_update_model(None, abi.fptr(v), no_i, 3, no_f, no_i, 0) == 7
    assert lib.osqp_amd_batch_common_update_model_dev(None, None, no_i, 0, None, no_i, 0) == 7


def test_update_model_belongs_to_the_common_engine():
    import osqp_amd
    bs = osqp_amd.BatchOSQP()
    for engine in ("streamed", "auto"):
        bs.engine = engine
        with pytest.raises(RuntimeError, match="update_matrices"):
            bs.update_model(Px=np.ones(3))
    bs.engine, bs._shared_kkt = "common", True
    with pytest.raises(RuntimeError, match="update_model"):
        bs._unserved("update_matrices", never=True)
