"""Polish and the solution derivatives (OSQP.solve with polish = 1, OSQP.adjoint, OSQP.tangent) on every linear-solve form the
KKT instance can take.  The instance is a second engine on (P~, A~[active rows]) with rho = 1 / d on every row and sigma = d,
d = max(delta, 1e-3) (kkt_instance in osqp_host.c); it chooses its form from (P, A_red) on its own, and every call goes through
hipeng_kkt_solve, kkt_refined_solve and three hipeng_spmv products on it.

Cases: tests/_kkt_instance_cases.py -- planted solutions and active sets on the structured problems of the per-form linear-solve
tests, chosen so that the instance sits on the form (and, where noted, differs from the main engine); tests/
test_kkt_instance_cases_host.py proves on the CPU that each case is what it claims, that the route itself is within 1e-10 of the
truth, and that no case on a PCG form is harder for CG than the members tests/test_gpu_single_sens.py already runs.

Every test asserts the instance's form before it compares a number: osqp_amd_polish_info for the instance polish built and freed,
hipeng_resident_info / hipeng_pcg_layout / hipeng_elim_count on osqp_amd_sens_engine for the live one, after the adjoint call (which
builds it) and again after the tangent call -- the form still in use, no launch that gave up, no negative-curvature stop -- so a
silent fallback to the launch-per-step kernels fails the test.  Reference: the truth of the case (a refined solve of the
unregularised KKT system on the planted rows), never the device's own numbers.  Bar: the project's parity bar, 1e-6 by
_batch_parity.rel, for x, y, obj, dq, dl, du, dPx, dAx, dx, dy.  Every error, kkt_res, the solve count and the instance's PCG
iterations are printed.

The last two tests run the benchmark's own families small (a portfolio QP on the block-direct instance, a Lasso on the
dense-direct one with its eliminated variables) against tests/_adjoint_reference.py / _tangent_reference.py at the CPU oracle's
polished point, with the reference's guards asserted.  (The third family of that kind, portfolio_qp(4, 64, sector_rows=20), has
no test: at that size every seed from 1 to 300 leaves at least one sector row on its lower bound with all its variables at zero
-- margin 0 and dependent active rows -- so the reference cannot pass its own guards and there is no unique derivative to compare.)

Measured on an MI355X (test_instance_form_and_truth; form, info [2] / [3] / [15], eliminated, active rows; worst of the ten
errors; linear solves of the two calls; the live instance's PCG iterations in total / at most per solve; the test's time):
    ki_f0_blocks     0  0/0/0    elim 0   mred 114   8.7e-14  27 solves  9423 / 175  1.3 s
    ki_f0_long_on    0  0/0/0    elim 0   mred 13    1.0e-15  15 solves  4842 / 183  1.0 s   (layout long 1)
    ki_f0_long_off   0  0/0/0    elim 0   mred 13    7.9e-16  15 solves  2283 / 81   0.9 s   (layout long 0)
    ki_f1_e8         1  8/7/0    elim 0   mred 70    2.1e-13  21 solves  5479 / 146  1.3 s
    ki_f1_e20        1  20/10/0  elim 0   mred 100   5.3e-14  21 solves  7484 / 188  0.8 s
    ki_f2_nh0        2  64/248/0 elim 0   mred 21    3.8e-14  21 solves   370 / 8    0.7 s
    ki_f3_plain      3  0/5/0    elim 0   mred 128   6.4e-15  21 solves    42 / 1    0.7 s
    ki_f3_kc16       3  0/5/16   elim 0   mred 119   3.2e-15  21 solves    42 / 1    0.7 s
    ki_f3_kc17       3  0/5/17   elim 0   mred 119   1.9e-13  20 solves    40 / 1    1.1 s
    ki_f3_kc0        3  0/5/0    elim 0   mred 128   5.4e-15  21 solves    42 / 1    0.7 s
    ki_f3_huge1      3  0/64/0   elim 0   mred 2731  6.8e-13  24 solves    48 / 1    1.5 s   (layout huge 1, folded 1)
    ki_f0_huge1      0  0/0/0    elim 0   mred 2731  1.8e-12  22 solves  1240 / 41   1.5 s   (layout huge 1, folded 1)
    ki_f4_b2         4  0/100/3  elim 1   mred 14    1.9e-13  24 solves    48 / 1    0.6 s
    ki_f4_slack      4  0/100/0  elim 10  mred 18    6.5e-13  30 solves    60 / 1    0.7 s
    ki_mred0         0  0/0/0    elim 0   mred 0     1.9e-14  24 solves   335 / 5    0.7 s
    ki_all_eq        4  0/100/0  elim 0   mred 22    1.4e-13  21 solves    42 / 1    0.6 s
Duality |lhs - rhs| <= 4.8e-11 under bars >= 2.0e-4; the two families <= 2.0e-14.

What the file found: form_Ared wrote each column of A_red in A's row order, lows and upps interleaved, so a column with an upper-
bound row ahead of a lower-bound row was not sorted by reduced row index; build_resident refuses such a matrix, and the instance
of ki_f1_e8 went to the launch-per-step kernels without a word (polish_info form 0 where 1 was claimed; the run stopped there, and
ki_f1_e20 is built the same way).  form_Ared now writes a column's lows, then its upps; without that change
test_instance_form_and_truth[ki_f1_e8] fails."""
import ctypes as C
import time

import numpy as np
import pytest
from scipy import sparse

import _kkt_instance_cases as KI
import _planted_qp as pq
import _single_sens_reference as sr
from _adjoint_reference import adjoint_reference
from _batch_parity import oracle, rel
from _tangent_reference import tangent_reference
from tests import _elim_cases as EC
from tests import _form_cases as FC
from tests import _hipeng as HE

pytestmark = pytest.mark.gpu

GRADS, TANS = pq.ADJOINT, pq.TANGENT
LAYOUT = dict(dense=0, dense_rows=1, long=3, huge=4, folded=5)          # slots of hipeng_pcg_layout
BAR = 1e-6


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _engine_view(eng):
    """dict(info, layout, elim, stats) of a raw engine handle."""
    L = HE._lib()
    assert eng
    info, lay, st = (C.c_longlong * 16)(), (C.c_longlong * 16)(), HE.HipengStats()
    assert L.hipeng_resident_info(eng, info) == 0 and L.hipeng_pcg_layout(eng, lay) == 0 and L.hipeng_get_stats(eng, C.byref(st)) == 0
    return dict(info=list(info), layout=list(lay), elim=int(L.hipeng_elim_count(eng)), stats={k: int(getattr(st, k)) for k, _ in HE.HipengStats._fields_})


def _assert_instance(what, v, claims):
    """The live instance is what the case claims, its form is in use and served every solve."""
    info = v["info"]
    assert info[9] == claims["form"], (what, "form", info[9], "claimed", claims["form"], info)
    for slot, want in claims["info"].items():
        assert info[slot] == want, (what, "info[%d]" % slot, info[slot], want, info)
    for key, want in claims["layout"].items():
        assert v["layout"][LAYOUT[key]] == want, (what, key, v["layout"], want)
    assert v["elim"] == claims["elim"], (what, "eliminated", v["elim"], claims["elim"])
    if claims["form"] != 0:
        assert info[1] == 1, (what, "the form is no longer in use", info)
    assert info[10] == 0 and info[14] == 0, (what, "a resident launch gave up", info)
    assert v["stats"]["neg_curvature"] == 0 and v["stats"]["pcg_forced"] == 0, (what, v["stats"])


def _run(c, monkeypatch, **kw):
    """setup with polish = 1 under the case's environment, solve, adjoint with the matrices, tangent with all five tangents:
    (handle, result, adjoint, tangent, dict of what was read on the way)."""
    import osqp_amd
    _setenv(monkeypatch, c.env)
    i = pq.member_inc(c, 0)
    t0 = time.perf_counter()
    h = osqp_amd.OSQP().setup(**sr.member_qp(c, 0), **{"polish": 1, **c.settings, **kw})
    main0 = _engine_view(h.engine())["info"][9]
    r = h.solve()
    pol = h.polish_info()
    assert h.sens_engine() is None and h.sens_info()["alive"] == 0          # polish's instance is gone, none built yet
    a = h.adjoint(i.gx, i.gy, matrices=True)
    v1 = _engine_view(h.sens_engine())
    t = h.tangent(i.dQ, i.dL, i.dU, i.dPx, i.dAx)
    v2 = _engine_view(h.sens_engine())
    wall = time.perf_counter() - t0
    return h, r, a, t, dict(pol=pol, after_adjoint=v1, after_tangent=v2, main_before=main0, main_after=_engine_view(h.engine())["info"][9],
                            sens=h.sens_info(), wall=wall)


def _check(what, c, r, a, t, seen):
    """Forms first, then the numbers against the truth."""
    cl, tr = c.claims, KI.truth(c.name)
    mred = int(np.count_nonzero(c.act[0]))
    assert r.info.status_val == 1 and r.info.status_polish == 1, (what, r.info.status_val, r.info.status_polish)
    assert a.status_adjoint == 1 and t.status_tangent == 1, (what, a.status_adjoint, t.status_tangent)
    assert np.array_equal(a.active, c.act[0]) and np.array_equal(t.active, c.act[0]), (what, np.flatnonzero(a.active != c.act[0]))
    assert seen["pol"] == dict(runs=1, form=cl["form"], active_rows=mred, troubles=0), (what, seen["pol"], cl)
    _assert_instance(what + " after adjoint", seen["after_adjoint"], cl)
    _assert_instance(what + " after tangent", seen["after_tangent"], cl)
    assert seen["sens"]["built"] == 1 and seen["sens"]["alive"] == 1 and seen["sens"]["active_rows"] == mred, (what, seen["sens"])
    assert seen["main_before"] == seen["main_after"] == c.main["form"], (what, seen["main_before"], seen["main_after"], c.main)
    errs = dict(x=rel(r.x, tr.x), y=rel(r.y, tr.y), obj=rel([r.info.obj_val], tr.obj))
    errs.update({g: rel(getattr(a, g), getattr(tr, g)) for g in GRADS})
    errs.update({g: rel(getattr(t, g), getattr(tr, g)) for g in TANS})
    v = seen["after_tangent"]
    print("%s: form %d info[2] %d [3] %d [15] %d layout %s elim %d | %s | worst %.2e | kkt_res adjoint %.1e tangent %s | mred %d solves %d, "
          "instance PCG iterations total %d max %d | %.2f s"
          % (what, v["info"][9], v["info"][2], v["info"][3], v["info"][15], v["layout"][:6], v["elim"], " ".join("%s %.2e" % kv for kv in errs.items()),
             max(errs.values()), a.kkt_res, " ".join("%.1e" % k for k in t.kkt_res), mred, seen["sens"]["solves"], v["stats"]["pcg_iters_total"],
             v["stats"]["pcg_iters_max"], seen["wall"]))
    assert all(e < BAR for e in errs.values()), (what, errs)
    return errs


@pytest.mark.parametrize("name", KI.NAMES)
def test_instance_form_and_truth(gpu_lib, monkeypatch, name):
    """Every case: statuses, the planted active set, the claimed form and slots of polish's instance and of the live one, the main
    engine's form unchanged, and all ten outputs within 1e-6 of the truth."""
    c = KI.make(name)
    h, r, a, t, seen = _run(c, monkeypatch)
    try:
        _check(name, c, r, a, t, seen)
        if name == "ki_mred0":                   # an instance with m = 0: nothing flows to the rows
            assert seen["sens"]["active_rows"] == 0 and not a.dl.any() and not a.du.any() and not a.dAx.any() and not t.dy.any()
        if name == "ki_f4_slack":
            assert seen["after_tangent"]["elim"] == 10
    finally:
        h.cleanup()


@pytest.mark.parametrize("name", ["ki_f1_e20", "ki_f3_kc17", "ki_f4_slack"])
def test_duality_on_the_device(gpu_lib, monkeypatch, name):
    """gx . dx + gy . dy = dq_adj . dq + dl_adj . dl + du_adj . du + dPx_adj . dPx + dAx_adj . dAx, both sides from one handle: the
    identity and the bar of test_gpu_single_sens.test_duality_on_the_device (each side's terms are held to 1e-6, so the sides agree
    within 2e-6 times the smaller sum of absolute terms)."""
    c = KI.make(name)
    i = pq.member_inc(c, 0)
    h, r, a, t, seen = _run(c, monkeypatch)
    h.cleanup()
    assert a.status_adjoint == 1 and t.status_tangent == 1
    _assert_instance(name, seen["after_tangent"], c.claims)
    for k in range(pq.NDIR):
        left = [i.gx * t.dx[k], i.gy * t.dy[k]]
        right = [a.dq * i.dQ[k], a.dl * i.dL[k], a.du * i.dU[k], a.dPx * i.dPx[k], a.dAx * i.dAx[k]]
        lhs, rhs = sum(float(v.sum()) for v in left), sum(float(v.sum()) for v in right)
        bar = 2e-6 * min(sum(float(np.abs(v).sum()) for v in left), sum(float(np.abs(v).sum()) for v in right))
        print("duality %s direction %d: lhs %.12e rhs %.12e |lhs - rhs| %.2e (bar %.1e)" % (name, k, lhs, rhs, abs(lhs - rhs), bar))
        assert abs(lhs - rhs) <= bar


def _info_no_times(r):
    return {k: v for k, v in vars(r.info).items() if not k.endswith("_time")}


@pytest.mark.parametrize("name", ["ki_f3_kc17", "ki_f1_e8"])
def test_main_engine_untouched(gpu_lib, monkeypatch, name):
    """The main engine keeps its form through the derivative calls, and a second solve returns the bits of a twin handle that
    made no derivative call (as test_gpu_single_sens.test_untouched)."""
    import osqp_amd
    c = KI.make(name)
    h, r, a, t, seen = _run(c, monkeypatch)
    twin = osqp_amd.OSQP().setup(**sr.member_qp(c, 0), **{"polish": 1, **c.settings})
    rt = twin.solve()
    try:
        _assert_instance(name, seen["after_tangent"], c.claims)
        assert seen["main_before"] == seen["main_after"] == c.main["form"] == _engine_view(twin.engine())["info"][9]
        assert np.array_equal(r.x, rt.x) and np.array_equal(r.y, rt.y) and _info_no_times(r) == _info_no_times(rt)
        assert twin.sens_info() == dict(built=0, alive=0, active_rows=0, solves=0) and twin.sens_engine() is None
        r2, rt2 = h.solve(), twin.solve()
        assert np.array_equal(r2.x, rt2.x) and np.array_equal(r2.y, rt2.y) and _info_no_times(r2) == _info_no_times(rt2)
        assert h.stats() == twin.stats()
        assert h.sens_engine() is None and h.polish_info()["runs"] == 2          # the solve dropped the instance; polish ran again
    finally:
        h.cleanup(); twin.cleanup()


@pytest.mark.parametrize("scaling", [0, 10])
@pytest.mark.parametrize("name", ["ki_f3_kc16", "ki_f4_slack"])
def test_scaling_folded(gpu_lib, monkeypatch, name, scaling):
    """Without scaling and with ten Ruiz passes, against the same truth: the D, E, c folding on a direct-form instance."""
    c = KI.make(name)
    h, r, a, t, seen = _run(c, monkeypatch, scaling=scaling)
    try:
        assert bool(h.work.scaling) == (scaling != 0)
        _check("%s scaling=%d" % (name, scaling), c, r, a, t, seen)
    finally:
        h.cleanup()


# ------------------------------------------------------------------------------------------------ the benchmark's families, small
def _family(monkeypatch, oracle_mod, what, pb, env, want_form):
    """One QP of a benchmark family under `env` against the CPU oracle's polished point and the references there: the same
    status, status_polish and iteration count, x and y within 1e-6, every derivative within 1e-6 (rel); the reference's guards
    asserted first (margin >= 1e-6, sv_ratio >= 1e-8, route_err <= 1e-7).  Returns (instance view, active rows of the reference)."""
    import osqp_amd
    _setenv(monkeypatch, env)
    P, A = sparse.triu(pb["P"], format="csc"), sparse.csc_matrix(pb["A"])
    n, m = A.shape[1], A.shape[0]
    rng = np.random.default_rng(99)
    d = pq.SimpleNamespace(gx=rng.standard_normal(n), gy=rng.standard_normal(m), dq=rng.standard_normal((2, n)), dl=rng.standard_normal((2, m)),
                           du=rng.standard_normal((2, m)), dPx=rng.standard_normal((2, P.nnz)), dAx=rng.standard_normal((2, A.nnz)))
    ro = oracle(oracle_mod, polish=1, **pb).solve()
    ref = adjoint_reference(pb["P"], pb["A"], pb["l"], pb["u"], ro.x, ro.y, d.gx, d.gy)
    rts = [tangent_reference(pb["P"], pb["A"], ro.x, ro.y, d.dq[k], d.dl[k], d.du[k], d.dPx[k], d.dAx[k]) for k in range(2)]
    assert ro.info.status_val == 1 and ro.info.status_polish == 1
    assert ref.margin >= 1e-6 and ref.sv_ratio >= 1e-8 and ref.route_err <= 1e-7 and all(rt.route_err <= 1e-7 for rt in rts), (ref.margin, ref.sv_ratio, ref.route_err)
    h = osqp_amd.OSQP().setup(**pb, polish=1)
    r = h.solve()
    pol = h.polish_info()
    a = h.adjoint(d.gx, d.gy, matrices=True)
    t = h.tangent(d.dq, d.dl, d.du, d.dPx, d.dAx)
    v = _engine_view(h.sens_engine())
    h.cleanup()
    assert v["info"][9] == want_form and pol["form"] == want_form and pol["active_rows"] == ref.rows.size and pol["troubles"] == 0, (what, v["info"], pol)
    assert v["info"][10] == 0 and v["stats"]["neg_curvature"] == 0, (what, v)
    assert (r.info.status_val, r.info.status_polish, r.info.iter) == (ro.info.status_val, ro.info.status_polish, ro.info.iter), (what, r.info.iter, ro.info.iter)
    assert a.status_adjoint == 1 and t.status_tangent == 1 and np.array_equal(a.active, ref.active) and np.array_equal(t.active, ref.active)
    errs = dict(x=rel(r.x, ro.x), y=rel(r.y, ro.y))
    errs.update({g: rel(getattr(a, g), getattr(ref, g)) for g in GRADS})
    for k, rt in enumerate(rts):
        errs["dx%d" % k], errs["dy%d" % k] = rel(t.dx[k], rt.dx), rel(t.dy[k], rt.dy)
    print(what, "form %d info[3] %d [15] %d elim %d mred %d |" % (v["info"][9], v["info"][3], v["info"][15], v["elim"], ref.rows.size),
          " ".join("%s %.2e" % kv for kv in errs.items()), "| kkt_res %.1e" % a.kkt_res, t.kkt_res)
    assert all(e < BAR for e in errs.values()), (what, errs)
    return v, ref.rows


def test_portfolio_family_small(gpu_lib, oracle_mod, monkeypatch):
    """portfolio_qp(n_blocks=4, block=64) under OSQP_AMD_BLOCK_DIRECT=1: the budget row and the active box rows; the instance is
    block-direct with the budget row as its one coupling row.  (Seed 3: the reference alone passes its guards there.)"""
    from osqp_amd.problems import portfolio_qp
    pb = portfolio_qp(n_blocks=4, block=64, seed=3)
    v, rows = _family(monkeypatch, oracle_mod, "portfolio 4 x 64", pb, FC.BD_ENV, 3)
    Ar = sparse.csc_matrix(sparse.csr_matrix(pb["A"])[rows])
    bd = FC.bd_structure(dict(Pu=sparse.triu(pb["P"], format="csc"), A=Ar, n=256, m=rows.size))
    assert 0 in rows and bd["eligible"] and (v["info"][3], v["info"][15]) == (bd["blocks"], bd["kc"]) == (4, 1), (v["info"], bd)


def test_lasso_family_small(gpu_lib, oracle_mod, monkeypatch):
    """lasso_qp(60, 150) on the dense-direct solve, where the main engine eliminates the 150 residual variables (as
    test_gpu_dense_direct.test_lasso_family_matches_oracle): the instance eliminates them too, and with them every bound variable
    t_i of which one row alone is active -- P_tt = 0, so the back-substitution runs without curvature.  (Seed 1.)"""
    from osqp_amd.problems import lasso_qp
    pb = {k: v for k, v in lasso_qp(60, 150, seed=1).items() if k in "PqAlu"}
    v, rows = _family(monkeypatch, oracle_mod, "lasso 60 x 150", pb, FC.DD_ENV, 4)
    Pu = sparse.triu(pb["P"], format="csc")
    erow, _ = EC.eliminated(Pu, sparse.csc_matrix(sparse.csr_matrix(pb["A"])[rows]))
    want = int((erow >= 0).sum())
    assert want >= 150 and np.all(erow[60:210] >= 0) and v["elim"] == want, (v["elim"], want)
