"""GPU tests of OSQP.verify (osqp_amd_verify; osqp_amd/csrc/verify.h: k_ver_point, k_ver_cert, k_ver_combine): the verdict
on a point against the raw problem of a single-QP workspace.

Reference: tests/_verify_sparse_reference.py, the 16 slots in sparse long double with written bars, never the device's own
numbers.  Cases: tests/_verify_single_cases.py; tests/test_verify_cases_host.py proves on the CPU that the reference is the
dense one of BatchOSQP.verify's tests, that every verdict of every case is 1000 bars from its threshold and that each
one-place defect (a value, a bound, half of a symmetric pair, the last entry of a long row, the last row of the second grid
trip, a stale part after an update) moves a slot by more than ten bars on the case meant to catch it.

  1 cases        every case, on points given straight after setup with no solve, scaling = 10 and 0: floats within their
                 bars, verdicts equal
  2 forms        one problem per linear-solve form (tests/_form_cases.PER_FORM, the form asserted): after solve(), verify()
                 on the workspace's own point gives optimal, obj and dua_res within SCALED bars of info's, pri_res <=
                 info.pri_res plus a bar
  3 independence the same problem and point under two forms and two scalings, and twice on one handle: records equal bit
                 for bit
  4 statuses     problems that end primal / dual infeasible: verify() on the handle's own certificates agrees
  5 updates      after each of the seven update entries (full arrays and index lists, both scalings) verify matches the
                 reference on the new data, only the touched part was uploaded, a repeat uploads nothing, and update_rho,
                 warm starts and update_settings upload nothing
  6 nothing changes   twin workspaces, one calling verify between two solves and around an adjoint: x, y, info (timings
                 apart), the engine statistics and the adjoint are bit-equal
  7 batch        a one-member BatchOSQP of the same problem gives a record within two bars of the single-QP one"""
import ctypes as C

import numpy as np
import pytest

import _verify_single_cases as sc
from _verify_reference import FIELDS, SCALED
from _verify_sparse_reference import assert_matches
from tests import _form_cases as FC
from tests import _hipeng as HE

pytestmark = pytest.mark.gpu

TIMINGS = ("setup_time", "solve_time", "update_time", "polish_time", "run_time")


def _point(c):
    return dict(x=c["x"], y=c["y"], dx=c["dx"], dy=c["dy"], eps_abs=c["eps"] and c["eps"][0], eps_rel=c["eps"] and c["eps"][1])


def _form(h):
    info = (C.c_longlong * 16)()
    assert HE._lib().hipeng_resident_info(h.engine(), info) == 0
    return list(info)


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("name", sc.NAMES)
def test_cases_on_given_points_without_a_solve(name, scaling):
    c = sc.case(name)
    k = sc.constants()
    if name == "trip":                # the sizes the case stands for, from the kernels' own constants
        assert c["A"].shape == (k["CAP"] * k["ROWS"] + 1,) * 2 and sc.grid(*c["A"].shape) == k["CAP"]
    if name == "lengths":
        assert max(np.diff(c["A"].indptr)) == k["LONG"] + 1 == max(np.diff(c["A"].tocsr().indptr))
    h = sc.handle(c, scaling=scaling)
    assert (h.nnzP, h.nnzA) == (c["P"].nnz, c["A"].nnz)          # stored zeros are entries
    assert h.verify_info() == dict(calls=0, uploads_P=0, uploads_A=0, uploads_qlu=0)
    v = h.verify(**_point(c))
    ref = sc.reference(name)
    print(name, scaling, "worst error in bars:", float(np.max(np.abs(v.V[:13] - ref.val[:13]) / np.where(ref.bar[:13] > 0, ref.bar[:13], np.inf))))
    assert_matches(v.V, ref, (name, scaling))
    for kf, f in enumerate(FIELDS):
        got = getattr(v, f)
        assert (isinstance(got, bool) and got == (ref.val[kf] != 0.0)) if kf >= 13 else (isinstance(got, float) and got == v.V[kf]), f
    assert h.verify_info() == dict(calls=1, uploads_P=1, uploads_A=1, uploads_qlu=3)


def test_argument_errors():
    c = sc.case("e65")
    h = sc.handle(c)
    for bad in (dict(x=np.zeros(64)), dict(y=np.zeros(3)), dict(dx=np.zeros((65, 1))), dict(dy=np.zeros(130)), dict(eps_abs=-1.0),
                dict(eps_rel=np.inf), dict(eps_abs=np.nan)):
        with pytest.raises(ValueError):
            h.verify(**bad)
    assert h.verify_info()["calls"] == 0
    api = h._api["verify"]
    from osqp_amd import _abi as abi
    nf, V = C.cast(None, abi.c_float_p), np.full(16, 7.5)
    assert api(h._work, nf, nf, nf, nf, -1.0, -1.0, nf) == 1                       # OSQP_DATA_VALIDATION_ERROR: no V
    assert api(h._work, nf, nf, nf, nf, float("nan"), -1.0, abi.fptr(V)) == 1 and api(h._work, nf, nf, nf, nf, -1.0, float("inf"), abi.fptr(V)) == 1
    assert np.all(V == 7.5) and h.verify_info() == dict(calls=0, uploads_P=0, uploads_A=0, uploads_qlu=0)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def _form_handle(monkeypatch, name, env=None, **kw):
    import osqp_amd
    c = FC.make(name)
    _setenv(monkeypatch, c["env"] if env is None else env)
    h = osqp_amd.OSQP().setup(P=c["Pu"], q=c["q"], A=c["A"], l=c["l"], u=c["u"], **kw)
    return c, h


@pytest.mark.parametrize("name", FC.PER_FORM)
def test_own_point_after_a_solve_on_every_form(monkeypatch, name):
    c, h = _form_handle(monkeypatch, name)
    assert _form(h)[9] == c["claims"]["form"], (name, _form(h))
    r = h.solve()
    info = _form(h)
    assert info[9] == c["claims"]["form"] and (info[1] == 1 or info[9] == 0) and info[10] == 0, (name, info)
    assert r.info.status_val == 1, (name, r.info.status)
    v = h.verify()
    case = dict(P=c["Pu"], A=c["A"], q=c["q"], l=np.maximum(c["l"], -1e30), u=np.minimum(c["u"], 1e30), x=r.x, y=r.y,
                dx=r.dual_inf_cert, dy=r.prim_inf_cert, eps=None)
    ref = sc.reference_of(case)
    print(name, "form", info[9], "obj", v.obj, r.info.obj_val, "bar", ref.bar[0], "| dua_res", v.dua_res, r.info.dua_res, "bar", ref.bar[2],
          "| pri_res", v.pri_res, r.info.pri_res, "bar", ref.bar[1], "| margins", ref.margin)
    assert_matches(v.V, ref, name)
    assert v.optimal and not v.prim_inf and not v.dual_inf
    assert abs(v.obj - r.info.obj_val) <= SCALED * ref.bar[0], (name, v.obj, r.info.obj_val, ref.bar[0])
    assert abs(v.dua_res - r.info.dua_res) <= SCALED * ref.bar[2], (name, v.dua_res, r.info.dua_res, ref.bar[2])
    assert v.pri_res <= r.info.pri_res + ref.bar[1], (name, v.pri_res, r.info.pri_res, ref.bar[1])
    assert np.array_equal(h.verify(r.x, r.y, r.dual_inf_cert, r.prim_inf_cert).V, v.V)       # NULL is the workspace's own


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_a_record_does_not_depend_on_the_form_the_scaling_or_earlier_calls(monkeypatch):
    rng = np.random.default_rng(7)
    c = FC.make("f4_b2")
    pt = dict(x=rng.standard_normal(c["n"]), y=rng.standard_normal(c["m"]), dx=rng.standard_normal(c["n"]), dy=rng.standard_normal(c["m"]))
    seen = {}
    for tag, env, kw in (("dense-direct", None, {}), ("pcg", FC.STEPS, {}), ("pcg unscaled", FC.STEPS, dict(scaling=0))):
        with monkeypatch.context() as mp:
            _, h = _form_handle(mp, "f4_b2", env, **kw)
            form = _form(h)[9]
            a = h.verify(**pt).V
            h.solve()
            other = sc.case("e65")           # (a call of another handle in between)
            sc.handle(other).verify(**_point(other))
            b = h.verify(**pt).V
            assert np.array_equal(a, b), tag
            seen[tag] = (form, a)
    assert seen["dense-direct"][0] == 4 and seen["pcg"][0] == 0 and seen["pcg unscaled"][0] == 0, {k: v[0] for k, v in seen.items()}
    for tag in ("pcg", "pcg unscaled"):
        assert np.array_equal(seen[tag][1].view(np.int64), seen["dense-direct"][1].view(np.int64)), (tag, seen[tag][1], seen["dense-direct"][1])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, status, field", [("pinf_true", -3, "prim_inf"), ("dinf_true", -4, "dual_inf")])
def test_own_certificates_agree_with_the_status(name, status, field):
    c = sc.case(name)
    h = sc.handle(c)
    r = h.solve()
    assert r.info.status_val == status, (name, r.info.status)
    v = h.verify()
    ref = sc.reference_of(dict(c, x=r.x, y=r.y, dx=r.dual_inf_cert, dy=r.prim_inf_cert))
    print(name, "margins", ref.margin, "V", v.V[13:])
    assert (v.prim_inf, v.dual_inf) == (field == "prim_inf", field == "dual_inf") and not v.optimal
    assert np.array_equal(v.V[13:], ref.val[13:])


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("what, partial", [(w, False) for w in sc.UPDATES] + [(w, True) for w in ("P", "A", "P_A")])
def test_after_an_update_only_the_touched_part_is_uploaded(what, partial, scaling):
    c = sc.case("e65")
    h = sc.handle(c, scaling=scaling)
    pt = _point(c)
    assert_matches(h.verify(**pt).V, sc.reference("e65"), "before")
    i0 = h.verify_info()
    kw, new = sc.update_data(c, what, partial)
    assert h.update(**kw) == 0
    assert h.verify_info() == i0                                   # the update itself uploads nothing
    assert_matches(h.verify(**pt).V, sc.reference_of(new), (what, partial, scaling))
    i1 = h.verify_info()
    parts = sc.PARTS[what]
    assert _delta(i0, i1) == dict(calls=1, uploads_P=int("P" in parts), uploads_A=int("A" in parts),
                                  uploads_qlu=sum(p in parts for p in "qlu")), (what, i0, i1)
    v = h.verify(**pt).V
    assert _delta(i1, h.verify_info()) == dict(calls=1, uploads_P=0, uploads_A=0, uploads_qlu=0)
    h.update_rho(0.3); h.warm_start(x=c["x"], y=c["y"]); h.warm_start(x=c["x"]); h.warm_start(y=c["y"])
    h.update_settings(max_iter=50, eps_prim_inf=1e-4, alpha=1.5, polish=1, check_termination=10)
    i2 = h.verify_info()
    w = h.verify(**pt).V
    assert _delta(i2, h.verify_info()) == dict(calls=1, uploads_P=0, uploads_A=0, uploads_qlu=0)
    assert np.array_equal(v, w)
    # a second, different update of the same kind is seen too
    kw2, new2 = sc.update_data(new, what, partial, seed=1)
    assert h.update(**kw2) == 0
    assert_matches(h.verify(**pt).V, sc.reference_of(new2), (what, partial, scaling, "second"))


def test_eps_defaults_follow_the_settings():
    c = sc.case("e65")
    h = sc.handle(c, eps_abs=0.25, eps_rel=0.125)
    pt = {k: c[k] for k in ("x", "y", "dx", "dy")}
    assert_matches(h.verify(**pt).V, sc.reference_of(dict(c, eps=(0.25, 0.125))), "settings")
    assert_matches(h.verify(**pt, eps_abs=0.0).V, sc.reference_of(dict(c, eps=(0.0, 0.125))), "eps_abs given")
    h.update_settings(eps_abs=2.0, eps_rel=0.5)
    assert_matches(h.verify(**pt).V, sc.reference_of(dict(c, eps=(2.0, 0.5))), "updated settings")
    assert h.verify_info() == dict(calls=3, uploads_P=1, uploads_A=1, uploads_qlu=3)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def _same_result(a, b, what):
    assert np.array_equal(a.x.view(np.int64), b.x.view(np.int64)) and np.array_equal(a.y.view(np.int64), b.y.view(np.int64)), what
    assert np.array_equal(a.prim_inf_cert, b.prim_inf_cert, equal_nan=True) and np.array_equal(a.dual_inf_cert, b.dual_inf_cert, equal_nan=True), what
    for k, va in vars(a.info).items():
        if k not in TIMINGS:
            assert va == getattr(b.info, k) or (va != va and getattr(b.info, k) != getattr(b.info, k)), (what, k, va, getattr(b.info, k))


@pytest.mark.parametrize("scaling", [10, 0])
def test_verify_changes_nothing(scaling):
    c = sc.case("e257")
    rng = np.random.default_rng(3)
    gx = rng.standard_normal(c["A"].shape[1])
    q2 = c["q"] * 1.25
    twins = [sc.handle(c, scaling=scaling) for _ in range(2)]
    out = []
    for t, h in enumerate(twins):
        if t:
            h.verify(**_point(c))                                  # before any solve
        r1 = h.solve()
        if t:
            h.verify(); h.verify(**_point(c))
        a1 = h.adjoint(gx)
        if t:
            h.verify()                                             # beside a live KKT instance
        a2 = h.adjoint(gx)
        built = h.sens_info()["built"]
        h.update(q=q2)
        if t:
            h.verify(**_point(c))
        r2 = h.solve()
        if t:
            assert h.verify().optimal
        a3 = h.adjoint(gx)
        out.append((r1, r2, a1, a2, a3, built, h.stats()))
    (r1, r2, a1, a2, a3, built, st), (s1, s2, b1, b2, b3, builtb, stb) = out
    assert r1.info.status_val == 1 and r2.info.status_val == 1 and a1.status_adjoint == 1
    _same_result(r1, s1, "first solve"); _same_result(r2, s2, "second solve")
    assert built == builtb == 1 and st == stb, (built, builtb, st, stb)
    for k, (a, b) in enumerate(((a1, b1), (a2, b2), (a3, b3), (a1, a2))):
        for f in ("dq", "dl", "du", "active"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (k, f)
        assert a.kkt_res == b.kkt_res and a.status_adjoint == b.status_adjoint, k
    assert twins[0].verify_info()["calls"] == 0 and twins[1].verify_info() == dict(calls=6, uploads_P=1, uploads_A=1, uploads_qlu=4)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e65", "inf_nonzero", "pinf_true", "dinf_true", "nan_x"])
def test_a_one_member_batch_agrees_within_two_bars(name):
    import osqp_amd
    c = sc.case(name)
    ref = sc.reference(name)
    hb = osqp_amd.BatchOSQP().setup(c["P"], c["A"], c["q"][None, :], c["l"][None, :], c["u"][None, :])
    e = sc.eps_of(c)
    vb = hb.verify(c["x"][None, :], c["y"][None, :], c["dx"][None, :], c["dy"][None, :], eps_abs=e[0], eps_rel=e[1]).V[0]
    v = sc.handle(c).verify(**_point(c)).V
    print(name, "single - batch in bars:", (np.abs(v[:13] - vb[:13]) / np.where(ref.bar[:13] > 0, ref.bar[:13], np.inf)).max())
    assert np.all(np.abs(v[:13] - vb[:13]) <= 2 * ref.bar[:13]) and np.array_equal(v[13:], vb[13:]), (name, v, vb)
