"""Host side of the infeasibility and live-handle entry points of the row-partitioned solve (include/osqp_amd_rowpart.h) without a device:
the symbols are exported and bind with the documented signatures, a NULL handle is refused by each before any device call, and the
Python classes accept the new settings and carry the new calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HIPENG_ERR_ARG = -103
NAMES = ("osqp_amd_rp_set_infeasibility", "osqp_amd_rp_get_certificates", "osqp_amd_rp_update_lin_cost", "osqp_amd_rp_update_bounds",
         "osqp_amd_rp_warm_start", "osqp_amd_rp_update_rho")


@pytest.fixture(scope="module")
def lib():
    import osqp_amd
    from osqp_amd.rowpart import bind_live
    osqp_amd.build()
    return bind_live(osqp_amd.lib())


def test_symbols_bind_with_the_documented_signatures(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "osqp_amd_rowpart.h")).read(), flags=re.S)
    for name in NAMES:
        f = getattr(lib, name)
        decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl is not None, name
        kinds = [C.c_double if p.strip().startswith("double ") and "*" not in p else C.c_void_p for p in decl.group(1).split(",")]
        assert f.restype is C.c_int and list(f.argtypes) == kinds, (name, decl.group(1))
    enum = re.search(r"enum\s*\{([^}]*)\}", hdr).group(1).replace("= 0", "").split(",")
    from osqp_amd.rowpart import NativeRowPartitionedOSQP as N
    assert [e.strip().replace("OSQP_AMD_RP_PEEK_", "").lower() for e in enum] == [
        {"rv": "rho_vec"}.get(k, k).lower() for k in N._PEEK]                   # the selectors are appended; the first ten keep their values
    assert N._PEEK[:10] == ("x", "xt", "z", "y", "rv", "minv", "b", "r", "sc15", "S")


def test_null_handle_is_refused(lib):
    v = np.ones(4)
    p = v.ctypes.data_as(C.c_void_p)
    assert lib.osqp_amd_rp_set_infeasibility(None, 1e-4, 1e-4) == HIPENG_ERR_ARG
    assert lib.osqp_amd_rp_get_certificates(None, p, p) == HIPENG_ERR_ARG
    assert lib.osqp_amd_rp_update_lin_cost(None, p) == HIPENG_ERR_ARG
    assert lib.osqp_amd_rp_update_bounds(None, p, p) == HIPENG_ERR_ARG
    assert lib.osqp_amd_rp_warm_start(None, p, p) == HIPENG_ERR_ARG
    assert lib.osqp_amd_rp_update_rho(None, 0.1) == HIPENG_ERR_ARG


def test_c_verdict_is_strict_on_the_thresholds(lib):
    """osqp_amd_rp_test_verdict: the host arithmetic that decides at a check of osqp_amd_rp_solve, on given scalars.  lhs, |A'dy|, q'dx,
    |P dx| exactly on eps |d.| do not pass (<); a row violation exactly on it does not fail (>); a norm exactly on OSQP_DIVISION_TOL is
    too small; 10 x the tolerances in the approximate branch; the cost scaling only with the unscaled forms; no primal test without rows;
    a residual that passes switches its side's test off.  The torch model's _verdict must agree on every case."""
    from osqp_amd import rowpart
    f = lib.osqp_amd_rp_test_verdict
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int]
    names = ("ndy", "viol", "lhs", "nAtdy", "ndx", "qdx", "nPdx")
    base = dict(ndy=4.0, viol=0.0, lhs=-1.0, nAtdy=0.5, ndx=4.0, qdx=-1.0, nPdx=0.5)
    word = {0: None, 1: "solved", 3: "primal infeasible", 4: "dual infeasible"}

    def both(change, approximate=0, un=0, c=1.0, m_total=5, pri_res=1.0, dua_res=1.0, eps=(1e-3, 1e-3, 0.25, 0.25)):
        cs = dict(base, **change)
        sc = np.zeros(22); sc[15:] = [cs[k] for k in names]
        e4 = np.array(eps, dtype=np.float64)
        got = f(sc.ctypes.data_as(C.c_void_p), un, c, m_total, e4.ctypes.data_as(C.c_void_p), pri_res, dua_res, approximate)
        s = rowpart.RowPartitionedOSQP.__new__(rowpart.RowPartitionedOSQP)
        s.scaled_data, s.m, s.c, s.cinv = bool(un), m_total, c, 1.0 / c
        s.st = dict(rowpart._DEFAULTS, eps_abs=eps[0], eps_rel=eps[1], eps_prim_inf=eps[2], eps_dual_inf=eps[3])
        s.sc = dict.fromkeys(("z_u", "Ax_u", "z_s", "Ax_s", "q_u", "Aty_u", "Px_u", "q_s", "Aty_s", "Px_s"), 0.0)
        s.pri_res, s.dua_res, s.cs = pri_res, dua_res, cs
        assert s._verdict(approximate=bool(approximate)) == word[got], (change, got)
        return got
    one = np.nextafter(1.0, 2.0)
    assert both({}) == 3 and both(dict(lhs=1.0)) == 4 and both(dict(lhs=np.nextafter(1.0, 0.0))) == 3 and both(dict(nAtdy=1.0)) == 4
    assert both(dict(nAtdy=np.nextafter(1.0, 0.0))) == 3 and both(dict(ndy=1e-30)) == 4 and both(dict(ndy=np.nextafter(1e-30, 1.0), lhs=-1.0, nAtdy=0.0)) == 3
    assert both(dict(ndy=1e-30, qdx=1.0)) == 0 and both(dict(ndy=1e-30, qdx=np.nextafter(1.0, 0.0))) == 4 and both(dict(ndy=1e-30, nPdx=1.0)) == 0
    assert both(dict(ndy=1e-30, viol=1.0)) == 4 and both(dict(ndy=1e-30, viol=one)) == 0 and both(dict(ndy=1e-30, ndx=1e-30)) == 0
    assert both(dict(lhs=9.0)) == 4 and both(dict(lhs=9.0), approximate=1) == 3 and both(dict(lhs=10.0), approximate=1) == 4
    assert both(dict(ndy=1e-30, viol=10.0), approximate=1) == 4 and both(dict(ndy=1e-30, viol=np.nextafter(10.0, 11.0)), approximate=1) == 0
    assert both(dict(ndy=1e-30, nPdx=2.0), un=1, c=2.0) == 0 and both(dict(ndy=1e-30, nPdx=np.nextafter(2.0, 0.0)), un=1, c=2.0) == 4
    assert both(dict(ndy=1e-30, nPdx=np.nextafter(2.0, 0.0)), un=0, c=2.0) == 0
    assert both({}, m_total=0) == 4 and both({}, eps=(1e-3, 1e-3, 0.0, 0.25)) == 4 and both({}, eps=(1e-3, 1e-3, 0.25, 0.0)) == 3
    assert both({}, eps=(1e-3, 1e-3, 0.0, 0.0)) == 0 and both({}, pri_res=0.0) == 4 and both(dict(lhs=1.0), dua_res=0.0) == 0
    assert both({}, pri_res=0.0, dua_res=0.0) == 1 and both({}, pri_res=1e-3, dua_res=0.0) == 3         # pri_res exactly on eps_abs does not pass
    assert f(None, 0, 1.0, 1, None, 0.0, 0.0, 0) == HIPENG_ERR_ARG


def test_verdict_with_both_tests_off_is_the_residual_test_alone(lib):
    """With eps4 = (ea, er, 0, 0) osqp_amd_rp_test_verdict returns 1 or 0 exactly as the residual test dictates and consults none of the
    seven certificate scalars (NaN here); the torch class's _verdict agrees on an object that has no `cs` at all.  This is what lets one
    verdict serve a solve with the infeasibility tests off."""
    from osqp_amd import rowpart
    f = lib.osqp_amd_rp_test_verdict
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int]
    order = ("pri_u", "z_u", "Ax_u", "pri_s", "z_s", "Ax_s", "dua_u", "dua_s", "q_u", "q_s", "Aty_u", "Aty_s", "Px_u", "Px_s", "obj")
    ea, er = 1e-3, 1e-2

    def both(pri_res, dua_res, approximate=0, un=0, c=1.0, m_total=5, **norms):
        s15 = dict(dict.fromkeys(order, 0.0), **norms)
        sc = np.full(22, np.nan); sc[:15] = [s15[k] for k in order]
        e4 = np.array([ea, er, 0.0, 0.0])
        got = f(sc.ctypes.data_as(C.c_void_p), un, c, m_total, e4.ctypes.data_as(C.c_void_p), pri_res, dua_res, approximate)
        s = rowpart.RowPartitionedOSQP.__new__(rowpart.RowPartitionedOSQP)
        s.scaled_data, s.m, s.c, s.cinv = bool(un), m_total, c, 1.0 / c
        s.st = dict(rowpart._DEFAULTS, eps_abs=ea, eps_rel=er)
        s.sc, s.pri_res, s.dua_res = s15, pri_res, dua_res
        assert not hasattr(s, "cs") and s._verdict(approximate=bool(approximate)) == {0: None, 1: "solved"}[got]
        return got
    below = lambda v: np.nextafter(v, 0.0)
    assert both(0.0, 0.0) == 1 and both(below(ea), below(ea)) == 1                                    # pass
    assert both(ea, 0.0) == 0 and both(0.0, ea) == 0                                                 # exactly on eps_abs: no pass
    pt, dt = ea + er * 3.0, ea + er * 7.0                                                            # with the relative terms (scaled forms)
    nrm = dict(z_s=2.0, Ax_s=3.0, q_s=5.0, Aty_s=7.0, Px_s=6.0, z_u=90.0, Ax_u=90.0, q_u=90.0, Aty_u=90.0, Px_u=90.0)
    assert both(below(pt), below(dt), **nrm) == 1 and both(pt, below(dt), **nrm) == 0 and both(below(pt), dt, **nrm) == 0
    assert both(1e9, 0.0, m_total=0) == 1 and both(1e9, ea, m_total=0) == 0                          # no rows: no primal test
    assert both(ea, ea) == 0 and both(ea, ea, approximate=1) == 1                                    # approximate: 10 x each
    assert both(below(10.0 * ea), below(10.0 * ea), approximate=1) == 1 and both(10.0 * ea, 0.0, approximate=1) == 0
    # the unscaled forms with c = 2: the _u norms decide, the dual one divided by c
    nu = dict(z_u=2.0, Ax_u=3.0, q_u=10.0, Aty_u=14.0, Px_u=12.0, z_s=90.0, Ax_s=90.0, q_s=90.0, Aty_s=90.0, Px_s=90.0)
    assert both(below(pt), below(dt), un=1, c=2.0, **nu) == 1 and both(pt, 0.0, un=1, c=2.0, **nu) == 0
    assert both(0.0, dt, un=1, c=2.0, **nu) == 0 and both(0.0, below(ea + er * 14.0), un=0, c=2.0, **dict(nu, q_s=0.0, Aty_s=14.0, Px_s=0.0, z_s=0.0, Ax_s=0.0)) == 1


def test_python_classes_carry_the_settings_and_the_calls():
    from osqp_amd import rowpart
    for cls in (rowpart.RowPartitionedOSQP, rowpart.NativeRowPartitionedOSQP):
        for name in ("update", "warm_start", "update_rho"):
            assert callable(getattr(cls, name))
    st = rowpart._settings(dict(eps_prim_inf=1e-4))
    assert st["eps_prim_inf"] == 1e-4 and st["eps_dual_inf"] == 0.0
    with pytest.raises(ValueError):
        rowpart._settings(dict(eps_dual_inf=-1.0))
    with pytest.raises(ValueError):
        rowpart._settings(dict(polish=1))
