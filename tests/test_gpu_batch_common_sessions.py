"""GPU tests of a common-K handle's life against tests/_common_reference.py, the same loop in long double with
`solve(members=)`, `update` and `warm_start`: subset solves whose scaling is the batch's and nobody else's, sessions of
several calls, the refinement verdict after a subset solve, a pack while a verdict is open, and packs of chosen shapes.
tests/test_common_session_cases_host.py proves on the CPU what is taken for granted here about every case.

Bars: status, iter and rho_updates identical per listed member; `r.rho[b]` within RHO_BAR of the reference; x, y within
1e-6 relative and the objective within 1e-8 (`_batch_parity.assert_parity`).  A member that is not listed keeps the bits of
x, y, info_raw and both certificates it had before the call."""
from types import SimpleNamespace

import numpy as np
import pytest

from _batch_parity import assert_parity, rel
from _common_cases import FIXED
from _common_members_cases import packs_of
from _common_reference import RHO_BAR
from _common_session_cases import (GEOMETRY, GEOMETRY_PROVED, PROBING_REFINE_TOL, VERDICT_B, VERDICT_S, VERDICT_SETTINGS, geometry_case,
                                   geometry_reference, play, session_case, session_reference, verdict_case,
                                   verdict_reference)

pytestmark = pytest.mark.gpu

ARRAYS = ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert")


def _common(P, A, Q, L, U, **kw):
    import osqp_amd
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **kw)


def _unpacked(monkeypatch, *args, **kw):
    monkeypatch.setenv("OSQP_AMD_BATCH_COMMON_PACK", "0")
    try:
        return _common(*args, **kw)
    finally:
        monkeypatch.delenv("OSQP_AMD_BATCH_COMMON_PACK")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(r1, r2, i1=slice(None), i2=slice(None), what=""):
    for k in ARRAYS:
        assert np.array_equal(_bits(getattr(r1, k)[i1]), _bits(getattr(r2, k)[i2])), (what, k)


def _assert_listed_parity(r, rr, listed, what):
    """The listed members of the engine's result r against the reference's rr; prints the worst figures first."""
    drho = np.abs(r.rho[listed] - rr.rho[listed]) / rr.rho[listed]
    dx = max(rel(r.x[b], rr.x[b]) for b in listed); dy = max(rel(r.y[b], rr.y[b]) for b in listed)
    dobj = (np.abs(r.obj_val - rr.obj_val) / np.maximum(1.0, np.abs(rr.obj_val)))[listed].max()
    print(what, "listed", len(listed), "iter", sorted(set(r.iter[listed].tolist())), "reference",
          sorted(set(rr.iter[listed].tolist())), "worst: rho %.2e x %.2e y %.2e obj %.2e" % (drho.max(), dx, dy, dobj))
    for k, b in enumerate(listed):
        ro = SimpleNamespace(x=rr.x[b], y=rr.y[b], info=SimpleNamespace(status_val=int(rr.status_val[b]), iter=int(rr.iter[b]),
                                                                        rho_updates=int(rr.rho_updates[b]), obj_val=rr.obj_val[b]))
        assert_parity(r, b, ro, what)
        assert drho[k] <= RHO_BAR, (what, b, r.rho[b], rr.rho[b], drho[k])


def _play_against_the_reference(bs, steps, runs, name):
    """Every step of the session on the handle; after every solve the listed members against the reference, the others
    against results() before the step, the handle's rho and the inversions it made."""
    by_step = dict(runs)
    B = bs.B
    for k, step in enumerate(steps):
        before = bs.results() if step[0] == "solve" else None
        r = play(bs, step)
        if r is None:
            continue
        rr = by_step[k]
        listed = rr.listed
        rest = np.setdiff1d(np.arange(B), listed)
        what = "%s step %d" % (name, k)
        _assert_listed_parity(r, rr, listed, what)
        _same(r, before, i1=rest, i2=rest, what=what + " unlisted")
        rho = bs.member_workspace(0)["rho"]
        assert abs(rho - rr.final_rho) <= RHO_BAR * rr.final_rho, (what, rho, rr.final_rho)
        assert bs.rounds()[0] == 1 + len(rr.moves), (what, bs.rounds(), rr.moves)
        assert bs.columns().started == len(listed)


# ---- C1: sessions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general", "cut", "cut-cold"])
def test_session_against_the_reference(gpu_lib, oracle_mod, name):
    """ "general": subsets under the batch's own scaling, an overlapping subset, update, update_rho, a full solve.
    "cut": max_iter = 40, members continued by later subsets, one warm_start with given values.  "cut-cold": with the
    setting warm_start = 0 a subset solve restarts its members from zero and leaves the others alone."""
    (P, A, Q, L, U), kw, steps = session_case(name)
    _, runs = session_reference(oracle_mod, name)
    bs = _common(P, A, Q, L, U, **kw)
    _play_against_the_reference(bs, steps, runs, name)
    bs.cleanup()


# ---- C2: the verdict after a subset solve ------------------------------------------------------------------------------------
def test_verdict_binds_only_probed_members(gpu_lib, oracle_mod):
    """solve(members=S) on a fresh handle probes S alone, and no member of S needs refinement (their ill-conditioned block
    is exactly zero); solve(members=rest) then probes again, because nobody of `rest` was probed under this K^-1, and
    refines: the rest members get the bits of a handle set up on them alone (scaling = 0: same K), the verdict is on,
    and they hold the parity bars."""
    P, A, Q, L, U = verdict_case()
    S, rest = VERDICT_S, np.setdiff1d(np.arange(VERDICT_B), VERDICT_S)
    _, rr = verdict_reference(oracle_mod)
    h1, alone = _common(P, A, Q, L, U, **VERDICT_SETTINGS), _common(P, A, Q[rest], L[rest], U[rest], **VERDICT_SETTINGS)
    r0 = h1.solve(members=S)
    print("after solve(S): rounds", h1.rounds())
    assert h1.rounds()[1] == 0
    _assert_listed_parity(r0, rr, S, "verdict case, S")
    r1, ra = h1.solve(members=rest), alone.solve()
    print("after solve(rest): rounds", h1.rounds(), "alone", alone.rounds(), "worst x against alone %.2e" %
          max(rel(r1.x[b], ra.x[k]) for k, b in enumerate(rest)))
    assert alone.rounds()[1] == len(rest)
    _same(r1, ra, i1=rest, what="the rest against a handle of their own")
    assert h1.rounds()[1] == VERDICT_B
    _same(r1, r0, i1=S, i2=S, what="S after the rest was solved")
    _assert_listed_parity(r1, rr, rest, "verdict case, the rest")
    # "on" stays: a later solve of S is refined too
    h1.solve(members=S)
    assert h1.rounds()[1] == VERDICT_B
    h1.cleanup(); alone.cleanup()


# ---- C3: a pack while a verdict is open --------------------------------------------------------------------------------------
def test_pack_inside_the_probed_iterations(gpu_lib, oracle_mod, monkeypatch):
    """The probes of iterations 1 to 4 leave the verdict off, rho moves at 24, and the pack at the check point 25 finds
    the verdict of the second window open (all proved on the CPU).  No other window follows before max_iter, so a verdict
    that ends on shows that iterations 25 to 28 were probed; the packed run takes it at the pack, the unpacked twin at 28."""
    monkeypatch.setenv("OSQP_AMD_BATCH_REFINE_TOL", repr(PROBING_REFINE_TOL))        # read at setup
    (P, A, Q, L, U), kw, steps = session_case("probing")
    _, runs = session_reference(oracle_mod, "probing")
    bs, off = _common(P, A, Q, L, U, **kw), _unpacked(monkeypatch, P, A, Q, L, U, **kw)
    ro = off.solve()
    _play_against_the_reference(bs, steps, runs, "probing")
    r = bs.results()
    print("probing", bs.columns(), bs.rounds(), off.rounds())
    _same(r, ro, what="probing against the unpacked solve")
    assert bs.rounds() == off.rounds() == (2, Q.shape[0])
    rr = runs[0][1]
    assert bs.columns().packs >= 1 and bs.columns() == (Q.shape[0],) + packs_of(rr.iter) and off.columns().packs == 0
    bs.cleanup(); off.cleanup()


# ---- C4: pack geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_pack_geometry(gpu_lib, oracle_mod, monkeypatch, name):
    """src[c] = c + 1 over a whole row ("shift-1") and across the 256-column chunk boundary ("shift-1-chunk"), every
    survivor behind column 256 ("back"), a first pack to exactly 256 and 257 columns."""
    P, A, Q, L, U, _ = geometry_case(name)
    B = Q.shape[0]
    _, rr = geometry_reference(oracle_mod, name)
    bs, off = _common(P, A, Q, L, U, **FIXED), _unpacked(monkeypatch, P, A, Q, L, U, **FIXED)
    r, ro = bs.solve(), off.solve()
    print(name, bs.columns(), "iterations", dict(zip(*np.unique(r.iter, return_counts=True))))
    _same(r, ro, what=name + " against the unpacked solve")
    _, packs, ended = GEOMETRY_PROVED[name]
    assert bs.columns() == (B, packs, ended) and off.columns() == (B, 0, B)
    assert np.array_equal(r.iter, rr.iter) and np.array_equal(r.status_val, rr.status_val)
    bs.cleanup(); off.cleanup()
