"""GPU tests of the common-K engine's batch loop (`bc_solve` / `bc_rebuild` / `bc_batch_estimate` in batch.hip, the
kernels of batch_common.h) against tests/_common_reference.py, the same loop in long double: one rho for the batch,
adapted to the geometric mean of the running members' estimates, finished members frozen; and the engine at batch sizes
that reach the second workgroup of its element-wise kernels (B > 64), of k_bc_probe / k_bc_adopt (B > 256) and the second
column tile of the GEMM (Bp > 64).

Bars: status, iter and rho_updates identical per member; `r.rho[b]` within RHO_BAR of the reference (100 x the
reference's own measured rho difference to the oracle, see _common_reference.py); x, y within 1e-6 relative and the
objective within 1e-8 (`_batch_parity.assert_parity`).  tests/test_common_reference_host.py shows on the CPU that every
decision of these cases is at least 1e-2 (adaptation) and 1e-3 (termination) away from its threshold."""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse

from _batch_parity import assert_parity, check_member_kinv, oracle_ws
from _common_cases import FIXED, common_family, common_oracle, prescaled_oracle, unscale
from _common_reference import RHO_BAR, case_reference, loop_case

pytestmark = pytest.mark.gpu


def _common(P, A, Q, L, U, **kw):
    import osqp_amd
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **kw)


def _assert_loop_parity(r, rr, what):
    """Every member of the engine's result r against the reference's rr."""
    B = rr.x.shape[0]
    drho = np.abs(r.rho - rr.rho) / rr.rho
    print(what, "status", r.status_val.tolist(), "iter", r.iter.tolist(), "rho_updates", r.rho_updates.tolist(),
          "reference", rr.status_val.tolist(), rr.iter.tolist(), rr.rho_updates.tolist(), "max rho difference %.2e" % drho.max())
    for b in range(B):
        ro = SimpleNamespace(x=rr.x[b], y=rr.y[b], info=SimpleNamespace(status_val=int(rr.status_val[b]), iter=int(rr.iter[b]),
                                                                        rho_updates=int(rr.rho_updates[b]), obj_val=rr.obj_val[b]))
        assert_parity(r, b, ro, what)
        assert drho[b] <= RHO_BAR, (what, b, r.rho[b], rr.rho[b], drho[b])


def _assert_final_rho(bs, r):
    """The handle's rho is the rho of the member that finished last: no move follows the last finish."""
    assert bs.member_workspace(0)["rho"] == r.rho[int(np.argmax(r.iter))]


# ---- A. adaptive rho, differing members -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A1", "A2-scaled", "A2-default", "A3"])
def test_adaptive_batch_against_the_reference(gpu_lib, oracle_mod, name):
    P, A, Q, L, U, kw = loop_case(name)
    _, runs = case_reference(oracle_mod, name)
    bs = _common(P, A, Q, L, U, **kw)
    r = bs.solve()
    _assert_loop_parity(r, runs[0], name)
    _assert_final_rho(bs, r)
    assert bs.rounds()[0] == 1 + len(runs[0].moves), (bs.rounds(), runs[0].moves)
    bs.cleanup()


# ---- B. batch-size edges at a fixed rho -------------------------------------------------------------------------------
def _as_member(ws, ro):
    x, y, obj = unscale(ws, ro)
    return SimpleNamespace(x=x, y=y, info=SimpleNamespace(status_val=ro.info.status_val, iter=ro.info.iter,
                                                          rho_updates=ro.info.rho_updates, obj_val=obj))


@pytest.mark.parametrize("B", [63, 64, 65, 257])
def test_batch_size_edges(gpu_lib, oracle_mod, B):
    """The 64-member workgroups of the element-wise kernels, the 256-member ones of k_bc_probe / k_bc_adopt and the
    64-column tiles of the GEMM (Bp = 64 | 64 | 80 | 272), every member against its pre-scaled oracle run."""
    P, A, Q, L, U, _ = common_family(33, 66, B, 1099)
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **FIXED))
    bs = _common(P, A, Q, L, U, **FIXED)
    r = bs.solve()
    for b in range(B):
        ro = prescaled_oracle(oracle_mod, ws, Q, L, U, b, **FIXED).solve()
        assert_parity(r, b, _as_member(ws, ro), "B=%d" % B)
    assert np.all(r.status_val == 1) and len(set(r.iter.tolist())) >= 2
    assert bs.rounds()[0] == 1 and bs.rounds()[1] in (0, B)
    bs.cleanup()


def test_member_bits_across_the_batch_boundaries(gpu_lib):
    """Member 200 of a batch of 257 (fourth workgroup of the element-wise kernels, fourth column tile of the GEMM), the
    same member alone and at index 0 of a batch of 65: bit-equal x, y and info.  scaling = 0 as in
    test_member_bits_do_not_depend_on_the_batch -- the common scaling would differ with the batch's q^ -- and max_iter =
    200, since unscaled members of this size need thousands of iterations: every member ends solved or at max_iter."""
    P, A, Q, L, U, _ = common_family(33, 66, 257, 1099)
    kw = dict(FIXED, scaling=0, max_iter=200)
    idx = [200] + list(range(64))
    out = []
    for sel in (slice(None), slice(200, 201), idx):
        bs = _common(P, A, Q[sel], L[sel], U[sel], **kw)
        out.append(bs.solve())
        bs.cleanup()
    r257, r1, r65 = out
    assert r257.status_val[200] in (1, 2, -2) and r257.iter[200] > 0
    for k in ("x", "y", "info_raw"):
        assert np.array_equal(getattr(r257, k)[200], getattr(r1, k)[0]), k
        assert np.array_equal(getattr(r257, k)[200], getattr(r65, k)[0]), k
        assert np.array_equal(getattr(r257, k)[:64], getattr(r65, k)[1:]), k


# ---- C. rho moves at max_iter; warm continuations ----------------------------------------------------------------------
def test_rho_moves_at_max_iter_then_warm_solve(gpu_lib, oracle_mod):
    P, A, Q, L, U, kw = loop_case("C20")
    B, n = Q.shape
    ref, (r1, r2) = case_reference(oracle_mod, "C20")
    assert r1.moves[-1] == 20
    bs = _common(P, A, Q, L, U, **kw)
    g = bs.solve()
    _assert_loop_parity(g, r1, "max_iter 20")
    assert np.all(g.status_val == -2)
    # the solve ended with a rebuild: K^-1 is that of the moved rho
    ws0 = bs.member_workspace(B - 1)
    assert ws0["rho"] == g.rho[B - 1] and abs(ws0["rho"] - r1.final_rho) <= RHO_BAR * r1.final_rho
    so0 = common_oracle(oracle_mod, P, A, Q, L, U, **kw)
    check_member_kinv(bs, B - 1, so0, "after the move at max_iter", 64)
    o = oracle_ws(so0)
    rho_vec = np.where(o["ctype"] == -1, 1e-6, np.where(o["ctype"] == 1, 1e3 * ws0["rho"], ws0["rho"]))
    Pf = (o["Pu"] + sparse.triu(o["Pu"], 1).T).toarray(); Ad = o["A"].toarray()
    K = Pf + o["sigma"] * np.eye(n) + Ad.T @ (rho_vec[:, None] * Ad)
    res = np.abs(ws0["Kinv"][:n, :n] @ K - np.eye(n)).max()
    # eps cond(K) = 1.1e-16 x 4.5e5 = 5e-11, and a factor 20; a K^-1 left at the rho before the move leaves O(1)
    assert res <= 1e-9, res
    # the warm second solve on that handle
    g2 = bs.solve()
    _assert_loop_parity(g2, r2, "second 20 iterations")
    bs.cleanup()
    # 40 iterations in one run: the rebuild and the refreshed w = rho z - y in mid-run
    P, A, Q, L, U, kw40 = loop_case("C40")
    _, (r40,) = case_reference(oracle_mod, "C40")
    bs = _common(P, A, Q, L, U, **kw40)
    g40 = bs.solve()
    _assert_loop_parity(g40, r40, "max_iter 40")
    assert bs.rounds()[0] == 1 + len(r40.moves)
    bs.cleanup()


def test_update_rho_after_an_adaptive_solve(gpu_lib, oracle_mod):
    P, A, Q, L, U, kw = loop_case("A1")
    _, (r1, r2) = case_reference(oracle_mod, "A1")
    bs = _common(P, A, Q, L, U, **kw)
    _assert_loop_parity(bs.solve(), r1, "A1")
    assert bs.update_rho(0.3) == 0
    g = bs.solve()
    _assert_loop_parity(g, r2, "A1 after update_rho(0.3)")
    _assert_final_rho(bs, g)
    assert bs.rounds()[0] == 1 + len(r2.moves)
    bs.cleanup()


# ---- D. the refinement branch on and off -------------------------------------------------------------------------------
@pytest.mark.parametrize("env,value,name,refined", [(None, None, "A1", None), ("OSQP_AMD_BATCH_REFINE", "2", "A1", None),
                                                    ("OSQP_AMD_BATCH_REFINE_TOL", "0", "A1", "all"),
                                                    ("OSQP_AMD_BATCH_REFINE_TOL", "1e300", "D-wide", "none")])
def test_refinement_on_and_off(gpu_lib, oracle_mod, monkeypatch, env, value, name, refined):
    """The switch is read at setup.  An unrefined explicit inverse leaves eps cond(K) per solve: with cond(K) <= 1e4
    (case D-wide, asserted on the host) that is 1e-12, far inside the 1e-6 bar over a few hundred iterations."""
    if env:
        monkeypatch.setenv(env, value)
    P, A, Q, L, U, kw = loop_case(name)
    B = Q.shape[0]
    _, runs = case_reference(oracle_mod, name)
    bs = _common(P, A, Q, L, U, **kw)
    r = bs.solve()
    _assert_loop_parity(r, runs[0], "%s %s=%s" % (name, env, value))
    rounds, members = bs.rounds()
    assert rounds == 1 + len(runs[0].moves), (rounds, members)
    assert members == {None: members, "all": B, "none": 0}[refined] and members in (0, B), "refined members: %d" % members
    bs.cleanup()
