"""Infeasibility certificates and the live handle of the row-partitioned solve, on the CPU: RowPartitionedOSQP (the torch model of the loop
of osqp_amd_rp_solve, with the same reductions and the same budget of two more collectives per check) with scipy SpMVs, at one rank in
this process and through ONE gloo spawn each at two and at three ranks (tests/_rowpart_cert_worker.py solves every problem of
tests/_rowpart_cert_reference.py and its update sequence in that one process group).

Against the oracle: status and iteration count equal, certificates within 1e-5 relative (the bar of tests/test_gpu_batch_edges.py),
x and y of the feasible solves within 1e-6 (the bar of tests/test_rowpart.py); every rank's record equal to rank 0's bit for bit; the
collectives of a solve with the tests on at most those of the same iterations with them off + 2 per check.  The iteration counts are
only fixed after the oracle alone has kept them under changes of q of 1e-15."""
import io
import os
import sys

import numpy as np
import pytest

import _rowpart_cert_reference as CR
from conftest import ROOT

WORKER = os.path.join(ROOT, "tests", "_rowpart_cert_worker.py")


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if np.size(b) else 0.0


@pytest.fixture(scope="module")
def oracle_runs(oracle_mod):
    """The oracle's answers, computed once: every whole solve, and the update sequence driven through the same calls."""
    out = {}
    for name in CR.SOLVE_NAMES:
        pb, kw = CR.solve_problem(name)
        out[name] = oracle_mod.OracleOSQP().setup(**pb, **kw).solve()
    pb, kw, steps = CR.sequence()
    so = oracle_mod.OracleOSQP().setup(**pb, **kw)
    seq, rcs = [], {}
    for j, (call, args) in enumerate(steps):
        r = getattr(so, call)(**args)
        if call == "solve":
            seq.append(r)
        else:
            rcs[j] = int(r)
    out["seq"], out["rcs"] = seq, rcs
    return out


def _results(world, tmp_path):
    if world == 1:
        import _rowpart_cert_worker as W
        from osqp_amd import rowpart
        return W.run(lambda scaled, **kw: rowpart.RowPartitionedOSQP().setup(scaled, rowpart.ScipyOps, **kw))
    from osqp_amd.launch import spawn_ranks
    out = str(tmp_path / ("cert_%d.npz" % world))
    assert spawn_ranks(world, [sys.executable, WORKER, out], stdout=io.StringIO()) == 0
    r = np.load(out)
    assert int(r["world"]) == world
    return r


def test_oracle_keeps_its_iteration_counts_under_1e_15_changes_of_q(oracle_mod, oracle_runs):
    """Before any iteration count is fixed: the oracle alone, with q moved by 1e-15 relative up and down, ends every problem with the same
    status at the same iteration (no member excused)."""
    for name in CR.SOLVE_NAMES:
        pb, kw = CR.solve_problem(name)
        for f in (1.0 - 1e-15, 1.0 + 1e-15):
            r = oracle_mod.OracleOSQP().setup(**dict(pb, q=pb["q"] * f), **kw).solve()
            assert (r.info.status, r.info.iter) == (oracle_runs[name].info.status, oracle_runs[name].info.iter), (name, f)
    want = dict(primal="primal infeasible", dual="dual infeasible", dual_m0="dual infeasible", primal_inaccurate="primal infeasible inaccurate",
                dual_inaccurate="dual infeasible inaccurate", feasible="solved", primal_empty_rank="primal infeasible",
                dual_empty_rank="dual infeasible")
    assert {k: oracle_runs[k].info.status for k in CR.SOLVE_NAMES} == want
    assert [r.info.status for r in oracle_runs["seq"]] == ["primal infeasible"] + ["solved"] * 4


@pytest.mark.parametrize("world", [1, 2, 3])
def test_infeasible_problems_and_the_update_sequence_match_the_oracle(tmp_path, oracle_runs, world):
    from osqp_amd.rowpart import shard_rows
    r = _results(world, tmp_path)
    for name in CR.SOLVE_NAMES:
        ro, g = oracle_runs[name], (lambda k: r[name + "/" + k])
        assert (str(g("status")), int(g("iter"))) == (ro.info.status, ro.info.iter), name
        assert bool(g("ranks_equal")), name
        checks = -(-int(g("iter")) // 25)
        print("%s world %d: %s at %d, collectives %d on / %d off, %d checks" % (name, world, g("status"), g("iter"), g("collectives"), g("collectives_off"), checks))
        assert int(g("iter_off")) == int(g("iter")) and int(g("collectives")) <= int(g("collectives_off")) + 2 * checks, name
        if world > 1 and name != "dual_m0":
            assert int(g("collectives")) > int(g("collectives_off")), name
        if ro.info.status in CR.INFEASIBLE:
            prim = ro.info.status.startswith("primal")
            assert float(g("obj")) == (1e30 if prim else -1e30) == ro.info.obj_val, name
            assert np.isnan(g("x")).all() and np.isnan(g("y")).all() and bool(g("iterates_zero")), name
            mine, theirs = (g("prim_inf_cert"), ro.prim_inf_cert) if prim else (g("dual_inf_cert"), ro.dual_inf_cert)
            assert abs(np.abs(theirs).max() - 1.0) < 1e-12 and _rel(mine, theirs) < 1e-5, (name, _rel(mine, theirs))
            assert np.isnan(g("dual_inf_cert") if prim else g("prim_inf_cert")).all(), name
        else:
            assert _rel(g("x"), ro.x) < 1e-6 and _rel(g("y"), ro.y) < 1e-6 and bool(g("same_bits_off")), name
    # a rank without rows inside a problem that has rows: rank 1 of two, with the tests on
    if world == 2:
        for name in ("primal_empty_rank", "dual_empty_rank"):
            assert [tuple(int(v) for v in ab) for ab in r[name + "/rows"]] == [(0, 4), (4, 4)], name
    # the contradicting rows of the primal-infeasible problem all sit on one rank
    rows = shard_rows(CR.solve_problem("primal")[0]["A"], world)
    assert [tuple(int(v) for v in ab) for ab in r["primal/rows"]] == rows and rows[0][0] == 0 and rows[0][1] >= 2
    # the sequence, step by step
    seq, rcs = oracle_runs["seq"], oracle_runs["rcs"]
    assert int(r["seq/solves"]) == len(seq) == 5
    for k, ro in enumerate(seq):
        g = lambda f: r["seq/%d/%s" % (k, f)]
        assert (str(g("status")), int(g("iter")), int(g("rho_updates"))) == (ro.info.status, ro.info.iter, ro.info.rho_updates), k
        assert bool(g("ranks_equal")), k
        if k:
            assert _rel(g("x"), ro.x) < 1e-6 and _rel(g("y"), ro.y) < 1e-6, (k, _rel(g("x"), ro.x), _rel(g("y"), ro.y))
            # bounds with l > u on the last rank's last row: refused on every rank (the record of every rank is equal), nothing changed
            for f in ("x", "y"):
                assert np.array_equal(g(f), r["seq_clean/%d/%s" % (k, f)]), (k, f)
            assert int(g("iter")) == int(r["seq_clean/%d/iter" % k])
    assert {j: int(r["seq/rc%d" % j]) for j in rcs} == {j: int(bool(v)) for j, v in rcs.items()}
    assert int(r["seq/rc1"]) == 1 and int(r["seq/rc2"]) == 0 and int(r["seq/rc6"]) == 1 and int(r["seq/rc7"]) == 0


def test_verdicts_exactly_on_the_thresholds_are_strict():
    """lhs, |A'dy|, q'dx, |P dx| exactly on eps |d.| do not pass (the reference asks <); a row violation exactly on it does not fail (>);
    a norm exactly on OSQP_DIVISION_TOL is too small."""
    from osqp_amd import rowpart
    s = rowpart.RowPartitionedOSQP.__new__(rowpart.RowPartitionedOSQP)
    s.scaled_data, s.m, s.c, s.cinv = False, 5, 1.0, 1.0
    s.st = dict(rowpart._DEFAULTS, eps_prim_inf=0.25, eps_dual_inf=0.25)
    s.sc = dict.fromkeys(("z_u", "Ax_u", "z_s", "Ax_s", "q_u", "Aty_u", "Px_u", "q_s", "Aty_s", "Px_s"), 0.0)
    s.pri_res = s.dua_res = 1.0                             # neither residual passes
    base = dict(ndy=4.0, viol=0.0, lhs=-1.0, nAtdy=0.5, ndx=4.0, qdx=-1.0, nPdx=0.5)
    for change, want in ((dict(), "primal infeasible"), (dict(lhs=1.0), "dual infeasible"), (dict(nAtdy=1.0), "dual infeasible"),
                         (dict(ndy=1e-30), "dual infeasible"), (dict(ndy=1e-30, qdx=1.0), None), (dict(ndy=1e-30, nPdx=1.0), None),
                         (dict(ndy=1e-30, viol=1.0), "dual infeasible"), (dict(ndy=1e-30, viol=np.nextafter(1.0, 2.0)), None),
                         (dict(ndy=1e-30, ndx=1e-30), None), (dict(lhs=np.nextafter(1.0, 0.0)), "primal infeasible")):
        s.cs = dict(base, **change)
        assert s._verdict() == want, change
    s.cs = dict(base, lhs=9.0)                              # passes only at 10 x eps
    assert s._verdict() == "dual infeasible" and s._verdict(approximate=True) == "primal infeasible"
