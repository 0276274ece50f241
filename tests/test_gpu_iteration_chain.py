"""GPU tests of what the early, unconditional loads of k_pcg_init and k_admm_finalize could break: both kernels issue their
loads in three flights before they know whether the segment runs at all, so every prefetch has to be in bounds in every thread
whatever the verdict, and a segment that returns at once (beyond the target, a stalled solve's continuation) must leave
the iteration untouched.  Cases and reference: tests/_engine_reference.py (make_case, admm_step, step_bars); the bars are the
ones of tests/test_gpu_engine_kernels.py (pcg_eps_rel = 1e-12 on the PCG forms, ten times numpy's unrefined solve on the direct
forms), none tuned on the device's output.

  segments        run_admm(7) in one call (two single-segment graphs, then one graph of five segments), seven run_admm(1), and
                  run_admm(7) in a process with OSQP_AMD_GRAPH_SEGS=1: x, y, z bit-equal among the three, on `offtile` (257 x 300)
                  and `empty` (300 x 2100: 2061 empty rows in one block, several rounds of rows per workgroup) on the
                  launch-per-step kernels, and on `offtile` with the defaults.
  stall           `offtile` on the launch-per-step kernels: the first solve needs more than the initial unroll, so
                  k_admm_finalize leaves the iteration untouched once and a second graph launch finishes it.
  from_start      `tiny3` and `m0` on the launch-per-step kernels, alpha = 1 (x+ = x~ exactly): iterated until a solve's start
                  vector passes the stop test itself (iteration 154 and 14; `bounds` and `offtile` never get there within 500
                  iterations at any pcg_eps_rel from 1e-12 to 1e-6, before or after the change); that x~ is the start vector
                  2 x~_k - x~_{k-1} bit for bit, and that step and the next lie within the bar.
  resident        the resident PCG forced onto `offtile` and `bounds` (k_pcg_init scatters u0 into the exchanged vector's
                  layout, k_form_K re-forms K) and whatever form the defaults choose: a step after a set_rho spanning 1e-3 .. 1e3.
  edges           `tiny3` (one thread has work), `m0` (no row: nothing valid to prefetch by row), `long` (rows of 511 - 513 entries:
                  the long-row branch beside stream blocks), each on the launch-per-step kernels and with the defaults (dense-direct
                  for `tiny3` and `long`); `long` also on the resident PCG (the flights of k_pcg_init, its scatter into the
                  exchanged vector's layout and the long-row branch together; `tiny3` and `m0` are below the 256 variables a
                  resident plan needs).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _engine_reference as R
from tests._iteration_chain_worker import PCG_EPS, open_case

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_iteration_chain_worker.py")


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.make_case(name)


def _check_step(tag, e, pb, o, alpha, rho, before, after, pcg_eps_rel=PCG_EPS):
    """One ADMM step from `before` = (x, y, z) to `after` against the reference and its bars; returns the reference's dict."""
    (x0, y0, z0), (x1, y1, z1) = before, after
    inf = e.info()
    direct = inf[9] in (3, 4) and inf[1] == 1
    st = R.admm_step(pb, R.SIGMA, alpha, rho, x0, z0, y0)
    bars = R.step_bars(st, alpha, rho, direct, pcg_eps_rel)
    assert np.all(o["l"] <= z1) and np.all(z1 <= o["u"])
    for k, got in (("x", x1), ("z", z1), ("y", y1)):
        err = np.abs(got.astype(R.LD) - st[k]).astype(float)
        ratio = float((err / np.maximum(bars[k], 1e-300)).max()) if err.size else 0.0
        print(f"[iteration-chain] {tag} form {inf[9]} direct {direct} {k}+: max err {err.max() if err.size else 0.0:.2e}, err/bar {ratio:.3e}")
        assert np.all(err <= bars[k]), (tag, k, ratio)
    return st


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name,env", [("offtile", "steps"), ("empty", "steps"), ("offtile", "default")])
def test_segments_that_return_at_once(name, env, tmp_path):
    """Seven iterations in one call, one by one, and in single-segment graphs: the same bits."""
    c = _case(name)
    runs = {}
    for how in ("one call", "one by one"):
        e, _, _, _ = open_case(c, env)
        try:
            if how == "one call":
                e.run_admm(7)
            else:
                for _ in range(7):
                    e.run_admm(1)
            runs[how] = e.download(False)[:3]
            print(f"[iteration-chain] {name}/{env} {how}: form {e.info()[9]}, graph launches {e.stats()['graph_launches']}")
        finally:
            e.close()
    out = tmp_path / "segs1.npz"
    p = subprocess.run([sys.executable, WORKER, name, env, "7", str(out)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OSQP_AMD_GRAPH_SEGS="1"))
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.load(out)
    runs["single segments"] = (got["x"], got["y"], got["z"])
    ref = runs["one call"]
    for how, vec in runs.items():
        for k, a, b in zip("xyz", ref, vec):
            diff = int((_bits(a) != _bits(b)).sum())
            print(f"[iteration-chain] {name}/{env} {how} {k}: {diff} of {a.size} elements differ from one call")
            assert diff == 0, (name, env, how, k)


def test_a_solve_that_stalls():
    """The first solve outruns the initial unroll: finalize returns once without touching the iteration."""
    c = _case("offtile")
    e, o, pb, (x0, y0, z0) = open_case(c, "steps")
    try:
        e.run_admm(1)
        x1, y1, z1, _, _ = e.download(False)
        st = e.stats()
        print(f"[iteration-chain] stall: {st}")
        assert (st["admm_done"], st["pcg_forced"], st["neg_curvature"]) == (1, 0, 0), st
        assert st["graph_launches"] > st["admm_done"], st
        _check_step("stall offtile/steps", e, pb, o, 1.6, c["rho"], (x0, y0, z0), (x1, y1, z1))
    finally:
        e.close()


@pytest.mark.parametrize("name", ["tiny3", "m0"])
def test_start_vector_that_passes_the_stop_test(name):
    """from_start: no PCG update ran, x~ is the extrapolated start vector itself."""
    c = _case(name)
    e, o, pb, _ = open_case(c, "steps", alpha=1.0)
    try:
        hist = [e.download(False)[:3]]
        hit = None
        for k in range(1, 501):
            e.run_admm(1)
            hist.append(e.download(False)[:3])
            if e.stats()["pcg_iters_last"] == 0 and k >= 14:       # (the full extrapolation step from the 12th iteration on)
                hit = k
                break
        print(f"[iteration-chain] from_start {name}: iteration {hit} started from a vector that passed the stop test")
        assert hit is not None
        # alpha = 1: x_k = x~_k exactly, so the start vector of iteration k is x_{k-1} + 1.0 * (x_{k-1} - x_{k-2})
        xa, xb = hist[hit - 1][0], hist[hit - 2][0]
        start = xa + 1.0 * (xa - xb)
        assert np.array_equal(_bits(hist[hit][0]), _bits(start))
        _check_step(f"from_start {name}/steps", e, pb, o, 1.0, c["rho"], hist[hit - 1], hist[hit])
        e.run_admm(1)
        _check_step(f"after from_start {name}/steps", e, pb, o, 1.0, c["rho"], hist[hit], e.download(False)[:3])
    finally:
        e.close()


@pytest.mark.parametrize("env", ["resident", "default"])
@pytest.mark.parametrize("name", ["offtile", "bounds"])
def test_resident_form_after_a_rho_update(name, env):
    """u0 scattered into the exchanged vector's layout, K re-formed for weights over six decades."""
    c = _case(name)
    rho = np.logspace(-3, 3, c["m"])[np.random.default_rng(5).permutation(c["m"])]
    e, o, pb, (x0, y0, z0) = open_case(c, env)
    try:
        assert e.elim() == 0
        inf = e.info()
        assert inf[1] == 1, inf
        if env == "resident":
            assert inf[9] == 1, inf
        e.run_admm(2)
        e.set_rho(rho)
        before = e.download(False)[:3]
        e.run_admm(1)
        after = e.download(False)[:3]
        inf = e.info()
        assert inf[1] == 1 and inf[10] == 0, inf
        _check_step(f"rho update {name}/{env}", e, pb, o, 1.6, rho, before, after)
    finally:
        e.close()


@pytest.mark.parametrize("name,env", [("tiny3", "steps"), ("tiny3", "default"), ("m0", "steps"), ("m0", "default"), ("long", "steps"),
                                      ("long", "default"), ("long", "resident")])
def test_edges_of_the_prefetch(name, env):
    c = _case(name)
    e, o, pb, (x0, y0, z0) = open_case(c, env)
    try:
        assert e.elim() == 0
        inf = e.info()
        print(f"[iteration-chain] edge {name}/{env}: form {inf[9]} in use {inf[1]}")
        if env == "resident":
            assert (inf[9], inf[1]) == (1, 1), inf
        e.run_admm(1)
        x1, y1, z1, _, _ = e.download(False)
        st = e.stats()
        assert (st["admm_done"], st["pcg_forced"], st["neg_curvature"]) == (1, 0, 0), st
        _check_step(f"edge {name}/{env}", e, pb, o, 1.6, c["rho"], (x0, y0, z0), (x1, y1, z1))
        e.run_admm(1)
        _check_step(f"edge {name}/{env} second step", e, pb, o, 1.6, c["rho"], (x1, y1, z1), e.download(False)[:3])
    finally:
        e.close()
