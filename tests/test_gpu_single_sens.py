"""Derivatives of the solution on the single-QP engine (OSQP.adjoint / OSQP.tangent, osqp_amd_adjoint / osqp_amd_tangent,
osqp_amd.QPLayer; kernels k_sens_grad and k_sens_tan_rhs of csrc/kkt_sens.h).

References: the truth of tests/_planted_qp.py (a refined solve of the unregularised KKT system on the planted rows) for
the planted members run as single QPs; tests/_adjoint_reference.py and tests/_tangent_reference.py at the CPU oracle's
point elsewhere -- never the device's own numbers.  Bar: the project's parity bar, 1e-6 by _batch_parity.rel, for every
output of every member: tests/test_single_sens_host.py proves on the CPU that the route itself is within 1e-10 of the
truth on each of them, so none is excused.  Every test runs on the default linear solver (dense-direct at these sizes)
and on the PCG paths (`both_linear_solvers`).  Every error and kkt_res is printed."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _planted_qp as pq
import _single_sens_reference as sr
from _adjoint_reference import adjoint_reference
from _batch_parity import oracle, rel
from _tangent_reference import tangent_matrices, tangent_reference
from conftest import load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("both_linear_solvers")]

NOT_INIT, DATA_VALIDATION = 7, 1
GRADS, TANS = ("dq", "dl", "du", "dPx", "dAx"), ("dx", "dy")


def _handle(c, b, **kw):
    import osqp_amd
    return osqp_amd.OSQP().setup(**sr.member_qp(c, b), **{"polish": 1, **kw})


def _derivatives(h, c, b):
    """adjoint with both incoming gradients and the matrices, tangent with all five tangents and pq.NDIR directions."""
    i = pq.member_inc(c, b)
    return h.adjoint(i.gx, i.gy, matrices=True), h.tangent(i.dQ, i.dL, i.dU, i.dPx, i.dAx)


def _against_truth(what, c, b, r, a, t):
    tr = pq.truth(c, b)
    assert r.info.status_val == 1 and r.info.status_polish == 1, (what, r.info.status_val, r.info.status_polish)
    assert a.status_adjoint == 1 and t.status_tangent == 1, (what, a.status_adjoint, t.status_tangent)
    assert np.array_equal(a.active, c.act[b]) and np.array_equal(t.active, c.act[b]), (what, np.flatnonzero(a.active != c.act[b]))
    assert a.dPx.shape == (c.P.nnz,) and a.dAx.shape == (c.A.nnz,) and t.dx.shape == (pq.NDIR, c.n) and t.dy.shape == (pq.NDIR, c.m)
    errs = {g: rel(getattr(a, g), getattr(tr, g)) for g in GRADS}
    errs.update({g: rel(getattr(t, g), getattr(tr, g)) for g in TANS})
    print(what, "x %.1e y %.1e |" % (rel(r.x, tr.x), rel(r.y, tr.y)), " ".join("%s %.2e" % kv for kv in errs.items()),
          "| kkt_res adjoint %.1e tangent %s, active rows %d" % (a.kkt_res, " ".join("%.1e" % v for v in t.kkt_res), np.count_nonzero(a.active)))
    assert all(e < 1e-6 for e in errs.values()), (what, errs)
    return max(errs.values())


@pytest.mark.parametrize("name", ["one", "pad", "lp", "scan", "rows", "lds64k"])
def test_planted_members(gpu_lib, both_linear_solvers, name):
    """1. Every planted member of the case as a single QP with polish = 1: `active` is the planted set, the statuses are
    1, the five gradients and the two tangents (D = 2, all five tangents given) are within 1e-6 of the truth."""
    c = pq.case(name)
    worst = 0.0
    for b in [m for n_, m in sr.PLANTED_MEMBERS if n_ == name]:
        h = _handle(c, b)
        r = h.solve()
        a, t = _derivatives(h, c, b)
        info = h.sens_info()
        assert info["built"] == 1 and info["alive"] == 1 and info["active_rows"] == np.count_nonzero(c.act[b]), info
        worst = max(worst, _against_truth("%s[%d] %s" % (name, b, both_linear_solvers), c, b, r, a, t))
        h.cleanup()
    print(name, both_linear_solvers, "worst rel %.3e" % worst)


@pytest.mark.parametrize("scaling", [0, 10])
def test_scaling_folded(gpu_lib, both_linear_solvers, scaling):
    """2. The `pad` members without scaling and with ten Ruiz passes, against the same truth: the D, E, c folding."""
    c = pq.case("pad")
    for b in range(c.B):
        h = _handle(c, b, scaling=scaling)
        r = h.solve()
        sc = h.work.scaling
        assert bool(sc) == (scaling != 0)
        if scaling:
            assert not np.allclose(h._vec(sc.contents.D, c.n), 1.0) and sc.contents.c != 1.0
        _against_truth("pad[%d] scaling=%d %s" % (b, scaling, both_linear_solvers), c, b, r, *_derivatives(h, c, b))
        h.cleanup()


def test_without_polish(gpu_lib, oracle_mod, both_linear_solvers):
    """3. At the ADMM point (eps 1e-9, no polish), against the references at the oracle's unpolished x, y.  Bars as
    test_gpu_batch_adjoint._admm_bars and test_gpu_batch_tangent.test_without_polish derive them, from the parity bar of
    x, y and the reference's own quantities: 1e-6 for dq, dl, du; 1e-6 plus the bilinear terms for dPx, dAx; for the
    tangents 1e-6 + |M^-1|_inf 1e-6 (|dP|_inf max(1, |x|) + |dA'|_inf max(1, |y|) + |dA|_inf max(1, |x|)) relative to
    max(1, |[dx; dy]|_inf)."""
    from test_gpu_batch_adjoint import _admm_bars
    c = pq.case("pad")
    kw = dict(polish=0, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
    mx = lambda v: max(1.0, float(np.abs(v).max()) if np.size(v) else 0.0)
    ninf = lambda M: float(np.abs(M).sum(axis=1).max()) if M.size else 0.0
    fails = []
    for b in (1, 3):
        pb, i = sr.member_qp(c, b), pq.member_inc(c, b)
        ro = oracle(oracle_mod, **pb, **kw).solve()
        h = _handle(c, b, **kw)
        r = h.solve()
        assert r.info.status_val == ro.info.status_val == 1 and r.info.status_polish == 0
        assert rel(r.x, ro.x) < 1e-6 and rel(r.y, ro.y) < 1e-6
        a = h.adjoint(i.gx, i.gy, matrices=True)
        t = h.tangent(i.dQ[0], i.dL[0], i.dU[0], i.dPx[0], i.dAx[0])
        h.cleanup()
        ref = adjoint_reference(pb["P"], pb["A"], pb["l"], pb["u"], ro.x, ro.y, i.gx, i.gy)
        rt = tangent_reference(pb["P"], pb["A"], ro.x, ro.y, i.dQ[0], i.dL[0], i.dU[0], i.dPx[0], i.dAx[0])
        assert ref.margin >= 1e-6 and ref.sv_ratio >= 1e-8 and ref.route_err <= 1e-7 and rt.route_err <= 1e-7
        assert a.status_adjoint == 1 and t.status_tangent == 1
        assert np.array_equal(a.active, ref.active) and np.array_equal(t.active, ref.active)
        errs, bars = [rel(getattr(a, g), getattr(ref, g)) for g in GRADS], _admm_bars(ref, ro)
        dP, dA = tangent_matrices(pb["P"], pb["A"], i.dPx[0], i.dAx[0])
        scale = mx(np.concatenate([rt.dx, rt.dy]))
        tbar = 1e-6 + rt.minv_norm * 1e-6 * (ninf(dP) * mx(ro.x) + ninf(dA.T) * mx(ro.y) + ninf(dA) * mx(ro.x)) / scale
        te = max(np.abs(t.dx - rt.dx).max(), np.abs(t.dy - rt.dy).max()) / scale
        print("admm pad[%d] %s" % (b, both_linear_solvers), " ".join("%s %.2e (bar %.1e)" % z for z in zip(GRADS, errs, bars)),
              "tangent %.2e (bar %.1e) kkt_res %.1e %.1e" % (te, tbar, a.kkt_res, t.kkt_res))
        if not (all(e < w for e, w in zip(errs, bars)) and te < tbar):
            fails.append((b, errs, bars, te, tbar))
    assert not fails, fails


def _random_qp():
    from osqp_amd.problems import random_sparse_qp
    return random_sparse_qp(sr.RANDOM_QP["n"], sr.RANDOM_QP["m"], seed=sr.RANDOM_QP["seed"])


def _random_draws(pb):
    rng = np.random.default_rng(99)
    n, m = pb["A"].shape[1], pb["A"].shape[0]
    return SimpleNamespace(gx=rng.standard_normal(n), gy=rng.standard_normal(m), dq=rng.standard_normal((3, n)),
                           dl=rng.standard_normal((3, m)), du=rng.standard_normal((3, m)),
                           dPx=rng.standard_normal((3, pb["P"].nnz)), dAx=rng.standard_normal((3, pb["A"].nnz)))


def test_random_sparse_qp(gpu_lib, oracle_mod, both_linear_solvers):
    """4. The config-2 generator at n = 200, m = 400 against adjoint_reference / tangent_reference at the oracle's
    polished point (test_single_sens_host.py: the reference alone excuses nothing at this seed)."""
    import osqp_amd
    pb = _random_qp()
    d = _random_draws(pb)
    ro = oracle(oracle_mod, polish=1, **pb).solve()
    h = osqp_amd.OSQP().setup(**pb, polish=1)
    r = h.solve()
    assert r.info.status_val == 1 and r.info.status_polish == ro.info.status_polish == 1
    a = h.adjoint(d.gx, d.gy, matrices=True)
    t = h.tangent(d.dq, d.dl, d.du, d.dPx, d.dAx)
    h.cleanup()
    ref = adjoint_reference(pb["P"], pb["A"], pb["l"], pb["u"], ro.x, ro.y, d.gx, d.gy)
    assert a.status_adjoint == 1 and t.status_tangent == 1 and np.array_equal(a.active, ref.active) and np.array_equal(t.active, ref.active)
    errs = {g: rel(getattr(a, g), getattr(ref, g)) for g in GRADS}
    for k in range(3):
        rt = tangent_reference(pb["P"], pb["A"], ro.x, ro.y, d.dq[k], d.dl[k], d.du[k], d.dPx[k], d.dAx[k])
        assert rt.route_err <= 1e-7
        errs["dx%d" % k], errs["dy%d" % k] = rel(t.dx[k], rt.dx), rel(t.dy[k], rt.dy)
    print("random qp", both_linear_solvers, " ".join("%s %.2e" % kv for kv in errs.items()), "kkt_res %.1e" % a.kkt_res, t.kkt_res)
    assert all(e < 1e-6 for e in errs.values()), errs


@pytest.mark.parametrize("name,b", [("pad", 1), ("rows", 0), ("lp", 1)])
def test_duality_on_the_device(gpu_lib, both_linear_solvers, name, b):
    """5. gx . dx + gy . dy = dq_adj . dq + dl_adj . dl + du_adj . du + dPx_adj . dPx + dAx_adj . dAx, both sides from one
    handle.  Each side's terms are held to the parity bar 1e-6, so the two sides agree within 2e-6 times the sum of the
    absolute terms (the smaller of the two sides' sums is used)."""
    c = pq.case(name)
    i = pq.member_inc(c, b)
    h = _handle(c, b)
    h.solve()
    a, t = _derivatives(h, c, b)
    h.cleanup()
    assert a.status_adjoint == 1 and t.status_tangent == 1
    for k in range(pq.NDIR):
        left = [i.gx * t.dx[k], i.gy * t.dy[k]]
        right = [a.dq * i.dQ[k], a.dl * i.dL[k], a.du * i.dU[k], a.dPx * i.dPx[k], a.dAx * i.dAx[k]]
        lhs, rhs = sum(float(v.sum()) for v in left), sum(float(v.sum()) for v in right)
        bar = 2e-6 * min(sum(float(np.abs(v).sum()) for v in left), sum(float(np.abs(v).sum()) for v in right))
        print("duality %s[%d] %s direction %d: lhs %.12e rhs %.12e |lhs - rhs| %.2e (bar %.1e)"
              % (name, b, both_linear_solvers, k, lhs, rhs, abs(lhs - rhs), bar))
        assert abs(lhs - rhs) <= bar


def _state(h):
    w = h.work
    info = bytes(C.string_at(C.addressof(w.info.contents), C.sizeof(w.info.contents)))
    sol = w.solution.contents
    return dict(x=h._vec(w.x, h.n), y=h._vec(w.y, h.m), z=h._vec(w.z, h.m), sx=h._vec(sol.x, h.n), sy=h._vec(sol.y, h.m),
                rho=h._vec(w.rho_vec, h.m), info=info, stats=h.stats(), rho_setting=h.settings().rho)


def _info_no_times(r):
    return {k: v for k, v in vars(r.info).items() if not k.endswith("_time")}


def test_untouched(gpu_lib, both_linear_solvers):
    """6. The workspace before and after the calls, bit for bit (x, y, z, solution, the whole OSQPInfo, rho and
    osqp_amd_get_stats), and against a twin handle that made no derivative call (OSQPInfo without its wall-clock
    fields), a following warm-started solve included."""
    c, b = pq.case("pad"), 1
    h, twin = _handle(c, b), _handle(c, b)
    r, rt = h.solve(), twin.solve()
    before = _state(h)
    a0, t0 = _derivatives(h, c, b)
    a1, t1 = _derivatives(h, c, b)
    after, other = _state(h), _state(twin)
    for k in before:
        same = before[k] == after[k] if not isinstance(before[k], np.ndarray) else np.array_equal(before[k], after[k])
        assert same, k
        if k != "info":
            same = before[k] == other[k] if not isinstance(before[k], np.ndarray) else np.array_equal(before[k], other[k])
            assert same, ("twin", k)
    assert _info_no_times(r) == _info_no_times(rt)
    for k in GRADS + ("active", "status_adjoint", "kkt_res"):      # the second pair of calls reused the instance: same bits
        assert np.array_equal(getattr(a0, k), getattr(a1, k)), k
    for k in TANS + ("active", "status_tangent", "kkt_res"):
        assert np.array_equal(getattr(t0, k), getattr(t1, k)), k
    assert h.sens_info()["built"] == 1 and twin.sens_info() == dict(built=0, alive=0, active_rows=0, solves=0)
    r2, rt2 = h.solve(), twin.solve()                              # warm-started from what each handle holds
    assert np.array_equal(r2.x, rt2.x) and np.array_equal(r2.y, rt2.y) and _info_no_times(r2) == _info_no_times(rt2)
    assert h.stats() == twin.stats()
    # dy = None is dy = 0, and without matrices=True the matrix gradients are not computed
    i = pq.member_inc(c, b)
    a2, a3 = h.adjoint(i.gx), h.adjoint(i.gx, np.zeros(c.m), matrices=True)
    assert a2.dPx is None and a2.dAx is None
    for k in ("dq", "dl", "du", "active", "status_adjoint"):
        assert np.array_equal(getattr(a2, k), getattr(a3, k)), k
    h.cleanup(); twin.cleanup()


def test_directions_share_the_instance(gpu_lib, both_linear_solvers):
    """A direction's bits depend on neither ndir nor the other directions; a missing tangent is a tangent of zeros; [k]
    is [1, k]."""
    c, b = pq.case("rows"), 0
    i = pq.member_inc(c, b)
    h = _handle(c, b)
    h.solve()
    both = h.tangent(i.dQ, i.dL, i.dU, i.dPx, i.dAx)
    for k in range(pq.NDIR):
        one = h.tangent(i.dQ[k], i.dL[k], i.dU[k], i.dPx[k], i.dAx[k])
        assert one.dx.shape == (c.n,) and np.array_equal(one.dx, both.dx[k]) and np.array_equal(one.dy, both.dy[k])
        assert one.kkt_res == both.kkt_res[k]
    swapped = h.tangent(i.dQ[::-1], i.dL[::-1], i.dU[::-1], i.dPx[::-1], i.dAx[::-1])
    assert np.array_equal(swapped.dx[::-1], both.dx) and np.array_equal(swapped.dy[::-1], both.dy)
    part = h.tangent(dq=i.dQ, dAx=i.dAx)
    zeros = h.tangent(i.dQ, np.zeros_like(i.dL), np.zeros_like(i.dU), np.zeros_like(i.dPx), i.dAx)
    assert np.array_equal(part.dx, zeros.dx) and np.array_equal(part.dy, zeros.dy)
    none = h.tangent()
    assert none.status_tangent == 1 and not none.dx.any() and not none.dy.any()
    assert h.sens_info()["built"] == 1
    h.cleanup()


def test_cache_and_refusals(gpu_lib, both_linear_solvers):
    """7. One KKT instance per solved problem; refusals before a solve and after an update or a warm start; status 0
    and zero outputs where the solve did not end `solved`; the validation errors of the C entry points."""
    import osqp_amd
    c, b = pq.case("pad"), 1
    i = pq.member_inc(c, b)
    h = _handle(c, b)
    assert h.sens_info() == dict(built=0, alive=0, active_rows=0, solves=0)
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.adjoint(i.gx, i.gy)                                 # no solve yet
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.tangent(i.dQ)
    assert h.sens_info()["built"] == 0
    r = h.solve()
    h.adjoint(i.gx, i.gy, matrices=True)
    s1 = h.sens_info()
    three = h.tangent(np.stack([i.dQ[0], i.dQ[1], i.dQ[0]]))
    s2 = h.sens_info()
    assert three.status_tangent == 1 and np.array_equal(three.dx[0], three.dx[2])
    assert s1["built"] == s2["built"] == 1 and s2["alive"] == 1 and s2["active_rows"] == np.count_nonzero(c.act[b])
    assert s1["solves"] >= 4 and s2["solves"] >= s1["solves"] + 3 * 4      # at least the first solve and three refinement steps each
    assert h.update(q=c.Q[b] * 1.01) == 0
    assert h.sens_info()["alive"] == 0
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.adjoint(i.gx, i.gy)                                 # the data moved and no solve has run on it
    h.solve()
    assert h.adjoint(i.gx, i.gy).status_adjoint == 1
    assert h.sens_info()["built"] == 2 and h.sens_info()["alive"] == 1
    assert h.warm_start(x=r.x, y=r.y) == 0
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.tangent(i.dQ)
    h.solve()
    assert h.update_rho(0.3) == 0
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.adjoint(i.gx)
    h.solve()
    assert h.update(Ax=c.Ax_all[b]) == 0
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        h.adjoint(i.gx)
    h.solve()
    # a new delta drops the instance (it was built with the old one) but not the permission to call
    built = h.sens_info()["built"]
    assert h.adjoint(i.gx).status_adjoint == 1 and h.sens_info()["built"] == built + 1
    h.update_settings(delta=1e-2)
    assert h.sens_info()["alive"] == 0
    assert h.adjoint(i.gx).status_adjoint == 1 and h.sens_info()["built"] == built + 2
    # the C entry points' own validation (the Python methods check before they call)
    adj, tan, W = h._sens("adjoint"), h._sens("tangent"), C.POINTER(osqp_amd.abi.OSQPWorkspace)
    F, I = lambda v: osqp_amd.abi.fptr(v), lambda v: osqp_amd.abi.iptr(v)
    NF, NI = C.cast(None, osqp_amd.abi.c_float_p), C.cast(None, osqp_amd.abi.c_int_p)
    gx, dq, dl, du, dx = np.array(i.gx), np.zeros(c.n), np.zeros(c.m), np.zeros(c.m), np.zeros(c.n)
    st = np.zeros(1, np.int64)
    assert adj(W(), F(gx), NF, F(dq), F(dl), F(du), NF, NF, NI, I(st), NF) == NOT_INIT
    assert tan(W(), 1, NF, NF, NF, NF, NF, F(dx), NF, NI, I(st), NF) == NOT_INIT
    assert adj(h._work, NF, NF, F(dq), F(dl), F(du), NF, NF, NI, I(st), NF) == DATA_VALIDATION
    assert adj(h._work, F(gx), NF, NF, F(dl), F(du), NF, NF, NI, I(st), NF) == DATA_VALIDATION
    assert adj(h._work, F(gx), NF, F(dq), NF, F(du), NF, NF, NI, I(st), NF) == DATA_VALIDATION
    assert adj(h._work, F(gx), NF, F(dq), F(dl), NF, NF, NF, NI, I(st), NF) == DATA_VALIDATION
    assert tan(h._work, 1, NF, NF, NF, NF, NF, NF, NF, NI, I(st), NF) == DATA_VALIDATION
    assert tan(h._work, 0, NF, NF, NF, NF, NF, F(dx), NF, NI, I(st), NF) == DATA_VALIDATION
    assert tan(h._work, -2, NF, NF, NF, NF, NF, F(dx), NF, NI, I(st), NF) == DATA_VALIDATION
    assert tan(h._work, 65536, NF, NF, NF, NF, NF, F(dx), NF, NI, I(st), NF) == DATA_VALIDATION      # the documented limit, before anything is written
    assert adj(h._work, F(gx), NF, F(dq), F(dl), F(du), NF, NF, NI, I(st), NF) == 0 and st[0] == 1 and dq.any()
    assert tan(h._work, 1, NF, NF, NF, NF, NF, F(dx), NF, NI, I(st), NF) == 0 and st[0] == 1 and not dx.any()
    h.cleanup()
    # not solved: status 0, zero outputs, no instance
    pb, _ = load_golden("primal_infeasibility")
    rng = np.random.default_rng(3)
    for what, hh in (("primal infeasible", osqp_amd.OSQP().setup(**pb, max_iter=10000, alpha=1.6, scaling=0, polish=1)),
                     ("max_iter", _handle(c, b, max_iter=5))):
        rr = hh.solve()
        assert rr.info.status_val != 1, what
        a = hh.adjoint(rng.standard_normal(hh.n), rng.standard_normal(hh.m), matrices=True)
        t = hh.tangent(dq=rng.standard_normal((2, hh.n)))
        assert a.status_adjoint == 0 and t.status_tangent == 0, what
        for k in GRADS + ("active",):
            assert not np.any(getattr(a, k)), (what, k)
        assert not t.dx.any() and not t.dy.any() and not t.active.any() and a.kkt_res == 0.0
        assert hh.sens_info() == dict(built=0, alive=0, active_rows=0, solves=0), what
        hh.cleanup()


def test_layer(gpu_lib, both_linear_solvers, tmp_path):
    """8. osqp_amd.QPLayer on the `pad` member, with CPU tensors and with CUDA tensors: the backward pass and the
    forward_ad tangents equal adjoint() / tangent() of a plain handle to the bit.  The layer runs in a child process
    (tests/_single_layer_worker.py says why); the comparison is made here."""
    c, b = pq.case("pad"), 1
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_single_layer_worker.py")
    p = subprocess.run([sys.executable, worker, "pad", str(b), str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = dict(np.load(tmp_path / "out.npz"))
    assert list(got["status"]) == [1, 1, 1, 1]
    tr = pq.truth(c, b)
    assert rel(got["dq"], tr.dq) < 1e-6 and rel(got["dx"], tr.dx[0]) < 1e-6       # the plain handle itself is right
    for dev in ("cpu", "cuda"):
        assert list(got[dev + "_status"]) == [1, 1] and int(got[dev + "_status_tangent"]) == 1 and bool(got[dev + "_q_only"])
        for k in ("x", "y") + GRADS + TANS:
            assert np.array_equal(got["%s_%s" % (dev, k)], got[k]), (dev, k, np.abs(got["%s_%s" % (dev, k)] - got[k]).max())
