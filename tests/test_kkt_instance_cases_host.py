"""CPU proof of tests/_kkt_instance_cases.py, the cases tests/test_gpu_kkt_instance_forms.py runs on the device (no GPU).

For every case:
  structure    the instance's form and slots, stated by hand in WANT below, follow from the host restatements applied to
               (P, A[active rows]) (instance_claims: _form_cases.bd_structure / dd_structure, _pcg_cases.structure,
               _elim_cases.eliminated, in the order of hipeng_create); where the case says the instance differs from the main
               engine, the same restatement applied to (P, A) gives another value.
  planting     x*, y* satisfy the KKT conditions to 1e-12, strict complementarity holds with 0.5 on both sides, the active rows
               are independent by construction (peels) with sigma_min / sigma_max >= 1e-2, M is nonsingular (the refined solve
               returns the planted point to 1e-12), and the CPU oracle with polish = 1 ends solved, polished, on the planted
               active set -- at the default eps_abs = eps_rel = 1e-3 for every case.
  route        with the oracle's D, E, c, _single_sens_reference.route_solve / scaled_adjoint / scaled_tangent reproduce every
               output of the truth to 1e-10 (relative to max(1, |truth|_inf)): the bound tests/test_single_sens_host.py proves
               for the members already run, so the device's parity bar 1e-6 excuses nothing.
  conditioning cond_2(P~ + d I + A~r' A~r / d), d = 1e-3, equals the module's table to 2 %, and on the PCG forms (0, 1, 2) lies
               at or below COND_CAP -- the largest value of the same quantity over the members tests/test_gpu_single_sens.py
               already runs on the PCG paths, recomputed here -- so no new case is harder for CG than what already passes.
  sensitivity  a relative change of 1e-4 to one value of P, to one value of an active row of A, or one active row dropped
               moves at least one output by more than ten times the parity bar."""
import numpy as np
import pytest
from scipy import sparse

import _kkt_instance_cases as KI
import _planted_qp as pq
import _single_sens_reference as sr
from _adjoint_reference import active_set
from _batch_parity import oracle, oracle_ws, rel

LD = np.longdouble
BAR = 1e-6

# name: (form, info slots, layout slots, eliminated variables) of the instance, by hand
WANT = {
    "ki_f0_blocks": (0, {1: 0}, dict(dense=8, dense_rows=608), 0),
    "ki_f0_long_on": (0, {1: 0}, dict(long=1), 0),
    "ki_f0_long_off": (0, {1: 0}, dict(long=0), 0),
    "ki_f1_e8": (1, {}, dict(dense=0, long=0), 0),
    "ki_f1_e20": (1, {}, dict(dense=0, long=0), 0),
    "ki_f2_nh0": (2, {2: 64}, dict(dense=2, dense_rows=64, huge=0), 0),
    "ki_f3_plain": (3, {3: 5, 15: 0}, {}, 0),
    "ki_f3_kc16": (3, {3: 5, 15: 16}, {}, 0),
    "ki_f3_kc17": (3, {3: 5, 15: 17}, {}, 0),
    "ki_f3_kc0": (3, {3: 5, 15: 0}, {}, 0),
    "ki_f3_huge1": (3, {3: 64, 15: 0}, dict(huge=1, folded=1), 0),
    "ki_f0_huge1": (0, {1: 0}, dict(dense=64, dense_rows=8192, huge=1, folded=1), 0),
    "ki_f4_b2": (4, {3: 100, 15: 3}, {}, 1),
    "ki_f4_slack": (4, {3: 100, 15: 0}, {}, 10),
    "ki_mred0": (0, {1: 0}, dict(dense=0), 0),
    "ki_all_eq": (4, {3: 100, 15: 0}, {}, 0),
}
# what `differs` names: where the value sits in instance_claims' result
DIFFERS = dict(form=lambda d: d["form"], long=lambda d: d["layout"]["long"], kc=lambda d: d["info"].get(15), na=lambda d: d["info"].get(3),
               nd=lambda d: d.get("nd"), elim=lambda d: d["elim"])
MUST_DIFFER = {"ki_f0_long_off": ("long",), "ki_f3_kc16": ("kc",), "ki_f3_kc17": ("kc",), "ki_f3_kc0": ("kc",), "ki_f3_huge1": ("kc",),
               "ki_f4_b2": ("na", "nd", "elim"), "ki_mred0": ("form",)}


def test_every_case_is_listed():
    assert set(WANT) == set(KI.NAMES) == set(KI.COND) and set(KI.LARGE) <= set(KI.NAMES)


@pytest.mark.parametrize("name", KI.NAMES)
def test_structure(name):
    c = KI.make(name)
    form, info, layout, elim = WANT[name]
    cl = c.claims
    assert cl["form"] == form and cl["elim"] == elim, (name, cl)
    assert {k: cl["info"].get(k) for k in info} == info and {k: cl["layout"][k] for k in layout} == layout, (name, cl)
    assert set(c.differs) == set(MUST_DIFFER.get(name, ())), (name, c.differs)
    for key in c.differs:
        assert DIFFERS[key](cl) != DIFFERS[key](c.main), (name, key, cl, c.main)
    if name == "ki_f0_long_on":
        assert c.act[0][0] != 0 and np.diff(sparse.csr_matrix(c.A).indptr)[0] >= 512
    if name in ("ki_f3_kc16", "ki_f3_kc17", "ki_f3_kc0"):
        assert c.main["info"][15] == KI.KC_MAIN == 33 and c.main["form"] == 3
    if name == "ki_f3_plain":                    # only single-block rows exist at all
        assert np.diff(sparse.csr_matrix(c.A).indptr).max() == 1
    if name == "ki_f4_slack":                    # every slack row is an equality, and the main engine eliminates the ten as well
        slack = np.arange(c.m - 10, c.m)
        assert np.all(c.act[0][slack] != 0) and np.array_equal(c.L[0][slack], c.U[0][slack]) and c.main["elim"] == 10
        assert np.all(c.P.diagonal()[-10:] == 0.0) and np.all(np.diff(c.P.indptr)[-10:] == 1)      # pyy = 0, stored
    if name == "ki_mred0":
        assert not c.act[0].any() and c.rows.size == 0 and not c.y[0].any() and c.main["form"] == 4
    if name == "ki_all_eq":
        assert c.m <= c.n and np.all(c.act[0] != 0) and np.array_equal(c.L[0], c.U[0]) and cl == c.main
    if c.large:                                  # both grid-stride loops of csrc/kkt_sens.h run more than one turn
        assert c.n == 8192 and (c.n + c.m) / (KI.TB // 64) > KI.MAX_PARTS and c.P.nnz > KI.MAX_PARTS * KI.TB
        lenA = np.diff(sparse.csr_matrix(c.A).indptr)
        assert c.act[0][c.n] != 0 and c.L[0][c.n] == c.U[0][c.n] and lenA[c.n] == 8192
    if name == "ki_f3_huge1":
        assert c.A.nnz > KI.MAX_PARTS * KI.TB and c.main["layout"]["huge"] == KI.HUGE_MAIN


@pytest.mark.parametrize("name", KI.NAMES)
def test_planting(oracle_mod, name):
    c, t = KI.make(name), KI.truth(name)
    mem = t.mem
    x, y, act = c.x[0], c.y[0], c.act[0]
    # KKT at the planted point, residual in long double, relative to the largest term
    s = np.concatenate([x, y[mem.rows]])
    g = np.concatenate([-mem.q, mem.l[mem.low], mem.u[mem.upp]])
    r = float(np.abs(t.route.residual_ld(s, g)).max())
    assert r <= 1e-12 * max(1.0, float(np.abs(g).max())), (name, r)
    assert np.array_equal(np.sign(y).astype(np.int64), act)
    assert rel(t.x, x) <= 1e-12 and rel(t.y, y) <= 1e-12, (name, rel(t.x, x), rel(t.y, y))       # M is nonsingular: the solve finds the point
    ax = np.asarray(mem.Ad @ x).ravel()
    if act.any():
        assert np.abs(y[act != 0]).min() >= 0.5
    eq = mem.l == mem.u
    gap_l = np.where((act < 0) | eq, np.inf, ax - mem.l)
    gap_u = np.where((act > 0) | eq, np.inf, mem.u - ax)
    if c.m:
        assert min(gap_l.min(), gap_u.min()) >= 0.5 - 1e-12, (name, gap_l.min(), gap_u.min())
    k = mem.rows.size
    if k:
        assert k <= c.n and KI.peels(c.A, mem.rows), name
        Ar = sparse.csr_matrix(mem.Ad)[mem.rows]
        if c.large:                              # through the Gram matrix (k = 2731): the ratio is far from the rounding of its square
            w = np.linalg.eigvalsh((Ar @ Ar.T).toarray())
            ratio = float(np.sqrt(w[0] / w[-1]))
        else:
            sv = np.linalg.svd(Ar.toarray(), compute_uv=False)
            ratio = float(sv.min() / sv.max())
        assert ratio >= 1e-2, (name, ratio)
    kinds = {(int(a), "eq" if lo == hi else (bool(np.isfinite(lo)), bool(np.isfinite(hi)))) for a, lo, hi in zip(act, mem.l, mem.u)}
    if k >= 6 and name != "ki_all_eq":           # the kinds in turn: equality, one-sided and two-sided active rows all occur
        assert {v for a, v in kinds if a != 0} >= {"eq", (True, True)} and len({v for a, v in kinds if a != 0}) >= 3, (name, kinds)
    # the CPU oracle: solved, polished, on the planted set (default eps_abs = eps_rel: no case needs a tighter one)
    assert "eps_abs" not in c.settings and "eps_rel" not in c.settings
    ro = oracle(oracle_mod, **sr.member_qp(c, 0), polish=1, **c.settings).solve()
    assert ro.info.status_val == 1 and ro.info.status_polish == 1, (name, ro.info.status_val, ro.info.status_polish)
    assert np.array_equal(active_set(ro.y)[2], act), name
    assert rel(ro.x, t.x) < BAR and rel(ro.y, t.y) < BAR
    print(name, "mred %d iter %d oracle x %.1e y %.1e" % (k, ro.info.iter, rel(ro.x, t.x), rel(ro.y, t.y)))


def _scaled(orc, c):
    ws = oracle_ws(oracle(orc, **sr.member_qp(c, 0), polish=1, **c.settings))
    return np.asarray(ws["D"], float), np.asarray(ws["E"], float).reshape(c.m), float(ws["c"])


def _route_outputs(c, t, D, E, cs):
    """Every output through the route model on the scaled data, at the truth's point for the derivatives (as
    test_single_sens_host.py takes them); also the scaled matrices."""
    mem, inc = t.mem, pq.member_inc(c, 0)
    Pfs, Ads, rows = sr.scaled_problem(mem.Pu, mem.Ac, mem.act, D, E, cs, dense=not mem.sparse)
    assert np.array_equal(rows, mem.rows)
    Ars = Ads[rows]
    solve = lambda g: sr.route_solve(Pfs, Ars, g)[0]
    s = solve(np.concatenate([-(cs * D * mem.q), (E * mem.l)[mem.low], (E * mem.u)[mem.upp]]))
    x = D * s[:c.n]
    y = np.zeros(c.m); y[rows] = E[rows] * s[c.n:] / cs
    a = sr.scaled_adjoint(mem.Pu, mem.Ac, mem.act, D, E, cs, t.x, t.y, inc.gx, inc.gy, solve)
    tn = sr.scaled_tangent(mem.Pu, mem.Ac, mem.act, D, E, cs, t.x, t.y, inc.dQ, inc.dL, inc.dU, inc.dPx, inc.dAx, solve, keep_sparse=mem.sparse)
    return pq.SimpleNamespace(x=x, y=y, obj=np.array([pq._obj(mem, x)]), **vars(a), **vars(tn)), Pfs, Ars


@pytest.mark.parametrize("name", KI.NAMES)
def test_route_and_conditioning(oracle_mod, name):
    c, t = KI.make(name), KI.truth(name)
    D, E, cs = _scaled(oracle_mod, c)
    if c.settings.get("scaling", 10):
        assert not np.allclose(D, 1.0)
    got, Pfs, Ars = _route_outputs(c, t, D, E, cs)
    errs = {k: rel(getattr(got, k), getattr(t, k)) for k in KI.OUTPUTS}
    cond = KI.cond_reduced(Pfs, Ars)
    print(name, "route worst %.2e (%s) cond %.3e (table %.3e, cap %.3e)" % (max(errs.values()), max(errs, key=errs.get), cond, KI.COND[name], KI.COND_CAP))
    assert max(errs.values()) <= 1e-10, (name, errs)
    assert abs(cond - KI.COND[name]) <= 0.02 * KI.COND[name], (name, cond, KI.COND[name])
    if c.claims["form"] in (0, 1, 2):
        assert cond <= KI.COND_CAP, (name, cond, KI.COND_CAP)


def test_conditioning_cap(oracle_mod):
    """COND_CAP is the largest cond_2(P~ + d I + A~r' A~r / d) over the members the suite already differentiates on the PCG
    paths: every planted member of _single_sens_reference.PLANTED_MEMBERS and its random sparse QP (active rows: the oracle's
    polished point)."""
    from osqp_amd.problems import random_sparse_qp
    seen = {}
    for name, b in sr.PLANTED_MEMBERS:
        c = pq.case(name)
        mem = pq.member(c, b)
        ws = oracle_ws(oracle(oracle_mod, **sr.member_qp(c, b), polish=1))
        Pfs, Ads, rows = sr.scaled_problem(mem.Pu, mem.Ac, mem.act, np.asarray(ws["D"], float), np.asarray(ws["E"], float).reshape(c.m), float(ws["c"]))
        seen[(name, b)] = KI.cond_reduced(Pfs, Ads[rows])
    pb = random_sparse_qp(sr.RANDOM_QP["n"], sr.RANDOM_QP["m"], seed=sr.RANDOM_QP["seed"])
    so = oracle(oracle_mod, polish=1, **pb)
    ws = oracle_ws(so)
    ro = so.solve()
    assert ro.info.status_val == 1 and ro.info.status_polish == 1
    Pu = sparse.triu(pb["P"], format="csc")
    Pfs, Ads, rows = sr.scaled_problem(Pu, sparse.csc_matrix(pb["A"]), active_set(ro.y)[2], np.asarray(ws["D"], float),
                                       np.asarray(ws["E"], float).reshape(-1), float(ws["c"]))
    seen[("random_qp", 0)] = KI.cond_reduced(Pfs, Ads[rows])
    worst = max(seen, key=seen.get)
    print("cond per member:", {k: "%.2e" % v for k, v in seen.items()}, "largest", worst)
    assert abs(seen[worst] - KI.COND_CAP) <= 0.02 * KI.COND_CAP, (worst, seen[worst], KI.COND_CAP)


@pytest.mark.parametrize("name", KI.NAMES)
def test_sensitivity(name):
    c, t = KI.make(name), KI.truth(name)
    muts = KI.mutations(c)
    assert len(muts) == (3 if c.act[0].any() else 1)
    for label, mem in muts:
        o = KI.outputs(c, mem)
        moved = {k: rel(getattr(o, k), getattr(t, k)) for k in KI.OUTPUTS}
        worst = max(moved, key=moved.get)
        print(name, label, "moves %s by %.2e" % (worst, moved[worst]))
        assert moved[worst] > 10.0 * BAR, (name, label, moved)
