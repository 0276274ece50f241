"""CPU tests of tests/_form_cases.py: each case is what it claims (the structure that selects its form and route, predicted from
(P, A) alone; the row classes; cond(K) <= 1e4 after ten Ruiz sweeps), the reference does not change with admm_step's `reuse`, and
the step bars are sharp: along the host-call sequence that tests/test_gpu_form_steps.py runs on the device, every one-place
defect of _form_cases.Sim.defects -- the old q in b, the old l, u in the clip, the old rho / P, A / sigma in K^-1, the old rho or
the old A in the m-part of the start vector only, z~ from before the call, v_n extrapolated with theta = 1 and v_m with 0.5,
x~ = K^-1 r without v_n -- misses the bars of _engine_reference.step_bars / _elim_cases.step_bars_elim by more than 10 x on at
least one element of x+, z+, y+.  A defect that a call cannot leave behind (the old q after a call that did not touch q) is not
counted.  The last test does the same for the defect the GPU module found: reset_start leaving the previous vector (vold) as it
was, seen one step later from a call that leaves the start vector alone."""
import time

import numpy as np
import pytest

from tests import _elim_cases as EC
from tests import _engine_reference as R
from tests import _form_cases as FC
from tests import _pcg_cases as PC

LD = R.LD
SCHED = (1, 2)


def _bars(c, cur, st, x, z, y, vn):
    kind = c["claims"]["bars"]
    if kind == "direct_inv":
        return R.step_bars(dict(st, plain_err=FC.inverse_residual_error(c, cur, st, x, z, y, vn)), FC.ALPHA, cur["rho"], True, FC.PCG_EPS)
    if kind == "direct_elim":
        pb = FC.problem(c, cur)
        erow, _ = EC.claimed(c)
        red = EC.reduced(pb, cur["sigma"], cur["rho"], erow, EC.rhs(pb, cur["sigma"], cur["rho"], x, z, y))
        return EC.step_bars_elim(pb, st, red, erow, cur["sigma"], FC.ALPHA, cur["rho"], FC.PCG_EPS, x, z, y, direct=True)
    return R.step_bars(st, FC.ALPHA, cur["rho"], kind == "direct", FC.PCG_EPS)


def _ratio(got, st, bars):
    return max(float((np.abs(np.asarray(g, dtype=LD) - st[k]).astype(float) / np.maximum(bars[k], 1e-300)).max()) for k, g in zip("xzy", got))


@pytest.mark.parametrize("name", FC.NAMES)
def test_case_is_what_it_claims(name):
    c = FC.make(name)
    cl = c["claims"]
    form = cl["form"]
    erow, _ = EC.eliminated(c["Pu"], c["A"])
    assert {int(j): int(erow[j]) for j in np.flatnonzero(erow >= 0)} == dict(cl.get("gone", {}))
    if form <= 2:
        s = PC.structure(c)
        got = dict(dense=len(s["dense"]), dense_rows=s["dense_rows"], long=len(s["long"]), huge=len(s["huge"]), folded=s["folded"], split=s["split"])
        want = cl.get("layout", {})
        assert {k: got[k] for k in want} == want, (name, got, want)
        if form == 2:                                # k_pcg_blockres: dense blocks only, a single-entry row per variable, every huge row folded
            bd = FC.bd_structure(c)
            assert bd["blocks"] == want["dense"] and bd["kc"] == 0 and bd["eligible"] and bd["folded"] == want["huge"], bd
        if form == 1:
            assert PC.RESIDENT[cl["E"]][4] == cl["nwg"] and c["n"] == PC.RESIDENT[cl["E"]][0]
    elif form == 3:
        bd = FC.bd_structure(c)
        assert bd["eligible"] and bd["blocks"] == cl["info"][3] and bd["kc"] == cl["info"][15], (name, bd)
        assert bd["folded"] == (cl["huge"] if cl["huge"] <= PC.MAX_HUGE_FOLD else 0)
        assert bd["fin_dots"] >= cl["fin_dots"] and (cl["fin_dots"] == bd["fin_dots"] or c["env"].get("OSQP_AMD_BLOCK_FIN_DOTS") == 0)
        assert cl["plain_rhs"] == c["env"].get("OSQP_AMD_BLOCK_PLAIN", 0)
        if name.startswith("f3_kc17"):               # a second 16-row group of k_blk_apply_multi
            assert bd["kc"] > 16
    else:
        dd = FC.dd_structure(c)
        assert (dd["na"], dd["nb2"]) == (cl["info"][3], cl["info"][15]) and dd["gone"] == dict(cl["gone"]) and dd["nd"] == cl["nd"], (name, dd)
        assert dd["vd"] == cl["vd"]
        if cl["symv"]:
            assert c["env"]["OSQP_AMD_DENSE_SYMV"] == 1 and dd["nap"] == {"f4_symv384": 384, "f4_symv1152": 1152}[name] and dd["nap"] < 2048
        elif not cl["vd"]:
            assert dd["nap"] == 128
    # row classes, consistent with rho
    l, u, rho = c["l"], c["u"], c["rho"]
    eq, free = l == u, (l < -1e20) & (u > 1e20)
    assert np.all(rho[eq] == 1e3 * FC.RHO) and np.all(free[rho == FC.RHO_MIN]) and np.all(l <= u)
    assert eq.any() and (~eq & ~free).any() and (free.any() or name == "f0_long_split")
    # conditioning, after the reference's ten Ruiz sweeps
    cur = FC.scaled(c)
    cond = FC.cond_K(c, cur)
    print(f"[form-cases] {name}: form {form} n {c['n']} m {c['m']} cond(K) after Ruiz {cond:.2e} claims {cl['info']}")
    assert cond <= FC.COND_CAP, (name, cond)


def test_reuse_does_not_change_the_reference_step():
    c = FC.make("f4_b2")
    cur = FC.scaled(c)
    pb = FC.problem(c, cur)
    x, y, z = R.iterates(c)
    keep = {}
    for k in range(2):
        a = R.admm_step(pb, cur["sigma"], FC.ALPHA, cur["rho"], x, z, y)
        b = R.admm_step(pb, cur["sigma"], FC.ALPHA, cur["rho"], x, z, y, reuse=keep)
        assert all(np.array_equal(a[key], b[key]) for key in a), k
        x, z, y = (a[key].astype(float) for key in "xzy")
    assert set(keep) == {"kkt", "lam_min"}


def _walk(name, order, stale=None):
    """The model along one order of host calls: yields (op, sim, old, reference step, bars) before each step is taken."""
    c = FC.make(name)
    rng = np.random.default_rng(40 + order)
    sim = FC.Sim(c, FC.scaled(c), SCHED)
    x, y, z = R.iterates(c)
    sim.set_iterates(x, y, z)
    for _ in range(3):
        sim.step()
    for k, op in enumerate(FC.orders(c)[order]):
        data, it = FC.op_changes(op, c, sim.cur, (sim.x, sim.y, sim.z), rng)
        old = sim.apply(op, data, it, stale_vold=stale is not None and op in stale)
        st = R.admm_step(FC.problem(c, sim.cur), sim.cur["sigma"], FC.ALPHA, sim.cur["rho"], sim.x, sim.z, sim.y)
        yield op, sim, old, st, _bars(c, sim.cur, st, sim.x, sim.z, sim.y, sim.vn)
        sim.step()


@pytest.mark.parametrize("name", FC.NAMES)
def test_bars_see_each_one_place_defect(name):
    t = time.time()
    worst_none, table = 0.0, {}
    for op, sim, old, st, bars in _walk(name, 0):
        none = _ratio(sim.solve_step()[:3], st, bars)
        worst_none = max(worst_none, none)
        assert none <= 1.0, (name, op, "the model without a defect misses the bar", none)
        for label, got in sim.defects(old).items():
            r = _ratio(got, st, bars)
            table.setdefault(label, []).append((r, op))
            assert r > 10.0, (name, op, label, r)
    for label, v in table.items():
        r, op = min(v)
        print(f"[form-cases] {name}: {label}: counted after {len(v)} calls, smallest miss {r:.2e} x bar (after {op})")
    print(f"[form-cases] {name}: the model without a defect: worst err/bar {worst_none:.2e}; {time.time() - t:.1f} s")
    want = {"old q in b", "old rho in K^-1", "old P, A in K^-1", "old rho in v_m", "old A in v_m", "z~ from before the call",
            "v_n with theta 1, v_m with 0.5", "x~ = K^-1 r without v_n"}
    if not FC.make(name)["claims"]["large"]:
        want |= {"old l, u in the clip", "old sigma in K^-1"}
    assert want <= set(table), (name, want - set(table))


@pytest.mark.parametrize("name", FC.PER_FORM)
def test_bars_see_a_previous_vector_from_before_the_call(name):
    """reset_start that leaves vold as it was: with OSQP_AMD_EXTRAP_SCHED=1,2 the first k_admm_finalize after a call that changed
    rho or A extrapolates with theta = 0.5 from a vector formed with the old rho / A, so the m-part of the next start vector is
    not rho A times its n-part; a call that leaves the start vector alone (q, bounds, sigma) then steps from it."""
    seen = 0
    order = FC.orders(FC.make(name))[0]
    after = {order[k + 1]: order[k] for k in range(len(order) - 1) if order[k] in ("rho", "matrices", "bounds+rho") and order[k + 1] in ("q", "bounds", "sigma")}
    prev = None
    for op, sim, old, st, bars in _walk(name, 0, stale=("rho", "matrices", "bounds+rho")):
        if prev in ("rho", "matrices", "bounds+rho") and after.get(op) == prev:
            r = _ratio(sim.solve_step()[:3], st, bars)
            print(f"[form-cases] {name}: vold from before {prev}, seen by the step after {op}: {r:.2e} x bar")
            assert r > 10.0, (name, prev, op, r)
            seen += 1
        prev = op
    assert seen >= 2
