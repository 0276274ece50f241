"""CPU checks of tests/_engine_reference.py, the reference the kernel-level GPU tests of the engine compare with
(tests/test_gpu_engine_kernels.py):

  * against the CPU oracle: D, E, c and the scaled data after set-up, and info.pri_res / dua_res / obj_val after a fixed number
    of iterations.  The oracle works in float64 in the same order as the device kernels, so the bars are the reference's own
    (R U relative for the Ruiz outputs, the dot-product bounds for the scalars), doubled where both sides round;
  * on every case of the GPU tests, from the same generator: the reference stays inside its own conditions -- clip thresholds and
    the infinite-bound threshold at least 1e-3 / 1e-9 relative away, every row of the A dx test decided beyond its rounding bound,
    lam_min(K) > 0, every kind of row clamped below, above and left free.  A case that misses one gets another seed in
    _engine_reference.SEEDS; nothing is excused on the device."""
import numpy as np
import pytest

from tests import _engine_reference as R
from tests.conftest import load_golden

U = R.U


def _problems():
    from osqp_amd.problems import random_sparse_qp
    pb, _ = load_golden("basic_qp")
    return [("basic_qp", pb), ("random 30x50", random_sparse_qp(30, 50, seed=11)), ("random 120x90", random_sparse_qp(120, 90, seed=12))]


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=R.LD), np.asarray(ref, dtype=R.LD)
    den = np.where(ref == 0, 1, np.abs(ref))
    return float((np.abs(a - ref) / den).max()) if a.size else 0.0


@pytest.mark.parametrize("which", [0, 1, 2])
def test_ruiz_against_oracle_setup(oracle_mod, which):
    from scipy import sparse
    name, pb = _problems()[which]
    s = oracle_mod.OracleOSQP().setup(**pb, scaling=10)
    w, n, m = s.work, s.n, s.m
    Pu, A = sparse.triu(sparse.csc_matrix(pb["P"]), format="csc"), sparse.csc_matrix(pb["A"])
    Pu.sort_indices(); A.sort_indices()
    l, u = np.maximum(pb["l"], -1e30), np.minimum(pb["u"], 1e30)
    r = R.ruiz(Pu, A, pb["q"], l, u, 10)
    assert r["margin"] >= 1e-3, r["margin"]
    d, sc = w.data.contents, w.scaling.contents
    got = dict(D=s._vec(sc.D, n), E=s._vec(sc.E, m), c=np.array([sc.c]), q=s._vec(d.q, n), l=s._vec(d.l, m), u=s._vec(d.u, m),
               Px=s._vec(d.P.contents.x, Pu.nnz), Ax=s._vec(d.A.contents.x, A.nnz))
    for k, v in got.items():
        err = _rel(v, np.atleast_1d(r[k]))
        print(f"[engine-ref] {name} {k}: rel err {err / U:.1f} U, R {r['R'][k]}")
        assert err <= r["R"][k] * U, (name, k, err / U, r["R"][k])


@pytest.mark.parametrize("which", [0, 1, 2])
def test_residual_scalars_against_oracle_info(oracle_mod, which):
    from scipy import sparse
    name, pb = _problems()[which]
    s = oracle_mod.OracleOSQP().setup(**pb, scaling=10, max_iter=6, adaptive_rho=0, polish=0, eps_abs=1e-30, eps_rel=1e-30)
    res = s.solve()
    assert res.info.iter == 6
    w, n, m = s.work, s.n, s.m
    d, sc = w.data.contents, w.scaling.contents
    Pu, A = sparse.triu(sparse.csc_matrix(pb["P"]), format="csc"), sparse.csc_matrix(pb["A"])
    Pu.sort_indices(); A.sort_indices()
    Pu.data, A.data = s._vec(d.P.contents.x, Pu.nnz), s._vec(d.A.contents.x, A.nnz)
    prob = R.Problem(Pu, A, s._vec(d.q, n), s._vec(d.l, m), s._vec(d.u, m), s._vec(sc.D, n), s._vec(sc.E, m))
    x, z, y = s.iterates()
    val, bar, _ = R.residual_scalars(prob, x, y, z, np.zeros(n), np.zeros(m))
    cinv = 1.0 / sc.c
    for what, ref, b, got in (("pri_res", val["pri_res_u"], bar["pri_res_u"], res.info.pri_res),
                              ("dua_res", cinv * val["dua_res_u"], cinv * bar["dua_res_u"], res.info.dua_res),
                              ("obj_val", cinv * val["obj_scaled"], cinv * bar["obj_scaled"], res.info.obj_val)):
        tol = 2.0 * b + 4 * U * abs(ref)
        print(f"[engine-ref] {name} {what}: |oracle - ref| {abs(got - ref):.2e} tol {tol:.2e}")
        assert abs(got - ref) <= tol, (name, what, got, ref, tol)


def _passes(name):
    return (1,) if name.startswith("scales") else (0, 1, 10)


@pytest.mark.parametrize("name", R.CASES)
def test_case_scaling_conditions(name):
    """Clip thresholds and the infinite-bound threshold: nothing computed comes near them."""
    case = R.make_case(name)
    for p in _passes(name):
        r = R.ruiz(case["Pu"], case["A"], case["q"], case["l"], case["u"], p)
        assert r["margin"] >= 1e-3, (name, p, r["margin"])
        if p:
            assert min(R.bound_margin(r["l"]), R.bound_margin(r["u"])) >= 1e-9, (name, p)
    # the largest entry of the long and huge rows sits where the generator says: lane 63, lane 0 of a later turn, the row's end
    for which, row, offset in case["peaks"]:
        assert R.peak_offset(case, which, row) == offset, (name, which, row)
    if name in ("long", "huge"):
        assert {o % 64 for _, _, o in case["peaks"]} >= {63} and any(o % 64 not in (0, 63) for _, _, o in case["peaks"])
    if name == "bounds":
        r = R.ruiz(case["Pu"], case["A"], case["q"], case["l"], case["u"], 1)
        assert float(r["E"][5]) == pytest.approx(1e-2, rel=1e-12) and abs(float(r["u"][5])) == pytest.approx(1e25, rel=1e-12)
        l, u = case["l"], case["u"]
        assert (l[5], u[5]) == (-1e27, 1e27)
        for b in (1e25, 1e26):            # finite large bounds on both sides, as given; 1e26 also next to an infinite one
            assert (l == -b).any() and (u == b).any(), b
        assert ((l == -1e26) & (u == 1e30)).any() and ((l == -1e30) & (u == 1e26)).any()
        assert (l == u).sum() >= 5 and ((l == -1e30) & (u == 1e30)).sum() >= 5
    if name == "empty":
        r = R.ruiz(case["Pu"], case["A"], case["q"], case["l"], case["u"], 10)
        assert np.all(r["D"][case["special_cols"]] == 1) and np.all(r["E"][10:2071] == 1)      # norm 0 -> 1
    if name == "scales":
        r = R.ruiz(case["Pu"], case["A"], case["q"], case["l"], case["u"], 1)
        assert [float(v) for v in r["E"][:6]] == pytest.approx([1.0, 100.0, 0.01, 0.01, 1.0, 0.01], rel=1e-15)
    if name == "scales_p0":
        r = R.ruiz(case["Pu"], case["A"], case["q"], case["l"], case["u"], 1)
        assert float(r["c"]) == 1.0                      # P = 0 and a tiny q: both norms clipped to 1


STEP_CASES = [n for n in R.CASES if not n.startswith("scales")]


@pytest.mark.parametrize("name", STEP_CASES)
def test_case_step_and_certificate_conditions(name):
    """lam_min(K) > 0, the A dx rows decided, and on `bounds` every kind of row clamped below, above and free."""
    case = R.make_case(name)
    x, y, z = R.iterates(case)
    for p in (0, 10):
        pb, _ = R.scaled_problem(case, p)
        for alpha in (1.0, 1.6):
            st = R.admm_step(pb, R.SIGMA, alpha, case["rho"], x, z, y)
            assert st["lam_min"] > 0.0
            bars = R.step_bars(st, alpha, case["rho"], False, 1e-12)
            assert np.all(np.isfinite(bars["x"]))
            if case["m"] == 0:
                continue
            _, _, dyp = R.residual_scalars(pb, st["x"], st["y"], st["z"], st["dx"], st["dy"].astype(float))
            for un in (0, 1):
                for eps in R.eps_pair(pb, st["dx"], un):
                    _, _, count, gap = R.certificate_scalars(pb, st["dx"], dyp, eps, un)
                    assert gap > 0.0, (name, p, alpha, un, eps, gap)
            if name == "bounds":
                v, l, u = st["v"], pb.l, pb.u
                fin_l, fin_u = ~pb.inf_l, ~pb.inf_u
                kinds = dict(both=fin_l & fin_u & (l < u), lower=fin_l & ~fin_u, upper=~fin_l & fin_u)
                for kname, k in kinds.items():
                    got = dict(below=(k & (v < l)).any(), above=(k & (v > u)).any(), free=(k & (v > l) & (v < u)).any())
                    want = dict(both=("below", "above", "free"), lower=("below", "free"), upper=("above", "free"))[kname]
                    assert all(got[t] for t in want), (kname, got, p, alpha)
                assert (l == u).sum() >= 5 and (pb.inf_l & pb.inf_u).sum() >= 5
                assert v[0] == l[0] and v[1] == u[1]                 # lands exactly on a bound
                assert (st["dy"].astype(float) == 0).any()


def test_bounds_delta_y_signs():
    """On the iterates the GPU residual test uses (alpha 1.6, no sweep and ten): delta_y of both signs on every kind of row of
    `bounds` -- both bounds finite, only l, only u, equality, free -- and delta_y == 0, so that a swapped fmin / fmax in the
    projection changes the projected vector on the device.  (k_admm_finalize forms delta_y = rho (w - z+) with rho > 0: a zero is
    always +0.0 there, and the shim has no call that sets delta_y, so -0.0 is tried on the reference's projection alone.)"""
    case = R.make_case("bounds")
    x, y, z = R.iterates(case)
    for p in (0, 10):
        pb, _ = R.scaled_problem(case, p)
        dy = R.admm_step(pb, R.SIGMA, 1.6, case["rho"], x, z, y)["dy"].astype(float)
        fin_l, fin_u = ~pb.inf_l, ~pb.inf_u
        kinds = dict(both=fin_l & fin_u & (pb.l < pb.u), lower=fin_l & ~fin_u, upper=~fin_l & fin_u, equality=pb.l == pb.u,
                     free=~fin_l & ~fin_u)
        for kname, k in kinds.items():
            assert (dy[k] > 0).any() and (dy[k] < 0).any(), (kname, p, dy[k])
        assert (dy == 0).any()
        proj = pb.project_dy(dy)
        # only l finite: u is infinite, the cone keeps delta_y <= 0; only u finite: delta_y >= 0
        assert np.array_equal(proj[kinds["lower"]], np.minimum(dy[kinds["lower"]], 0)) and (proj[kinds["free"]] == 0).all()
        assert np.array_equal(proj[kinds["upper"]], np.maximum(dy[kinds["upper"]], 0))
        assert np.array_equal(proj[kinds["both"] | kinds["equality"]], dy[kinds["both"] | kinds["equality"]])
    mz = np.full(case["m"], -0.0)
    assert np.all(pb.project_dy(mz) == 0.0) and np.all(pb.project_dy(-mz) == 0.0)
