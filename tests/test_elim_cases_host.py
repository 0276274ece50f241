"""CPU checks of the cases of tests/_elim_cases.py (no device): each case is what it claims, the bars that
tests/test_gpu_elim_edges.py puts on an eliminated step are sharp, the reference they are held against is better than they
are, and they fail when the model of the eliminated step is wrong in one place.

  claims      eliminated(), the restatement of build_elim's rule, gives exactly claims['gone'], and every variable is either
              there or in claims['stay']; the stated shapes (row lengths, offsets of the eliminated entry, stored zeros) hold
  sharp       on the problem after 10 Ruiz sweeps of the reference, pcg_eps_rel = 1e-12, alpha = 1.0 and 1.6: lam_min(S) > 0 and the
              bar on x~_X is at most 1e-8 ||x~||_2
  reference   admm_step's x~ (the full K, which knows nothing of elimination) is refined until its long-double residual stops
              falling; it moves by less than a tenth of the bars (2-norm on X, per element on the eliminated variables)
  clamps      on every row the unclipped z+ is farther from l and from u than its bar, and over the cases' rows with an eliminated
              variable z+ lands on l, on u and inside, in each rho class that has finite bounds
  can fail    the unmutated reduced model agrees with admm_step within the bars; six mutations of it (_elim_cases.mutated_steps)
              each move x+, z+ or y+ by more than 10 bars on an eliminated variable or its row, in every case where the mutated
              quantity is there to be moved (stated per mutation below)
  oracle      at batch size 1 the CPU oracle's first iteration from the same iterates agrees with the reference step
Wall time: 94 tests in 7 s."""
import functools

import numpy as np
import pytest
from scipy import sparse

from tests import _elim_cases as EC
from tests import _engine_reference as R
from tests import _pcg_cases as PC

ALPHAS = (1.0, 1.6)


@functools.lru_cache(maxsize=None)
def _setup(name, alpha):
    c = EC.make(name)
    pb, _ = R.scaled_problem(c, 10)
    erow, ecol = EC.claimed(c)
    x, y, z = R.iterates(c)
    st = R.admm_step(pb, R.SIGMA, alpha, c["rho"], x, z, y)
    b = EC.rhs(pb, R.SIGMA, c["rho"], x, z, y)
    red = EC.reduced(pb, R.SIGMA, c["rho"], erow, b)
    bars = EC.step_bars_elim(pb, st, red, erow, R.SIGMA, alpha, c["rho"], EC.PCG_EPS, x, z, y)
    return c, pb, erow, ecol, (x, y, z), st, b, red, bars


@pytest.mark.parametrize("name", EC.NAMES)
def test_claims(name):
    c = EC.make(name)
    erow, ecol = EC.eliminated(c["Pu"], c["A"])
    want_row, want_col = EC.claimed(c)
    assert np.array_equal(erow, want_row) and np.array_equal(ecol, want_col), (name, np.flatnonzero(erow != want_row)[:8])
    gone, stay = c["claims"]["gone"], c["claims"]["stay"]
    assert not set(gone) & set(stay) and sorted(set(gone) | set(stay)) == list(range(c["n"])), name
    A, Pu = sparse.csr_matrix(c["A"]), sparse.csc_matrix(c["Pu"])
    A.sort_indices()
    lenA = np.diff(A.indptr)
    s = PC.structure(c)
    assert [tuple(d) for d in s["dense"]] == [tuple(d) for d in c["claims"]["dense"]]
    for k in ("long", "huge"):
        if k in c["claims"]:
            assert s[k] == c["claims"][k], (name, k, s[k])
    rho = c["rho"]
    rows = np.array(sorted(gone.values()))
    if name not in ("all_gone_1", "one_gone_1", "one_gone_2", "res_gone_e8", "res_gone_e20"):         # the three rho classes on rows with an eliminated variable
        assert {float(v) for v in rho[rows]} == {EC.RHO, 1e3 * EC.RHO, EC.RHO_MIN}, (name, set(rho[rows]))
    assert np.all((c["l"] == c["u"]) == (rho == 1e3 * EC.RHO)) and np.all((c["l"] < -1e29) == (rho == EC.RHO_MIN))
    if name == "all_gone":
        assert (c["n"], c["m"], len(gone), Pu.nnz, A.nnz) == (300, 300, 300, 300, 300)
    if name == "all_gone_1":
        assert (c["n"], c["m"], gone) == (1, 1, {0: 0})
    if name.startswith("one_gone"):
        assert (c["n"], c["m"]) == (257, 300) and gone == ({256: 0} if name.endswith("1") else {0: 299})
    if name == "pyy":
        d = {j: Pu[j, j] for j in range(20, 40)}
        stored = {j: j in Pu.indices[Pu.indptr[j]:Pu.indptr[j + 1]] for j in range(20, 40)}
        assert not any(stored[j] for j in range(20, 26)) and all(stored[j] and d[j] == 0.0 for j in range(26, 32)) and all(d[j] > 0 for j in range(32, 40))
        a = np.array([c["A"][gone[j], j] for j in range(20, 40)])
        assert list(np.abs(a[[2, 8, 14]])) == [1e-2] * 3 and list(np.abs(a[[3, 9, 15]])) == [1e2] * 3 and a[16] == 0.0
        assert sparse.csc_matrix(c["A"]).indptr[37] - sparse.csc_matrix(c["A"]).indptr[36] == 1 and (a > 0).any() and (a < 0).any()
    if name == "rivals":
        Ac = sparse.csc_matrix(c["A"])
        cnt = np.diff(Ac.indptr)
        assert cnt[30] == cnt[31] == 1 and Ac.indices[Ac.indptr[30]] == Ac.indices[Ac.indptr[31]] == 0
        assert 32 in Pu.indices[Pu.indptr[33]:Pu.indptr[34]] and Pu[32, 33] == 0.0 and cnt[32] == cnt[33] == 1
        assert cnt[34] == 2 and sorted(Ac.data[Ac.indptr[34]:Ac.indptr[35]] == 0.0) == [False, True] and cnt[35] == 0
    if name == "lone_rows":
        assert all(lenA[i] == 1 for i in gone.values()) and all(lenA[i] == 0 for i in c["claims"]["empty_rows"])
    if name == "rounds":
        assert c["m"] == 2100 and int(A.indptr[2048]) <= 256          # rows 0..2047: one stream block (at most 256 products, 2048 rows)
        assert {gone[250 + k] for k in range(11)} == set(EC.ROUND_ROWS) and min(gone) < 256 <= max(gone)
        assert {i // 256 for i in EC.ROUND_ROWS} >= {0, 1, 3, 4, 7}
    if name == "long_rows":
        assert list(lenA[:3]) == [511, 512, 513]
        pos = [int(np.flatnonzero(A.indices[A.indptr[i]:A.indptr[i + 1]] == j)[0]) for i, j in ((0, 0), (1, 100), (2, 599))]
        assert pos == [0, 63, 512]
    if name == "huge_gone":
        assert c["n"] == 8200 and list(lenA[:2]) == [8192, 8191] and A.indices[A.indptr[2] - 1] == 8192 and s["folded"] == 1
        Ac = sparse.csc_matrix(c["A"])
        assert all(Ac.indptr[j + 1] - Ac.indptr[j] == 1 and Ac.indices[Ac.indptr[j]] == 0 for j in (8190, 8191))
    if name == "blocks_gone":
        assert [b for _, b, _ in s["dense"]] == [32, 64, 128]
    if name.startswith("res_gone"):
        n0 = PC.RESIDENT[c["claims"]["E"]][0]
        assert len(gone) == n0 // 10 and all(c["l"][i] == c["u"][i] for i in gone.values())


@pytest.mark.parametrize("E", sorted(EC.RES_GONE))
def test_resident_cases_get_their_E(E, monkeypatch):
    from tests.test_resident_plan import _plan
    monkeypatch.setenv("OSQP_AMD_RESIDENT_MIN_N", "1")
    c = EC.make("res_gone_e%d" % E)
    Pf = c["Pu"] + sparse.triu(c["Pu"], 1).T
    st, _ = _plan(Pf, c["A"], c["claims"]["nwg"])
    assert st[0] == 1 and st[1] == E, (E, st)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", EC.NAMES)
def test_bars_are_sharp_and_the_reference_is_better(name, alpha):
    c, pb, erow, ecol, (x, y, z), st, b, red, bars = _setup(name, alpha)
    assert red["lam_min"] > 0.0
    print(f"[elim-cases] {name} alpha {alpha}: n {c['n']} m {c['m']} gone {len(red['Y'])} lam_min(S) {red['lam_min']:.3g} lam_min(K) {st['lam_min']:.3g}"
          f" bar on x~_X / ||x~|| {bars['x_tilde'] / st['norm_xt']:.2e}")
    assert bars["x_tilde"] <= 1e-8 * st["norm_xt"], (name, bars["x_tilde"], st["norm_xt"])
    xt, res = EC.refine(pb, R.SIGMA, c["rho"], b, st["x_tilde"])
    d = np.abs(xt - st["x_tilde"]).astype(float)
    X, Y = red["X"], red["Y"]
    assert np.linalg.norm(d[X]) <= 0.1 * bars["x_tilde"], (name, np.linalg.norm(d[X]), bars["x_tilde"])
    assert np.all(d[Y] <= 0.1 * bars["x_tilde_each"][Y]), (name, float((d[Y] / bars["x_tilde_each"][Y]).max()))
    if Y.size:
        print(f"[elim-cases] {name} alpha {alpha}: largest bar on an eliminated x~ / ||x~|| {float(bars['x_tilde_each'][Y].max()) / st['norm_xt']:.2e}")


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", EC.NAMES)
def test_clamp_rows_are_decided(name, alpha):
    c, pb, erow, ecol, (x, y, z), st, b, red, bars = _setup(name, alpha)
    v, bz = st["v"].astype(float), bars["z"]
    l, u = pb.l.astype(float), pb.u.astype(float)
    assert np.all(np.abs(v - l) > bz) and np.all(np.abs(v - u) > bz), name


def test_clamps_cover_l_u_and_interior():
    seen = set()
    for name in EC.NAMES:
        c, pb, erow, ecol, (x, y, z), st, b, red, bars = _setup(name, 1.6)
        v, l, u = st["v"].astype(float), pb.l.astype(float), pb.u.astype(float)
        for i in np.flatnonzero(ecol >= 0):
            kind = "eq" if l[i] == u[i] else ("free" if l[i] < -1e20 else "plain")
            seen.add((kind, "l" if v[i] < l[i] else ("u" if v[i] > u[i] else "in")))
        if name in ("all_gone", "pyy", "rivals", "lone_rows", "blocks_gone"):       # enough such rows to ask it of the case alone
            assert {("plain", "l"), ("plain", "u"), ("plain", "in"), ("eq", "l"), ("eq", "u"), ("free", "in")} <= seen, (name, seen)
            seen = set()


MUTS = ("rho_for_rhoe", "by_without_a", "by_previous_q", "zt_incomplete", "Dy_without_sigma", "x_without_alpha")


@pytest.mark.parametrize("name", EC.NAMES)
def test_the_bars_see_each_model_mutation(name):
    """Where a mutation has nothing to move, that is a property of the case and is stated here, not an excuse:
      rho_for_rhoe      changes S only: needs a row that holds an eliminated variable AND others (not all_gone*, lone_rows)
      Dy_without_sigma  a relative change of sigma / D_y to x~_y: 1e-6 / 100 on an equality row with P_yy of 1 -- still hundreds of bars
      x_without_alpha   needs alpha != 1: asked at alpha = 1.6"""
    alpha = 1.6
    c, pb, erow, ecol, (x, y, z), st, b, red, bars = _setup(name, alpha)
    q_prev = pb.q.astype(float) * (1.0 + 1e-4)
    out = EC.mutated_steps(pb, red, erow, R.SIGMA, alpha, c["rho"], x, z, y, q_prev)
    Y = red["Y"]
    rows = erow[Y]

    def ratio(t):
        xn, zn, yn = t
        e = [np.abs(xn - st["x"]).astype(float)[Y] / bars["x"][Y], np.abs(zn - st["z"]).astype(float)[rows] / np.maximum(bars["z"][rows], 1e-300),
             np.abs(yn - st["y"]).astype(float)[rows] / np.maximum(bars["y"][rows], 1e-300)]
        return max(float(v.max()) for v in e)

    def ratio_all(t):
        return max(float((np.abs(g - st[k]).astype(float) / np.maximum(bars[k], 1e-300)).max()) for k, g in zip("xzy", t))

    base = ratio_all(out["none"])
    print(f"[elim-cases] {name}: the reduced model against admm_step: worst err / bar {base:.3f}")
    assert base <= 1.0, (name, base)
    for mut in MUTS:
        r = ratio(out[mut])
        print(f"[elim-cases] {name}: {mut} moves an eliminated variable or its row by {r:.3g} bars")
        if mut == "rho_for_rhoe" and name in ("all_gone", "all_gone_1", "lone_rows"):
            assert r <= 1.0          # no row of S to weigh: the mutation is the same model
            continue
        assert r > 10.0, (name, mut, r)


@pytest.mark.parametrize("name", EC.NAMES)
def test_oracle_first_iteration(name):
    """The CPU oracle (the checker of the whole solves) at batch size 1: one iteration, no scaling, from the same x, y with
    z = A x (its warm start), against admm_step on the unscaled problem with the oracle's own rho vector."""
    import oracle.oracle as orc
    orc.build()
    c = EC.make(name)
    x0, y0, _ = R.iterates(c)
    P = sparse.csc_matrix(c["Pu"] + sparse.triu(c["Pu"], 1).T)
    s = orc.OracleOSQP().setup(P=P, q=c["q"], A=sparse.csc_matrix(c["A"]), l=c["l"], u=c["u"], scaling=0, max_iter=1, alpha=1.6,
                               rho=EC.RHO, sigma=R.SIGMA, adaptive_rho=0, polish=0, check_termination=0, warm_start=1)
    s.warm_start(x=x0, y=y0)
    r = s.solve()
    pb = R.Problem(c["Pu"], c["A"], c["q"], c["l"], c["u"])
    rho = np.full(c["m"], EC.RHO)
    rho[c["l"] == c["u"]] = 1e3 * EC.RHO
    rho[(c["l"] < -1e20) & (c["u"] > 1e20)] = EC.RHO_MIN
    z0 = np.asarray(pb.A @ np.asarray(x0, dtype=R.LD)).astype(float)
    st = R.admm_step(pb, R.SIGMA, 1.6, rho, x0, z0, y0)
    scale = max(1.0, float(np.abs(st["x"]).max()))
    ex, ey = float(np.abs(r.x - st["x"].astype(float)).max()), float(np.abs(r.y - st["y"].astype(float)).max())
    print(f"[elim-cases] {name}: oracle's first iteration against admm_step: x {ex:.2e} y {ey:.2e}")
    cond = 1e-13 * (st["norm_b"] / st["lam_min"] + scale) * 1e3
    assert ex <= cond and ey <= cond * max(1.0, float(rho.max()) * float(st["a1"].max())), (name, ex, ey, cond)
