"""GPU tests of the three PCG forms of the single-QP engine -- form 0, launch per step (k_pcg_init / k_cg_A / k_cg_B /
k_huge_reduce); form 1, k_pcg_resident<E>; form 2, k_pcg_blockres<NH> -- at their structural edges, one linear solve at a time
through the C shim, against the long-double reference of tests/_engine_reference.py.  Every test opens the engine with the raw
q, l, u, pcg_eps_rel = 1e-12 and pcg_max_iter = 20 000, runs Ruiz with 10 passes, hipeng_matrices_changed and
hipeng_upload_rho, asserts the form (hipeng_resident_info [9], [1], [2], [3]) and the slots of hipeng_pcg_layout the case is
about, then takes one ADMM step (alpha = 1.6) from non-zero x, y, z -- so k_pcg_init forms b - K x~0 through the same operator
pieces as the iterations -- and compares x, z, y with _engine_reference.admm_step on the scaled data the device returned.  It
asserts stats (admm_done 1, pcg_forced 0, neg_curvature 0) and that no variable is eliminated, and prints form, layout and error / bar.

Cases (tests/_pcg_cases.py; tests/test_pcg_cases_host.py proves on the CPU that each is what it claims, that its bar is below
1e-8 ||x~|| and that a relative change of 1e-4 to one value of P, A or rho misses it by more than 10 x):
  (a) dense diagonal blocks of P on form 0: k_pcg_init<true>, k_cg_B<true, *>, dense_block_mv_x, k_repack, the remainder Mr
      blocks_mixed      blocks of 32, 31, 33, 64, 129, 63, 65, 96, 127, 128 (n = 768): 8 dense blocks, 608 dense rows, pitches
                        34, 34, 66, 66, 66, 98, 128, 128; the 31 and 129 blocks stay in the remainder; second steps after
                        hipeng_upload_matrices (P -> S P S with S^2 = 0.9 or 1.1 per variable, every entry of A times 0.9 or
                        1.1, same pattern: the k_repack of blocks and remainder) and after a rho spanning 1e-3 .. 1e3
      blocks_threshold  two blocks of 64, 2 nnz - b = b^2 / 2 exactly (dense) and one pair fewer (not dense)
      blocks_holes      a block of 128 at 60 % fill, last row and column only the diagonal in value, explicit zeros, map < 0
  (b) huge rows on form 0, P diagonal, n = 8200: nh = 1, 4, 5 rows of 8192, 8193, 8200, 8192, 8193 entries, a long row of 8191, 40
      short rows: folded into k_cg_B<*, true> through hcol (nh <= 4), k_huge_reduce (nh = 5, or nh = 4 with OSQP_AMD_HFOLD=0);
      blocks_huge4 / 5: 64 dense blocks of 128 with 4 / 5 huge rows and a box row per variable (k_cg_B<true, true> /
      <true, false>); a second step after a rho that changes on the huge rows only
  (c) split mode (k_cg_A as update-only + apply-only): _engine_reference's `long` and blocks_mixed with OSQP_AMD_SPLIT=0 and 1;
      split3 (three rows of 600 entries, n = 700) reports split = 1 with the variable unset
  (d) 16-bit column ids in the long-row passes (upload_mat: a matrix with long rows and max col <= 0xffff): A four rows of 600
      entries and 50 short ones; n + m = 65536 (M narrow, holds column 65535), 65537 (M wide, A narrow), n = 65537 (both wide).
      c16d_*: P diagonal -- M has no long row then and gets no 16-bit ids at any size (layout [8] = [9] = 0), so the switch is
      A's alone; c16_*: P a diagonal and one row of 600 entries, the long row of M, which then crosses the boundary as stated
  (e) form 2: dense blocks only, a single-entry row per variable, NH huge rows over every variable
      br_sizes   blocks 32, 33, 63, 64, 65, 96, 127, 128 x 14 (n = 8512), NH = 0, 1, 4; second steps after rho and matrices (NH = 1)
      br_pairs   2 nwg blocks in the order 128, 128, 32, 32, 128, 32, 32, 128: two per workgroup (128 + 128 = 256 rows among
                 them), NH = 1; with 2 nwg + 1 blocks form 2 must refuse, and whatever serves meets the same bar
  (f) form 1: one problem per E in 8, 16, 20, 24, 32, 48, 64 with a tenth of the rows equalities, OSQP_AMD_RESIDENT_PIPE 1 and 0;
      for E = 20 and 64 hipeng_resident_dump against K = P + sigma I + A' rho A (1e-13 max|K|, symmetric to the bit)
Environments: `steps` OSQP_AMD_RESIDENT=0 OSQP_AMD_DENSE_DIRECT=0; `blockres` OSQP_AMD_BLOCK_DIRECT=0 OSQP_AMD_DENSE_DIRECT=0;
(f) OSQP_AMD_DENSE_DIRECT=0 OSQP_AMD_RESIDENT_MIN_N=1 OSQP_AMD_RESIDENT_NWG=<the case's grid>.

Bars: those of test_gpu_engine_kernels.test_admm_step, none tuned on the device's output:
  ||x~_dev - x~||_2 <= pcg_eps_rel ||b||_2 / lam_min(K) + 50 U ||x~||_2, times alpha for x, alpha ||A_i||_1 for z, rho_i times that
  for y, each plus the rounding of its own update formula (_engine_reference.step_bars, direct = False).
Wall time of the module on an MI355X: 40 tests in 8.2 s (the slowest, br_pairs with 39 680 variables, 1.4 s)."""
import time

import numpy as np
import pytest
from scipy import sparse

from tests import _engine_reference as R
from tests import _pcg_cases as PC
from tests._hipeng import Engine
from tests._kkt_reference import reduced_matrix

pytestmark = pytest.mark.gpu

ALPHA = 1.6
STEPS = dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=0)
BLOCKRES = dict(OSQP_AMD_BLOCK_DIRECT=0, OSQP_AMD_DENSE_DIRECT=0)
FORM0 = (0, 0, 0, 0)                     # hipeng_resident_info [9], [1], [2], [3] of a launch-per-step engine


def _open(c, env):
    t = time.time()
    e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=env, q=c["q"], l=c["l"], u=c["u"], alpha=ALPHA, pcg_eps_rel=PC.PCG_EPS,
               pcg_max_iter=20000)
    e.t_create = time.time() - t
    return e


def _scaled(c, e):
    """Ruiz on the device and the rho vector, in the order of the solver's set-up; (l, u) and the values of triu(P), A it returned."""
    o = e.ruiz_scale(10)
    e.matrices_changed()
    e.set_rho(c["rho"])
    return o


def _problem(c, o, Px=None, Ax=None):
    Pu, A = c["Pu"].copy(), c["A"].copy()
    Pu.data, A.data = (o["Px"] if Px is None else Px).copy(), (o["Ax"] if Ax is None else Ax).copy()
    return R.Problem(Pu, A, o["q"], o["l"], o["u"], o["D"], o["E"])


def _forms(tag, e, want):
    inf = e.info()
    assert (inf[9], inf[1], inf[2], inf[3]) == tuple(want), (tag, "form, in use, E, workgroups", inf[:10], want)
    return inf


def _layout(tag, c, e, hfold=True, split=None, **slots):
    """Every slot of hipeng_pcg_layout that tests/_pcg_cases.structure() predicts from (P, A), then the ones the case names."""
    lay, s = e.layout(), PC.structure(c, hfold)
    want = dict(dense=len(s["dense"]), dense_rows=s["dense_rows"], long=len(s["long"]), huge=len(s["huge"]), folded=s["folded"],
                split=s["split"] if split is None else split, a16=s["a16"], m16=s["m16"], b16=s["b16"], long_b=s["long_b"])
    want.update(slots)
    got = dict(dense=lay[0], dense_rows=lay[1], long=lay[3], huge=lay[4], folded=lay[5], split=lay[6], a16=lay[7], m16=lay[8],
               b16=lay[9], long_b=lay[10])
    assert got == want, (tag, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
    assert lay[6] == e.is_split() and lay[11] >= 1 and lay[12] >= 1 and lay[13:] == [0, 0, 0]
    return lay


def _step(tag, c, e, o, pb, rho, salt=0):
    """One ADMM step from the seeded iterates against the reference; returns the worst error / bar over x, z, y."""
    assert e.elim() == 0                          # the bar is that of the whole reduced system
    x0, y0, z0 = R.iterates(c, salt)
    e.set_iterates(x0, y0, z0)
    t = time.time()
    e.run_admm(1)
    x1, y1, z1, dx, dy = e.download(False)
    t = time.time() - t
    s8 = e.stats()
    assert (s8["admm_done"], s8["pcg_forced"], s8["neg_curvature"]) == (1, 0, 0), (tag, s8)
    st = R.admm_step(pb, R.SIGMA, ALPHA, rho, x0, z0, y0)
    bars = R.step_bars(st, ALPHA, rho, False, PC.PCG_EPS)
    l, u = o["l"], o["u"]
    assert np.all(l <= z1) and np.all(z1 <= u)
    assert np.array_equal(y0 + dy, y1) and np.array_equal(x1 - x0, dx)
    v, bz = st["v"].astype(float), bars["z"]
    lo, hi = v < l - bz, v > u + bz
    assert np.array_equal(z1[lo], l[lo]) and np.array_equal(z1[hi], u[hi]), tag
    inf, lay, worst, text = e.info(), e.layout(), 0.0, []
    for k, got in (("x", x1), ("z", z1), ("y", y1)):
        err = np.abs(got.astype(R.LD) - st[k]).astype(float)
        ratio = float((err / np.maximum(bars[k], 1e-300)).max()) if err.size else 0.0
        worst = max(worst, ratio)
        text.append(f"{k}+ {err.max() if err.size else 0.0:.2e} err/bar {ratio:.3e}")
    print(f"[pcg-edges] {tag}: form {inf[9]} in use {inf[1]} E {inf[2]} nwg {inf[3]} gave up {inf[10]} layout {lay[:13]} pcg iterations {inf[6]}"
          f" step {t:.3f} s; {'; '.join(text)} (bar on x~ {bars['x_tilde']:.2e} = {bars['x_tilde'] / st['norm_xt']:.1e} ||x~||, lam_min {st['lam_min']:.2e})"
          f" worst err/bar {worst:.3e}")
    for k, got in (("x", x1), ("z", z1), ("y", y1)):
        err = np.abs(got.astype(R.LD) - st[k]).astype(float)
        assert np.all(err <= bars[k]), (tag, k, float((err / np.maximum(bars[k], 1e-300)).max()))
    return worst


def _run(tag, c, env, forms=FORM0, hfold=True, split=None, **slots):
    """Open, scale, assert form and layout, take the step; returns (engine, Ruiz output, problem) for second steps."""
    e = _open(c, env)
    try:
        o = _scaled(c, e)
        _forms(tag, e, forms)
        _layout(tag, c, e, hfold, split, **slots)
        pb = _problem(c, o)
        _step(tag, c, e, o, pb, c["rho"])
    except BaseException:
        e.close()
        raise
    return e, o, pb


def _changed_matrices(c, o, seed):
    """P -> S P S with S^2 = 0.9 or 1.1 per variable (every diagonal entry moves by 10 %, P stays definite), every entry of A
    times 0.9 or 1.1; same pattern."""
    rng = np.random.default_rng(seed)
    s = np.sqrt(rng.choice([0.9, 1.1], c["n"]))
    Pu, A = sparse.csc_matrix(c["Pu"]), sparse.csc_matrix(c["A"])
    pcol = np.repeat(np.arange(c["n"]), np.diff(Pu.indptr))
    return o["Px"] * s[Pu.indices] * s[pcol], o["Ax"] * rng.choice([0.9, 1.1], A.nnz)


def _second_steps(tag, c, e, o, rho2, matrices_first):
    """A step after hipeng_upload_matrices and one after hipeng_upload_rho, in the order given."""
    salt, rho, Px, Ax = 0, c["rho"], o["Px"], o["Ax"]
    for what in (("matrices", "rho") if matrices_first else ("rho", "matrices")):
        if what == "matrices":
            Px, Ax = _changed_matrices(c, o, 7)
            Pu, A = c["Pu"].copy(), c["A"].copy()
            Pu.data, A.data = Px.copy(), Ax.copy()
            e.set_matrices(Pu, A)
        else:
            rho = rho2
            e.set_rho(rho)
        salt += 1
        _step(f"{tag} after {what}", c, e, o, _problem(c, o, Px, Ax), rho, salt=salt)


# ---------------------------------------------------------------------------------------------------------------
# (a) dense diagonal blocks of P, form 0
# ---------------------------------------------------------------------------------------------------------------
def test_dense_blocks_mixed_and_updates():
    c = PC.make("blocks_mixed")
    e, o, pb = _run("a blocks_mixed", c, STEPS, dense=8, dense_rows=608, long=0, huge=0, folded=0)
    try:
        rho2 = 10.0 ** np.random.default_rng(5).uniform(-3.0, 3.0, c["m"])
        rho2[:2] = 1e-3, 1e3
        _second_steps("a blocks_mixed", c, e, o, rho2, matrices_first=True)
    finally:
        e.close()


def test_the_bar_sees_one_entry_of_a_dense_block():
    """Control: the device gets P with the entry (127, 126) of the last dense block of blocks_mixed (and its mirror image) off by a
    relative 1e-4 -- the first mutation of tests/test_pcg_cases_host.py -- and the reference does not: x+ must miss its bar."""
    c = PC.make("blocks_mixed")
    e, o, pb = _run("a blocks_mixed (control)", c, STEPS, dense=8, dense_rows=608)
    try:
        Pu, A = c["Pu"].copy(), c["A"].copy()
        Pu.data, A.data = o["Px"].copy(), o["Ax"].copy()
        k = Pu.indptr[c["n"]] - 2                                    # triu(P) by columns: the last entry is (n - 1, n - 1), before it (n - 2, n - 1)
        assert Pu.indices[k] == c["n"] - 2
        Pu.data[k] *= 1.0 + 1e-4
        e.set_matrices(Pu, A)
        x0, y0, z0 = R.iterates(c, 3)
        e.set_iterates(x0, y0, z0)
        e.run_admm(1)
        x1 = e.download(False)[0]
        st = R.admm_step(pb, R.SIGMA, ALPHA, c["rho"], x0, z0, y0)
        bars = R.step_bars(st, ALPHA, c["rho"], False, PC.PCG_EPS)
        ratio = float((np.abs(x1.astype(R.LD) - st["x"]).astype(float) / bars["x"]).max())
        print(f"[pcg-edges] a blocks_mixed (control): one entry of P off by 1e-4 on the device only: x+ err/bar {ratio:.1f}")
        assert ratio > 10.0
    finally:
        e.close()


@pytest.mark.parametrize("name,dense,rows", [("blocks_threshold", 1, 64), ("blocks_holes", 1, 128)])
def test_dense_block_threshold_and_holes(name, dense, rows):
    _run("a " + name, PC.make(name), STEPS, dense=dense, dense_rows=rows)[0].close()


# ---------------------------------------------------------------------------------------------------------------
# (b) huge rows, form 0
# ---------------------------------------------------------------------------------------------------------------
def _huge_rho(c):
    rho2 = c["rho"].copy()
    rho2[c["claims"]["huge"]] *= np.linspace(3.0, 30.0, len(c["claims"]["huge"]))
    return rho2


@pytest.mark.parametrize("nh,hfold", [(1, 1), (4, 1), (5, 1), (4, 0)])
def test_huge_rows(nh, hfold):
    c = PC.make("huge_nh%d" % nh)
    folded = nh if hfold and nh <= 4 else 0
    env = dict(STEPS, OSQP_AMD_HFOLD=0) if not hfold else STEPS
    tag = f"b huge_nh{nh}{'' if hfold else ' HFOLD=0'}"
    e, o, pb = _run(tag, c, env, hfold=bool(hfold), huge=nh, folded=folded, long=1, dense=0)
    try:
        rho2 = _huge_rho(c)
        e.set_rho(rho2)
        _step(tag + " after rho of the huge rows", c, e, o, pb, rho2, salt=1)
    finally:
        e.close()


@pytest.mark.parametrize("nh", [4, 5])
def test_dense_blocks_with_huge_rows(nh):
    c = PC.make("blocks_huge%d" % nh)
    e, o, pb = _run(f"b blocks_huge{nh}", c, STEPS, dense=64, dense_rows=8192, huge=nh, folded=nh if nh <= 4 else 0)
    try:
        rho2 = _huge_rho(c)
        e.set_rho(rho2)
        _step(f"b blocks_huge{nh} after rho of the huge rows", c, e, o, pb, rho2, salt=1)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# (c) split mode
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", ["long", "blocks_mixed"])
def test_split_mode(name, split):
    c = R.make_case("long") if name == "long" else PC.make(name)
    _run(f"c {name} SPLIT={split}", c, dict(STEPS, OSQP_AMD_SPLIT=split), split=split)[0].close()


def test_split_chosen_for_long_rows_only():
    _run("c split3", PC.make("split3"), STEPS, split=1, long=3)[0].close()


# ---------------------------------------------------------------------------------------------------------------
# (d) 16-bit column ids
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,a16,m16,long_m", [("c16_narrow", 1, 1, 1), ("c16_m_wide", 1, 0, 1), ("c16_wide", 0, 0, 1),
                                                 ("c16d_narrow", 1, 0, 0), ("c16d_m_wide", 1, 0, 0), ("c16d_wide", 0, 0, 0)])
def test_16_bit_column_ids(name, a16, m16, long_m):
    _run("d " + name, PC.make(name), STEPS, a16=a16, m16=m16, b16=m16, long=4, long_b=long_m)[0].close()


# ---------------------------------------------------------------------------------------------------------------
# (e) block-resident, form 2
# ---------------------------------------------------------------------------------------------------------------
def _br_nwg():
    c = PC.br_probe()
    e = _open(c, BLOCKRES)
    try:
        inf = e.info()
        assert inf[9] == 2 and inf[1] == 1, inf
        return int(inf[3])
    finally:
        e.close()


@pytest.mark.parametrize("nh", [0, 1, 4])
def test_blockres_sizes(nh):
    c = PC.make("br_sizes_nh%d" % nh)
    nwg = _br_nwg()
    e, o, pb = _run(f"e br_sizes NH={nh}", c, BLOCKRES, forms=(2, 1, 64, nwg), dense=112, dense_rows=8512, huge=nh, folded=nh)
    try:
        if nh == 1:
            rho2 = 10.0 ** np.random.default_rng(6).uniform(-2.0, 2.0, c["m"])
            _second_steps("e br_sizes NH=1", c, e, o, rho2, matrices_first=False)
        assert e.info()[9] == 2 and e.info()[10] == 0
    finally:
        e.close()


@pytest.mark.parametrize("extra", [0, 1])
def test_blockres_two_blocks_per_workgroup(extra):
    nwg = _br_nwg()
    c = PC.br_pairs(nwg, extra)
    e = _open(c, BLOCKRES)
    try:
        o = _scaled(c, e)
        inf = e.info()
        if extra:
            assert inf[9] != 2, inf                    # more than two blocks per workgroup: refused
        else:
            assert (inf[9], inf[1], inf[2], inf[3]) == (2, 1, 64, nwg), inf
        _layout(f"e br_pairs+{extra}", c, e, dense=2 * nwg + extra, dense_rows=c["n"], huge=1, folded=1)
        _step(f"e br_pairs+{extra}", c, e, o, _problem(c, o), c["rho"])
        assert e.info()[10] == 0
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# (f) resident, form 1
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", [1, 0])
@pytest.mark.parametrize("E", sorted(PC.RESIDENT))
def test_resident_every_E(E, pipe):
    c = PC.make("res_e%d" % E)
    nwg = c["claims"]["nwg"]
    env = dict(OSQP_AMD_DENSE_DIRECT=0, OSQP_AMD_RESIDENT_MIN_N=1, OSQP_AMD_RESIDENT_NWG=nwg, OSQP_AMD_RESIDENT_PIPE=pipe)
    tag = f"f res_e{E} PIPE={pipe}"
    e, o, pb = _run(tag, c, env, forms=(1, 1, E, nwg), dense=0, huge=0)
    try:
        assert e.info()[10] == 0, (tag, "a resident launch gave up", e.info())
        if E in (20, 64):
            K = e.resident_dump()
            Pu, A = c["Pu"].copy(), c["A"].copy()
            Pu.data, A.data = o["Px"].copy(), o["Ax"].copy()
            Kref = reduced_matrix(Pu, A, R.SIGMA, c["rho"])
            err = float(np.abs(K - Kref).max())
            print(f"[pcg-edges] {tag}: max |K - (P + sigma I + A' rho A)| {err:.2e}, bar {1e-13 * np.abs(Kref).max():.2e}")
            assert err <= 1e-13 * np.abs(Kref).max() and np.array_equal(K, K.T)
    finally:
        e.close()
