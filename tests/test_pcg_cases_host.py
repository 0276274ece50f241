"""CPU checks of the cases of tests/_pcg_cases.py (no device): each case is what it claims to be, the bar that
tests/test_gpu_pcg_edges.py puts on x~ is sharp on it, and that bar fails when one value of the operator is off by 1e-4.

  structure   a Python restatement of build_dense's rule (block starts, 32 <= b <= 128, half-full test, pitch), of build_blocks' row
              classes (< 512, >= 512, >= 8192), of the fold / split rules and of upload_mat's 16-bit switch gives exactly the
              dense blocks, pitches, long / huge rows and flags the generator states by hand; for the 16-bit cases the largest
              column id of A and of M lies on the stated side of 65535
  sharp       on the problem after 10 Ruiz sweeps of the reference, with pcg_eps_rel = 1e-12:
              step_bars(...)['x_tilde'] / ||x~||_2 <= 1e-8
  can fail    three mutations of the reference operator, one at a time, each a relative change of 1e-4 to a single value (an
              entry of P in the last row of the last dense block -- 1e-4 at a structural zero --, the last entry of the longest
              row of A, rho of that row) move x~ by more than 10 x the bar in the 2-norm
  resident    hipeng_resident_plan (host only) with the grid the GPU test forces reports `qualifies` and the E of the case's name"""
import functools

import numpy as np
import pytest
from scipy import sparse

from tests import _engine_reference as R
from tests import _pcg_cases as PC

ALPHA = 1.6
# the grid of an MI355X as build_blockres sizes it (256 CUs, one per XCD left free); the GPU test reads it from the device
BR_NWG = 248


@functools.lru_cache(maxsize=None)
def _make(name):
    if name == "br_pairs":
        return PC.br_pairs(BR_NWG)
    if name == "br_pairs_plus1":
        return PC.br_pairs(BR_NWG, 1)
    return PC.make(name)


ALL = PC.NAMES + ("br_pairs", "br_pairs_plus1")


@pytest.mark.parametrize("name", ALL)
def test_structure(name):
    c = _make(name)
    s, claims = PC.structure(c), c["claims"]
    for k in ("dense", "long", "huge", "folded", "split", "long_b", "a16", "m16", "b16"):
        if k in claims:
            assert s[k] == claims[k], (name, k, s[k], claims[k])
    assert s["dense_rows"] == sum(b for _, b, _ in claims["dense"])
    for c0, b, pitch in s["dense"]:                       # even, and never a multiple of 32 below 128
        assert pitch == {32: 34, 33: 34, 63: 66, 64: 66, 65: 66, 96: 98, 127: 128, 128: 128}[b], (name, b, pitch)
    # no variable qualifies for elimination from the linear system (build_elim): uncoupled in P, one entry in its column of A,
    # the row not a huge one
    Pu, A = sparse.csc_matrix(c["Pu"]), sparse.csc_matrix(c["A"])
    coupled = PC._full_row_lengths(Pu) > 1
    lenA = np.diff(sparse.csr_matrix(A).indptr)
    single = np.flatnonzero(~coupled & (np.diff(A.indptr) == 1))
    assert all(lenA[A.indices[A.indptr[j]]] >= PC.HUGE_ROW for j in single), (name, single[:8])
    # stated sizes
    if name == "blocks_mixed":
        assert (len(s["dense"]), s["dense_rows"], c["n"]) == (8, 608, 768)
        assert sorted(b for _, b, _ in s["dense"]) == sorted(b for b in PC.MIXED_SIZES if b not in (31, 129))
        assert int((np.diff(A.indptr) == 0).sum()) == 5
    if name == "blocks_threshold":
        nnz = [int(Pu.indptr[k + 64] - Pu.indptr[k]) for k in (0, 64)]
        assert [2 * z - 64 for z in nnz] == [2048, 2046] and len(s["dense"]) == 1
    if name == "blocks_holes":
        P = (Pu + sparse.triu(Pu, 1).T).toarray()
        assert np.count_nonzero(P[127]) == 1 and np.count_nonzero(P[:, 127]) == 1 and P[127, 127] != 0
        assert abs(PC._full_row_lengths(Pu).sum() / 128.0 ** 2 - 0.6) < 0.01 and int((Pu.data == 0).sum()) == 22
        assert Pu[126, 127] == 0 and 126 not in Pu.indices[Pu.indptr[127]:Pu.indptr[128]]      # a structural zero
    if name.startswith("huge_nh"):
        nh = int(name[7:])
        assert list(lenA[: nh + 1]) == list(PC.HUGE_LENGTHS[:nh]) + [8191] and c["n"] == 8200 and c["m"] == nh + 41
    if name.startswith("c16"):
        want = dict(narrow=(True, True), m_wide=(True, False), wide=(False, False))[name.split("_", 1)[1]]
        assert (s["max_col_A"] <= 65535, s["max_col_M"] <= 65535) == want, (name, s["max_col_A"], s["max_col_M"])
        if name.endswith("narrow"):
            assert s["max_col_M"] == 65535
        if name.startswith("c16d"):                       # a diagonal P, four rows of 600 entries, 50 short ones
            assert Pu.nnz == c["n"] and sorted(lenA)[-4:] == [600] * 4 and c["m"] == 54 and s["long_b"] == 0
    if name.startswith("br_pairs"):
        sizes = [b for _, b, _ in s["dense"]]
        assert len(sizes) == 2 * BR_NWG + (name == "br_pairs_plus1")
        pairs = {(sizes[2 * g], sizes[2 * g + 1]) for g in range(BR_NWG)}
        assert pairs == {(128, 128), (32, 32), (128, 32), (32, 128)} and lenA.max() >= PC.HUGE_ROW


@pytest.mark.parametrize("name", ALL)
def test_bar_is_sharp_and_can_fail(name):
    c = _make(name)
    pb, _ = R.scaled_problem(c, 10)
    x, y, z = R.iterates(c)
    st = R.admm_step(pb, R.SIGMA, ALPHA, c["rho"], x, z, y)
    bar = R.step_bars(st, ALPHA, c["rho"], False, PC.PCG_EPS)["x_tilde"]
    print(f"[pcg-cases] {name}: n {c['n']} m {c['m']} lam_min {st['lam_min']:.3g} bar / ||x~|| {bar / st['norm_xt']:.2e}")
    assert bar / st["norm_xt"] <= 1e-8, (name, bar, st["norm_xt"])
    sv = PC.Solver(pb, c["rho"])
    xt = sv.x_tilde(x, z, y)
    assert np.linalg.norm(xt - st["x_tilde"].astype(float)) <= 0.1 * bar           # the two references agree
    for label, kw in sv.mutations(c):
        d = float(np.linalg.norm(sv.x_tilde(x, z, y, **kw) - xt))
        print(f"[pcg-cases] {name}: {label} * (1 + 1e-4) moves x~ by {d:.2e} = {d / bar:.1f} bars")
        assert d > 10.0 * bar, (name, label, d, bar)


@pytest.mark.parametrize("E", sorted(PC.RESIDENT))
def test_resident_cases_get_their_E(E, monkeypatch):
    from tests.test_resident_plan import _plan
    monkeypatch.setenv("OSQP_AMD_RESIDENT_MIN_N", "1")
    c = PC.make("res_e%d" % E)
    Pf = c["Pu"] + sparse.triu(c["Pu"], 1).T
    st, _ = _plan(Pf, c["A"], c["claims"]["nwg"])
    assert st[0] == 1 and st[1] == E, (E, st)
    eq = c["l"] == c["u"]
    assert int(eq.sum()) == c["m"] // 10
