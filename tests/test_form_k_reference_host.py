"""The host replay of the resident K (tests/_form_k_reference.py) on every case of tests/_form_k_cases.py, no device: replay() --
from (P, A, sigma, rho) and the pattern of K alone -- and replay_lists() -- from the lists hipeng_resident_plan_lists returns and the
slots they point to -- give the same bits, so the lists are tied to values and not only to patterns; the float64 sequence stays
within its derived distance of the same sum in long double; the reference is symmetric to the bit.  rho is spread over six decades
and sigma is large enough to matter, so a term taken with another row's weight cannot hide."""
import numpy as np
import pytest
from scipy import sparse

from tests import _form_k_cases as FC
from tests import _form_k_reference as FR
from tests.test_form_k_lists_plan import _lists
from tests.test_resident_plan import _plan

SIGMA = 1e-3
_DONE = {}


def _both(name):
    """The two replays of a case, computed once and shared by the tests (nothing changes them)."""
    if name not in _DONE:
        P, A = FC.case(name)
        st, pl = _plan(P, A)
        if not st[0]:
            _DONE[name] = None
            return None
        terms, Kcp, Kcm, Kca = _lists(P, A)
        assert terms >= 0, terms
        rho = 10.0 ** np.random.default_rng(len(name)).uniform(-3.0, 3.0, A.shape[0])
        one = FR.replay(P, A, SIGMA, rho, pl["Kptr"], pl["Kcol"])
        Mval, Mrow, Aval = FR.m_image(P, A)
        p, s = FR.base(P, SIGMA, pl["Kptr"], pl["Kcol"])
        two = FR.replay_lists(Mval, Aval, rho, Kcp, Kcm, Kca, Mrow, p, s)
        _DONE[name] = (pl, Kcp, one, two)
    return _DONE[name]


@pytest.fixture
def plan_env(monkeypatch):
    monkeypatch.setenv("OSQP_AMD_RESIDENT_MIN_N", "1")


@pytest.mark.parametrize("name", FC.HOST_CASES)
def test_replay_and_lists_give_the_same_bits(name, plan_env):
    got = _both(name)
    if got is None:
        assert name == "m0"                              # (where the plan does not take m = 0 there are no lists)
        return
    pl, Kcp, (v, vl, mag, cnt), (v2, vl2, mag2, cnt2) = got
    assert np.array_equal(cnt, np.diff(Kcp)) and np.array_equal(cnt2, np.diff(Kcp))
    assert np.isfinite(v).all() and np.isfinite(v2).all()
    assert np.array_equal(v.view(np.int64), v2.view(np.int64))
    assert np.array_equal(vl, vl2) and np.array_equal(mag, mag2)
    longest, over = FC.check_premise(name, pl["Kptr"], pl["Kcol"], cnt)
    print(f"[form-k-replay] {name}: {len(v)} entries of K, {int(cnt.sum())} terms, longest list {longest}, {over} lists over 66")


@pytest.mark.parametrize("name", FC.HOST_CASES)
def test_replay_stays_within_its_rounding_bound(name, plan_env):
    """An entry with len terms takes len + 1 additions at most (P_ij + sigma, then one per term) and two multiplications per
    term, each correctly rounded: |float64 - long double| <= (len + 3) 2^-53 mag, mag = |P_ij + sigma [i == j]| + sum |terms|."""
    got = _both(name)
    if got is None:
        return
    _, _, (v, vl, mag, cnt), _ = got
    err = np.abs(v.astype(FR.LD) - vl)
    bar = (cnt + 3).astype(FR.LD) * FR.U * mag
    tight = (cnt + 1).astype(FR.LD) * FR.U * mag
    worst = float((err[tight > 0] / tight[tight > 0]).max()) if (tight > 0).any() else 0.0
    print(f"[form-k-replay] {name}: worst |float64 - long double| / ((len + 1) 2^-53 mag) = {worst:.3f}")
    assert (err <= bar).all(), (name, worst)


@pytest.mark.parametrize("name", FC.HOST_CASES)
def test_replay_is_symmetric_to_the_bit(name, plan_env):
    got = _both(name)
    if got is None:
        return
    pl, _, (v, vl, mag, cnt), _ = got
    n = len(pl["Kptr"]) - 1
    K = sparse.csr_matrix((v.view(np.int64), pl["Kcol"], pl["Kptr"]), shape=(n, n))          # (the bit patterns: a stored 0 stays stored)
    C = sparse.csr_matrix((cnt + 1, pl["Kcol"], pl["Kptr"]), shape=(n, n))
    assert (K != K.T).nnz == 0 and (C != C.T).nnz == 0


def test_replay_with_eliminated_variables():
    """gone: unit diagonal, zeros elsewhere in those rows and columns; every other entry untouched."""
    P, A = FC.case("row_one")
    n = P.shape[0]
    pat = ((abs(sparse.csr_matrix(P)) + sparse.eye(n) + abs(A).T @ abs(A)) != 0).tocsr(); pat.sort_indices()
    rho = np.linspace(0.1, 3.0, A.shape[0])
    v, vl, mag, cnt = FR.replay(P, A, SIGMA, rho, pat.indptr, pat.indices)
    g, gl, gmag, gcnt = FR.replay(P, A, SIGMA, rho, pat.indptr, pat.indices, gone=[23, 3])
    rows = np.repeat(np.arange(n), np.diff(pat.indptr))
    out = np.isin(rows, [3, 23]) | np.isin(pat.indices, [3, 23])
    assert np.array_equal(g[~out], v[~out]) and np.array_equal(gcnt, cnt)
    assert np.array_equal(g[out], (rows[out] == pat.indices[out]).astype(float)) and np.array_equal(gl[out], g[out])
    # build_elim's rule on the same case: variable 23 is alone in row 11 (row_one) and not coupled in P only if P says so
    gone, taken = FR.eliminated(sparse.triu(P), A)
    assert len(gone) == len(taken) == len(set(taken))
