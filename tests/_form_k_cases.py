"""Seeded patterns for the contribution lists of k_form_K_lists (engine.hip: build_resident), shared by
tests/test_form_k_lists_plan.py (host side, against scipy) and tests/test_gpu_form_k_lists.py (values against k_form_K).
Each case is (P, A): P symmetric (both triangles), A, both canonical CSC without stored zeros.  P need not be positive
semidefinite: these cases are about the pattern and the values of K, no problem is solved on them."""
import numpy as np
from scipy import sparse


def _canon(M):
    M = sparse.csc_matrix(M)
    M.sum_duplicates(); M.eliminate_zeros(); M.sort_indices()
    return M


def _rand(m, n, dens, rng):
    # values away from zero, so that a stored entry never cancels to a stored zero
    return sparse.random(m, n, density=dens, random_state=rng, data_rvs=lambda k: rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k), format="lil")


def _psd(n, dens, rng):
    B = sparse.csc_matrix(_rand(n, n, dens, rng))
    return _canon(B @ B.T + 0.05 * sparse.eye(n))


def _line(count, among, rng):
    return np.sort(rng.choice(among, count, replace=False)), rng.uniform(0.5, 1.5, count)


def case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "n1":                      # one variable, two rows
        return _canon([[2.0]]), _canon([[1.0], [-0.5]])
    if name == "empty_col":               # a variable no row of A touches: its row of K is P and sigma alone
        P, A = _psd(40, 0.08, rng), _rand(30, 40, 0.12, rng)
        A[:, 7] = 0.0
        return P, _canon(A)
    if name == "row_one":                 # a row of A with one entry: one term, on a diagonal
        P, A = _psd(40, 0.08, rng), _rand(30, 40, 0.12, rng)
        A[11, :] = 0.0; A[11, 23] = 1.25
        return P, _canon(A)
    if name == "row65":                   # a row of A with 65 entries (the 64-lane turn of k_form_K's inner loop)
        P, A = _psd(120, 0.03, rng), _rand(40, 120, 0.04, rng)
        A[3, :] = 0.0
        c, v = _line(65, 120, rng)
        for cc, vv in zip(c, v): A[3, cc] = vv
        return P, _canon(A)
    if name == "col65":                   # a column of A with 65 entries (the 64-lane turn of its outer loop; a 65-term diagonal)
        P, A = _psd(60, 0.05, rng), _rand(130, 60, 0.04, rng)
        A[:, 5] = 0.0
        r, v = _line(65, 130, rng)
        for rr, vv in zip(r, v): A[rr, 5] = vv
        return P, _canon(A)
    if name == "no_diag":                 # P stores no diagonal entry: the diagonal of K exists through sigma (and A'A) alone
        B = sparse.csc_matrix(_rand(50, 50, 0.06, rng))
        P = sparse.triu(B, 1)
        return _canon(P + P.T), _canon(_rand(35, 50, 0.1, rng))
    if name == "m0":                      # no constraint at all
        return _psd(30, 0.1, rng), sparse.csc_matrix((0, 30))
    if name == "krow300":                 # rows of K with more than 256 entries (k_form_K's `eb += 256` turn): a row of A with 280
        P, A = _psd(300, 0.01, rng), _rand(60, 300, 0.02, rng)
        A[9, :] = 0.0
        c, v = _line(280, 300, rng)
        for cc, vv in zip(c, v): A[9, cc] = vv
        return P, _canon(A)
    raise KeyError(name)


PLAN_CASES = ("n1", "empty_col", "row_one", "row65", "col65", "no_diag", "m0")
GPU_CASES = PLAN_CASES + ("krow300",)
