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
    if name == "row65":                   # a row of A with 65 entries: the 64-lane turn of k_form_K's inner loop (`ec += 64`), not a turn of
                                          # k_form_K_lists -- its lists have one term per shared row, here a handful at most
        P, A = _psd(120, 0.03, rng), _rand(40, 120, 0.04, rng)
        A[3, :] = 0.0
        c, v = _line(65, 120, rng)
        for cc, vv in zip(c, v): A[3, cc] = vv
        return P, _canon(A)
    if name == "col65":                   # a column of A with 65 entries: the 64-lane turn of k_form_K's outer loop (`kc += 64`).  For
                                          # k_form_K_lists a 65-term diagonal is 2 + 63: ONE gather, partly filled (its turns: col66 ...)
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
    # ---- the turns of k_form_K_lists: a lane adds an entry's first FKL_T = 2 terms, the wavefront gathers the rest 64 at a time ----
    if name in LONG_COL:                  # col65's recipe with a column of L entries; the diagonal list is 2 + (L - 2): a full last lane of
        L = LONG_COL[name]                # the one gather (66), a second gather of 1 (67), two full ones (130), a third (131)
        m = max(L + 20, 90)
        P, A = _psd(60, 0.05, rng), _rand(m, 60, 0.04, rng)
        A[:, 5] = 0.0
        r, v = _line(L, m, rng)
        for rr, vv in zip(r, v): A[rr, 5] = vv
        return P, _canon(A)
    if name in ("pair2", "pair3"):        # three columns on one and the same set of 2 (3) rows: off-diagonal lists of exactly FKL_T
        k = int(name[-1])                 # (FKL_T + 1) terms -- nothing (one term) left for the wavefront
        P, A = _psd(33, 0.08, rng), _rand(30, 33, 0.1, rng)
        r = np.sort(rng.choice(30, k, replace=False))
        for cc in PAIR_COLS:
            A[:, cc] = 0.0
            for rr in r: A[rr, cc] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
        return P, _canon(A)
    if name == "shared70x67":             # columns 0 .. 69 all hold the same 67 rows: 4 900 entries of K, off-diagonal ones included, with
        P, A = _psd(100, 0.03, rng), _rand(107, 100, 0.03, rng)      # a two-gather list; in their rows every lane of slot 0 and six of slot 1
        r = np.sort(rng.choice(107, 67, replace=False))
        for cc in range(70):
            A[:, cc] = 0.0
            for rr in r: A[rr, cc] = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
        return P, _canon(A)
    if name == "krow300_tail":            # krow300 with variable n - 1 in the 280-entry row and 70 rows in column n - 1: the diagonal of the
        P, A = _psd(300, 0.01, rng), _rand(90, 300, 0.02, rng)       # last row of K, a 70-term list, sits in the second `eb += 256` pass
        A[9, :] = 0.0; A[:, 299] = 0.0
        c, v = _line(279, 299, rng)
        for cc, vv in zip(c, v): A[9, cc] = vv
        r, v = _line(69, np.delete(np.arange(90), 9), rng)
        for rr, vv in zip(r, v): A[rr, 299] = vv
        A[9, 299] = 1.25
        return P, _canon(A)
    raise KeyError(name)


LONG_COL = dict(col66=66, col67=67, col130=130, col131=131)
PAIR_COLS = (4, 17, 29)


def check_premise(name, Kptr, Kcol, lens):
    """What a case is there for, from the lengths of its lists (diff(Kcp), entries in the order of Kcol): a change of recipe cannot
    empty the case without notice.  Returns (longest list, lists of 67 terms or more)."""
    Kptr, Kcol, lens = np.asarray(Kptr), np.asarray(Kcol), np.asarray(lens)
    rows = np.repeat(np.arange(len(Kptr) - 1), np.diff(Kptr))
    longest, over = int(lens.max()) if len(lens) else 0, int((lens > 66).sum())
    if name in LONG_COL:
        L = LONG_COL[name]
        assert longest == L and over == (1 if L > 66 else 0), (name, longest, over)
        assert lens[(rows == 5) & (Kcol == 5)] == L                                  # the diagonal of the planted column
        assert int((lens > 2).sum()) > 1                                             # and shorter lists for the wavefront next to it
    if name in ("pair2", "pair3"):
        k = int(name[-1])
        among = np.isin(rows, PAIR_COLS) & np.isin(Kcol, PAIR_COLS)
        assert among.sum() == 9 and (lens[among] == k).all(), (name, lens[among])     # six of them off the diagonal
    if name == "shared70x67":
        among = (rows < 70) & (Kcol < 70)
        assert among.sum() == 4900 and (lens[among] == 67).all() and longest == 67 and over == 4900, (name, longest, over)
        assert (Kcol[Kptr[0]:Kptr[0] + 70] == np.arange(70)).all() and Kptr[1] - Kptr[0] > 70      # slot 0 of row 0: 64 lanes pending
    if name == "krow300_tail":
        n = len(Kptr) - 1
        at = np.flatnonzero((rows == n - 1) & (Kcol == n - 1))
        assert len(at) == 1 and at[0] - Kptr[n - 1] >= 256 and lens[at[0]] == 70 and longest == 70 and over == 1, (name, at, longest, over)
    if name in ("krow300", "krow300_tail"):
        assert np.diff(Kptr).max() > 256
    return longest, over


PLAN_CASES = ("n1", "empty_col", "row_one", "row65", "col65", "no_diag", "m0", "col66", "col67", "col130", "col131", "pair2", "pair3", "shared70x67")
GPU_CASES = PLAN_CASES + ("krow300", "krow300_tail")
HOST_CASES = PLAN_CASES + ("krow300_tail",)
