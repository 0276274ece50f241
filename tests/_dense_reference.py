"""References and case tables for the dense-direct GEMM kernels and inversion routes (csrc/dense_direct.h), shared by
tests/test_dense_reference_host.py (CPU: the references and bars themselves) and tests/test_gpu_dense_kernels.py (the device).
Nothing here touches the device or the library.

GEMM.  gemm_reference restates, in np.longdouble, what one launch of k_dd_gemm_tn / k_dd_gemm_tn_lds must leave in C:
    C = beta C0 + alpha T' diag(w) B    on every 128 x 128 tile that is not masked,
with the kernels' masks: a tile whose first row lies in [sr0, sr1) or first column in [sc0, sc1) is untouched; with `lower` so is
a tile above the diagonal (col0 > row0); kmode 1 sums k >= col0, kmode 2 sums k >= row0; beta == 0 does not read C0; rows >= M and
columns >= N are untouched.  The elementwise bound is derived, not tuned:
    (K + 5) 2^-53 (|beta| |C0| + |alpha| |T|' diag|w| |B|)      (the sums over the same k)
-- gamma_K for a sum of K products in any order (so with or without FMA, for any chunking and for split K, whose slice sums only
regroup the same K terms), plus one rounding each for the weight, alpha, beta and the final add; (K + 4) u / (1 - (K + 4) u) <=
(K + 5) u for every K here.  No margin on top.

Inversion.  sweep_reference / chol_reference are float64 numpy restatements of dd_invert_sweep / dd_invert_chol block by block
(128-wide blocks, lower tiles only kept up to date, mirrored at the end); truth_inverse is numpy's inverse refined by two
Newton-Schulz steps in np.longdouble.  The bar of a route on a matrix is 10 x the error of that route's restatement on the same
matrix (the standing margin for "same algorithm, different summation order") + n 2^-53 max|A^-1|.

`defect=` plants the one-place defects of GEMM_DEFECTS / SWEEP_DEFECTS in the float64 models; the CPU test shows each misses its
bar by more than 10 x."""
import numpy as np
from scipy.linalg import solve_triangular

LD = np.longdouble
NB = 128
U = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------
# GEMM cases
# ---------------------------------------------------------------------------------------------------------------
def _entries(rng, shape):
    """Magnitudes in [0.5, 2], either sign."""
    return rng.choice([-1.0, 1.0], size=shape) * rng.uniform(0.5, 2.0, size=shape)


def _gemm_case(name, M, N, K, seed, ld=None, w=True, alpha=1.0, beta=0.0, sr=(-1, -1), sc=(-1, -1), lower=0, kmode=0, ksl=0, c0="rand"):
    rng = np.random.default_rng(seed)
    Mp = -(-M // NB) * NB
    ldt, ldb, ldc = (ld, ld, ld) if ld else (M + (M & 1), N + (N & 1), N + (N & 1))
    C0 = np.full((Mp, ldc), np.nan) if c0 == "nan" else _entries(rng, (Mp, ldc))
    return dict(name=name, M=M, N=N, K=K, ldt=ldt, ldb=ldb, ldc=ldc, T=_entries(rng, (K, ldt)), B=_entries(rng, (K, ldb)),
                w=rng.uniform(0.5, 2.0, K) if w else None, C0=C0, alpha=alpha, beta=beta, sr=sr, sc=sc, lower=lower, kmode=kmode, ksl=ksl)


def _gemm_table():
    t = []
    # K across the chunk edges of both kernels (8 = 4 DD_CH, 16 = DD_KC): K = 16 never takes the `more` branch, K = 17 leaves one
    # valid row in the second LDS buffer
    for K in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 129):
        t.append(_gemm_case(f"k{K}", 128, 128, K, seed=1000 + K))
    for K in (5, 17):
        t.append(_gemm_case(f"k{K}_no_w", 128, 128, K, seed=2000 + K, w=False))
    t.append(_gemm_case("beta0_nan", 128, 128, 17, seed=3001, c0="nan"))
    t.append(_gemm_case("beta1_alpha-1", 128, 128, 128, seed=3002, w=False, alpha=-1.0, beta=1.0))
    # the sweep's trailing update at kb = 1 of three blocks: only tiles (0,0), (2,0), (2,2) change
    t.append(_gemm_case("sweep_kb1", 384, 384, 128, seed=3003, w=False, alpha=-1.0, beta=1.0, sr=(128, 256), sc=(128, 256), lower=1))
    # the Cholesky route's at kb = 0
    t.append(_gemm_case("chol_kb0", 384, 384, 128, seed=3004, w=False, alpha=-1.0, beta=1.0, sr=(0, 128), sc=(0, 128), lower=1))
    # X'X: operands that are NOT lower triangular, so where k starts is visible
    t.append(_gemm_case("kmode2", 256, 256, 256, seed=3005, w=False, lower=1, kmode=2))
    # a block row of the triangular inverse: two K slices, the second of 128 k; for the column tile 512 kbeg = max(col0, z ksl)
    t.append(_gemm_case("kmode1_split2", 128, 640, 640, seed=3006, w=False, kmode=1, ksl=512))
    t.append(_gemm_case("kmode1_split1", 128, 384, 384, seed=3007, w=False, kmode=1, ksl=512))
    # the M / N guards (even: the double2 loads end on the edge) and odd ones (the scalar tail of the LDS kernel)
    t.append(_gemm_case("guards", 130, 254, 20, seed=3008, ld=256))
    t.append(_gemm_case("guards_odd", 129, 253, 20, seed=3009, ld=256))
    return t


GEMM_CASES = {c["name"]: c for c in _gemm_table()}

# defect -> the cases it is planted in
GEMM_DEFECTS = {
    "last k dropped when K % 4 != 0": ("k1", "k5", "k17", "k33", "k129", "k5_no_w"),
    "weight taken from k - 1": ("k3", "k16", "k17", "guards"),
    "skip range off by one tile": ("sweep_kb1", "chol_kb0"),
    "upper tile written under lower": ("sweep_kb1", "chol_kb0", "kmode2"),
    "kmode starting at 0": ("kmode2", "kmode1_split2", "kmode1_split1"),
    "slice dropped from the split-K sum": ("kmode1_split2",),
}


def _gemm(c, dtype, defect=None):
    """(result, touched, magnitude): the product in `dtype` with the kernels' masks; magnitude = |beta||C0| + |alpha||T|'|w||B|."""
    M, N, K, alpha, beta, ksl = c["M"], c["N"], c["K"], c["alpha"], c["beta"], c["ksl"]
    T, B, C0 = c["T"].astype(dtype), c["B"].astype(dtype), c["C0"]
    w = (np.ones(K) if c["w"] is None else c["w"]).astype(dtype)
    (sr0, sr1), (sc0, sc1) = c["sr"], c["sc"]
    Kend = K
    if defect == "last k dropped when K % 4 != 0" and K % 4:
        Kend = K - 1
    if defect == "weight taken from k - 1":
        w = np.roll(w, 1)
    if defect == "skip range off by one tile":
        sr0, sr1 = sr0 + NB, sr1 + NB
    out = C0.astype(dtype)
    touched = np.zeros(C0.shape, dtype=bool)
    mag = np.zeros(C0.shape)
    for r0 in range(0, M, NB):
        for c0 in range(0, N, NB):
            if sr0 <= r0 < sr1 or sc0 <= c0 < sc1:
                continue
            if c["lower"] and c0 > r0 and defect != "upper tile written under lower":
                continue
            kbeg = (0, c0, r0)[c["kmode"]]
            if defect == "kmode starting at 0":
                kbeg = 0
            rows, cols = slice(r0, min(r0 + NB, M)), slice(c0, min(c0 + NB, N))
            spans = [(kbeg, Kend)] if not ksl else [(max(kbeg, z * ksl), min(Kend, (z + 1) * ksl)) for z in range(-(-K // ksl))]
            if defect == "slice dropped from the split-K sum":
                spans = spans[:-1]
            acc = np.zeros((rows.stop - rows.start, cols.stop - cols.start), dtype=dtype)
            for a, b in spans:                                 # (a slice's own sum first, then the slices in order: k_dd_sum_slices)
                if b > a:
                    acc = acc + T[a:b, rows].T @ (w[a:b, None] * B[a:b, cols])
            val = dtype(alpha) * acc
            m = abs(alpha) * (np.abs(c["T"][kbeg:K, rows]).T @ (np.abs(w[kbeg:K, None].astype(float)) * np.abs(c["B"][kbeg:K, cols])))
            if beta != 0.0:
                val = dtype(beta) * C0[rows, cols].astype(dtype) + val
                m = m + abs(beta) * np.abs(C0[rows, cols])
            out[rows, cols], touched[rows, cols], mag[rows, cols] = val, True, m
    return out, touched, mag


def gemm_reference(c):
    """(result in np.longdouble, mask of the entries that must stay bit-for-bit C0, elementwise bound)."""
    ref, touched, mag = _gemm(c, LD)
    return ref, ~touched, (c["K"] + 5) * U * mag


def gemm_model(c, defect=None):
    """The same product in float64 numpy, with one of GEMM_DEFECTS planted if named."""
    return _gemm(c, np.float64, defect)[0]


def gemm_miss(got, c, ref, untouched, bound):
    """(worst err / bound, number of untouched entries that changed).  A NaN, or any change to an untouched entry (its bound is
    zero), counts as infinitely far."""
    changed = int((untouched & (got.view(np.uint64) != c["C0"].view(np.uint64))).sum())
    err = np.abs(got.astype(LD) - ref)[~untouched].astype(float)
    err = np.where(np.isfinite(err), err, np.inf)
    b = bound[~untouched]
    ratio = np.where(err == 0.0, 0.0, err / np.where(b > 0.0, b, 1e-300))
    return (np.inf if changed else float(ratio.max())), changed


# ---------------------------------------------------------------------------------------------------------------
# inversion: the two routes restated, the truth, the cases
# ---------------------------------------------------------------------------------------------------------------
SWEEP, CHOL = 0, 1
SWEEP_DEFECTS = ("the sweep without its final negation", "the mirror taken from the wrong triangle", "one trailing tile not updated")


def _mirror(S, neg, wrong_triangle=False):
    """k_dd_mirror: the lower triangle (element-wise) copied over the upper one, negated when neg."""
    L = np.triu(S).T if wrong_triangle else np.tril(S)
    L = -L if neg else L
    return L + np.tril(L, -1).T


def sweep_reference(A, defect=None):
    """dd_invert_sweep in float64 numpy.  Per pivot block k: D = inv(A_kk); W = column panel k (below the block from the column
    panel, left of it from the row panel: only lower tiles are current); V = W D; A_ij -= V_i W_j' on the lower tiles outside block
    row / column k; panel <- V, A_kk <- -D.  Then mirrored and negated."""
    n = A.shape[0]
    nb = n // NB
    S = A.copy()
    blk = lambda i: slice(i * NB, (i + 1) * NB)
    for kb in range(nb):
        p0, p1 = kb * NB, (kb + 1) * NB
        D = np.linalg.inv(S[p0:p1, p0:p1])
        W = np.concatenate([S[p0:p1, :p0].T, S[p0:, p0:p1]], axis=0)          # n x 128 (rows p0:p1: the pivot block itself, unused)
        V = W @ D
        for i in range(nb):
            for j in range(i + 1):
                if i == kb or j == kb:
                    continue
                if defect == "one trailing tile not updated" and kb == 0 and (i, j) == (nb - 1, nb - 1):
                    continue
                S[blk(i), blk(j)] -= V[blk(i)] @ W[blk(j)].T
        S[p1:, p0:p1] = V[p1:]
        S[p0:p1, :p0] = V[:p0].T
        S[p0:p1, p0:p1] = -D
    return _mirror(S, defect != "the sweep without its final negation", defect == "the mirror taken from the wrong triangle")


def chol_reference(A):
    """dd_invert_chol in float64 numpy: (a) A = L L' by block columns (diagonal factor, panel solved against it, trailing lower
    tiles), (b) X = L^-1 in place block row by block row, (c) A^-1 = X'X on the lower tiles with k from the row tile on, mirrored."""
    n = A.shape[0]
    nb = n // NB
    S = A.copy()
    blk = lambda i: slice(i * NB, (i + 1) * NB)
    for kb in range(nb):
        p0, p1 = kb * NB, (kb + 1) * NB
        L = np.linalg.cholesky(S[p0:p1, p0:p1])
        S[p0:p1, p0:p1] = L
        if p1 >= n:
            break
        Z = solve_triangular(L, S[p1:, p0:p1].T, lower=True).T               # Z_i = W_i L^-T
        for i in range(kb + 1, nb):
            for j in range(kb + 1, i + 1):
                S[blk(i), blk(j)] -= Z[(i - kb - 1) * NB:(i - kb) * NB] @ Z[(j - kb - 1) * NB:(j - kb) * NB].T
        S[p1:, p0:p1] = Z
    for kb in range(nb):
        p0, p1 = kb * NB, (kb + 1) * NB
        L = S[p0:p1, p0:p1].copy()
        if kb > 0:
            Y = np.zeros((NB, p0))
            for j in range(kb):                                                   # X_0:i,0:i is lower triangular: k from the column tile on
                Y[:, blk(j)] = S[p0:p1, j * NB:p0] @ S[j * NB:p0, blk(j)]
            S[p0:p1, :p0] = -solve_triangular(L, Y, lower=True)
        S[p0:p1, p0:p1] = solve_triangular(L, np.eye(NB), lower=True)
    X2 = np.zeros((n, n))
    for i in range(nb):
        for j in range(i + 1):
            X2[blk(i), blk(j)] = S[i * NB:, blk(i)].T @ S[i * NB:, blk(j)]
    return _mirror(X2, False)


def _mm(a, b):
    """a @ b in np.longdouble (numpy has no BLAS for it; rows against contiguous rows is four times faster than its matmul)."""
    return np.inner(a.astype(LD), np.ascontiguousarray(b.T.astype(LD)))


def truth_inverse(A):
    """numpy's inverse, then two Newton-Schulz steps X <- X (2 I - A X) in np.longdouble."""
    X = np.linalg.inv(A).astype(LD)
    two = 2 * np.eye(A.shape[0], dtype=LD)
    for _ in range(2):
        X = _mm(X, two - _mm(A, X))
    return X


def _spd(n, seed, lo=1.0, hi=10.0, log=False):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n) if log else rng.uniform(lo, hi, n)
    ev[0], ev[-1] = lo, hi
    A = (Q * ev) @ Q.T
    return 0.5 * (A + A.T)


def _invert_matrix(name):
    if name == "n128":                        # one block: no panel, no GEMM
        return _spd(128, 11)
    if name == "n256":
        return _spd(256, 12)
    if name == "n768":                        # the first n at which step (b) of the Cholesky route has two K slices (p0 = 640)
        return _spd(768, 13)
    if name == "tail256":                     # what padding na = 129 to nap = 256 leaves: the last 127 rows and columns are the identity
        A = np.eye(256)
        A[:129, :129] = _spd(129, 14)
        return A
    if name == "spread384":                   # eigenvalues spread over [1, 1e3]
        return _spd(384, 15, 1.0, 1e3, log=True)
    raise KeyError(name)


INVERT_NAMES = ("n128", "n256", "n768", "tail256", "spread384")
_cache = {}


def invert_case(name):
    """The matrix, its truth, and per route the restatement's error and the bar -- computed once per process, never changed."""
    if name not in _cache:
        A = _invert_matrix(name)
        n = A.shape[0]
        truth = truth_inverse(A)
        c = dict(name=name, n=n, A=A, truth=truth, resid0=(_mm(truth, A) - np.eye(n, dtype=LD)).astype(float),
                 amax=float(np.abs(truth).max()), floor=n * U * float(np.abs(truth).max()))
        c["numpy"] = invert_errors(c, np.linalg.inv(A))
        for route, f in ((SWEEP, sweep_reference), (CHOL, chol_reference)):
            e = invert_errors(c, f(A))
            c[route] = dict(err=e, bar=(10.0 * e[0] + c["floor"], 10.0 * e[1] + c["floor"]))
        for v in (A, truth, c["resid0"]):
            v.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def invert_errors(c, X):
    """(max |X - truth|, max |X A - I|) of a float64 inverse X.  X A - I = (truth A - I) + (X - truth) A: the first term (long
    double roundings times cond: 1e-19 .. 4e-16 here) is computed once in long double, the second is a float64 product of a difference that is itself O(eps)."""
    E = (X.astype(LD) - c["truth"]).astype(float)
    if not np.all(np.isfinite(E)):
        return np.inf, np.inf
    return float(np.abs(E).max()), float(np.abs(c["resid0"] + E @ c["A"]).max())


def verdict_cases():
    """(tag, 256 x 256 matrix, verdict): 1 = a pivot is not positive."""
    out = [("identity", np.eye(256), 0)]
    for i in (0, 31, 32, 127, 128, 255):      # sub-block edges of k_dd_pivot, the block edge, the last pivot
        A = np.eye(256); A[i, i] = -1.0
        out.append((f"-1 at {i}", A, 1))
    A = np.eye(256); A[40, 40] = 0.0
    out.append(("0 at 40", A, 1))
    A = np.eye(256); A[5, 200] = A[200, 5] = 3.0      # positive diagonal, indefinite through the Schur complement only (1 - 9), across two blocks
    out.append(("coupling 3 between 5 and 200", A, 1))
    return out
