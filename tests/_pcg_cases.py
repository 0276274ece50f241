"""Seeded cases for the three PCG forms of the single-QP engine at their structural edges (tests/test_pcg_cases_host.py checks
them on the CPU, tests/test_gpu_pcg_edges.py runs them on the device), a Python restatement of the engine's host-side
classification of (P, A) (engine.hip: build_dense, build_blocks, upload_mat, the split rule) and the operator mutations that
show what the bar on x~ does not forgive.  Nothing here touches the library.

make(name) returns the keys of _engine_reference.make_case (name, n, m, Pu, A, q, l, u, rho, ...) and `claims`: what the case
is built to be -- dense (start, size, pitch) blocks, long / huge rows of A, long rows of M, split, 16-bit flags -- stated by
hand in each generator and compared with structure() by the CPU test.  Every K = P + sigma I + A' rho A is well conditioned:
blocks of P have eigenvalues in about [1, 10], a row of A with k entries is scaled by 1 / sqrt(k), and rho takes the classes
RHO, 1e3 RHO (equality rows) and RHO_MIN (free rows)."""
import functools

import numpy as np
from scipy import sparse

from tests import _engine_reference as R

RHO, RHO_MIN, INF = R.RHO, 1e-6, R.INF
PCG_EPS = 1e-12
LONG_ROW, HUGE_ROW, DENSE_MIN, DENSE_MAX, MAX_HUGE_FOLD = 512, 8192, 32, 128, 4
MIXED_SIZES = (32, 31, 33, 64, 129, 63, 65, 96, 127, 128)
BR_SIZES = (32, 33, 63, 64, 65, 96, 127, 128)
HUGE_LENGTHS = (8192, 8193, 8200, 8192, 8193)
# resident cases: E -> (n, m, off-diagonal entries per row of P, entries per row of A, forced grid); found with
# hipeng_resident_plan, which tests/test_pcg_cases_host.py asks again
RESIDENT = {8: (427, 210, 6, 3, 7), 16: (610, 300, 85, 4, 10), 20: (610, 300, 120, 4, 10), 24: (610, 300, 150, 4, 10),
            32: (610, 300, 195, 4, 10), 48: (610, 300, 280, 4, 10), 64: (610, 300, 400, 4, 10)}

NAMES = (("blocks_mixed", "blocks_threshold", "blocks_holes", "huge_nh1", "huge_nh4", "huge_nh5", "blocks_huge4", "blocks_huge5",
          "split3", "c16_narrow", "c16_m_wide", "c16_wide", "c16d_narrow", "c16d_m_wide", "c16d_wide", "br_sizes_nh0", "br_sizes_nh1", "br_sizes_nh4")
         + tuple("res_e%d" % e for e in RESIDENT))
SEEDS = {name: 101 + k for k, name in enumerate(NAMES)}
SEEDS.update(br_probe=200, br_pairs=201, br_pairs_plus1=202)
R.SEEDS.update(SEEDS)          # R.iterates(case) draws from its table by name


# ---------------------------------------------------------------------------------------------------------------
# the engine's host-side classification, restated
# ---------------------------------------------------------------------------------------------------------------
def dense_blocks(Pu):
    """build_dense: column j starts a diagonal block iff no later column of triu(P) reaches above row j; a block of 32 <= b <= 128
    rows with 2 nnz - b >= b^2 / 2 (nnz: stored entries of triu(P) in its columns, explicit zeros included; integer division)
    is dense, with pitch b rounded up to even, plus 2 when that is a multiple of 32 below 128.  Returns [(start, b, pitch)]."""
    Pu = sparse.csc_matrix(Pu)
    n = Pu.shape[0]
    lo = np.arange(n)
    for j in range(n):
        if Pu.indptr[j + 1] > Pu.indptr[j]:
            lo[j] = min(j, int(Pu.indices[Pu.indptr[j]:Pu.indptr[j + 1]].min()))
    smin = np.minimum.accumulate(lo[::-1])[::-1]
    out, s0 = [], 0
    for j in range(1, n + 1):
        if j < n and smin[j] < j:
            continue
        b, nnz = j - s0, int(Pu.indptr[j] - Pu.indptr[s0])
        pitch = (b + 1) & ~1
        if pitch % 32 == 0 and pitch < DENSE_MAX:
            pitch += 2
        if DENSE_MIN <= b <= DENSE_MAX and 2 * nnz - b >= (b * b) // 2:
            out.append((s0, b, pitch))
        s0 = j
    return out


def structure(case, hfold=True):
    """What hipeng_pcg_layout reports for the case, from (triu(P), A) alone: dense blocks, row classes of A (build_blocks: < 512
    stream, >= 512 long, >= 8192 huge) and of the matrix k_cg_B streams, folded huge rows, the split rule, 16-bit column ids."""
    Pu, A = sparse.csc_matrix(case["Pu"]), sparse.csr_matrix(case["A"])
    n, m = case["n"], case["m"]
    dense = dense_blocks(Pu)
    in_dense = np.zeros(n, bool)
    for c0, b, _ in dense:
        in_dense[c0:c0 + b] = True
    lenA = np.diff(A.indptr)
    huge = [int(i) for i in np.flatnonzero(lenA >= HUGE_ROW)]
    longs = [int(i) for i in np.flatnonzero((lenA >= LONG_ROW) & (lenA < HUGE_ROW))]
    folded = huge if hfold and len(huge) <= MAX_HUGE_FOLD else []
    lenP = _full_row_lengths(Pu)
    Ac = sparse.csc_matrix(case["A"])
    lenAT = np.diff(Ac.indptr)
    lenM = lenP + lenAT
    if dense or folded:
        fold_cnt = np.zeros(n, int)
        for h in folded:
            fold_cnt[A.indices[A.indptr[h]:A.indptr[h + 1]]] += 1
        lenB = np.where(in_dense, 0, lenP) + lenAT - fold_cnt
        rowsB = np.flatnonzero(~in_dense) if dense else np.arange(n)
    else:
        lenB, rowsB = lenM, np.arange(n)
    lnnz = int(lenA[longs].sum())
    maxA = int(A.indices.max()) if A.nnz else -1
    maxM = max(n - 1 if Pu.nnz else -1, n + int(np.flatnonzero(lenA > 0).max()) if A.nnz else -1)
    longM, longB = int((lenM >= LONG_ROW).sum()), int((lenB[rowsB] >= LONG_ROW).sum())
    # the remainder Mr keeps the P part of the rows outside dense blocks and every A' entry that is not in a folded row
    keep_rows = np.setdiff1d(np.flatnonzero(lenA > 0), folded)
    pcol = np.repeat(np.arange(n), np.diff(Pu.indptr))
    p_ids = np.concatenate([pcol[~in_dense[Pu.indices]], Pu.indices[~in_dense[pcol]], [-1]])
    maxB = maxM if not (dense or folded) else max(n + int(keep_rows.max()) if keep_rows.size else -1, int(p_ids.max()))
    return dict(dense=dense, dense_rows=int(in_dense.sum()), long=longs, huge=huge, folded=len(folded),
                split=int(A.nnz > 0 and 2 * lnnz >= A.nnz), a16=int(bool(longs) and maxA <= 0xffff), m16=int(longM > 0 and maxM <= 0xffff),
                b16=int(longB > 0 and maxB <= 0xffff), long_b=longB, max_col_A=maxA, max_col_M=maxM)


def _full_row_lengths(Pu):
    """Stored entries per row of the full symmetric P (both triangles, explicit zeros included)."""
    Pu = sparse.csc_matrix(Pu)
    n = Pu.shape[0]
    col = np.repeat(np.arange(n), np.diff(Pu.indptr))
    off = Pu.indices != col
    return np.bincount(Pu.indices, minlength=n) + np.bincount(col[off], minlength=n)


# ---------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------
def _full_block(rng, b):
    """Dense symmetric b x b with eigenvalues uniform in [1, 10]."""
    Q, _ = np.linalg.qr(rng.standard_normal((b, b)))
    B = (Q * rng.uniform(1.0, 10.0, b)) @ Q.T
    return 0.5 * (B + B.T)


def _pattern_block(rng, b, pairs, zero_pairs=()):
    """Symmetric b x b on the given off-diagonal pairs (i < j): diagonal in [3, 8], off-diagonal rows sum to at most 2 in
    modulus (Gershgorin: eigenvalues in [1, 10]).  Returns (rows, cols, values) of the upper triangle, diagonal included,
    with an explicit zero at each of `zero_pairs`."""
    pairs = np.asarray(pairs, int).reshape(-1, 2)
    cnt = np.bincount(pairs.ravel(), minlength=b).max() if pairs.size else 1
    v = rng.uniform(0.5, 1.0, len(pairs)) * rng.choice([-1.0, 1.0], len(pairs)) * 2.0 / cnt
    zp = np.asarray(zero_pairs, int).reshape(-1, 2)
    r = np.concatenate([np.arange(b), pairs[:, 0], zp[:, 0]])
    c = np.concatenate([np.arange(b), pairs[:, 1], zp[:, 1]])
    return r, c, np.concatenate([rng.uniform(3.0, 8.0, b), v, np.zeros(len(zp))])


def _csc_keep_zeros(r, c, v, n):
    """CSC from unique triplets, explicit zeros kept, indices sorted."""
    order = np.lexsort((r, c))
    r, c, v = np.asarray(r)[order], np.asarray(c)[order], np.asarray(v, float)[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))])
    return sparse.csc_matrix((v, r, indptr), shape=(n, n))


def _block_diag_triu(blocks):
    """triu of the block diagonal of dense arrays, as CSC."""
    r, c, v, s = [], [], [], 0
    for B in blocks:
        b = B.shape[0]
        i, j = np.triu_indices(b)
        r.append(s + i); c.append(s + j); v.append(B[i, j])
        s += b
    return _csc_keep_zeros(np.concatenate(r), np.concatenate(c), np.concatenate(v), s)


def _scaled_row(i, cols, rng):
    """Row i over `cols`: entries of about 1 / sqrt(length), and +-1 on the last one (the entry the A mutation changes, at the odd
    end of the kernels' strides)."""
    cols = np.sort(np.asarray(cols))
    v = np.clip(rng.standard_normal(cols.size), -3.0, 3.0) / np.sqrt(cols.size)
    v[-1] = rng.choice([-1.0, 1.0])
    return (i, cols, v)


def _short(rng, rows_idx, cols, lo=2, hi=6):
    return [(i, c, v / np.sqrt(len(c))) for i, c, v in R._short_rows(rng, rows_idx, 0, lo, hi, cols=cols)]


def _finish(name, rng, Pu, rows, n, m, claims, eq_rows=(), free_rows=(), rho_hi=()):
    """q, bounds and rho by class: equality rows 1e3 RHO, free rows RHO_MIN, `rho_hi` 1e3 RHO, the rest RHO."""
    A = R._rows_to_csc(rows, m, n)
    A.sort_indices()
    longest = int(np.diff(sparse.csr_matrix(A).indptr).argmax())          # (its rho is one of the mutated values: not a free row)
    free_rows = [i for i in free_rows if i != longest]
    q = rng.standard_normal(n)
    l, u = -rng.uniform(0.1, 1.0, m), rng.uniform(0.1, 1.0, m)
    eq, free = np.asarray(eq_rows, int), np.asarray(free_rows, int)
    u[eq] = l[eq]
    l[free], u[free] = -INF, INF
    rho = np.full(m, RHO)
    rho[eq] = 1e3 * RHO
    rho[np.asarray(rho_hi, int)] = 1e3 * RHO
    rho[free] = RHO_MIN
    Pu = sparse.csc_matrix(Pu)
    Pu.sort_indices()
    return dict(name=name, n=n, m=m, Pu=Pu, A=A, q=q, l=l, u=u, rho=rho, special_rows=[], special_cols=[], peaks=[], claims=claims)


def _classes(rng, m, skip=()):
    """A tenth of the rows equalities, a twentieth free, none of `skip`."""
    pool = np.setdiff1d(np.arange(m), np.asarray(skip, int))
    pick = rng.permutation(pool)
    ne, nf = max(1, len(pool) // 10), max(1, len(pool) // 20)
    return pick[:ne], pick[ne:ne + nf]


def _pitch(b):
    p = (b + 1) & ~1
    return p + 2 if p % 32 == 0 and p < DENSE_MAX else p


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
def _blocks_mixed(name, rng):
    sizes = MIXED_SIZES
    n = sum(sizes)
    Pu = _block_diag_triu([_full_block(rng, b) for b in sizes])
    starts = np.concatenate([[0], np.cumsum(sizes)])
    dead = np.array([5, 40, 300, 500, n - 1])                       # no entry in A (the last variable of the last dense block among them)
    live = rng.permutation(np.setdiff1d(np.arange(n), dead))
    rows, i, k = [], 0, 0
    while k < live.size:                                            # 2-3-entry rows over a permutation: across blocks
        w = min(int(rng.integers(2, 4)), live.size - k)
        if live.size - k - w == 1:
            w += 1
        c = np.sort(live[k:k + w])
        rows.append((i, c, rng.uniform(0.5, 2.0, w) * rng.choice([-1.0, 1.0], w) / np.sqrt(w)))
        i, k = i + 1, k + w
    for s, b in zip(starts[:-1], sizes):                            # four single-entry rows per block
        for j in rng.choice(np.setdiff1d(np.arange(s, s + b), dead), 4, replace=False):
            rows.append((i, np.array([j]), rng.uniform(0.5, 2.0, 1) * rng.choice([-1.0, 1.0], 1)))
            i += 1
    m = i
    eq, free = _classes(rng, m)
    dense = [(int(s), b, _pitch(b)) for s, b in zip(starts[:-1], sizes) if b not in (31, 129)]
    return _finish(name, rng, Pu, rows, n, m, dict(dense=dense, long=[], huge=[], folded=0, split=0, long_b=0), eq, free)


def _chain_pairs(b, extra, rng, last_free=False):
    """The superdiagonal (it ties the block together) and `extra` more off-diagonal pairs; last_free: none of them in the last
    row and column."""
    top = b - 1 if last_free else b
    chain = [(i, i + 1) for i in range(top - 1)]
    pool = [(i, j) for i in range(top) for j in range(i + 2, top)]
    pick = rng.choice(len(pool), extra - len(chain), replace=False)
    return chain + [pool[k] for k in pick]


def _blocks_threshold(name, rng):
    """Two blocks of 64: 2 nnz - b = b^2 / 2 = 2048 needs nnz = 1056 = 64 + 992 pairs; the second block has 991."""
    b, n = 64, 128
    r0, c0, v0 = _pattern_block(rng, b, _chain_pairs(b, 992, rng))
    r1, c1, v1 = _pattern_block(rng, b, _chain_pairs(b, 991, rng))
    Pu = _csc_keep_zeros(np.concatenate([r0, b + r1]), np.concatenate([c0, b + c1]), np.concatenate([v0, v1]), n)
    m = 60
    rows = _short(rng, range(m), np.arange(n), 1, 3)
    eq, free = _classes(rng, m)
    return _finish(name, rng, Pu, rows, n, m, dict(dense=[(0, 64, 66)], long=[], huge=[], folded=0, split=0, long_b=0), eq, free)


def _blocks_holes(name, rng):
    """One block of 128 at 60 % fill; the last row and column hold only the diagonal in value: two explicit zeros, at (0, 127)
    and (64, 127), keep them in the block's pattern, (126, 127) is a structural zero; twenty more explicit zeros inside."""
    b = n = 128
    want = int(0.6 * b * b)                                         # stored entries of the full block
    pairs = _chain_pairs(b, (want - b) // 2 - 22, rng, last_free=True)
    have = set(pairs)
    zeros = [(0, 127), (64, 127)]
    while len(zeros) < 22:
        i, j = sorted(int(t) for t in rng.choice(b - 1, 2, replace=False))
        if (i, j) not in have and (i, j) not in zeros:
            zeros.append((i, j))
    r, c, v = _pattern_block(rng, b, pairs, zeros)
    Pu = _csc_keep_zeros(r, c, v, n)
    m = 70
    rows = _short(rng, range(m), np.arange(n), 1, 3)
    eq, free = _classes(rng, m)
    return _finish(name, rng, Pu, rows, n, m, dict(dense=[(0, 128, 128)], long=[], huge=[], folded=0, split=0, long_b=0), eq, free)


def _huge(name, rng, nh):
    """P diagonal, n = 8200; rows 0..nh-1 huge (8192, 8193, 8200, 8192, 8193 entries over the first variables), row nh long
    (8191 entries), 40 short rows on the first 8192 variables.  No column has exactly one entry in a row that is not huge, so no
    variable is eliminated."""
    n, m = 8200, nh + 41
    Pu = sparse.diags(rng.uniform(1.0, 10.0, n), format="csc")
    rows = [_scaled_row(i, np.arange(HUGE_LENGTHS[i]), rng) for i in range(nh)]
    rows.append(_scaled_row(nh, np.arange(8191), rng))
    rows += _short(rng, range(nh + 1, m), np.arange(8192))
    eq, free = _classes(rng, m, skip=range(nh + 1))
    hi = [nh - 1] if nh > 1 else []                                 # the last huge row carries 1e3 RHO
    claims = dict(dense=[], long=[nh], huge=list(range(nh)), folded=nh if nh <= MAX_HUGE_FOLD else 0, split=0, long_b=0)
    return _finish(name, rng, Pu, rows, n, m, claims, eq, free, rho_hi=hi)


def _blocks_with_rows(name, rng, sizes, nh):
    """Dense diagonal blocks only, one single-entry (box) row per variable, then nh huge rows over every variable."""
    n = int(sum(sizes))
    cache = {}
    blocks = []
    for k, b in enumerate(sizes):
        if b not in cache or k % 7 == 0:                            # (a handful of distinct blocks per size: the set-up stays quick)
            cache[b] = _full_block(rng, b)
        blocks.append(cache[b] * rng.uniform(0.8, 1.0))
    Pu = _block_diag_triu(blocks)
    m = n + nh
    rows = [(j, np.array([j]), rng.uniform(0.5, 2.0, 1) * rng.choice([-1.0, 1.0], 1)) for j in range(n)]
    rows += [_scaled_row(n + k, np.arange(n), rng) for k in range(nh)]
    eq, free = _classes(rng, m, skip=range(n, m))
    starts = np.concatenate([[0], np.cumsum(sizes)])
    claims = dict(dense=[(int(s), int(b), _pitch(int(b))) for s, b in zip(starts[:-1], sizes)], long=[], huge=list(range(n, m)),
                  folded=nh if nh <= MAX_HUGE_FOLD else 0, split=0, long_b=0)
    return _finish(name, rng, Pu, rows, n, m, claims, eq, free, rho_hi=[m - 1] if nh > 1 else [])


def br_probe():
    """Two dense blocks of 32 and a box row per variable: the smallest problem form 2 takes (the GPU test reads its grid)."""
    return _blocks_with_rows("br_probe", np.random.default_rng(SEEDS["br_probe"]), [32, 32], 0)


def br_pairs(nwg, extra=0):
    """2 nwg (+ extra) dense blocks in the order 128, 128, 32, 32, 128, 32, 32, 128: a grid of nwg workgroups takes them two
    each, as 128 + 128 = 256, 32 + 32, 128 + 32 and 32 + 128 rows; one huge row over every variable."""
    name = "br_pairs_plus1" if extra else "br_pairs"
    sizes = [(128, 128, 32, 32, 128, 32, 32, 128)[k % 8] for k in range(2 * nwg + extra)]
    return _blocks_with_rows(name, np.random.default_rng(SEEDS[name]), sizes, 1)


def _split3(name, rng):
    n, m = 700, 3
    Pu = R._tridiag(n, rng)
    rows = [_scaled_row(i, rng.choice(n, 600, replace=False), rng) for i in range(m)]
    return _finish(name, rng, Pu, rows, n, m, dict(dense=[], long=[0, 1, 2], huge=[], folded=0, split=1, long_b=0), eq_rows=[1])


def _c16(name, rng, n, arrow):
    """A: 50 short rows, then four rows of 600 entries in two pairs on the same columns; the last one touches variable 0 and the
    last variable, so A holds column n - 1 and M = [P | A'] column n + m - 1.  No variable has exactly one entry in A: none is
    eliminated.  P: a diagonal (c16d_*: M has no long row then, and upload_mat gives it no 16-bit ids at any size) or, `arrow`,
    a diagonal and one row of 600 entries (c16_*: row 0 of M is long and holds column n + m - 1)."""
    m = 54
    d = rng.uniform(1.0, 10.0, n)
    if arrow:
        d[0] = 10.0
        pc = np.sort(np.concatenate([[n - 1], 1 + rng.choice(n - 2, 598, replace=False)]))
        Pu = _csc_keep_zeros(np.concatenate([np.arange(n), np.zeros(599, int)]), np.concatenate([np.arange(n), pc]),
                             np.concatenate([d, 0.01 * rng.choice([-1.0, 1.0], 599)]), n)
    else:
        Pu = sparse.diags(d, format="csc")
    s1 = rng.choice(n - 2, 600, replace=False) + 1
    s2 = np.concatenate([[0, n - 1], 1 + rng.choice(n - 2, 598, replace=False)])
    rows = _short(rng, range(50), np.concatenate([s1, s2[2:]]))
    rows += [_scaled_row(50 + k, s1 if k < 2 else s2, rng) for k in range(4)]
    eq, free = _classes(rng, m, skip=range(50, 54))
    m16 = int(arrow and n + m - 1 <= 0xffff)
    claims = dict(dense=[], long=[50, 51, 52, 53], huge=[], folded=0, split=1, long_b=int(arrow), a16=int(n - 1 <= 0xffff), m16=m16, b16=m16)
    return _finish(name, rng, Pu, rows, n, m, claims, eq, free, rho_hi=[53])


def _resident(name, rng, E):
    """A sparse P (a chain plus random pairs, diagonally dominant: eigenvalues in about [1, 10]) and m short rows, a tenth of
    them equalities; sized so that the forced grid holds K with E entries per thread."""
    n, m, kp, ka, nwg = RESIDENT[E]
    npairs = n * kp // 2
    i, j = rng.integers(0, n, 2 * npairs), rng.integers(0, n, 2 * npairs)
    keep = np.abs(i - j) > 1
    key = np.unique(np.minimum(i, j)[keep] * n + np.maximum(i, j)[keep])
    key = rng.permutation(key)[: npairs - (n - 1)]
    pairs = np.concatenate([np.stack([np.arange(n - 1), np.arange(1, n)], 1), np.stack([key // n, key % n], 1)])
    r, c, v = _pattern_block(rng, n, pairs)
    Pu = _csc_keep_zeros(r, c, v, n)
    rows = _short(rng, range(m), np.arange(n), max(1, ka - 1), ka + 1)
    eq = rng.permutation(m)[: m // 10]
    free = np.setdiff1d(np.arange(m), eq)[:3]
    return _finish(name, rng, Pu, rows, n, m, dict(dense=[], long=[], huge=[], folded=0, split=0, long_b=0, E=E, nwg=nwg), eq, free)


@functools.lru_cache(maxsize=None)
def make(name):
    rng = np.random.default_rng(SEEDS[name])
    if name == "blocks_mixed":
        return _blocks_mixed(name, rng)
    if name == "blocks_threshold":
        return _blocks_threshold(name, rng)
    if name == "blocks_holes":
        return _blocks_holes(name, rng)
    if name.startswith("huge_nh"):
        return _huge(name, rng, int(name[7:]))
    if name.startswith("blocks_huge"):
        return _blocks_with_rows(name, rng, [128] * 64, int(name[11:]))
    if name == "split3":
        return _split3(name, rng)
    if name.startswith("c16"):
        return _c16(name, rng, {"narrow": 65536 - 54, "m_wide": 65537 - 54, "wide": 65537}[name.split("_", 1)[1]], arrow=name.startswith("c16_"))
    if name.startswith("br_sizes_nh"):
        return _blocks_with_rows(name, rng, list(BR_SIZES) * 14, int(name[11:]))
    if name.startswith("res_e"):
        return _resident(name, rng, int(name[5:]))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# x~ of a perturbed operator
# ---------------------------------------------------------------------------------------------------------------
class Solver:
    """x~ = K^-1 (sigma x - q + A'(rho z - y)) in float64 for the scaled problem `pb` and operators near it: one LU of K (dense or
    sparse, as _engine_reference.admm_step chooses), then refinement steps against the operator asked for -- a relative
    change of 1e-4 to one value contracts by 1e-4 a step -- until the residual is at rounding level."""

    def __init__(self, pb, rho, sigma=R.SIGMA):
        self.pb, self.sigma = pb, sigma
        self.P, self.A, self.q = sparse.csr_matrix(pb.P.astype(float)), sparse.csr_matrix(pb.A.astype(float)), pb.q.astype(float)
        self.rho = np.asarray(rho, float)
        self.kkt = (R._DenseKKT if pb.n <= R.DENSE_MAX else R._SparseKKT)(pb, float(sigma), self.rho)

    def x_tilde(self, x, z, y, P=None, A=None, rho=None):
        P, A, rho = self.P if P is None else P, self.A if A is None else A, self.rho if rho is None else rho
        AT = A.T.tocsr()
        b = self.sigma * x - self.q + AT @ (rho * z - y)
        K = lambda v: P @ v + self.sigma * v + AT @ (rho * (A @ v))
        xt = self.kkt.solve(b)
        for _ in range(8):
            r = b - K(xt)
            xt = xt + self.kkt.solve(r)
        assert np.linalg.norm(b - K(xt)) <= 1e-13 * np.linalg.norm(b), "refinement did not settle"
        return xt

    def mutations(self, case):
        """(label, kwargs of x_tilde) of the three mutations, each a relative change of 1e-4 to one value:
          P     the entry in the last row of the last dense block, one column left of its diagonal, and its mirror image (a
                structural zero there: 1e-4 instead); without a dense block, the last entry of P's last column
          A     the last entry of the longest row of A
          rho   of that row"""
        n = self.pb.n
        P = sparse.lil_matrix(self.P)
        dense = case["claims"]["dense"]
        if dense:
            c0, b, _ = dense[-1]
            i, j = c0 + b - 1, c0 + b - 2
        else:
            i = n - 1
            j = int(self.P[i].indices.max())
        v = P[i, j]
        P[i, j] = P[j, i] = v * (1.0 + 1e-4) if v != 0.0 else 1e-4
        A = self.A.copy()
        row = int(np.diff(A.indptr).argmax())
        A.data[A.indptr[row + 1] - 1] *= 1.0 + 1e-4
        rho = self.rho.copy()
        rho[row] *= 1.0 + 1e-4
        return [("P[%d,%d]" % (i, j), dict(P=sparse.csr_matrix(P))), ("A[%d,last]" % row, dict(A=A)), ("rho[%d]" % row, dict(rho=rho))]
