"""Host replay of the values of the resident K (engine_pcg_resident.h: k_form_K, k_form_K_lists), independent of both kernels and of the
contribution lists.  The library is built with -ffp-contract=off and both kernels document one association and one order,

    v = (P_ij or 0) + (sigma if i == j else 0);   for the rows k of A holding both i and j, k ascending:  v = v + rho_k * (a_ki * a_kj)

a sequence of correctly rounded float64 operations, which numpy repeats to the bit: replay() from (P, A, sigma, rho) and the
pattern of K alone, replay_lists() from the lists and the slots they point to.  Both step through the terms by rank (the r-th
term of every entry at once), so no `dot` or `sum` decides an order.  Nothing here is tuned on a kernel's output."""
import numpy as np
from scipy import sparse

LD = np.longdouble
U = 2.0 ** -53


def _slots(P, A):
    """Where the engine keeps the entries of A (build_A, build_M): for every entry of the CSR copy of A (columns ascending in a
    row) its row, its column and its slot in M -- row i of M holds the stored entries of row i of P (both triangles), then
    column i of A with rows ascending."""
    n = P.shape[0]
    Pu = sparse.triu(P, format="coo")
    per_row = np.bincount(Pu.row, minlength=n) + np.bincount(Pu.col[Pu.row != Pu.col], minlength=n)
    Ac = sparse.csc_matrix(A); Ac.sort_indices()
    acol = np.diff(Ac.indptr)
    rowptr = np.concatenate([[0], np.cumsum(per_row + acol)])
    split = rowptr[:-1] + per_row
    in_m = np.repeat(split - Ac.indptr[:-1], acol) + np.arange(Ac.nnz)          # slot in M of every entry in CSC order
    tag = sparse.csc_matrix((np.arange(Ac.nnz) + 1.0, Ac.indices, Ac.indptr), shape=Ac.shape).tocsr()
    tag.sort_indices()
    csc_of_csr = tag.data.astype(np.int64) - 1
    return np.repeat(np.arange(A.shape[0]), np.diff(tag.indptr)), tag.indices.astype(np.int64), in_m[csc_of_csr], Ac


def _csr(A):
    """(rowptr, columns, values) of A row by row, columns ascending, stored zeros kept (they are terms of the kernels too)."""
    Ac = sparse.csc_matrix(A); Ac.sort_indices()
    m = Ac.shape[0]
    col = np.repeat(np.arange(Ac.shape[1], dtype=np.int64), np.diff(Ac.indptr))
    order = np.lexsort((col, Ac.indices))
    return np.concatenate([[0], np.cumsum(np.bincount(Ac.indices, minlength=m))]).astype(np.int64), col[order], Ac.data[order].astype(np.float64)


def _base(P, sigma, rows, cols):
    """P_ij (0.0 where P stores none) and sigma [i == j] (0.0 off the diagonal) for the entries (rows, cols); P is taken from
    its upper triangle, as the engine takes it."""
    n = P.shape[0]
    Pu = sparse.triu(sparse.csc_matrix(P), format="coo")
    key = np.concatenate([Pu.row.astype(np.int64) * n + Pu.col, Pu.col[Pu.row != Pu.col].astype(np.int64) * n + Pu.row[Pu.row != Pu.col]])
    val = np.concatenate([Pu.data, Pu.data[Pu.row != Pu.col]]).astype(np.float64)
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    assert (np.diff(key) > 0).all(), "P repeats an entry"
    want = rows * n + cols
    at = np.minimum(np.searchsorted(key, want), max(len(key) - 1, 0))
    hit = (key[at] == want) if len(key) else np.zeros(len(want), dtype=bool)
    p = np.where(hit, val[at] if len(key) else 0.0, 0.0)
    return p, np.where(rows == cols, np.float64(sigma), 0.0)


def _run(p, s, ent, w, ai, aj, nent):
    """The sequence itself.  Terms (entry ent, weight w, operands ai, aj) come entry by entry, in each entry's order.  Returns
    (float64 values, long-double values, mag, counts)."""
    cnt = np.bincount(ent, minlength=nent).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)])
    rank = np.arange(len(ent), dtype=np.int64) - start[ent]
    by_rank = np.lexsort((ent, rank))                        # all first terms, then all second terms, ...
    edge = np.concatenate([[0], np.cumsum(np.bincount(rank, minlength=1))]) if len(ent) else np.zeros(1, dtype=np.int64)
    v = p + s
    vl = p.astype(LD) + s.astype(LD)
    mag = np.abs(vl)
    for r in range(len(edge) - 1):
        t = by_rank[edge[r]:edge[r + 1]]
        e = ent[t]                                           # (each entry at most once: plain indexed assignment is an update)
        v[e] = v[e] + w[t] * (ai[t] * aj[t])
        tl = w[t].astype(LD) * (ai[t].astype(LD) * aj[t].astype(LD))
        vl[e] = vl[e] + tl
        mag[e] = mag[e] + np.abs(tl)
    return v, vl, mag, cnt


def replay(P, A, sigma, rho, Kptr, Kcol, gone=None):
    """(K, K in long double, mag, term counts) for every entry of the pattern (Kptr, Kcol), in that order.  mag = |P_ij + sigma
    [i == j]| + sum |terms|.  gone: the eliminated variables -- their rows and columns hold 1.0 on the diagonal and 0.0 elsewhere (the
    caller passes the effective weights rhoe as rho); the counts stay those of the pattern."""
    n = P.shape[0]
    Kptr, Kcol = np.asarray(Kptr, dtype=np.int64), np.asarray(Kcol, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(Kptr))
    key = rows * n + Kcol
    assert len(key) == 0 or (np.diff(key) > 0).all(), "the pattern is not row-major with ascending columns"
    rho = np.asarray(rho, dtype=np.float64)
    rp, ac, av = _csr(A)
    L = np.diff(rp)
    # one term per ordered pair of entries of a row of A: (k, i, j) with a_ki, a_kj
    ti, tj, tk, tai, taj = [], [], [], [], []
    for k in np.flatnonzero(L):
        c, a = ac[rp[k]:rp[k + 1]], av[rp[k]:rp[k + 1]]
        ti.append(np.repeat(c, L[k])); tj.append(np.tile(c, L[k])); tai.append(np.repeat(a, L[k])); taj.append(np.tile(a, L[k]))
        tk.append(np.full(L[k] * L[k], k, dtype=np.int64))
    if tk:
        ti, tj, tk, tai, taj = (np.concatenate(x) for x in (ti, tj, tk, tai, taj))
    else:
        ti = tj = tk = np.zeros(0, dtype=np.int64); tai = taj = np.zeros(0)
    order = np.lexsort((tk, ti * n + tj))                    # entry by entry, k ascending inside
    ti, tj, tk, tai, taj = ti[order], tj[order], tk[order], tai[order], taj[order]
    ent = np.searchsorted(key, ti * n + tj)
    assert (ent < len(key)).all() and np.array_equal(key[ent], ti * n + tj), "a term of A' rho A has no entry in the pattern of K"
    p, s = _base(P, sigma, rows, Kcol)
    v, vl, mag, cnt = _run(p, s, ent, rho[tk] if len(tk) else np.zeros(0), tai, taj, len(key))
    if gone is not None and len(gone):
        g = np.zeros(n, dtype=bool); g[np.asarray(sorted(gone), dtype=np.int64)] = True
        out = g[rows] | g[Kcol]
        unit = np.where(rows == Kcol, 1.0, 0.0)
        v = np.where(out, unit, v); vl = np.where(out, unit.astype(LD), vl); mag = np.where(out, unit.astype(LD), mag)
    return v, vl, mag, cnt


def m_image(P, A):
    """The engine's M = [P | A'] as far as the lists look at it: per slot the value (NaN in the P part: a list that points there
    poisons its entry) and the row of A (-1 in the P part); and the values of the CSR copy of A."""
    row_of, col_of, m_of, Ac = _slots(P, A)
    Pu = sparse.triu(P, format="coo")
    size = len(Pu.row) + int((Pu.row != Pu.col).sum()) + Ac.nnz
    rp, ac, av = _csr(A)
    assert np.array_equal(ac, col_of) and (len(m_of) == 0 or m_of.max() < size)
    Mval = np.full(size, np.nan); Mrow = np.full(size, -1, dtype=np.int64)
    Mval[m_of] = av; Mrow[m_of] = row_of
    return Mval, Mrow, av


def replay_lists(Mval, Aval, rho, Kcp, Kcm, Kca, Mrow, p, s):
    """The same sequence in list order from the slots: entry e adds, for q in Kcp[e] .. Kcp[e + 1], rho[Mrow[Kcm[q]]] * (Mval[Kcm[q]] *
    Aval[Kca[q]]) to p[e] + s[e].  Returns what replay() returns."""
    Kcp = np.asarray(Kcp, dtype=np.int64)
    nent = len(Kcp) - 1
    ent = np.repeat(np.arange(nent, dtype=np.int64), np.diff(Kcp))
    cm, ca = np.asarray(Kcm, dtype=np.int64)[:Kcp[-1]], np.asarray(Kca, dtype=np.int64)[:Kcp[-1]]
    k = Mrow[cm]
    assert (k >= 0).all(), "a list points into the P part of M"
    return _run(np.asarray(p, dtype=np.float64), np.asarray(s, dtype=np.float64), ent, np.asarray(rho, dtype=np.float64)[k], Mval[cm], Aval[ca], nent)


def base(P, sigma, Kptr, Kcol):
    """(P_ij or 0.0, sigma [i == j]) per entry of the pattern: the start of the sequence, for replay_lists."""
    Kptr, Kcol = np.asarray(Kptr, dtype=np.int64), np.asarray(Kcol, dtype=np.int64)
    return _base(P, sigma, np.repeat(np.arange(P.shape[0], dtype=np.int64), np.diff(Kptr)), Kcol)


def eliminated(Pu, A):
    """The variables build_elim takes out of the linear system, by its rule (engine.hip): exactly one entry in their column of A,
    no off-diagonal entry in P, the first such variable of a row only.  (Rows of 8192 entries or more are left alone; no test
    here has one.)"""
    n = Pu.shape[0]
    Pc = sparse.coo_matrix(Pu)
    coupled = np.zeros(n, dtype=bool)
    off = Pc.row != Pc.col
    coupled[Pc.row[off]] = True; coupled[Pc.col[off]] = True
    Ac = sparse.csc_matrix(A)
    assert Ac.shape[0] == 0 or np.bincount(Ac.indices, minlength=Ac.shape[0]).max() < 8192
    taken, gone = set(), []
    for j in np.flatnonzero((np.diff(Ac.indptr) == 1) & ~coupled):
        i = int(Ac.indices[Ac.indptr[j]])
        if i not in taken:
            taken.add(i); gone.append(int(j))
    return gone, sorted(taken)
