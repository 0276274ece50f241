"""Seeded problem builders for the two direct linear-solve forms of the single-QP engine, shared by
tests/test_gpu_direct_solve_edges.py (one KKT solve at a time) and tests/_form_cases.py (whole ADMM steps).  Nothing here touches
the library."""
import numpy as np
from scipy import sparse

RHO, RHO_MIN, EQ = 0.1, 1e-6, 1e3


def _classes(m, rng, eq=0.3, loose=0.2):
    r = rng.random(m)
    rho = np.full(m, RHO)
    rho[r < eq] = EQ * RHO
    rho[r > 1.0 - loose] = RHO_MIN
    return rho


def dd_problem(na, seed, row_len=40, nd=None, nshort=None, b2_nbrs=(), nslack=0, pyy=0.0, Pcore=None, a_scale=1.0):
    """Core variables 0..na-1 all coupled in P (tridiagonal unless Pcore is given: no B2 candidates, no elimination), so they
    are exactly the dense unknowns.  nd rows of row_len entries over the core (dense when row_len >= 32), nshort rows of 2-3
    entries.  Then one extra variable per entry of b2_nbrs with that many core neighbours (in two rows of A: never eliminated)
    and nslack slack variables (diagonal P = pyy, one entry each in a row of its own plus core entries: eliminated).
    Returns triu(P), A, rho."""
    rng = np.random.default_rng(seed)
    nb, ns = len(b2_nbrs), nslack
    n = na + nb + ns
    if Pcore is None:
        d = rng.uniform(2.0, 3.0, na)
        Pcore = sparse.diags([d, np.full(na - 1, -0.5)], [0, 1], shape=(na, na), format="csc") if na > 1 else sparse.csc_matrix(d.reshape(1, 1))
    parts = [sparse.triu(Pcore), sparse.diags(rng.uniform(0.5, 2.0, nb)) if nb else None, sparse.diags(np.full(ns, pyy)) if ns and pyy else None]
    P = sparse.block_diag([q for q in parts if q is not None], format="csc")
    if ns and pyy == 0.0:            # P_yy = 0 stored as explicit zeros on the diagonal
        P = sparse.coo_matrix(P, shape=(na + nb, na + nb))
        P = sparse.coo_matrix((np.concatenate([P.data, np.zeros(ns)]), (np.concatenate([P.row, np.arange(na + nb, n)]),
                                                                        np.concatenate([P.col, np.arange(na + nb, n)]))), shape=(n, n)).tocsc()
    rows = []
    nd = max(1, na // 64) if nd is None else nd
    nshort = max(1, na // 4) if nshort is None else nshort
    for _ in range(nd):
        k = min(row_len, na)
        cols = rng.choice(na, k, replace=False)
        rows.append((cols, rng.standard_normal(k) * a_scale / np.sqrt(k)))
    for _ in range(nshort):
        k = min(int(rng.integers(2, 4)), na)
        cols = rng.choice(na, k, replace=False)
        rows.append((cols, rng.standard_normal(k) * a_scale))
    for t, nbrs in enumerate(b2_nbrs):
        v = na + t
        nbr = rng.choice(na, nbrs, replace=False) if nbrs else np.zeros(0, int)
        half = (nbrs + 1) // 2
        for part in (nbr[:half], nbr[half:]):
            cols = np.concatenate([[v], part])
            rows.append((cols, np.concatenate([[1.0], 0.5 * rng.standard_normal(part.size)]) * a_scale))
    for s in range(ns):
        v = na + nb + s
        part = rng.choice(na, min(na, 3), replace=False)
        rows.append((np.concatenate([[v], part]), np.concatenate([[rng.uniform(0.5, 2.0) * rng.choice([-1, 1])], rng.standard_normal(part.size)]) * a_scale))
    m = len(rows)
    ri = np.concatenate([np.full(len(c), i) for i, (c, _) in enumerate(rows)])
    ci = np.concatenate([c for c, _ in rows])
    vi = np.concatenate([v for _, v in rows])
    A = sparse.csc_matrix((vi, (ri, ci)), shape=(m, n))
    return sparse.triu(P, format="csc"), A, _classes(m, rng)


def spectrum_p(nv, cond, seed, top=10.0):
    """Dense SPD matrix with eigenvalues log-spaced in [top / cond, top]."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((nv, nv)))
    P = (Q * np.logspace(np.log10(top), np.log10(top / cond), nv)) @ Q.T
    return 0.5 * (P + P.T)


def bd_problem(blocks, seed, kc=0, nhuge=0, cond=None, zeros_in=None, single=True):
    """P = dense diagonal blocks of the given sizes (cond: each block's spectrum spans cond; zeros_in: a block index whose
    upper triangle stores a third of its entries as explicit zeros), A = one single-entry row per variable (single), kc
    coupling rows of 2-6 entries across blocks, nhuge rows over every variable."""
    rng = np.random.default_rng(seed)
    n = int(sum(blocks))
    Pb = []
    for t, b in enumerate(blocks):
        if cond is not None:
            B = spectrum_p(b, cond, seed * 100 + t, top=10.0)
        else:
            G = rng.standard_normal((b, b)) / np.sqrt(b)
            B = G @ G.T + np.eye(b)
        if zeros_in == t:
            iu = np.triu_indices(b, 1)
            pick = rng.random(iu[0].size) < 1.0 / 3.0
            B[iu[0][pick], iu[1][pick]] = 0.0
            B[iu[1][pick], iu[0][pick]] = 0.0
            B += np.eye(b) * (1.0 + np.abs(np.linalg.eigvalsh(B)).max())
        U = np.triu(B)
        r, c = np.nonzero(np.triu(np.ones((b, b))))
        Pb.append(sparse.csc_matrix((U[r, c], (r, c)), shape=(b, b)))     # full upper triangle stored, zeros included
    Pu = sparse.block_diag(Pb, format="csc")
    rows = []
    if single:
        for j in range(n):
            rows.append(([j], [rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0]) * (0.3 / np.sqrt(cond) if cond else 1.0)]))   # (cond: at the scale of the smallest eigenvalues)
    for _ in range(kc):
        k = int(rng.integers(2, 7))
        cols = rng.choice(n, k, replace=False)
        rows.append((cols, rng.standard_normal(k) * (0.3 if cond else 1.0)))
    for _ in range(nhuge):
        rows.append((np.arange(n), rng.standard_normal(n) / np.sqrt(n)))
    m = len(rows)
    ri = np.concatenate([np.full(len(c), i) for i, (c, _) in enumerate(rows)])
    ci = np.concatenate([np.asarray(c) for c, _ in rows])
    vi = np.concatenate([np.asarray(v, float) for _, v in rows])
    A = sparse.csc_matrix((vi, (ri, ci)), shape=(m, n))
    return Pu, A, _classes(m, rng)
