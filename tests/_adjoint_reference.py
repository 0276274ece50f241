"""Adjoint derivatives of a QP's solution in plain numpy, for the adjoint tests.  It knows nothing of the library:
its inputs are the problem (P, A, l, u), a solution (x, y) and the incoming gradients gx = dl/dx, gy = dl/dy.

Active rows: low where y_i < -tau, upp where y_i > tau, tau = 1e-9 max(1, |y|_inf); ordered lows first, then upps.
With Ar those rows of A and nu = y on them, locally M [x; nu] = [-q; b_active], M = [P, Ar'; Ar, 0].  With
M [rx; rnu] = [gx; gy_active]:
    dl/dq = -rx;   dl/dl_i (dl/du_i) = rnu_a where row i is active at its lower (upper) bound, else 0;
    dl/dAx[k], slot k = entry (i, j) of A: -(nu_i rx_j + rnu_i x_j) on an active row, else 0;
    dl/dPx[k], slot (i, i) of triu(P): -rx_i x_i;   slot (i, j), i < j: -(rx_i x_j + rx_j x_i) (one stored value
    stands for both halves).
Diagnostics, from the same data alone:
    margin      strict complementarity: min over inactive rows of min(z - l, u - z), over active rows of |y|;
    sv_ratio    sigma_min(Ar) / sigma_max(Ar) (1 without active rows): dependent active rows make nu, rnu non-unique;
    route_err   error of a model of the device route -- the explicit inverse of [P + delta I, Ar'; Ar, -delta I] and
                `refine_iter` refinement steps against M -- against the direct solve, relative to max(1, |r|_inf)."""
from types import SimpleNamespace

import numpy as np
from scipy import sparse


def active_set(y):
    y = np.asarray(y, float)
    tau = 1e-9 * max(1.0, np.abs(y).max() if y.size else 0.0)
    low = np.flatnonzero(y < -tau)
    upp = np.flatnonzero(y > tau)
    act = np.zeros(y.size, np.int64)
    act[low] = -1; act[upp] = 1
    return low, upp, act


def adjoint_reference(P, A, l, u, x, y, gx, gy=None, delta=1e-6, refine_iter=3):
    """P: n x n sparse (any triangle content; the upper triangle is used), A: m x n sparse.  Returns a namespace
    dq, dl, du, dPx (CSC order of triu(P)), dAx (CSC order of A), active, margin, sv_ratio, route_err."""
    Pu = sparse.triu(sparse.csc_matrix(P), format="csc"); Pu.sort_indices()
    Ac = sparse.csc_matrix(A); Ac.sort_indices()
    n, m = Pu.shape[0], Ac.shape[0]
    x, y = np.asarray(x, float), np.asarray(y, float).reshape(m)
    gx = np.asarray(gx, float)
    gy = np.zeros(m) if gy is None else np.asarray(gy, float).reshape(m)
    Pf = (Pu + sparse.triu(Pu, 1).T).toarray()
    Ad = Ac.toarray().reshape(m, n)
    low, upp, act = active_set(y)
    rows = np.concatenate([low, upp]).astype(np.int64)
    k = rows.size
    Ar = Ad[rows]
    M = np.zeros((n + k, n + k))
    M[:n, :n] = Pf; M[:n, n:] = Ar.T; M[n:, :n] = Ar
    g = np.concatenate([gx, gy[rows]])
    with np.errstate(all="ignore"):
        try:
            r = np.linalg.solve(M, g)
        except np.linalg.LinAlgError:
            r = np.full(n + k, np.nan)
    rx, rnu = r[:n], r[n:]
    rnu_full = np.zeros(m); rnu_full[rows] = rnu
    nu_full = np.where(act != 0, y, 0.0)
    dl = np.zeros(m); du = np.zeros(m)
    dl[low] = rnu[:low.size]; du[upp] = rnu[low.size:]
    Ai, Aj = Ac.indices, np.repeat(np.arange(n), np.diff(Ac.indptr))
    dAx = np.where(act[Ai] != 0, -(nu_full[Ai] * rx[Aj] + rnu_full[Ai] * x[Aj]), 0.0) if Ac.nnz else np.zeros(0)
    Pi, Pj = Pu.indices, np.repeat(np.arange(n), np.diff(Pu.indptr))
    dPx = np.where(Pi == Pj, -rx[Pi] * x[Pi], -(rx[Pi] * x[Pj] + rx[Pj] * x[Pi]))
    # diagnostics
    l, u = np.asarray(l, float).reshape(m), np.asarray(u, float).reshape(m)
    z = Ad @ x
    inact = act == 0
    parts = []
    if inact.any():
        parts.append(np.minimum(z - l, u - z)[inact].min())
    if k:
        parts.append(np.abs(y[rows]).min())
    margin = float(min(parts)) if parts else np.inf
    if k:
        sv = np.linalg.svd(Ar, compute_uv=False)
        sv_ratio = float(sv.min() / sv.max()) if k <= n and sv.max() > 0 else 0.0
    else:
        sv_ratio = 1.0
    Mr = M.copy()
    Mr[np.arange(n), np.arange(n)] += delta
    Mr[np.arange(n, n + k), np.arange(n, n + k)] -= delta
    with np.errstate(all="ignore"):
        try:
            Minv = np.linalg.inv(Mr)
            s = Minv @ g
            for _ in range(refine_iter):
                s = s + Minv @ (g - M @ s)
            route_err = float(np.abs(s - r).max() / max(1.0, np.abs(r).max()))
        except np.linalg.LinAlgError:
            route_err = np.inf
    if not np.isfinite(route_err):
        route_err = np.inf
    return SimpleNamespace(dq=-rx, dl=dl, du=du, dPx=dPx, dAx=dAx, active=act, margin=margin, sv_ratio=sv_ratio,
                           route_err=route_err, rx=rx, rnu=rnu, rows=rows)
