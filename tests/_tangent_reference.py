"""Forward sensitivities of a QP's solution in plain numpy, for the tangent tests.  It knows nothing of the library:
its inputs are the problem's matrices (P, A), a solution (x, y) and the tangents of the data (dq, dl, du, dPx, dAx).

Active rows as in _adjoint_reference.py (active_set: low where y_i < -tau, upp where y_i > tau, lows first).  With Ar
those rows of A and nu = y on them, locally P x + q + Ar' nu = 0 and Ar x = b_active, so
    M [dx; dnu] = [-(dq + dP x + dA' y_act); db_active - (dA x)_active],    M = [P, Ar'; Ar, 0],
    dy = dnu on the active rows, 0 elsewhere,
with y_act = y on the active rows and 0 elsewhere, db = dl_i (du_i) on a row active at its lower (upper) bound, dPx on
the pattern of triu(P) (an off-diagonal slot stands for both halves) and dAx on the pattern of A, both in CSC order.
Diagnostics, from the same data alone:
    route_err   error of a model of the device route -- the explicit inverse of [P + delta I, Ar'; Ar, -delta I] and
                `refine_iter` refinement steps against M -- against the direct solve, relative to max(1, |r|_inf);
    minv_norm   |M^-1|_inf (inf where M is singular to numpy).
The strict-complementarity margin and sigma_min / sigma_max of the active rows are adjoint_reference's."""
from types import SimpleNamespace

import numpy as np
from scipy import sparse

from _adjoint_reference import active_set


def draws(shape, nnzP, nnzA):
    """The tangents and the duality gradients of the tangent tests for shape_family(n, m, B, seed): for each member in
    order, standard normals dq [n], dl [m], du [m], dPx [nnzP], dAx [nnzA], gx [n], gy [m] from
    default_rng(777 + seed).  Returns a namespace of [B, .] arrays."""
    n, m, B, seed = shape
    rng = np.random.default_rng(777 + seed)
    names, sizes = ("dq", "dl", "du", "dPx", "dAx", "gx", "gy"), (n, m, m, nnzP, nnzA, n, m)
    out = {k: np.zeros((B, s)) for k, s in zip(names, sizes)}
    for b in range(B):
        for k, s in zip(names, sizes):
            out[k][b] = rng.standard_normal(s)
    return SimpleNamespace(**out)


def tangent_matrices(P, A, dPx, dAx):
    """(dP as a full symmetric dense matrix, dA dense) from values on the patterns of triu(P) and A."""
    Pu = sparse.triu(sparse.csc_matrix(P), format="csc"); Pu.sort_indices()
    Ac = sparse.csc_matrix(A); Ac.sort_indices()
    n, m = Pu.shape[0], Ac.shape[0]
    dPu = sparse.csc_matrix((np.zeros(Pu.nnz) if dPx is None else np.asarray(dPx, float), Pu.indices, Pu.indptr), shape=(n, n))
    dA = sparse.csc_matrix((np.zeros(Ac.nnz) if dAx is None else np.asarray(dAx, float), Ac.indices, Ac.indptr), shape=(m, n))
    return (dPu + sparse.triu(dPu, 1).T).toarray(), dA.toarray().reshape(m, n)


def tangent_reference(P, A, x, y, dq=None, dl=None, du=None, dPx=None, dAx=None, delta=1e-6, refine_iter=3):
    """P: n x n sparse (any triangle content; the upper triangle is used), A: m x n sparse.  A tangent of None is zero.
    Returns a namespace dx, dy, active, route_err, minv_norm (and rows, the active rows in the order of M)."""
    Pu = sparse.triu(sparse.csc_matrix(P), format="csc"); Pu.sort_indices()
    Ac = sparse.csc_matrix(A); Ac.sort_indices()
    n, m = Pu.shape[0], Ac.shape[0]
    x, y = np.asarray(x, float), np.asarray(y, float).reshape(m)
    vec = lambda v, k: np.zeros(k) if v is None else np.asarray(v, float).reshape(k)
    dq, dl, du = vec(dq, n), vec(dl, m), vec(du, m)
    Pf = (Pu + sparse.triu(Pu, 1).T).toarray()
    Ad = Ac.toarray().reshape(m, n)
    dP, dA = tangent_matrices(Pu, Ac, dPx, dAx)
    low, upp, act = active_set(y)
    rows = np.concatenate([low, upp]).astype(np.int64)
    k = rows.size
    Ar = Ad[rows]
    M = np.zeros((n + k, n + k))
    M[:n, :n] = Pf; M[:n, n:] = Ar.T; M[n:, :n] = Ar
    y_act = np.where(act != 0, y, 0.0)
    db = np.concatenate([dl[low], du[upp]])
    g = np.concatenate([-(dq + dP @ x + dA.T @ y_act), db - (dA @ x)[rows]])
    with np.errstate(all="ignore"):
        try:
            r = np.linalg.solve(M, g)
            minv_norm = float(np.abs(np.linalg.inv(M)).sum(axis=1).max())
        except np.linalg.LinAlgError:
            r = np.full(n + k, np.nan); minv_norm = np.inf
    if not np.isfinite(minv_norm):
        minv_norm = np.inf
    dy = np.zeros(m); dy[rows] = r[n:]
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
    return SimpleNamespace(dx=r[:n], dy=dy, active=act, route_err=route_err, minv_norm=minv_norm, rows=rows)
