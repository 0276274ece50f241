"""A numpy model of the single-QP engine's derivative route (osqp_amd_adjoint / osqp_amd_tangent, osqp_host.c), for the
tests of that route.  It knows nothing of the library.

The route is polish's: with the active rows (lows first, then upps), Ar those rows of the scaled A~ and
M~ = [P~, Ar~'; Ar~, 0], one solve is
    the reduced solve   (P~ + d I + Ar~' Ar~ / d) x = g1 + Ar~' g2 / d,   nu = (Ar~ x - g2) / d,   d = max(delta, 1e-3),
    then refinement against M~: at least `refine_iter` steps, at most max(refine_iter, 15), ended once the residual
    is below 1e-14 max(|g|, 1) or has not halved (run_polish's stop rule).
`route_solve` is that solve in float64 with an exact (LU) reduced solve; `kkt_res` is the last |g - M~ s|_inf /
max(|g|_inf, 1) it evaluated.

Scaling (P~ = c D P D, A~ = E A D, q~ = c D q, x = D x~, y = E y~ / c; D, E, c constants), as the C side applies it:
    adjoint   rhs = [D gx; E gy_act / c];  dq = -c D rx~,  dl_i (du_i) = E_i rnu~_i on a row active at its lower (upper)
              bound,  dA_ij = -E_i D_j (y~_i rx~_j + rnu~_i x~_j) on active rows,  dP_ij = -c D_i D_j (rx~_i x~_j + rx~_j x~_i)
              (-c D_i^2 rx~_i x~_i on the diagonal);
    tangent   rhs = [-(c D dq + (c D dP D) x~ + (E dA D)' y~_act); E db_act - ((E dA D) x~)_act];  dx = D dx~,
              dy = E dnu~ / c on the active rows.
`scaled_adjoint` / `scaled_tangent` evaluate exactly these formulas over any solve of M~ that is handed to them.

Sparse matrices (tests/_kkt_instance_cases.py at n = 8192): `scaled_problem(..., dense=False)` returns them, `route_solve` then
takes the reduced solve from a sparse LU of [P~ + d I, Ar~'; Ar~, -d I] -- the same x and nu in exact arithmetic -- and
`scaled_tangent(..., keep_sparse=True)` keeps dP~, dA~ sparse."""
from types import SimpleNamespace

import numpy as np
from scipy import sparse
from scipy.sparse import linalg as spla

DELTA_MIN, MAX_REFINE = 1e-3, 15


def route_solve(Pf, Ar, g, delta=1e-6, refine_iter=3):
    """(s, kkt_res, steps): the model of one refined solve of M s = g, M = [Pf, Ar'; Ar, 0]."""
    n, k = Pf.shape[0], Ar.shape[0]
    d = max(delta, DELTA_MIN)
    if sparse.issparse(Pf):
        Pf, Ar = sparse.csr_matrix(Pf), sparse.csr_matrix(Ar)
        M = sparse.bmat([[Pf, Ar.T], [Ar, None]], format="csr") if k else Pf
        lu = spla.splu(sparse.bmat([[Pf + d * sparse.eye(n), Ar.T], [Ar, -d * sparse.eye(k)]], format="csc") if k
                       else sparse.csc_matrix(Pf + d * sparse.eye(n)))
        reduced = lu.solve                       # [x; nu] with Ar x - d nu = b2: nu = (Ar x - b2) / d
    else:
        M = np.zeros((n + k, n + k))
        M[:n, :n] = Pf; M[:n, n:] = Ar.T; M[n:, :n] = Ar
        K = Pf + d * np.eye(n) + Ar.T @ Ar / d

        def reduced(b):
            x = np.linalg.solve(K, b[:n] + Ar.T @ b[n:] / d)
            return np.concatenate([x, (Ar @ x - b[n:]) / d])
    g = np.asarray(g, float)
    s = reduced(g)
    prev, kkt_res, steps = np.inf, 0.0, 0
    scale = max(float(np.abs(g).max()) if g.size else 0.0, 1.0)
    for it in range(max(refine_iter, MAX_REFINE)):
        res = g - M @ s
        nres = float(np.abs(res).max()) if res.size else 0.0
        kkt_res = nres / scale
        if it >= refine_iter and (nres <= 1e-14 * scale or nres > 0.5 * prev):
            break
        prev = nres
        s = s + reduced(res)
        steps += 1
    return s, kkt_res, steps


def scaled_problem(Pu, Ac, act, D, E, c, dense=True):
    """The scaled matrices and the active rows of a member: Pf~ (full, dense), Ad~ (dense), rows (lows first, then upps).
    dense=False: both as CSR."""
    n, m = Pu.shape[0], Ac.shape[0]
    rows = np.concatenate([np.flatnonzero(act < 0), np.flatnonzero(act > 0)]).astype(np.int64)
    if not dense:
        Pf = sparse.csr_matrix(Pu + sparse.triu(Pu, 1).T)
        return sparse.csr_matrix(c * (sparse.diags(D) @ Pf @ sparse.diags(D))), sparse.csr_matrix(sparse.diags(E) @ Ac @ sparse.diags(D)), rows
    Pf = (Pu + sparse.triu(Pu, 1).T).toarray()
    Pfs = c * (D[:, None] * Pf * D[None, :])
    Ads = E[:, None] * Ac.toarray().reshape(m, n) * D[None, :]
    return Pfs, Ads, rows


def scaled_adjoint(Pu, Ac, act, D, E, c, x, y, gx, gy, solve):
    """The adjoint as the C side computes it.  Pu: triu(P) in CSC, Ac: A in CSC (unscaled: only their patterns are used),
    x, y: the unscaled point; solve(g) = M~^-1 g on the rows `rows` of scaled_problem."""
    n, m = Pu.shape[0], Ac.shape[0]
    rows = np.concatenate([np.flatnonzero(act < 0), np.flatnonzero(act > 0)]).astype(np.int64)
    xs, ys = x / D, c * y / E
    s = solve(np.concatenate([D * gx, E[rows] * gy[rows] / c]))
    rx = s[:n]
    rnu = np.zeros(m); rnu[rows] = s[n:]
    yact = np.where(act != 0, ys, 0.0)
    Ai, Aj = Ac.indices, np.repeat(np.arange(n), np.diff(Ac.indptr))
    Pi, Pj = Pu.indices, np.repeat(np.arange(n), np.diff(Pu.indptr))
    dAx = np.where(act[Ai] != 0, -(E[Ai] * D[Aj]) * (yact[Ai] * rx[Aj] + rnu[Ai] * xs[Aj]), 0.0)
    w = np.where(Pi == Pj, rx[Pi] * xs[Pi], rx[Pi] * xs[Pj] + rx[Pj] * xs[Pi])
    dPx = -(c * D[Pi] * D[Pj]) * w
    v = E * rnu
    return SimpleNamespace(dq=-(c * D) * rx, dl=np.where(act < 0, v, 0.0), du=np.where(act > 0, v, 0.0), dPx=dPx, dAx=dAx)


def scaled_tangent(Pu, Ac, act, D, E, c, x, y, dQ, dL, dU, dPx, dAx, solve, keep_sparse=False):
    """The tangent as the C side computes it, for the directions dQ [ndir, n], ...: dx [ndir, n], dy [ndir, m]."""
    n, m = Pu.shape[0], Ac.shape[0]
    low, upp = np.flatnonzero(act < 0), np.flatnonzero(act > 0)
    rows = np.concatenate([low, upp]).astype(np.int64)
    xs, ys = x / D, c * y / E
    yact = np.where(act != 0, ys, 0.0)
    ndir = np.shape(dQ)[0]
    dx = np.zeros((ndir, n)); dy = np.zeros((ndir, m))
    for d in range(ndir):
        dPu = sparse.csc_matrix((dPx[d], Pu.indices, Pu.indptr), shape=(n, n))
        dAu = sparse.csc_matrix((dAx[d], Ac.indices, Ac.indptr), shape=(m, n))
        if keep_sparse:
            dPs = sparse.csr_matrix(c * (sparse.diags(D) @ (dPu + sparse.triu(dPu, 1).T) @ sparse.diags(D)))
            dAs = sparse.csr_matrix(sparse.diags(E) @ dAu @ sparse.diags(D))
        else:
            dPs = c * (D[:, None] * (dPu + sparse.triu(dPu, 1).T).toarray() * D[None, :])
            dAs = E[:, None] * dAu.toarray().reshape(m, n) * D[None, :]
        db = np.concatenate([(E * dL[d])[low], (E * dU[d])[upp]])
        g = np.concatenate([-(c * D * dQ[d] + dPs @ xs + dAs.T @ yact), db - (dAs @ xs)[rows]])
        s = solve(g)
        dx[d] = D * s[:n]
        dy[d, rows] = E[rows] * s[n:] / c
    return SimpleNamespace(dx=dx, dy=dy)


# the planted members (tests/_planted_qp.py) the GPU tests run as single QPs, and the random sparse QP of
# osqp_amd.problems.random_sparse_qp they add: test_single_sens_host.py proves on the CPU that none needs an excuse
PLANTED_MEMBERS = [("one", 0), ("one", 1), ("one", 2), ("one", 3), ("pad", 0), ("pad", 1), ("pad", 2), ("pad", 3),
                   ("lp", 0), ("lp", 1), ("lp", 2), ("scan", 0), ("scan", 1), ("scan", 2), ("rows", 0), ("rows", 1),
                   ("lds64k", 0)]
RANDOM_QP = dict(n=200, m=400, seed=3)


def member_qp(c, b):
    """Member b of a planted case as the arguments of OSQP.setup."""
    P = sparse.csc_matrix((c.Px_all[b], c.P.indices, c.P.indptr), shape=(c.n, c.n))
    A = sparse.csc_matrix((c.Ax_all[b], c.A.indices, c.A.indptr), shape=(c.m, c.n))
    return dict(P=P, q=c.Q[b], A=A, l=c.L[b], u=c.U[b])
