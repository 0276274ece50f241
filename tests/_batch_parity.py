"""Shared helpers of the batch-engine tests: the parity bar against a per-member oracle run, the shape family
of mixed row classes, and the check of one member's scaled data and K^-1 through `BatchOSQP.member_workspace`.

Parity bar: status, iteration count and rho updates identical to the member's oracle run; x, y within 1e-6
relative; objective within 1e-8 relative."""
import numpy as np
from scipy import sparse


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    if b.size == 0:
        return 0.0
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def close(a, b, tol):
    """max |a - b| <= tol * max |b| (exact when b is all zero)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if b.size == 0:
        return True
    return np.abs(a - b).max() <= tol * np.abs(b).max()


def assert_parity(r, b, ro, what=""):
    tag = (what, b, int(r.status_val[b]), ro.info.status_val, int(r.iter[b]), ro.info.iter)
    assert r.status_val[b] == ro.info.status_val, tag
    assert r.iter[b] == ro.info.iter, tag
    assert r.rho_updates[b] == ro.info.rho_updates, tag + (int(r.rho_updates[b]), ro.info.rho_updates)
    if ro.info.status_val in (1, 2, -2):
        assert rel(r.x[b], ro.x) < 1e-6 and rel(r.y[b], ro.y) < 1e-6, tag + (rel(r.x[b], ro.x), rel(r.y[b], ro.y))
        assert abs(r.obj_val[b] - ro.info.obj_val) <= 1e-8 * max(1.0, abs(ro.info.obj_val)), tag


def shape_family(n, m, B, seed, per_row=None):
    """Shared diagonally dominant P (upper triangle) and A (up to three entries per row, or per_row, rows scaled
    over two decades); per member q of its own scale and its own mix of row classes (inequality, equality,
    one-sided, free).  Every row holds A x0, so every member is feasible."""
    rng = np.random.default_rng(seed)
    off = sparse.triu(sparse.random(n, n, density=min(1.0, 3.0 / n), random_state=rng, format="csc"), 1)
    off.data = rng.uniform(-0.3, 0.3, off.nnz)
    full = off + off.T
    d = 1.0 + np.asarray(abs(full).sum(axis=1)).ravel() + rng.uniform(0, 2, n)
    P = sparse.triu(full + sparse.diags(d), format="csc")
    rows, cols, vals = [], [], []
    for i in range(m):
        k = min(n, per_row or 1 + i % 3)
        c = rng.choice(n, k, replace=False)
        rows += [i] * k; cols += list(c); vals += list(rng.standard_normal(k) * 10.0 ** rng.uniform(-1, 1))
    A = sparse.csc_matrix((vals, (rows, cols)), shape=(m, n))
    x0 = rng.standard_normal(n); ax = A @ x0
    Q = np.array([rng.standard_normal(n) * 10.0 ** rng.uniform(-0.5, 1) for _ in range(B)])
    L = np.empty((B, m)); U = np.empty((B, m))
    for b in range(B):
        cls = rng.choice(4, m, p=[0.55, 0.15, 0.2, 0.1])
        lo = ax - rng.uniform(0.05, 1.0, m); hi = ax + rng.uniform(0.05, 1.0, m)
        lo[cls == 1] = hi[cls == 1] = ax[cls == 1]
        side = rng.random(m) < 0.5
        lo[(cls == 2) & side] = -np.inf; hi[(cls == 2) & ~side] = np.inf
        lo[cls == 3] = -np.inf; hi[cls == 3] = np.inf
        L[b], U[b] = lo, hi
    return P, A, Q, L, U, x0


def oracle(orc, P, q, A, l, u, **kw):
    so = orc.OracleOSQP().setup(P=P, q=q, A=A, l=l, u=u, **kw)
    so.settings_rho0 = so.settings().rho
    return so


def oracle_ws(so):
    """The oracle workspace's scaled data and rho classification."""
    w = so.work
    n, m = so.n, so.m
    if w.scaling:
        sc = w.scaling.contents
        D, E, c = so._vec(sc.D, n), so._vec(sc.E, m), float(sc.c)
    else:
        D, E, c = np.ones(n), np.ones(m), 1.0
    Pc, Ac = w.data.contents.P.contents, w.data.contents.A.contents
    Pv, Av = so._vec(Pc.x, so.nnzP), so._vec(Ac.x, so.nnzA)
    Pp, Pi = so._vec(Pc.p, n + 1).astype(np.int64), so._vec(Pc.i, so.nnzP).astype(np.int64)
    Ap, Ai = so._vec(Ac.p, n + 1).astype(np.int64), so._vec(Ac.i, so.nnzA).astype(np.int64)
    Pu = sparse.csc_matrix((Pv, Pi, Pp), shape=(n, n))
    Ah = sparse.csc_matrix((Av, Ai, Ap), shape=(m, n))
    return dict(D=D, E=E, c=c, rho=float(so.settings().rho), ctype=so._vec(w.constr_type, m).astype(np.int64),
                Pv=Pv, Av=Av, Pu=Pu, A=Ah, sigma=float(so.settings().sigma))


def kinv_reference(K):
    """np.linalg.inv, then one Newton-Schulz step with the residual I - K X formed in long double."""
    X = np.linalg.inv(K)
    Kl, Xl = K.astype(np.longdouble), X.astype(np.longdouble)
    R = np.eye(K.shape[0], dtype=np.longdouble) - Kl @ Xl
    return X, Xl + Xl @ R


def check_member_kinv(bs, qp, so, what, want_np):
    """The member's scaled data and classes equal the oracle's set-up workspace (so: an oracle after setup only)
    to 1e-14; K^-1 is NP x NP with NP = want_np and exact identity padding; where cond(K) <= 1e5, K^-1 is within
    10x numpy's error of a high-precision inverse of K formed from the oracle's scaled data with the member's
    rho.  Returns True when the accuracy check ran."""
    g, o = bs.member_workspace(qp), oracle_ws(so)
    n, NP = bs.n, g["NP"]
    tag = (what, qp, n, bs.m)
    assert NP == want_np, tag + (NP, want_np)
    for k in ("D", "E", "Pv", "Av"):
        assert g[k].shape == o[k].shape and close(g[k], o[k], 1e-14), tag + (k,)
    assert abs(g["c"] - o["c"]) <= 1e-14 * abs(o["c"]), tag
    assert np.array_equal(g["ctype"], o["ctype"]), tag
    rho_vec = np.where(o["ctype"] == -1, 1e-6, np.where(o["ctype"] == 1, 1e3 * g["rho"], g["rho"]))
    Pf = (o["Pu"] + sparse.triu(o["Pu"], 1).T).toarray()
    Ad = o["A"].toarray()
    K = Pf + o["sigma"] * np.eye(n) + Ad.T @ (rho_vec[:, None] * Ad)
    Xg = g["Kinv"]
    pad = np.eye(NP); pad[:n, :n] = Xg[:n, :n]
    assert np.array_equal(Xg, pad), tag + ("padding is not the identity",)
    if np.linalg.cond(K) > 1e5:
        return False
    X_np, X_ref = kinv_reference(K)
    err_np = float(np.abs(X_np - X_ref).max())
    bound = 10.0 * err_np + 1e-14 * float(np.abs(X_ref).max())
    err_g = float(np.abs(Xg[:n, :n] - X_ref).max())
    assert err_g <= bound, tag + ("K^-1 error", err_g, "numpy's", err_np)
    return True
