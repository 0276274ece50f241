"""GPU tests of the batched engine (osqp_amd/csrc/batch.hip) at its edges: the tile switch at n = 64 / 65,
the identity padding of K to NP = 64 / 128, n not a multiple of the tile, m = 0, empty rows and columns of A,
per-QP matrices, constraint-class changes, the LDS sizes above 64 KiB, member statuses inside one batch, and
the two setup contracts (non-convex members, settings the kernel does not implement).

Parity bar (as in test_gpu_batch.py): status, iteration count and rho updates identical to a per-member oracle
run; x, y within 1e-6 relative; objective within 1e-8 relative.  K^-1 itself is read through the
`BatchOSQP.member_workspace` test hook and compared with a high-precision inverse of K formed from the ORACLE's
scaled data."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

SHAPES_N = [1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 96, 127, 128]


def _ms(n):
    return [0, 1, 2 * n + 3]


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    if b.size == 0:
        return 0.0
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _close(a, b, tol):
    """max |a - b| <= tol * max |b| (relative to the largest entry; exact when b is all zero)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if b.size == 0:
        return True
    return np.abs(a - b).max() <= tol * np.abs(b).max()


def _assert_parity(r, b, ro, what="", replay=None):
    """The parity bar.  replay (section (a) only): the member's setup / update / solve sequence on the oracle with q
    moved by 1e-15 relative, returning the (iter, rho_updates) of its last solve.  When the count of rho updates
    differs, the member is let off THAT comparison (and the rho value) only if the oracle itself reaches several
    counts under roundoff, the batch's among them (measured: n = 1, m = 5, residuals 3e-16 / 7e-16 at the last
    adaptation, rho_updates 0 or 1).  Returns True when it was let off."""
    tag = (what, b, int(r.status_val[b]), ro.info.status_val, int(r.iter[b]), ro.info.iter)
    assert r.status_val[b] == ro.info.status_val, tag
    assert r.iter[b] == ro.info.iter, tag
    let_off = False
    if r.rho_updates[b] != ro.info.rho_updates and replay is not None:
        outcomes = replay()
        assert len({u for _, u in outcomes}) > 1 and (int(r.iter[b]), int(r.rho_updates[b])) in outcomes, tag + (sorted(outcomes),)
        let_off = True
    assert let_off or r.rho_updates[b] == ro.info.rho_updates, tag + (int(r.rho_updates[b]), ro.info.rho_updates)
    if ro.info.status_val in (1, 2, -2):
        assert _rel(r.x[b], ro.x) < 1e-6 and _rel(r.y[b], ro.y) < 1e-6, tag + (_rel(r.x[b], ro.x), _rel(r.y[b], ro.y))
        assert abs(r.obj_val[b] - ro.info.obj_val) <= 1e-8 * max(1.0, abs(ro.info.obj_val)), tag
    return let_off


def _replayer(orc, P, A, q, l, u, kw, updates, draws=20):
    """replay for _assert_parity: setup, solve, then for each update (dict of q / l / u) update and solve."""
    def replay():
        rng = np.random.default_rng(0)
        out = set()
        for _ in range(draws):
            so = orc.OracleOSQP().setup(P=P, q=q * (1 + 1e-15 * rng.standard_normal(q.size)), A=A, l=l, u=u, **kw)
            ro = so.solve()
            for up in updates:
                so.update(**up); ro = so.solve()
            out.add((ro.info.iter, ro.info.rho_updates))
        return out
    return replay


# ---------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------
def _shape_family(n, m, B, seed):
    """Shared diagonally dominant P (upper triangle) and A (up to three entries per row, rows scaled over two
    decades); per member q of its own scale and its own mix of row classes (inequality, equality, one-sided,
    free).  Every row holds A x0, so every member is feasible."""
    rng = np.random.default_rng(seed)
    off = sparse.triu(sparse.random(n, n, density=min(1.0, 3.0 / n), random_state=rng, format="csc"), 1)
    off.data = rng.uniform(-0.3, 0.3, off.nnz)
    full = off + off.T
    d = 1.0 + np.asarray(abs(full).sum(axis=1)).ravel() + rng.uniform(0, 2, n)
    P = sparse.triu(full + sparse.diags(d), format="csc")
    rows, cols, vals = [], [], []
    for i in range(m):
        k = min(n, 1 + i % 3)
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


def _oracle_ws(so):
    """The oracle workspace's scaled data and rho classification (what the batch hook must reproduce)."""
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
    return dict(D=D, E=E, c=c, rho=float(so.settings().rho), rho_vec=so._vec(w.rho_vec, m),
                ctype=so._vec(w.constr_type, m).astype(np.int64), Pv=Pv, Av=Av, Pu=Pu, A=Ah, sigma=float(so.settings().sigma))


def _kinv_reference(K):
    """np.linalg.inv, then one Newton-Schulz step with the residual I - K X formed in long double."""
    X = np.linalg.inv(K)
    Kl, Xl = K.astype(np.longdouble), X.astype(np.longdouble)
    R = np.eye(K.shape[0], dtype=np.longdouble) - Kl @ Xl
    return X, Xl + Xl @ R


def _check_member_workspace(bs, qp, so, what, max_cond=1e5, accuracy=True, rho_moved_ok=False):
    """Hook (a): the batch member's scaled data and classes equal the oracle's to 1e-14; the identity padding of
    K^-1 is exact; where cond(K) <= 1e5 (asserted when max_cond is given, else the condition for the rest) K^-1 is
    as close to a high-precision inverse of K as numpy's own inverse, up to a factor of 10, and symmetric to the
    same level."""
    g, o = bs.member_workspace(qp), _oracle_ws(so)
    n, m, NP = bs.n, bs.m, g["NP"]
    tag = (what, qp, n, m)
    for k in ("D", "E", "Pv", "Av"):
        assert g[k].shape == o[k].shape and _close(g[k], o[k], 1e-14), tag + (k,)
    assert abs(g["c"] - o["c"]) <= 1e-14 * abs(o["c"]), tag
    # rho: exact while adaptive rho has not moved it.  Once it has, rho = rho sqrt(pri / dua) of residuals of iterates
    # that agree to the parity bar, not to 1e-14 (measured: up to 5e-4 relative, 6e-3 on one- and five-row problems
    # whose residuals are smallest), so it is held to 1e-2 there -- an adaptation step is a factor of at least
    # adaptive_rho_tolerance = 5, so a wrong one is still caught.  K below is formed with the batch's own rho.
    if o["rho"] == float(so.settings_rho0):
        assert abs(g["rho"] - o["rho"]) <= 1e-14 * o["rho"], tag + (g["rho"], o["rho"])
        assert _close(np.where(o["ctype"] == -1, 1e-6, np.where(o["ctype"] == 1, 1e3 * g["rho"], g["rho"])), o["rho_vec"], 1e-14)
    elif not rho_moved_ok:
        assert abs(g["rho"] - o["rho"]) <= 1e-2 * o["rho"], tag + ("adapted rho", g["rho"], o["rho"])
    assert 1e-6 <= g["rho"] <= 1e6, tag
    assert np.array_equal(g["ctype"], o["ctype"]), tag
    # K from the oracle's scaled data and classes, with the batch's rho (the reference's rule, auxil.c:76-98)
    rho_vec = np.where(o["ctype"] == -1, 1e-6, np.where(o["ctype"] == 1, 1e3 * g["rho"], g["rho"]))
    Pf = (o["Pu"] + sparse.triu(o["Pu"], 1).T).toarray()
    Ad = o["A"].toarray()
    K = Pf + o["sigma"] * np.eye(n) + Ad.T @ (rho_vec[:, None] * Ad)
    Xg = g["Kinv"]
    pad = np.eye(NP); pad[:n, :n] = Xg[:n, :n]
    assert np.array_equal(Xg, pad), tag + ("padding is not the identity",)
    if not accuracy:
        return None
    cond = np.linalg.cond(K)
    if max_cond:
        assert cond <= max_cond, tag + (cond,)
    elif cond > 1e5:
        return None                          # the 10x-numpy bound is the one for cond(K) <= 1e5
    X_np, X_ref = _kinv_reference(K)
    err_np = float(np.abs(X_np - X_ref).max())
    bound = 10.0 * err_np + 1e-14 * float(np.abs(X_ref).max())
    err_g = float(np.abs(Xg[:n, :n] - X_ref).max())
    assert err_g <= bound, tag + ("K^-1 error", err_g, "numpy's", err_np)
    assert np.abs(Xg - Xg.T).max() <= bound, tag + ("asymmetry", float(np.abs(Xg - Xg.T).max()), bound)
    return err_g, err_np


def _oracle(orc, P, q, A, l, u, **kw):
    so = orc.OracleOSQP().setup(P=P, q=q, A=A, l=l, u=u, **kw)
    so.settings_rho0 = so.settings().rho
    so.problem = (P, q, A, l, u, kw)
    return so


def _oracles(orc, P, A, Q, L, U, **kw):
    return [_oracle(orc, P, Q[b], A, L[b], U[b], **kw) for b in range(Q.shape[0])]


# ---------------------------------------------------------------------------------------------------------------
# (a) K^-1 and the scaled data, at every edge shape, after adaptive rho, a class change and a value-only update
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES_N)
def test_kinv_and_scaled_data_at_edge_shapes(gpu_lib, oracle_mod, n):
    import osqp_amd
    kw = dict(adaptive_rho_interval=5, eps_abs=1e-5, eps_rel=1e-5)
    fired = checked = 0
    for m in _ms(n):
        B = 3
        # a single row drives adaptive rho towards its clamps: there the K^-1 bound applies where cond(K) <= 1e5; the
        # other families keep cond(K) <= 1e5 throughout (asserted)
        mc = None if m == 1 else 1e5
        P, A, Q, L, U, x0 = _shape_family(n, m, B, seed=1000 * n + m)
        bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **kw)
        sos = _oracles(oracle_mod, P, A, Q, L, U, **kw)
        r = bs.solve()
        hist = [[] for _ in range(B)]

        def check(b, so, ro, what):
            nonlocal checked
            rp = _replayer(oracle_mod, P, A, Q[b], L[b], U[b], kw, list(hist[b]))
            off = _assert_parity(r, b, ro, what, replay=rp)
            checked += _check_member_workspace(bs, b, so, what, max_cond=mc, rho_moved_ok=off) is not None
        for b, so in enumerate(sos):
            check(b, so, so.solve(), "after adaptive rho")
            fired += int(r.rho_updates[b] >= 1)
        if m == 0:
            Q2 = Q[::-1] * 0.5
            assert bs.update(Q=Q2) == 0
            r = bs.solve()
            for b, so in enumerate(sos):
                so.update(q=Q2[b]); hist[b].append(dict(q=Q2[b]))
                check(b, so, so.solve(), "after a q update")
            continue
        # classes change: equalities become inequalities, row 0 free (an inequality if it was free), the last row
        # free (no new equality rows: cond(K) stays <= 1e5)
        ax = A @ x0
        L2, U2 = L.copy(), U.copy()
        for b in range(B):
            eq = np.isclose(L[b], U[b])
            L2[b, eq] = ax[eq] - 0.5; U2[b, eq] = ax[eq] + 0.5
            if np.isinf(L[b, 0]) and np.isinf(U[b, 0]):
                L2[b, 0], U2[b, 0] = ax[0] - 0.5, ax[0] + 0.5
            else:
                L2[b, 0], U2[b, 0] = -np.inf, np.inf
            if m > 1:
                L2[b, -1], U2[b, -1] = -np.inf, np.inf
        before = [bs.member_workspace(b)["ctype"].copy() for b in range(B)]
        assert bs.update(L=L2, U=U2) == 0
        r = bs.solve()
        for b, so in enumerate(sos):
            so.update(l=L2[b], u=U2[b]); hist[b].append(dict(l=L2[b], u=U2[b]))
            ro = so.solve()
            assert not np.array_equal(before[b], _oracle_ws(so)["ctype"])      # the update did change classes
            check(b, so, ro, "after a class change")
        # values only: every bound moves by the same small amount, no row changes class
        L3 = L2 - 0.01; U3 = U2 + 0.01
        for b in range(B):
            eq = L2[b] == U2[b]
            L3[b, eq] = U3[b, eq] = L2[b, eq] + 0.01
        assert bs.update(L=L3, U=U3) == 0
        r = bs.solve()
        for b, so in enumerate(sos):
            ct = _oracle_ws(so)["ctype"].copy()
            so.update(l=L3[b], u=U3[b]); hist[b].append(dict(l=L3[b], u=U3[b]))
            ro = so.solve()
            assert np.array_equal(ct, _oracle_ws(so)["ctype"])
            check(b, so, ro, "after a value update")
    assert fired >= 1          # the first check point really is after an in-loop rebuild of K^-1
    assert checked >= 6        # the K^-1 bound ran (m = 0 and m = 2n + 3 always assert cond(K) <= 1e5)


# ---------------------------------------------------------------------------------------------------------------
# (b) parity at the edge shapes and structures
# ---------------------------------------------------------------------------------------------------------------
def _oracle_counts_under_roundoff(orc, P, q, A, l, u, kw, draws=20):
    """Iteration counts the oracle itself reaches when q moves by 1e-15 relative (cold solves)."""
    rng = np.random.default_rng(0)
    return {orc.OracleOSQP().setup(P=P, q=q * (1 + 1e-15 * rng.standard_normal(q.size)), A=A, l=l, u=u, **kw).solve().info.iter
            for _ in range(draws)}


@pytest.mark.parametrize("kw", [{}, dict(scaling=0)], ids=["default", "scaling0"])
@pytest.mark.parametrize("n", SHAPES_N)
def test_parity_at_edge_shapes(gpu_lib, oracle_mod, n, kw):
    import osqp_amd
    for m in _ms(n):
        P, A, Q, L, U, _ = _shape_family(n, m, 4, seed=7 + 1000 * n + m)
        bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **kw)
        r = bs.solve()
        assert r.x.shape == (4, n) and r.y.shape == (4, m)
        for b in range(4):
            so = _oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw)
            ro = so.solve()
            if r.iter[b] != ro.info.iter:
                # Only a member whose count the oracle itself cannot pin down is let off its count (and the iterate
                # it ends on): the oracle must reach several counts under 1e-15 changes of q, the batch's among them
                # (measured: n = 16, m = 35, member 1 of the default run -- 325, 375, 425, 475).  Everything else
                # about the member is still checked.
                counts = _oracle_counts_under_roundoff(oracle_mod, P, Q[b], A, L[b], U[b], kw)
                assert len(counts) > 1 and int(r.iter[b]) in counts, ((n, m), b, int(r.iter[b]), ro.info.iter, sorted(counts))
                assert r.status_val[b] == ro.info.status_val
                _check_member_workspace(bs, b, so, (n, m), accuracy=False, rho_moved_ok=True)
                continue
            # scaled data, classes and padding; the K^-1 bound is section (a)'s (measured here: up to 17x numpy's error)
            _check_member_workspace(bs, b, so, (n, m), accuracy=False)
            _assert_parity(r, b, ro, (n, m))


def _structure(kind, seed):
    rng = np.random.default_rng(seed)
    n, m = 24, 40
    P, A, Q, L, U, x0 = _shape_family(n, m, 4, seed)
    A = A.tolil()
    if kind == "empty_col":
        A[:, 5] = 0.0
    elif kind == "empty_row":
        A[7, :] = 0.0
        L[:, 7], U[:, 7] = -rng.uniform(0, 1, 4), rng.uniform(0, 1, 4)
    elif kind == "p_diag_missing":
        Pd = P.tolil()
        for j in (0, 3, 11):
            Pd[j, :] = 0.0; Pd[:, j] = 0.0
        P = sparse.triu(Pd.tocsc(), format="csc"); P.eliminate_zeros()
        assert all(P[j, j] == 0 for j in (0, 3, 11))
    elif kind == "dense_row_col":
        A[4, :] = rng.standard_normal(n); A[:, 9] = rng.standard_normal((m, 1))
    elif kind == "mixed_classes":
        pass                                   # the family already mixes them; below: all four in every member
    A = A.tocsc(); A.eliminate_zeros()
    ax = A @ x0
    lo, hi = ax - rng.uniform(0.1, 1.0, m), ax + rng.uniform(0.1, 1.0, m)
    for b in range(4):
        L[b], U[b] = lo, hi
        L[b, 0:3], U[b, 0:3] = -np.inf, np.inf                       # free
        L[b, 3:6] = U[b, 3:6] = ax[3:6]                              # equality
        L[b, 6] = -np.inf; U[b, 8] = np.inf                          # one-sided
        if kind == "empty_row":
            L[b, 7], U[b, 7] = -rng.uniform(0, 1), rng.uniform(0, 1)
    return P, A, Q, L, U


@pytest.mark.parametrize("kw", [{}, dict(scaling=0)], ids=["default", "scaling0"])
@pytest.mark.parametrize("kind", ["empty_col", "empty_row", "p_diag_missing", "dense_row_col", "mixed_classes"])
def test_parity_structures(gpu_lib, oracle_mod, kind, kw):
    import osqp_amd
    P, A, Q, L, U = _structure(kind, seed=sum(map(ord, kind)))
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **kw)
    r = bs.solve()
    checked = 0
    for b in range(4):
        so = _oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw)
        _assert_parity(r, b, so.solve(), kind)
        checked += _check_member_workspace(bs, b, so, kind, max_cond=None) is not None
    # the K^-1 bound ran on at least one member (it applies where cond(K) <= 1e5); unscaled, the dense row and column
    # put every member above that (9e4 at the initial rho, more once rho adapts)
    assert checked >= 1 or (kind, kw) == ("dense_row_col", dict(scaling=0))


@pytest.mark.parametrize("kw", [{}, dict(scaling=0)], ids=["default", "scaling0"])
def test_parity_lp(gpu_lib, oracle_mod, kw):
    """P = 0: K = sigma I + A' rho A, with equality rows at 1e3 rho and a box on every variable (ill-conditioned:
    the refinement probe of the kernel decides on refinement here)."""
    import osqp_amd
    rng = np.random.default_rng(11)
    n, B = 30, 4
    Ar = sparse.random(8, n, density=0.4, random_state=rng, format="csc")
    A = sparse.vstack([sparse.eye(n), Ar], format="csc")
    P = sparse.csc_matrix((n, n))
    x0 = rng.uniform(-0.5, 0.5, n); ax = Ar @ x0
    L = np.tile(np.r_[-np.ones(n), ax - 0.2], (B, 1)); U = np.tile(np.r_[np.ones(n), ax + 0.2], (B, 1))
    L[:, n:n + 2] = U[:, n:n + 2] = ax[:2]
    Q = rng.standard_normal((B, n))
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **kw)
    r = bs.solve()
    for b in range(B):
        so = _oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw)
        _assert_parity(r, b, so.solve(), "LP")


# ---------------------------------------------------------------------------------------------------------------
# (c) per-QP matrices
# ---------------------------------------------------------------------------------------------------------------
def _per_qp_matrices(n, m, B, seed):
    """Shared patterns (triu P with its diagonal, A with three entries per row) and per-member values whose scale
    differs by up to 1e3 between members, with explicit zeros inside the pattern."""
    rng = np.random.default_rng(seed)
    off = sparse.triu(sparse.random(n, n, density=3.0 / n, random_state=rng, format="csc"), 1)
    Pu = sparse.triu(off + sparse.eye(n), format="csc"); Pu.sort_indices(); Pu.data[:] = 1.0
    rows = np.repeat(np.arange(m), 3); cols = np.concatenate([rng.choice(n, 3, replace=False) for _ in range(m)])
    A = sparse.csc_matrix((np.ones(3 * m), (rows, cols)), shape=(m, n)); A.sort_indices()
    r_, c_ = Pu.indices, np.repeat(np.arange(n), np.diff(Pu.indptr))      # CSC order of triu(P)
    diag = r_ == c_
    Px = np.empty((B, Pu.nnz)); Ax = np.empty((B, A.nnz))
    for b in range(B):
        v = rng.uniform(-0.4, 0.4, Pu.nnz)
        v[rng.random(Pu.nnz) < 0.2] = 0.0                                   # explicit zeros inside the pattern
        absrow = np.zeros(n)
        np.add.at(absrow, r_[~diag], np.abs(v[~diag])); np.add.at(absrow, c_[~diag], np.abs(v[~diag]))
        v[diag] = 1.0 + absrow + rng.uniform(0, 1, n)                       # diagonally dominant: P_b is PD
        Px[b] = v * 10.0 ** (3.0 * b / max(B - 1, 1))
        a = rng.standard_normal(A.nnz) * 10.0 ** rng.uniform(-1.5, 1.5)
        a[rng.random(A.nnz) < 0.1] = 0.0
        Ax[b] = a
    Q = rng.standard_normal((B, n))
    x0 = rng.standard_normal(n)
    L = np.empty((B, m)); U = np.empty((B, m))
    for b in range(B):
        ax = sparse.csc_matrix((Ax[b], A.indices, A.indptr), shape=(m, n)) @ x0
        L[b] = ax - rng.uniform(0.05, 1, m); U[b] = ax + rng.uniform(0.05, 1, m)
        L[b, :4] = U[b, :4] = ax[:4]
    return Pu, A, Px, Ax, Q, L, U


@pytest.mark.parametrize("n, m", [(40, 60), (100, 150), (150, 200)])
@pytest.mark.parametrize("which", ["P", "A", "PA"])
def test_per_qp_matrices(gpu_lib, oracle_mod, n, m, which):
    """Px_all only, Ax_all only, both: every member equals an oracle set up from its own matrices (CSC order of
    triu(P) and of A).  n = 150 takes the one-engine-per-member path."""
    import osqp_amd
    B = 6
    Pu, A, Px, Ax, Q, L, U = _per_qp_matrices(n, m, B, seed=n + len(which))
    if "A" not in which:                       # shared A: bounds must hold for the shared values
        Ax = None
        x0 = np.random.default_rng(n).standard_normal(n); ax = A @ x0
        L = np.tile(ax - 0.5, (B, 1)); U = np.tile(ax + 0.5, (B, 1))
    if "P" not in which:                       # shared P: the first member's (positive definite) values
        Pu, Px = sparse.csc_matrix((Px[0], Pu.indices, Pu.indptr), shape=(n, n)), None
    bs = osqp_amd.BatchOSQP().setup(Pu, A, Q, L, U, Px_all=Px, Ax_all=Ax)
    r = bs.solve()
    checked = 0
    for b in range(B):
        Pb = Pu if Px is None else sparse.csc_matrix((Px[b], Pu.indices, Pu.indptr), shape=(n, n))
        Ab = A if Ax is None else sparse.csc_matrix((Ax[b], A.indices, A.indptr), shape=(m, n))
        so = _oracle(oracle_mod, Pb, Q[b], Ab, L[b], U[b])
        assert so.nnzP == Pu.nnz and so.nnzA == A.nnz          # the explicit zeros stay in the pattern
        _assert_parity(r, b, so.solve(), which)
        if n <= 128:
            checked += _check_member_workspace(bs, b, so, which, max_cond=None) is not None
    if n > 128:
        with pytest.raises(RuntimeError):
            bs.member_workspace(0)
    if n <= 128:
        assert checked >= 1    # the K^-1 bound ran on at least one member (it applies where cond(K) <= 1e5)
        D = np.array([bs.member_workspace(b)["D"] for b in range(B)])
        assert len({tuple(d) for d in D}) == B                  # Ruiz scaling differs per member


# ---------------------------------------------------------------------------------------------------------------
# (d) bound and cost updates that change constraint classes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [1, 0])
def test_updates_change_classes(gpu_lib, oracle_mod, ws):
    import osqp_amd
    n, m, B = 30, 63, 4
    P, A, Q, L, U, x0 = _shape_family(n, m, B, seed=77)
    ax = A @ x0
    L = np.tile(ax - 0.5, (B, 1)); U = np.tile(ax + 0.5, (B, 1))          # all inequalities to start
    kw = dict(warm_start=ws)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **kw)
    sos = _oracles(oracle_mod, P, A, Q, L, U, **kw)
    r = bs.solve()
    for b, so in enumerate(sos):
        _assert_parity(r, b, so.solve(), "start")
    steps = []
    L1, U1 = L.copy(), U.copy(); L1[:, :10] = U1[:, :10] = ax[:10]         # inequalities -> equalities
    steps.append(("ineq->eq", None, L1, U1, {1: 10, 0: 53, -1: 0}))
    L2, U2 = L1.copy(), U1.copy(); L2[:, 20:30], U2[:, 20:30] = -np.inf, np.inf
    steps.append(("rows free", None, L2, U2, {1: 10, 0: 43, -1: 10}))
    L3, U3 = L2.copy(), U2.copy(); L3[:, :10] = ax[:10] - 0.25; U3[:, :10] = ax[:10] + 0.25
    steps.append(("eq->ineq", None, L3, U3, {1: 0, 0: 53, -1: 10}))
    steps.append(("q only", Q[::-1] * 2.0, None, None, {1: 0, 0: 53, -1: 10}))
    for name, Qn, Ln, Un, counts in steps:
        assert bs.update(Q=Qn, L=Ln, U=Un) == 0
        r = bs.solve()
        for b, so in enumerate(sos):
            if Qn is not None:
                so.update(q=Qn[b])
            else:
                so.update(l=Ln[b], u=Un[b])
            ro = so.solve()
            ct = bs.member_workspace(b)["ctype"]
            for cls, k in counts.items():
                assert int(np.sum(ct == cls)) == k, (name, cls)
            _assert_parity(r, b, ro, name)
            _check_member_workspace(bs, b, so, name)


# ---------------------------------------------------------------------------------------------------------------
# (e) member statuses in one batch, and the termination settings
# ---------------------------------------------------------------------------------------------------------------
def test_member_statuses_in_one_batch(gpu_lib, oracle_mod):
    """Variable 5 has an empty column of A and P_55 = 0 (nothing else in its row of P): with q_5 != 0 the member is
    dual infeasible; two contradictory copies of row 0 make a member primal infeasible; the others are solved."""
    import osqp_amd
    from osqp_amd import abi
    rng = np.random.default_rng(5)
    n, m, B = 20, 30, 6
    P, A, Q, L, U, x0 = _shape_family(n, m, B, seed=55)
    Pd = P.tolil(); Pd[5, :] = 0.0; Pd[:, 5] = 0.0
    P = sparse.triu(Pd.tocsc(), format="csc"); P.eliminate_zeros()
    A = A.tolil(); A[:, 5] = 0.0; A[1, :] = A[0, :]
    if A[0, :].nnz == 0:
        A[0, 0] = A[1, 0] = 1.0
    A = A.tocsc(); A.eliminate_zeros()
    ax = A @ x0
    L = np.tile(ax - 0.5, (B, 1)); U = np.tile(ax + 0.5, (B, 1))
    Q[:, 5] = 0.0
    Q[1, 5] = 1.5; Q[4, 5] = -0.7                                            # dual infeasible
    L[3, 0], U[3, 0] = ax[0] + 5.0, ax[0] + 6.0; L[3, 1], U[3, 1] = ax[0] - 6.0, ax[0] - 5.0   # primal infeasible
    kw = dict(max_iter=4000)
    r = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **kw).solve()
    want = {1: abi.OSQP_DUAL_INFEASIBLE, 4: abi.OSQP_DUAL_INFEASIBLE, 3: abi.OSQP_PRIMAL_INFEASIBLE}
    for b in range(B):
        ro = oracle_mod.OracleOSQP().setup(P=P, q=Q[b], A=A, l=L[b], u=U[b], **kw).solve()
        assert ro.info.status_val == want.get(b, abi.OSQP_SOLVED), (b, ro.info.status)
        _assert_parity(r, b, ro, "statuses")
        if b in (1, 4):
            assert np.all(r.x[b] == abi.OSQP_NAN) and np.all(r.y[b] == abi.OSQP_NAN)
            assert _rel(r.dual_inf_cert[b], ro.dual_inf_cert) < 1e-5, b
        if b == 3:
            assert np.all(r.x[b] == abi.OSQP_NAN)
            assert _rel(r.prim_inf_cert[b], ro.prim_inf_cert) < 1e-5


@pytest.mark.parametrize("kw", [dict(max_iter=7), dict(max_iter=60, check_termination=0),
                                dict(scaled_termination=1), dict(scaled_termination=1, scaling=0)],
                         ids=["max_iter", "no_check", "scaled_term", "scaled_term_unscaled"])
def test_termination_settings(gpu_lib, oracle_mod, kw):
    import osqp_amd
    n, m, B = 33, 69, 4
    P, A, Q, L, U, _ = _shape_family(n, m, B, seed=91)
    r = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **kw).solve()
    for b in range(B):
        ro = oracle_mod.OracleOSQP().setup(P=P, q=Q[b], A=A, l=L[b], u=U[b], **kw).solve()
        if "max_iter" in kw and kw.get("check_termination", 25):
            assert ro.info.status_val == -2
        _assert_parity(r, b, ro, str(kw))


# ---------------------------------------------------------------------------------------------------------------
# (f) a non-convex member; (g) settings the kernel does not implement
# ---------------------------------------------------------------------------------------------------------------
def _nonconvex_batch(n, B, bad, seed):
    """Shared dense triu(P) pattern, per member values: convex members have eigenvalues in [0.5, 2], member `bad`
    has one negative eigenvalue; A touches the first 10 variables only (tests/test_gpu_statuses._indefinite_qp)."""
    rng = np.random.default_rng(seed)
    m = 10
    Pu = sparse.triu(np.ones((n, n)), format="csc"); Pu.sort_indices()
    r_, c_ = Pu.indices, np.repeat(np.arange(n), np.diff(Pu.indptr))
    Px = np.empty((B, Pu.nnz))
    for b in range(B):
        Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
        ev = rng.uniform(0.5, 2.0, n)
        if b == bad:
            ev[0] = -rng.uniform(0.5, 1.0)
        M = Qm @ np.diag(ev) @ Qm.T
        Px[b] = (0.5 * (M + M.T))[r_, c_]
    A = sparse.hstack([sparse.eye(m, format="csc"), sparse.csc_matrix((m, n - m))], format="csc")
    Q = rng.standard_normal((B, n))
    return Pu, A, Px, Q, -np.ones((B, m)), np.ones((B, m))


def _c_setup(P, A, Q, L, U, Px_all=None, **settings):
    """osqp_amd_batch_setup called directly (no Python-side checks): (return code, handle)."""
    import osqp_amd
    from osqp_amd import abi
    from osqp_amd.batch import _bind, _p
    lib = osqp_amd.lib(); _bind(lib)
    Ph, Ah = abi.CscHolder(sparse.triu(P, format="csc")), abi.CscHolder(A)
    st = abi.OSQPSettings()
    lib.osqp_set_default_settings.restype = None
    lib.osqp_set_default_settings.argtypes = [C.POINTER(abi.OSQPSettings)]
    lib.osqp_set_default_settings(C.byref(st)); st.verbose = 0
    for k, v in settings.items():
        setattr(st, k, v)
    Q, L, U = abi.as_f64(Q), abi.as_f64(L), abi.as_f64(U)
    Px_all = None if Px_all is None else abi.as_f64(Px_all)
    h = C.c_void_p()
    rc = lib.osqp_amd_batch_setup(C.byref(h), Q.shape[0], C.byref(Ph.struct), C.byref(Ah.struct), _p(Px_all), _p(None),
                                  abi.fptr(Q), abi.fptr(L), abi.fptr(U), C.byref(st), 0)
    if rc == 0:
        lib.osqp_amd_batch_cleanup(h)
    return int(rc)


@pytest.mark.parametrize("n", [60, 150])
def test_nonconvex_member_rejected(gpu_lib, oracle_mod, capfd, n):
    """One member's K is indefinite (sigma = 1e-6): the oracle refuses that member alone with error 5, and so must
    the batch, on the kernel path (n <= 128: the Gauss-Jordan pivots) and on the one-engine-per-member path."""
    import osqp_amd
    B, bad = 5, 2
    Pu, A, Px, Q, L, U = _nonconvex_batch(n, B, bad, seed=n)
    for b in range(B):
        Pb = sparse.csc_matrix((Px[b], Pu.indices, Pu.indptr), shape=(n, n))
        if b == bad:
            with pytest.raises(ValueError, match="error 5"):
                oracle_mod.OracleOSQP().setup(P=Pb, q=Q[b], A=A, l=L[b], u=U[b])
        else:
            oracle_mod.OracleOSQP().setup(P=Pb, q=Q[b], A=A, l=L[b], u=U[b]).cleanup()
    try:
        bs = osqp_amd.BatchOSQP().setup(Pu, A, Q, L, U, Px_all=Px)
    except ValueError as e:
        assert "error 5" in str(e), str(e)
    else:
        r = bs.solve()
        pytest.fail("the non-convex member was set up; its solve returned status %d after %d iterations"
                    % (r.status_val[bad], r.iter[bad]))
    if n <= 128:
        capfd.readouterr()
        assert _c_setup(Pu, A, Q, L, U, Px_all=Px) == 5             # OSQP_NONCVX_ERROR
        assert "QP %d of the batch is non-convex" % bad in capfd.readouterr().err
    keep = [b for b in range(B) if b != bad]
    r = osqp_amd.BatchOSQP().setup(Pu, A, Q[keep], L[keep], U[keep], Px_all=Px[keep]).solve()
    for k, b in enumerate(keep):
        Pb = sparse.csc_matrix((Px[b], Pu.indices, Pu.indptr), shape=(n, n))
        _assert_parity(r, k, oracle_mod.OracleOSQP().setup(P=Pb, q=Q[b], A=A, l=L[b], u=U[b]).solve(), "convex rest")


@pytest.mark.parametrize("n", [40, 150])
@pytest.mark.parametrize("setting", [dict(polish=1), dict(time_limit=1.0)], ids=["polish", "time_limit"])
def test_unimplemented_settings_rejected(gpu_lib, capfd, n, setting):
    import osqp_amd
    P, A, Q, L, U, _ = _shape_family(n, n, 3, seed=3)
    name = next(iter(setting))
    with pytest.raises(ValueError, match="error 2.*%s" % name):
        osqp_amd.BatchOSQP().setup(P, A, Q, L, U, **setting)
    if n <= 128:
        capfd.readouterr()
        assert _c_setup(P, A, Q, L, U, **setting) == 2               # OSQP_SETTINGS_VALIDATION_ERROR
        assert name in capfd.readouterr().err


# ---------------------------------------------------------------------------------------------------------------
# (h) LDS sizing above 64 KiB, interleaved live batches, dispatch order at B > 1024
# ---------------------------------------------------------------------------------------------------------------
def _lds_bytes(n, m, Pu, A):
    """The kernel's LDS size per QP (batch.hip, osqp_amd_batch_setup: b->lds_bytes)."""
    NP = 64 if n <= 64 else 128
    nnzP, nnzA = Pu.nnz, A.nnz
    nnzPf = 2 * nnzP - int(np.sum(Pu.indices == np.repeat(np.arange(n), np.diff(Pu.indptr))))
    b = 8 * (nnzP + nnzA + 1 + 7 * NP + 11 * m + 4 * NP + 64 + 256) + \
        4 * (m + 4 + 3 * (n + 1) + 2 * nnzP + 2 * nnzPf + 4 * nnzA + m + 1)
    return (b + 15) & ~15


def _lds_problem(n, m, per_row, B, seed):
    rng = np.random.default_rng(seed)
    Pu = sparse.diags(rng.uniform(1, 3, n), format="csc")
    rows = np.repeat(np.arange(m), per_row)
    cols = np.concatenate([rng.choice(n, per_row, replace=False) for _ in range(m)])
    A = sparse.csc_matrix((rng.standard_normal(m * per_row), (rows, cols)), shape=(m, n)); A.sort_indices()
    x0 = rng.standard_normal(n); ax = A @ x0
    Q = rng.standard_normal((B, n))
    L = np.array([ax - rng.uniform(0.1, 1, m) for _ in range(B)]); U = np.array([ax + rng.uniform(0.1, 1, m) for _ in range(B)])
    return Pu, A, Q, L, U


def test_lds_above_64k_matches_oracle(gpu_lib, oracle_mod):
    import osqp_amd
    Pu, A, Q, L, U = _lds_problem(128, 384, 8, 4, seed=1)
    lds = _lds_bytes(128, 384, Pu, A)
    assert 64 * 1024 < lds <= 160 * 1024, lds
    r = osqp_amd.BatchOSQP().setup(Pu, A, Q, L, U).solve()
    for b in range(4):
        _assert_parity(r, b, oracle_mod.OracleOSQP().setup(P=Pu, q=Q[b], A=A, l=L[b], u=U[b]).solve(), lds)


def test_lds_above_160k_rejected(gpu_lib, capfd):
    import osqp_amd
    Pu, A, Q, L, U = _lds_problem(128, 600, 8, 2, seed=2)
    assert _lds_bytes(128, 600, Pu, A) > 160 * 1024
    capfd.readouterr()
    with pytest.raises(ValueError, match="error 4"):                # OSQP_LINSYS_SOLVER_INIT_ERROR
        osqp_amd.BatchOSQP().setup(Pu, A, Q, L, U)
    assert "160 KiB" in capfd.readouterr().err


def test_two_live_batches_of_different_lds_sizes(gpu_lib, oracle_mod):
    """The dynamic-LDS limit belongs to the kernel function: setting up a second, smaller batch of the same tile
    must not break the first one.  Set up ~126 KiB then ~78 KiB; solve first, second, first (cold starts; rho and
    K^-1 carry over between solves, in the batch as in the oracle workspaces)."""
    import osqp_amd
    big = _lds_problem(128, 384, 8, 3, seed=4)
    small = _lds_problem(128, 230, 8, 3, seed=5)
    lb, ls = _lds_bytes(128, 384, big[0], big[1]), _lds_bytes(128, 230, small[0], small[1])
    assert 64 * 1024 < ls < lb <= 160 * 1024, (ls, lb)
    kw = dict(warm_start=0)
    b1 = osqp_amd.BatchOSQP().setup(*big, **kw)
    b2 = osqp_amd.BatchOSQP().setup(*small, **kw)
    o1, o2 = _oracles(oracle_mod, *big, **kw), _oracles(oracle_mod, *small, **kw)
    for k, (bs, sos) in enumerate(((b1, o1), (b2, o2), (b1, o1))):
        r = bs.solve()
        for b, so in enumerate(sos):
            _assert_parity(r, b, so.solve(), ("solve", k))
    b1.cleanup(); b2.cleanup()


@pytest.mark.parametrize("B", [1, 1025, 2500])
def test_dispatch_order_large_batches(gpu_lib, monkeypatch, B):
    """Longest-first dispatch is scheduling only: three solves in sequence are bit-identical to index order,
    also above 1024 QPs, where k_batch_order loops over the batch."""
    import osqp_amd
    from osqp_amd.problems import mpc_batch
    s, Q, L, U = mpc_batch(batch=B)
    Q = Q + 0.05 * np.random.default_rng(B).standard_normal(Q.shape)
    runs = {}
    for lpt in ("0", "1"):
        monkeypatch.setenv("OSQP_AMD_BATCH_LPT", lpt)
        bs = osqp_amd.BatchOSQP().setup(s["P"], s["A"], Q, L, U, warm_start=0)
        runs[lpt] = [bs.solve() for _ in range(3)]
        bs.cleanup()
    if B > 1:
        assert len(set(runs["0"][0].iter.tolist())) > 1
    for a, b in zip(runs["0"], runs["1"]):
        assert np.array_equal(a.iter, b.iter) and np.array_equal(a.status_val, b.status_val)
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)
