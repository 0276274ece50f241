"""Seeded cases for the slack-elimination path of the single-QP engine (engine.hip: build_elim, engine_aux_kernels.h: k_elim_refresh) at
its edges, a Python restatement of build_elim's rule, the reduced system in long double and the bar on an eliminated ADMM step.
tests/test_elim_cases_host.py checks all of it on the CPU, tests/test_gpu_elim_edges.py runs the cases on the device.  Nothing
here touches the library.

make(name) returns the keys of _pcg_cases.make and claims['gone'] = {variable: its row} -- which variables build_elim takes
out of the linear system -- and claims['stay'] = {variable: why not}, both stated by hand in each generator.  P on the
variables that stay has eigenvalues in about [1, 10], a row of A with k entries is scaled by 1 / sqrt(k), rows carrying an
eliminated variable cover the classes RHO, 1e3 RHO (equality rows) and RHO_MIN (free rows).

The expected iterates of every test come from _engine_reference.admm_step, which solves the full K = P + sigma I + A' rho A
and knows nothing of elimination; reduced() serves the bars and the comparison with hipeng_resident_dump only."""
import functools

import numpy as np
from scipy import sparse

from tests import _engine_reference as R
from tests import _pcg_cases as PC

LD, U = R.LD, R.U
RHO, RHO_MIN, INF = PC.RHO, PC.RHO_MIN, PC.INF
PCG_EPS = PC.PCG_EPS
HUGE_ROW = PC.HUGE_ROW
RES_GONE = {8: 8, 20: 11}                   # E -> forced grid, found with hipeng_resident_plan (the CPU test asks it again): _pcg_cases.RESIDENT plus a tenth more variables

NAMES = ("all_gone", "all_gone_1", "one_gone_1", "one_gone_2", "pyy", "rivals", "lone_rows", "rounds", "long_rows", "huge_gone",
         "blocks_gone", "res_gone_e8", "res_gone_e20")
SEEDS = {name: 301 + k for k, name in enumerate(NAMES)}
SEEDS["lone_rows"] = 403                    # (with it the reference's z+ lands on l, on u and inside on the plain lone rows: test_elim_cases_host)
R.SEEDS.update(SEEDS)


# ---------------------------------------------------------------------------------------------------------------
# build_elim, restated
# ---------------------------------------------------------------------------------------------------------------
def eliminated(Pu, A):
    """(erow [n], ecol [m]): erow[j] the row of variable j if it is eliminated, else -1; ecol[i] the eliminated variable of row i,
    else -1.  Columns in order; a variable qualifies when triu(P) stores no off-diagonal entry in its row or column (an explicit
    zero counts), its column of A stores exactly one entry (an explicit zero counts), no earlier variable took that row, and the
    row stores fewer than 8192 entries.  Nothing when m == 0."""
    Pu, A = sparse.csc_matrix(Pu), sparse.csc_matrix(A)
    n, m = Pu.shape[0], A.shape[0]
    erow, ecol = np.full(n, -1), np.full(m, -1)
    if m == 0 or n == 0:
        return erow, ecol
    coupled = np.zeros(n, bool)
    for j in range(n):
        for k in range(Pu.indptr[j], Pu.indptr[j + 1]):
            if Pu.indices[k] != j:
                coupled[j] = coupled[Pu.indices[k]] = True
    rowlen = np.bincount(A.indices, minlength=m)
    for j in range(n):
        if coupled[j] or A.indptr[j + 1] - A.indptr[j] != 1:
            continue
        i = int(A.indices[A.indptr[j]])
        if ecol[i] >= 0 or rowlen[i] >= HUGE_ROW:
            continue
        erow[j], ecol[i] = i, j
    return erow, ecol


# ---------------------------------------------------------------------------------------------------------------
# the reduced system, long double
# ---------------------------------------------------------------------------------------------------------------
class _ReducedOp:
    """S = P_XX + sigma I + A_X' diag(rho~) A_X: apply(v) in long double, solve(r) in float64, lam_min()."""

    def __init__(self, pb, X, AX, sigma, rhoe):
        self.n, self.m = X.size, pb.m
        self.P, self.A, self.AT = pb.P[X][:, X].tocsr(), AX, AX.T.tocsr()
        self.sg, self.rhoe = LD(sigma), np.asarray(rhoe, dtype=LD)
        self.S = None
        if self.n == 0:
            return
        if self.n <= R.DENSE_MAX:
            self.S = sparse.csr_matrix(self.P + self.sg * sparse.eye(self.n, dtype=LD) + self.AT @ sparse.diags(self.rhoe) @ self.A)
            self.kkt = R._DenseKKT(self, float(sigma), self.rhoe.astype(float))
        else:
            self.kkt = R._SparseKKT(self, float(sigma), self.rhoe.astype(float))

    def apply(self, v):
        return self.P @ v + self.sg * v + self.AT @ (self.rhoe * (self.A @ v))

    def solve(self, r):
        v = self.kkt.solve(np.asarray(r, float)).astype(LD)
        for _ in range(3):
            v = v + self.kkt.solve((r - self.apply(v)).astype(float)).astype(LD)
        return v

    def lam_min(self):
        return self.kkt.lam_min() if self.n else np.inf


def reduced(pb, sigma, rho, erow, b=None):
    """The system the PCG iterates once the variables with erow >= 0 are gone, in long double: dict of
      X        the variables that stay
      a, Dy    per row: the eliminated variable's coefficient (0 on a row without one) and D_y = P_yy + sigma + rho a^2 (1 there)
      rhoe     rho~_i = rho_i (P_yy + sigma) / D_y, rho_i on a row without one
      S        P_XX + sigma I + A_X' diag(rho~) A_X, sparse (None above 3000 variables, where a huge row would fill it)
      bX       b_X - A_X' (rho a b_y / D_y) for the right-hand side b (None: not asked for)
      lam_min  of S in float64 (dense up to 3000 variables; above, Lanczos on the inverse through the quasi-definite form
               [[P_XX + sigma I, A_X'], [A_X, -1 / rho~]], as _engine_reference does for K; inf when X is empty)"""
    erow = np.asarray(erow)
    n, m = pb.n, pb.m
    rl, sg = np.asarray(rho, float).astype(LD), LD(sigma)
    X, Y = np.flatnonzero(erow < 0), np.flatnonzero(erow >= 0)
    a, Dy, rhoe = np.zeros(m, dtype=LD), np.ones(m, dtype=LD), rl.copy()
    pd = pb.P.diagonal().astype(LD)
    A = pb.A.tocsc()
    for j in Y:
        i = erow[j]
        a[i] = A[i, j]
        Dy[i] = pd[j] + sg + rl[i] * a[i] * a[i]
        rhoe[i] = rl[i] * (pd[j] + sg) / Dy[i]
    AX = A[:, X].tocsr()
    op = _ReducedOp(pb, X, AX, sigma, rhoe)
    out = dict(X=X, Y=Y, a=a, Dy=Dy, rhoe=rhoe, S=op.S, bX=None, lam_min=op.lam_min())
    if b is not None:
        b = np.asarray(b, dtype=LD)
        by = np.zeros(m, dtype=LD)
        by[erow[Y]] = b[Y]
        out["bX"] = b[X] - AX.T.tocsr() @ (rl * a * by / Dy)
    return out


def rhs(pb, sigma, rho, x, z, y):
    """b = sigma x - q + A'(rho z - y), long double."""
    x, z, y = (np.asarray(v, dtype=LD) for v in (x, z, y))
    b = LD(sigma) * x - pb.q
    return b + pb.AT @ (np.asarray(rho, float).astype(LD) * z - y) if pb.m else b


def xtilde_bars(pb, red, erow, rho, pcg_eps_rel, xt, norm_xt, base_abs, vbn_abs, direct_err=None):
    """(bxt, per-variable bar on x~, per-row bar on z~) of one linear solve on the reduced system, as step_bars_elim derives them;
    base_abs [n]: |sigma x| + |q| (a plugin solve: |b1|), vbn_abs [m]: |rho z| + |y| (a plugin solve: |rho b2|).  direct_err: the
    2-norm error of an unrefined float64 LU solve of the same system -- the direct forms' term 10 x direct_err of
    _engine_reference.step_bars then stands in place of the PCG term."""
    erow = np.asarray(erow)
    rho = np.asarray(rho, float)
    X, Y = red["X"], red["Y"]
    assert red["lam_min"] > 0.0, red["lam_min"]
    nb = float(np.sqrt((red["bX"] * red["bX"]).sum())) if X.size else 0.0
    bxt = (pcg_eps_rel * nb / red["lam_min"] if X.size else 0.0) + 50 * U * norm_xt
    if direct_err is not None:
        bxt = 10.0 * direct_err + 50 * U * norm_xt
    mask = np.zeros(pb.n)
    mask[X] = 1.0
    a1X = np.asarray(pb.Aa @ mask.astype(LD)).astype(float) if pb.m else np.zeros(0)
    ztaX = np.asarray(pb.Aa @ (mask * np.abs(xt))).astype(float) if pb.m else np.zeros(0)
    L = np.diff(pb.A.indptr) if pb.m else np.zeros(0)
    bar_xt = np.full(pb.n, bxt)
    bar_zt = a1X * bxt
    for j in Y:
        i = erow[j]
        a, D = abs(float(red["a"][i])), float(red["Dy"][i])
        T = base_abs[j] + a * vbn_abs[i] + rho[i] * a * ztaX[i]
        bar_xt[j] = rho[i] * a / D * a1X[i] * bxt + (L[i] + 13) * U * T / D
        bar_zt[i] += a * bar_xt[j] + 2 * U * a * abs(float(xt[j]))
    return bxt, bar_xt, bar_zt


def step_bars_elim(pb, st, red, erow, sigma, alpha, rho, pcg_eps_rel, x, z, y, direct=False):
    """Bars of x+, z+, y+ per element for a step whose linear solve ran on the reduced system.

    The engine stops on ||r||_2 <= pcg_eps_rel ||b||_2 of the system it iterates: k_pcg_init sums pbb += bj * bj with bj = 0 on
    an eliminated variable and bj = base + sB elsewhere, sB the product of the A' part with vb's m-part -- which k_refresh_m /
    k_admm_finalize's elim_vb left as rho z - y - rho a b_y / D_y on a row with an eliminated variable.  So ||b|| is ||b~_X||_2 of
    reduced(), and with ||S^-1 r|| <= ||r|| / lam_min(S)
        bxt = ||x~_X,dev - x~_X||_2 <= pcg_eps_rel ||b~_X||_2 / lam_min(S) + 50 U ||x~||_2.
    An eliminated y of row i is back-substituted by k_admm_finalize's row_apply, x~_y = (b_y - rho a zt) / D_y with
    zt = (A_X x~_X)_i:  |err| <= |rho a| / D_y ||A_iX||_1 bxt + (L_i + 13) U T / D_y,  T = |sigma x_y| + |q_y| + |a rho z_i| + |a y_i| +
    |rho a| sum_j |A_ij x~_j|.  Roundings on the longest path: the row sum (L_i + 4 for a row of L_i entries, as everywhere in
    _engine_reference), rho a, its product with zt, the subtraction, the product with 1 / D_y (4), and 1 / D_y itself: P_yy + sigma,
    a a, rho times it, the sum, the reciprocal (5); the terms of b_y pass through fewer (sigma x, - q, rho z, - y, a times, +: at
    most 4 before the subtraction).
    z~_i = zt + a x~_y then carries ||A_iX||_1 bxt + |a| err(x~_y) (+ one more rounding of |a x~_y|), and x+, z+, y+ follow as in
    _engine_reference.step_bars: alpha times the bar for x, alpha times that of z~_i for z, rho_i times that for y, each plus the
    rounding of its own update formula (st['rnd_*']).  direct: the engine applied an explicit inverse (dense-direct form) -- the
    direct term of _engine_reference.step_bars in place of the PCG term.  Nothing here is tuned on device output."""
    xa, za, ya, qa = (np.abs(np.asarray(v, dtype=float)) for v in (x, z, y, pb.q))
    rho = np.asarray(rho, float)
    bxt, bar_xt, bar_zt = xtilde_bars(pb, red, erow, rho, pcg_eps_rel, st["x_tilde"], st["norm_xt"], sigma * xa + qa, rho * za + ya,
                                       st["plain_err"] if direct else None)
    al = abs(alpha)
    return dict(x_tilde=bxt, x_tilde_each=bar_xt, x=al * bar_xt + st["rnd_x"].astype(float),
                z=al * bar_zt + st["rnd_z"].astype(float), y=rho * al * bar_zt + st["rnd_y"].astype(float))


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
def _coupled_diag(rng, nx, extra):
    """triu(P) on nx + extra variables: the first nx a tridiagonal chain (every one coupled, eigenvalues >= 1), the others a
    diagonal in [1, 10] and nothing else; (rows, cols, values)."""
    n = nx + extra
    r = np.concatenate([np.arange(n), np.arange(nx - 1)])
    c = np.concatenate([np.arange(n), np.arange(1, nx)])
    v = np.concatenate([rng.uniform(2.0, 3.0, nx), rng.uniform(1.0, 10.0, extra), np.full(nx - 1, -0.5)])
    return r, c, v


def _with(row, j, a):
    """The row (i, cols, values) with the entry a in column j added; the others rescaled to 1 / sqrt of the new length."""
    i, c, v = row
    k = len(c) + 1
    return (i, np.concatenate([np.asarray(c, int), [j]]), np.concatenate([np.asarray(v, float) * np.sqrt(len(c) / k), [a]]))


def _coef(rng, k=1):
    return rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)


def _three_classes(rows_gone, m, rng, others=()):
    """Equality, free and plain rows among `rows_gone` in turn (rows 0, 1, 2 of the list: equality, free, plain; ...), and a tenth
    / twentieth of `others`."""
    rows_gone = list(rows_gone)
    eq, free = rows_gone[0::3], rows_gone[1::3]
    others = np.asarray(list(others), int)
    if others.size:
        pick = rng.permutation(others)
        eq, free = eq + list(pick[: max(1, others.size // 10)]), free + list(pick[others.size // 10 + 1: others.size // 10 + 1 + others.size // 20])
    return eq, free


def _finish(name, rng, Pu, rows, n, m, gone, stay, eq, free, **more):
    # (_pcg_cases._finish keeps the longest row out of the free class: its rho is one that _pcg_cases' mutations change)
    return PC._finish(name, rng, Pu, rows, n, m, dict(gone=dict(gone), stay=dict(stay), dense=[], **more), eq, free)


def _all_gone(name, rng, n):
    """P and A diagonal (A a permuted diagonal): a box QP, every variable eliminated; the PCG system is empty."""
    perm = rng.permutation(n)
    Pu = sparse.diags(rng.uniform(1.0, 10.0, n), format="csc")
    rows = [(int(perm[j]), np.array([j]), _coef(rng)) for j in range(n)]
    eq, free = _three_classes(range(n), n, rng) if n > 1 else ([], [])
    return _finish(name, rng, Pu, rows, n, n, {j: int(perm[j]) for j in range(n)}, {}, eq, free)


def _one_gone(name, rng, j, i, equality):
    """_engine_reference's `offtile` (257 x 300, P tridiagonal) with variable j cut out of P's chain and given one entry, in row i."""
    n, m = 257, 300
    Pu = sparse.lil_matrix(R._tridiag(n, rng, skip=[j]))
    Pu[j, j] = 4.0
    others = np.setdiff1d(np.arange(n), [j])
    rows = PC._short(rng, range(m), others)
    rows[i] = _with(rows[i], j, float(_coef(rng)[0]))
    eq, free = PC._classes(rng, m, skip=[i])
    eq = list(eq) + ([i] if equality else [])
    stay = {int(k): "coupled in P" for k in others}
    return _finish(name, rng, sparse.csc_matrix(Pu), rows, n, m, {j: i}, stay, eq, free)


def _pyy(name, rng):
    """40 variables, 60 rows: variables 0..19 a chain in P, 20..39 uncoupled with one entry each, in rows 0..19 next to entries of
    the chain.  20..25 have no stored P diagonal, 26..31 a stored 0.0, 32..39 P_yy > 0.  Coefficients +-[0.5, 2] but a = +-1e-2 on
    variables 22, 28, 34, +-1e2 on 23, 29, 35 and a stored 0.0 on 36."""
    n, m, nx = 40, 60, 20
    r, c, v = _coupled_diag(rng, nx, 20)
    v[nx + 6: nx + 12] = 0.0
    keep = np.ones(r.size, bool)
    keep[nx: nx + 6] = False
    Pu = PC._csc_keep_zeros(r[keep], c[keep], v[keep], n)
    rows = PC._short(rng, range(m), np.arange(nx), 2, 4)
    a = _coef(rng, 20)
    a[[2, 8, 14]] = 1e-2 * np.sign(a[[2, 8, 14]])
    a[[3, 9, 15]] = 1e2 * np.sign(a[[3, 9, 15]])
    a[16] = 0.0
    for k in range(20):
        rows[k] = _with(rows[k], nx + k, a[k])
    eq, free = _three_classes(range(20), m, rng, range(20, m))
    stay = {k: "coupled in P" for k in range(nx)}
    return _finish(name, rng, Pu, rows, n, m, {nx + k: k for k in range(20)}, stay, eq, free)


def _rivals(name, rng):
    """60 variables, 40 rows: 0..29 a chain in P; 30 and 31 both have their one entry in row 0 (30 wins); 32 and 33 share an
    explicit-zero off-diagonal of P (one entry each, rows 1 and 2); 34 has two entries, in rows 3 and 4, the second a stored 0.0;
    35 has no entry in A; 36..59 are eliminated in rows 5..28."""
    n, m, nx = 60, 40, 30
    r, c, v = _coupled_diag(rng, nx, 30)
    Pu = PC._csc_keep_zeros(np.concatenate([r, [32]]), np.concatenate([c, [33]]), np.concatenate([v, [0.0]]), n)
    rows = PC._short(rng, range(m), np.arange(nx), 2, 4)
    rows[0] = _with(_with(rows[0], 30, float(_coef(rng)[0])), 31, float(_coef(rng)[0]))
    rows[1], rows[2] = _with(rows[1], 32, float(_coef(rng)[0])), _with(rows[2], 33, float(_coef(rng)[0]))
    rows[3], rows[4] = _with(rows[3], 34, float(_coef(rng)[0])), _with(rows[4], 34, 0.0)
    gone = {30: 0}
    for k in range(36, 60):
        rows[k - 31] = _with(rows[k - 31], k, float(_coef(rng)[0]))
        gone[k] = k - 31
    stay = {k: "coupled in P" for k in range(nx)}
    stay.update({31: "row 0 is taken by variable 30", 32: "explicit-zero off-diagonal (32, 33) in P", 33: "explicit-zero off-diagonal (32, 33) in P",
                 34: "two stored entries in its column of A, one an explicit zero", 35: "no entry in A"})
    eq, free = _three_classes([0] + list(range(5, 29)), m, rng, range(29, m))
    return _finish(name, rng, Pu, rows, n, m, gone, stay, eq, free)


def _lone_rows(name, rng):
    """50 variables, 60 rows: 0..29 a chain in P; variable 30 + k is the only entry of row 2 k (k < 20), rows 1, 3, ..., 19 are
    empty, the rest short rows on the chain."""
    n, m, nx = 50, 60, 30
    r, c, v = _coupled_diag(rng, nx, 20)
    Pu = PC._csc_keep_zeros(r, c, v, n)
    lone = [2 * k for k in range(20)]
    rest = [i for i in range(20, m) if i not in lone]
    rows = [(2 * k, np.array([nx + k]), _coef(rng)) for k in range(20)] + PC._short(rng, rest, np.arange(nx), 2, 4)
    eq, free = _three_classes(lone, m, rng, rest)
    stay = {k: "coupled in P" for k in range(nx)}
    return _finish(name, rng, Pu, rows, n, m, {nx + k: 2 * k for k in range(20)}, stay, eq, free, empty_rows=list(range(1, 20, 2)))


ROUND_ROWS = (3, 7, 255, 256, 1000, 1023, 1024, 1279, 1792, 2040, 2047)


def _rounds(name, rng):
    """_engine_reference's `empty` layout, 300 variables and 2100 rows of which 10..2070 are empty or hold one entry: build_blocks
    ends a stream block at 2048 rows, so rows 0..2047 are one block that k_admm_finalize walks in eight rounds of 256 rows -- the
    first on the prefetched RowIn, the others through row_load.  Variables 0..249 are a chain in P; eliminated: 250 and 251 in the
    short rows 3 and 7, 252..260 the only entry of rows 255, 256 (end of the first round, start of the second), 1000, 1023, 1024,
    1279, 1792, 2040, 2047 (the last row of the block), 261..270 in the short rows 2080..2089 of the next block; 271..299 have no
    entry in A.  With the finalize grid forced to one workgroup, gridDim TB = 256: eliminated variables on either side of it."""
    n, m, nx = 300, 2100, 250
    r, c, v = _coupled_diag(rng, nx, 50)
    Pu = PC._csc_keep_zeros(r, c, v, n)
    short = list(range(0, 10)) + list(range(2071, m))
    rows = PC._short(rng, short, np.arange(nx), 2, 4)
    at = {i: k for k, (i, _, _) in enumerate(rows)}
    gone = {}
    for k, i in enumerate(ROUND_ROWS):
        j = 250 + k
        if i in at:
            rows[at[i]] = _with(rows[at[i]], j, float(_coef(rng)[0]))
        else:
            rows.append((i, np.array([j]), _coef(rng)))
        gone[j] = i
    for k in range(10):
        rows[at[2080 + k]] = _with(rows[at[2080 + k]], 261 + k, float(_coef(rng)[0]))
        gone[261 + k] = 2080 + k
    eq, free = _three_classes(list(ROUND_ROWS) + list(range(2080, 2090)), m, rng, [i for i in short if i not in (3, 7) and not 2080 <= i < 2090])
    stay = {k: "coupled in P" for k in range(nx)}
    stay.update({k: "no entry in A" for k in range(271, n)})
    return _finish(name, rng, Pu, rows, n, m, gone, stay, eq, free)


def _long_rows(name, rng):
    """600 variables, 40 rows: a chain in P on all but the six variables 0, 100, 599 and 300, 301, 302.  Row 0 has 511 entries, the
    eliminated 0 first; row 1 has 512, the eliminated 100 at offset 63 (63 columns below it); row 2 has 513, the eliminated 599
    last; 300..302 are eliminated in the short rows 3..5.  The long rows are an equality, a free and a plain row."""
    n, m = 600, 40
    ys = [0, 100, 599, 300, 301, 302]
    Pu = sparse.lil_matrix(R._tridiag(n, rng, skip=ys))
    for j in ys:
        Pu[j, j] = rng.uniform(1.0, 10.0)
    others = np.setdiff1d(np.arange(n), ys)
    rows = PC._short(rng, range(3, m), others)
    rows.append(_with(PC._scaled_row(0, rng.choice(others, 510, replace=False), rng), 0, float(_coef(rng)[0])))
    below, above = others[others < 100], others[others > 100]
    cols = np.concatenate([rng.choice(below, 63, replace=False), rng.choice(above, 448, replace=False)])
    rows.append(_with(PC._scaled_row(1, cols, rng), 100, float(_coef(rng)[0])))
    rows.append(_with(PC._scaled_row(2, rng.choice(others, 512, replace=False), rng), 599, float(_coef(rng)[0])))
    for k in range(3):
        rows[k] = _with(rows[k], 300 + k, float(_coef(rng)[0]))
    eq, free = _three_classes([0, 2, 1, 3, 4, 5], m, rng, range(6, m))       # row 0 equality, row 2 free, row 1 plain
    stay = {int(k): "coupled in P" for k in others}
    return _finish(name, rng, sparse.csc_matrix(Pu), rows, n, m, {0: 0, 100: 1, 599: 2, 300: 3, 301: 4, 302: 5}, stay, eq, free,
                   long=[1, 2], huge=[])          # (511 entries: still a stream row)


def _huge_gone(name, rng):
    """_pcg_cases' huge_nh1 layout, n = 8200, P diagonal (no variable coupled): row 0 holds 8192 entries, on variables 0..8191
    (huge, folded into k_cg_B); row 1 holds 8191, on 0..8189 and 8192; rows 2..41 are short rows on 0..8189, rows 2..5 also hold
    8193..8196.  Eliminated: 8192 (last of a row of 8191) and 8193..8196.  8190 and 8191 have their one entry in the huge row and
    stay; 8197..8199 have no entry."""
    n, m = 8200, 42
    Pu = sparse.diags(rng.uniform(1.0, 10.0, n), format="csc")
    rows = [PC._scaled_row(0, np.arange(8192), rng), _with(PC._scaled_row(1, np.arange(8190), rng), 8192, float(_coef(rng)[0]))]
    rows += PC._short(rng, range(2, m), np.arange(8190))
    gone = {8192: 1}
    for k in range(4):
        rows[2 + k] = _with(rows[2 + k], 8193 + k, float(_coef(rng)[0]))
        gone[8193 + k] = 2 + k
    stay = {k: "two or more entries in A" for k in range(8190)}
    stay.update({8190: "its one row holds 8192 entries", 8191: "its one row holds 8192 entries"})
    stay.update({k: "no entry in A" for k in range(8197, n)})
    eq, free = _three_classes([1, 2, 3, 4, 5], m, rng, range(6, m))
    return _finish(name, rng, Pu, rows, n, m, gone, stay, eq, free, long=[1], huge=[0])


def _blocks_gone(name, rng):
    """Dense diagonal blocks of P of 32, 64 and 128 variables (k_pcg_init<true>, k_cg_B<true, *>), then 60 uncoupled variables, one
    in each of the rows 0..59 next to entries on the blocks; 30 more short rows."""
    sizes, extra = (32, 64, 128), 60
    nx = sum(sizes)
    n, m = nx + extra, 90
    Pb = PC._block_diag_triu([PC._full_block(rng, b) for b in sizes])
    Pu = sparse.bmat([[Pb, None], [None, sparse.diags(rng.uniform(1.0, 10.0, extra))]], format="csc")
    rows = PC._short(rng, range(m), np.arange(nx), 2, 4)
    for k in range(extra):
        rows[k] = _with(rows[k], nx + k, float(_coef(rng)[0]))
    eq, free = _three_classes(range(extra), m, rng, range(extra, m))
    starts = np.concatenate([[0], np.cumsum(sizes)])
    stay = {k: "coupled in P" for k in range(nx)}
    c = _finish(name, rng, Pu, rows, n, m, {nx + k: k for k in range(extra)}, stay, eq, free)
    c["claims"]["dense"] = [(int(s), b, PC._pitch(b)) for s, b in zip(starts[:-1], sizes)]
    return c


def _res_gone(name, rng, E):
    """_pcg_cases' resident problem for E with n // 10 more variables after it: uncoupled, P_yy in [1, 10], each the slack of one of
    the first n // 10 rows, which are the equality rows."""
    n0, m, kp, ka, nwg = PC.RESIDENT[E]
    base = PC._resident(name, rng, E)
    extra = n0 // 10
    n = n0 + extra
    Pu = sparse.bmat([[base["Pu"], None], [None, sparse.diags(rng.uniform(1.0, 10.0, extra))]], format="csc")
    A = sparse.csr_matrix(base["A"])
    rows = [(i, A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]) for i in range(m)]
    for k in range(extra):
        rows[k] = _with(rows[k], n0 + k, float(_coef(rng)[0]))
    stay = {k: "coupled in P" for k in range(n0)}
    c = _finish(name, rng, Pu, rows, n, m, {n0 + k: k for k in range(extra)}, stay, list(range(extra)), [extra, extra + 1, extra + 2])
    c["claims"].update(E=E, nwg=RES_GONE[E])
    return c


@functools.lru_cache(maxsize=None)
def make(name):
    rng = np.random.default_rng(SEEDS[name])
    if name == "all_gone":
        return _all_gone(name, rng, 300)
    if name == "all_gone_1":
        return _all_gone(name, rng, 1)
    if name == "one_gone_1":
        return _one_gone(name, rng, 256, 0, True)
    if name == "one_gone_2":
        return _one_gone(name, rng, 0, 299, False)
    if name.startswith("res_gone_e"):
        return _res_gone(name, rng, int(name[10:]))
    return {"pyy": _pyy, "rivals": _rivals, "lone_rows": _lone_rows, "rounds": _rounds, "long_rows": _long_rows,
            "huge_gone": _huge_gone, "blocks_gone": _blocks_gone}[name](name, rng)


def claimed(c):
    """(erow, ecol) as the case's claims state them."""
    erow, ecol = np.full(c["n"], -1), np.full(c["m"], -1)
    for j, i in c["claims"]["gone"].items():
        erow[j], ecol[i] = i, j
    return erow, ecol


# ---------------------------------------------------------------------------------------------------------------
# the full-K reference, refined; model mutations
# ---------------------------------------------------------------------------------------------------------------
def refine(pb, sigma, rho, b, xt):
    """Refinement of K xt = b (float64 LU, residual in long double) until the residual stops falling: (xt, residual 2-norm)."""
    rl, sg = np.asarray(rho, float).astype(LD), LD(sigma)
    kkt = (R._DenseKKT if pb.n <= R.DENSE_MAX else R._SparseKKT)(pb, float(sigma), np.asarray(rho, float))
    K = lambda v: pb.P @ v + sg * v + (pb.AT @ (rl * (pb.A @ v)) if pb.m else 0)
    xt = np.asarray(xt, dtype=LD)
    r = b - K(xt)
    best = float(np.sqrt((r * r).sum()))
    for _ in range(20):
        cand = xt + kkt.solve(r.astype(float)).astype(LD)
        rc = b - K(cand)
        nr = float(np.sqrt((rc * rc).sum()))
        if nr >= best:
            break
        xt, r, best = cand, rc, nr
    return xt, best


def mutated_steps(pb, red, erow, sigma, alpha, rho, x, z, y, q_prev):
    """x+, z+, y+ (long double) of six wrong models of the eliminated step, each differing from the right one in one place of
    k_elim_refresh / elim_vb / row_apply.  The reduced solve itself is exact here (a dense long-double-residual solve of S):
      rho_for_rhoe    rho instead of rho~ weighs the eliminated rows in S
      by_without_a    b_y without its a (rho z - y) term
      by_previous_q   b_y with q_prev in place of q
      zt_incomplete   z~ of an eliminated row without a x~_y
      Dy_without_sigma   D_y = P_yy + rho a^2
      x_without_alpha    x+_y = x~_y
    Returns {label: (x+, z+, y+)} and 'none': the unmutated model, which must agree with admm_step."""
    erow = np.asarray(erow)
    X, Y = red["X"], red["Y"]
    rl, sg, al = np.asarray(rho, float).astype(LD), LD(sigma), LD(alpha)
    x, z, y = (np.asarray(v, dtype=LD) for v in (x, z, y))
    A = pb.A.tocsc()
    AX = A[:, X].tocsr()
    pd = pb.P.diagonal().astype(LD)
    rows = erow[Y]
    a = red["a"]

    def model(mut):
        Dy, rhoe = red["Dy"].copy(), red["rhoe"].copy()
        if mut == "Dy_without_sigma":
            Dy[rows] = pd[Y] + rl[rows] * a[rows] ** 2
        if mut == "rho_for_rhoe":
            rhoe = rl.copy()
        q = np.asarray(q_prev, dtype=LD) if mut == "by_previous_q" else pb.q
        vbn = rl * z - y
        by = np.zeros(pb.m, dtype=LD)
        by[rows] = sg * x[Y] - q[Y] + (0 if mut == "by_without_a" else a[rows] * vbn[rows])
        bX = sg * x[X] - pb.q[X] + AX.T.tocsr() @ (vbn - rl * a * by / Dy)
        xt = np.zeros(pb.n, dtype=LD)
        if X.size:
            xt[X] = _ReducedOp(pb, X, AX, sigma, rhoe).solve(bX)
        zt = AX @ xt[X] if X.size else np.zeros(pb.m, dtype=LD)
        xt[Y] = ((by - rl * a * zt) / Dy)[rows]
        if mut != "zt_incomplete":
            zt = zt + a * xty_rows(xt)
        xn = al * xt + (1 - al) * x
        if mut == "x_without_alpha":
            xn[Y] = xt[Y]
        w = al * zt + (1 - al) * z
        zn = np.minimum(np.maximum(w + y / rl, pb.l), pb.u)
        return xn, zn, y + rl * (w - zn)

    def xty_rows(xt):
        out = np.zeros(pb.m, dtype=LD)
        out[rows] = xt[Y]
        return out

    return {mut: model(mut) for mut in ("none", "rho_for_rhoe", "by_without_a", "by_previous_q", "zt_incomplete", "Dy_without_sigma", "x_without_alpha")}
