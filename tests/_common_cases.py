"""Cases of the common-K batch engine (BatchOSQP(engine="common")): `shape_family`'s matrices with the class of each
row drawn ONCE for the batch, and per member its own q, bounds and feasible point -- one model, many right-hand sides.

The yardstick for members that differ is the reference run on the member's PRE-SCALED data with scaling = 0: the
engine's common scaling (D, E, c of the reference's scale_data on (P, q^, A), q^_j = max_b |Q[b][j]|) is applied by
hand -- c D P D, c D q, E A D, E l, E u -- and the oracle solves that problem unscaled.  Its x~, y~, obj~ give the
member's x = D x~, y = E y~ / c, obj = obj~ / c, and its iteration count and status are the member's (with
scaled_termination = 1 on the engine: the residuals it tests are the scaled ones).  tests/test_common_cases_host.py
shows on the CPU that the reference with its own scaling and scaled_termination = 1 equals that run."""
import numpy as np
from scipy import sparse

from _batch_parity import oracle, shape_family

# (n, m) the GPU tests use with the common scaling; B = 5 members, seed 1000 + n + m
CASES = [(1, 0), (1, 1), (17, 37), (33, 66), (129, 258), (300, 600)]
# scaling = 0 with a fixed rho needs thousands of iterations from n = 33 upward: those cases stay at n <= 17
CASES_UNSCALED = [(1, 0), (1, 1), (17, 37)]
UNSCALED_MAX_ITER = 300    # some members of the (17, 37) case need more without scaling, some fewer
# (n, m, factor on q) of the adaptive-rho cases: with the default tolerance of 5 the plain family rarely moves rho; a
# q a hundred times larger makes every member's own reference run move it (test_common_cases_host.py)
ADAPTIVE_CASES = [(33, 66, 100.0), (129, 258, 100.0)]
ADAPTIVE = dict(adaptive_rho_interval=10)
FIXED = dict(adaptive_rho=0, scaled_termination=1)


def common_family(n, m, B, seed, PA=None):
    """P, A of shape_family(n, m, ., seed); one class per row for the whole batch (inequality 55 %, equality 15 %,
    one-sided 20 %, free 10 %); per member a feasible point x0_b, q_b of its own scale and its own bound widths.
    Every row holds A x0_b in member b, so every member is feasible."""
    P, A = PA if PA is not None else shape_family(n, m, 1, seed)[:2]
    m = A.shape[0]
    rng = np.random.default_rng(seed + 7)
    cls = rng.choice(4, m, p=[0.55, 0.15, 0.2, 0.1])
    side = rng.random(m) < 0.5
    Q = np.empty((B, n)); L = np.empty((B, m)); U = np.empty((B, m)); X0 = np.empty((B, n))
    for b in range(B):
        X0[b] = rng.standard_normal(n)
        ax = A @ X0[b]
        Q[b] = rng.standard_normal(n) * 10.0 ** rng.uniform(-0.5, 1)
        lo = ax - rng.uniform(0.05, 1.0, m); hi = ax + rng.uniform(0.05, 1.0, m)
        lo[cls == 1] = hi[cls == 1] = ax[cls == 1]
        lo[(cls == 2) & side] = -np.inf; hi[(cls == 2) & ~side] = np.inf
        lo[cls == 3] = -np.inf; hi[cls == 3] = np.inf
        L[b], U[b] = lo, hi
    return P, A, Q, L, U, X0


def qhat(Q):
    return np.abs(np.asarray(Q, float)).max(axis=0)


def common_oracle(orc, P, A, Q, L, U, **kw):
    """The oracle set up on the one-member image (P, q^, A, L[0], U[0]): its workspace carries the common D, E, c,
    the scaled matrix values and the row classes."""
    m = A.shape[0]
    return oracle(orc, P, qhat(Q), A, L[0] if m else np.zeros(0), U[0] if m else np.zeros(0), **kw)


def row_classes(l, u, E, rho_tol=1e-4):
    """auxil.c:76-98 on the scaled bounds: -1 loose, 1 equality, 0 inequality."""
    ls, us = np.maximum(l, -1e30) * E, np.minimum(u, 1e30) * E
    return np.where((ls < -1e26) & (us > 1e26), -1, np.where(us - ls < rho_tol, 1, 0))


def prescaled(ws, Q, L, U, b):
    """Member b's problem in the common scaled space: (c D P D, c D q, E A D, E l, E u)."""
    D, E, c = ws["D"], ws["E"], ws["c"]
    return ws["Pu"], c * D * Q[b], ws["A"], E * np.maximum(L[b], -1e30), E * np.minimum(U[b], 1e30)


def prescaled_oracle(orc, ws, Q, L, U, b, **kw):
    Pb, qb, Ab, lb, ub = prescaled(ws, Q, L, U, b)
    kw = dict(kw, scaling=0)
    kw.pop("scaled_termination", None)
    return oracle(orc, Pb, qb, Ab, lb, ub, **kw)


def unscale(ws, ro):
    """x, y, obj of the member from the pre-scaled oracle run."""
    return ws["D"] * ro.x, ws["E"] * ro.y / ws["c"], ro.info.obj_val / ws["c"]


def adaptive_family(n, m, B, qscale):
    P, A, Q, L, U, X0 = common_family(n, m, B, 1000 + n + m)
    return P, A, Q * qscale, L, U, X0


MIXED = dict(n=33, m=66, B=6, seed=1099, pinf=2, dinf=4)


def mixed_family():
    """One batch with solved members, one primal infeasible (member `pinf`) and one dual infeasible (member `dinf`),
    the classes of every row still common.  Variable 5 has zero curvature and meets one row only, x_5 >= bound (one
    sided: free above); q_5 = +1 keeps it at the bound, q_5 = -1 in member `dinf` sends it to infinity.  Two
    equality rows sit on variable 7 alone: equal values (the member's x0_7) everywhere, 1 and 2 in member `pinf`.
    Both members share |q| with a solved member and member 0 is a solved one, so the common scaling is that of the
    batch without the two."""
    n, m, B, seed = MIXED["n"], MIXED["m"], MIXED["B"], MIXED["seed"]
    P, A = shape_family(n, m, 1, seed)[:2]
    Pd = P.tolil(); Pd[5, :] = 0.0; Pd[:, 5] = 0.0
    P = sparse.triu(Pd.tocsc(), format="csc"); P.eliminate_zeros()
    Al = A.tolil(); Al[:, 5] = 0.0
    extra = sparse.lil_matrix((3, n)); extra[0, 5] = 1.0; extra[1, 7] = 1.0; extra[2, 7] = 1.0
    A = sparse.vstack([Al.tocsc(), extra.tocsc()], format="csc"); A.eliminate_zeros()
    P, A, Q, L, U, X0 = common_family(n, m, B, seed, PA=(P, A))
    for b in range(B):
        L[b, m], U[b, m] = X0[b, 5] - 1.0, np.inf
        L[b, m + 1] = U[b, m + 1] = L[b, m + 2] = U[b, m + 2] = X0[b, 7]
    Q[:, 5] = 1.0
    pinf, dinf = MIXED["pinf"], MIXED["dinf"]
    Q[pinf] = Q[1]; Q[dinf] = Q[3]
    Q[dinf, 5] = -1.0
    L[pinf, m + 1] = U[pinf, m + 1] = 1.0; L[pinf, m + 2] = U[pinf, m + 2] = 2.0
    return P, A, Q, L, U
