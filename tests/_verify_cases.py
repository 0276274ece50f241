"""Cases of BatchOSQP.verify (tests/test_gpu_batch_verify.py on the device, tests/test_verify_reference_host.py for the
proofs the device tests lean on): the problems, the given points and the tolerances, built once and never modified.

  SHAPES   the four shapes of tests/_limits_cases.py, one per code path of the engines;
  EDGES    the kernel's own edges -- n = 1, m = 0, n and m one below and one above 64 and 256 (a wavefront and the
           256-thread workgroup of k_batch_verify: the last pass of a strided loop is one thread wide or one short), each
           on the engine that takes the shape; from n = 4, m = 3 upward the matrices carry a dense row of A, an empty
           column of A and a column of triu(P) with nothing on the diagonal ("structured");
  per-member values (Px_all / Ax_all, stride != 0) against shared ones on the first two shapes.

The given points of a case: X, Y random, Y with exact zeros; in the even members no multiplier sits on an infinite bound
(slots 10-12 finite), in the odd ones some do (+-OSQP_INFTY); one member has an IEEE NaN in x, one the number OSQP_NAN in
y; DX, DY random (the verdicts that hold are those of the status mix below), one member's DY with a NaN."""
import numpy as np
from scipy import sparse

from _batch_parity import shape_family
from _limits_cases import SHAPES, problem as limits_problem

OSQP_NAN = float(0x7FC00000)
EPS_GIVEN = (3e-2, 5e-2)          # eps_abs, eps_rel of the calls that give them
EPS_INF = (1e-4, 1e-4)            # the default eps_prim_inf, eps_dual_inf
DEFAULT_EPS = (1e-3, 1e-3)        # the default eps_abs, eps_rel of a handle
EDGES = {                         # engine, n, m, B, seed
    "n1": ("auto", 1, 3, 3, 2101), "m0": ("auto", 9, 0, 3, 2102), "n1m0": ("streamed", 1, 0, 2, 2103),
    "63x65": ("auto", 63, 65, 3, 2104), "65x63": ("auto", 65, 63, 3, 2105),
    "255x257": ("streamed", 255, 257, 2, 2106), "257x255": ("common", 257, 255, 3, 2107),
}
_cache = {}


def structured(P, A, seed):
    """P, A with a dense row 0 of A, an empty column e of A (P_ee stays), and a column j of triu(P) that holds one
    off-diagonal entry and no diagonal; a row of A with the single entry 5 on j keeps K = P + sigma I + A' rho A
    positive definite.  Needs n >= 4, m >= 3."""
    rng = np.random.default_rng(seed)
    n, m = A.shape[1], A.shape[0]
    e, j, i = n - 1, n - 2, 0
    Al = sparse.lil_matrix(A)
    Al[0, :] = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    Al[:, e] = 0.0
    Al[1, :] = 0.0; Al[1, j] = 5.0
    Pl = sparse.lil_matrix(sparse.triu(P))
    Pl[:, j] = 0.0; Pl[j, :] = 0.0
    Pl[i, j] = 0.05
    P2 = sparse.triu(Pl.tocsc(), format="csc"); P2.eliminate_zeros()
    A2 = Al.tocsc(); A2.eliminate_zeros()
    assert P2[j, j] == 0 and A2[:, e].nnz == 0 and A2[0, :].nnz == n - 1
    return P2, A2


def case(name):
    """dict(engine, P, A, Q, L, U, Px_all, Ax_all) of a shape, an edge or "<shape>+values" (per-member values)."""
    if name in _cache:
        return _cache[name]
    base, _, values = name.partition("+")
    if base in SHAPES:
        engine, P, A, Q, L, U = limits_problem(base)
    else:
        engine, n, m, B, seed = EDGES[base]
        P, A, Q, L, U, _ = shape_family(n, max(m, 1), B, seed)
        if m == 0:
            A = sparse.csc_matrix((0, n)); L = np.zeros((B, 0)); U = np.zeros((B, 0))
        elif n >= 4 and m >= 3:
            P, A = structured(P, A, seed)
        if engine == "common":           # one class per row over the batch: member 0's bounds, widened per member
            w, eq = np.linspace(0.0, 0.2, B)[:, None], L[:1] == U[:1]
            L, U = np.where(eq, L[:1], L[:1] - w), np.where(eq, U[:1], U[:1] + w)
    P = sparse.triu(P, format="csc"); P.sort_indices()
    A = sparse.csc_matrix(A); A.sort_indices()
    L, U = np.maximum(L, -1e30), np.minimum(U, 1e30)
    Px_all = Ax_all = None
    if values:
        rng = np.random.default_rng(77)
        B = Q.shape[0]
        Px_all = P.data[None, :] * rng.uniform(0.9, 1.1, (B, P.nnz))
        Ax_all = A.data[None, :] * rng.uniform(0.5, 1.5, (B, A.nnz))
    _cache[name] = dict(engine=engine, P=P, A=A, Q=Q, L=L, U=U, Px_all=Px_all, Ax_all=Ax_all)
    return _cache[name]


GIVEN = list(SHAPES) + list(EDGES) + ["tile4+values", "streamed+values"]


def points(name):
    """(X, Y, DX, DY) of the case, as the docstring of this file says."""
    key = ("points", name)
    if key in _cache:
        return _cache[key]
    c = case(name)
    B, n = c["Q"].shape
    m = c["A"].shape[0]
    rng = np.random.default_rng(len(name) * 131 + n * 7 + m)
    X = rng.standard_normal((B, n)); Y = rng.standard_normal((B, m)) * 10.0 ** rng.uniform(-1, 1, (B, m))
    Y[rng.random((B, m)) < 0.3] = 0.0
    for b in range(0, B, 2):             # even members: no multiplier part on an infinite bound
        Y[b] = np.where((Y[b] > 0) & (c["U"][b] > 1e26), 0.0, Y[b])
        Y[b] = np.where((Y[b] < 0) & (c["L"][b] < -1e26), 0.0, Y[b])
    DX = rng.standard_normal((B, n)); DY = rng.standard_normal((B, m))
    if B >= 3:
        X[B - 1, n // 2] = np.nan
    if B >= 4 and m:
        Y[B - 2, m // 3] = OSQP_NAN
    if B >= 2 and m:
        DY[1, 0] = np.nan
    _cache[key] = (X, Y, DX, DY)
    return _cache[key]


def handle(name, **kw):
    import osqp_amd
    c = case(name)
    extra = dict(Px_all=c["Px_all"], Ax_all=c["Ax_all"]) if c["Px_all"] is not None else {}
    return osqp_amd.BatchOSQP().setup(c["P"], c["A"], c["Q"], c["L"], c["U"], engine=c["engine"], **extra, **kw)


def reference(name, X, Y, DX, DY, eps=DEFAULT_EPS, members=None, **data):
    """batch_reference on the case's data, or on `data` where given (Q, L, U, Px_all, Ax_all: what an update left)."""
    from _verify_reference import batch_reference
    c = dict(case(name), **data)
    return batch_reference(c["P"], c["A"], c["Q"], c["L"], c["U"], X, Y, DX, DY, eps[0], eps[1], EPS_INF[0], EPS_INF[1],
                           Px_all=c["Px_all"], Ax_all=c["Ax_all"], members=members)


# ---- the status mix of tests/test_gpu_batch_edges.py::test_member_statuses_in_one_batch -----------------------------------
MIX_WANT = {1: -4, 4: -4, 3: -3}      # OSQP_DUAL_INFEASIBLE, OSQP_PRIMAL_INFEASIBLE; the others end OSQP_SOLVED
MIX_CAPS = (4000, 50)                 # max_iter of setup: every member ends by itself (after 25, 75 and 100 iterations) ...
MIX_CUT = {3: -2, 5: 2}               # ... or member 3 ends OSQP_MAX_ITER_REACHED, 5 OSQP_SOLVED_INACCURATE, the others as before


def status_mix():
    """Variable 5 has an empty column of A and no curvature: q_5 != 0 makes a member dual infeasible; two contradictory
    copies of row 0 make one primal infeasible; the others are solved."""
    if "mix" in _cache:
        return _cache["mix"]
    n, m, B = 20, 30, 6
    P, A, Q, L, U, x0 = shape_family(n, m, B, seed=55)
    Pd = P.tolil(); Pd[5, :] = 0.0; Pd[:, 5] = 0.0
    P = sparse.triu(Pd.tocsc(), format="csc"); P.eliminate_zeros()
    A = A.tolil(); A[:, 5] = 0.0; A[1, :] = A[0, :]
    if A[0, :].nnz == 0:
        A[0, 0] = A[1, 0] = 1.0
    A = A.tocsc(); A.eliminate_zeros()
    ax = A @ x0
    L = np.tile(ax - 0.5, (B, 1)); U = np.tile(ax + 0.5, (B, 1))
    Q = Q.copy(); Q[:, 5] = 0.0
    Q[1, 5] = 1.5; Q[4, 5] = -0.7
    L[3, 0], U[3, 0] = ax[0] + 5.0, ax[0] + 6.0; L[3, 1], U[3, 1] = ax[0] - 6.0, ax[0] - 5.0
    P.sort_indices(); A.sort_indices()
    _cache["mix"] = dict(P=P, A=A, Q=Q, L=L, U=U, Px_all=None, Ax_all=None)
    return _cache["mix"]
