"""Long-double model of the infeasibility kernels of the row-partitioned solve (csrc/rowpart_native.h: k_rp_delta_x / k_rp_delta_y,
k_rp_cert_x / k_rp_cert_rows / k_rp_cert_fin, the host's verdict and the certificates) in the style of tests/_rowpart_reference.py, whose
Model, bounds and sizes it builds on, with the seeded cases they are tested on (tests/test_rowpart_cert_reference.py against the oracle on
the CPU, tests/test_gpu_rowpart_infeasible.py on the device), and the whole-solve problems of tests/test_rowpart_infeasible.py.

The seven scalars (SC7_NAMES), all in the scaled space except where E, D, Dinv unscale them (only when the data is scaled and
scaled_termination is 0, as is_primal_infeasible / is_dual_infeasible do, src/auxil.c:361-512):

  ndy    |E dy|_inf over all rows            max of single products: 2 U |value|
  viol   max(0, (Einv A dx)_i : u_i finite, -(Einv A dx)_i : l_i finite)     the bound of A dx (a sum of L terms) times Einv, + 2 U
  lhs    sum u_i max(dy_i, 0) + l_i min(dy_i, 0)                             (m + 6) U sum |terms|
  nAtdy  |Dinv A'dy|_inf                     (L + 4) U sum |terms| per element, times Dinv, + 2 U
  ndx    |D dx|_inf                          2 U |value|
  qdx    q'dx                                (n + 6) U sum |terms|
  nPdx   |Dinv P dx|_inf                     as nAtdy

dx and dy themselves are single float64 operations on the iterates (a subtraction, a selection), so the device's must equal them bit for
bit.  A verdict is `conditioned` when no comparison it takes lies within the bounds of its two sides; every seeded case is."""
import numpy as np
from scipy import sparse

import _rowpart_reference as R

LD, U = R.LD, R.U
INF_BOUND, DIV_TOL, OSQP_INFTY = R.INF_BOUND, R.DIV_TOL, 1e30
SC7_NAMES = ("ndy", "viol", "lhs", "nAtdy", "ndx", "qdx", "nPdx")
INFEASIBLE = ("primal infeasible", "primal infeasible inaccurate", "dual infeasible", "dual infeasible inaccurate")


def deltas(M, x0, y0, x1, y1):
    """dx = x1 - x0 and dy = y1 - y0 projected on the polar of the recession cone of [l, u] (src/auxil.c:374-387), in float64."""
    x0, y0, x1, y1 = (np.asarray(v, dtype=np.float64) for v in (x0, y0, x1, y1))
    dx, dy = x1 - x0, y1 - y0
    infu, infl = M.u > INF_BOUND, M.l < -INF_BOUND
    dy = np.where(infu & infl, 0.0, np.where(infu, np.minimum(dy, 0.0), np.where(infl, np.maximum(dy, 0.0), dy)))
    return dx, dy


def cert_scalars(M, dx, dy):
    """The seven scalars from dx, dy (float64 arrays) in long double, their bounds, and where each maximum sits."""
    n, m, un = M.n, M.m, M.unscaled_termination()
    dx, dy = np.asarray(dx, dtype=LD), np.asarray(dy, dtype=LD)
    val, bnd, at = np.zeros(7, dtype=LD), np.zeros(7, dtype=LD), dict()
    E, Einv = (M.E, M.Einv) if un else (np.ones(m), np.ones(m))
    D, Dinv = (M.D, M.Dinv) if un else (np.ones(n), np.ones(n))

    def mx(k, v, b):
        if v.size:
            i = int(np.argmax(v))
            val[k], bnd[k], at[SC7_NAMES[k]] = v[i], b.max(), i
    if m:
        mx(0, np.abs(E * dy), 2 * U * np.abs(E * dy))
        adx, aab = M.A_mul(dx)
        a, a_b = Einv * adx, Einv * (M.LAr + 4) * U * aab + 2 * U * np.abs(Einv * adx)
        finu, finl = M.u < INF_BOUND, M.l > -INF_BOUND
        cand = np.maximum(np.where(finu, a, 0), np.where(finl, -a, 0))
        mx(1, np.maximum(cand, 0), np.where(finu | finl, a_b, 0))
        t = M.u * np.maximum(dy, 0) + M.l * np.minimum(dy, 0)
        val[2], bnd[2] = t.sum(), (m + 6) * U * np.abs(t).sum()
        aty, tab = M.At_mul(dy)
        mx(3, np.abs(Dinv * aty), Dinv * (M.LAc + 4) * U * tab + 2 * U * np.abs(Dinv * aty))
    mx(4, np.abs(D * dx), 2 * U * np.abs(D * dx))
    t = M.q * dx
    val[5], bnd[5] = t.sum(), (n + 6) * U * np.abs(t).sum()
    px, pab = M.P_mul(dx)
    mx(6, np.abs(Dinv * px), Dinv * (M.LP + 4) * U * pab + 2 * U * np.abs(Dinv * px))
    return val, bnd, at


def tests(M, sc7, eps_p, eps_d, bnd=None):
    """is_primal_infeasible / is_dual_infeasible on the seven scalars: (primal, dual, conditioned).  The comparisons are the reference's,
    all strict; with bounds, `conditioned` says that none of them lies within the bounds of its two sides."""
    s = dict(zip(SC7_NAMES, sc7))
    b = dict(zip(SC7_NAMES, bnd)) if bnd is not None else dict.fromkeys(SC7_NAMES, 0)
    cs = M.c if M.unscaled_termination() else 1.0
    cmp_ = []          # (left, right, slack): the reference asks left < right

    def lt(a, c, slack):
        cmp_.append((a, c, slack))
        return bool(a < c)
    prim = dual = False
    if M.m and eps_p > 0 and lt(DIV_TOL, s["ndy"], b["ndy"]):
        p1 = lt(s["lhs"], eps_p * s["ndy"], b["lhs"] + eps_p * b["ndy"])
        p2 = lt(s["nAtdy"], eps_p * s["ndy"], b["nAtdy"] + eps_p * b["ndy"])
        prim = p1 and p2
    if eps_d > 0 and lt(DIV_TOL, s["ndx"], b["ndx"]):
        d1 = lt(s["qdx"], cs * eps_d * s["ndx"], b["qdx"] + cs * eps_d * b["ndx"])
        d2 = lt(s["nPdx"], cs * eps_d * s["ndx"], b["nPdx"] + cs * eps_d * b["ndx"])
        d3 = not lt(eps_d * s["ndx"], s["viol"], b["viol"] + eps_d * b["ndx"])
        dual = d1 and d2 and d3
    conditioned = all(abs(a - c) > 4 * slack + 4 * U * (abs(a) + abs(c)) for a, c, slack in cmp_)
    return prim, dual, conditioned


def certificates(M, dx, dy, sc7):
    """prim_inf_cert, dual_inf_cert as store_solution leaves them (src/auxil.c:545-555, 762-780): (E dy) / |E dy|_inf, (D dx) / |D dx|_inf."""
    un = M.unscaled_termination()
    s = dict(zip(SC7_NAMES, (float(v) for v in sc7)))
    with np.errstate(divide="ignore", invalid="ignore"):
        p = ((M.E * dy) if un else np.asarray(dy, dtype=np.float64)) * (1.0 / s["ndy"]) if M.m else np.zeros(0)
        d = ((M.D * dx) if un else np.asarray(dx, dtype=np.float64)) * (1.0 / s["ndx"])
    return p, d


# ---------------------------------------------------------------------------------------------------------------
# kernel cases: a scaled problem and the unscaled warm start (x0, y0) one ADMM iteration starts from
# ---------------------------------------------------------------------------------------------------------------
def planted(n, m, at, seed, scaled):
    """R.planted with, at index `at` (of the rows and of the columns), everything the one-workgroup reductions take a maximum of:
    row `at` has no lower bound and u = -1e6, so y moves by about +rho 1e6 there: the largest |E dy|;
    its entry in column `at` is 30 (no other entry of A exceeds 1.5), so |Dinv A'dy| is largest in column `at`;
    P[at, at] = 1e4 and x0 = -20 at column `at` (x~ is pulled to about 0 there, dx is about +32): the largest |Dinv P dx|;
    and (A dx) of row `at` is about 30 dx[at] > 0 against its finite u: the largest violation of a row.
    By turns the other rows have one, both and no infinite bounds, and the warm start y0 has both signs on every kind (so dy has
    both signs on every kind)."""
    sc = R.planted(n, m, at, seed, scaled)
    rng = np.random.RandomState(seed + 1000)
    l, u = sc["l"].copy(), sc["u"].copy()
    i = np.arange(m)
    j, r = at % n, at % m
    keep = i != r
    l[(i % 8 == 1) & keep], u[(i % 8 == 1) & keep] = -50.0, 1e30         # no upper bound
    l[(i % 8 == 5) & keep], u[(i % 8 == 5) & keep] = -1e30, 50.0         # no lower bound
    u[r] = -1e6
    P, A = sparse.lil_matrix(sc["P"]), sparse.lil_matrix(sc["A"])
    P[j, j] = 1e4
    A[r, j] = 30.0
    sc.update(l=l, u=u, P=sparse.triu(sparse.csc_matrix(P), format="csc"), A=sparse.csc_matrix(A))
    x0 = rng.randn(n)
    x0[j] = -20.0
    y0 = rng.randn(m)
    return sc, x0, y0


PLANTED = ("ndy", "viol", "nAtdy", "nPdx")          # the maxima whose place `planted` fixes (rows: at % m, columns: at % n)


def planted_at(where, n, m, at):
    return {k: where[k] for k in PLANTED} == dict(ndy=at % m, viol=at % m, nAtdy=at % n, nPdx=at % n)


def m0():
    sc = R.m0_case()
    return sc, np.random.RandomState(3).randn(sc["P"].shape[0]), np.zeros(0)


def still():
    """x0 = 0, y0 = 0, q = 0 and 0 inside every pair of bounds: nothing moves, |dx| = |dy| = 0 <= OSQP_DIVISION_TOL."""
    sc = R.zero_q_case()
    return sc, np.zeros(sc["P"].shape[0]), np.zeros(sc["A"].shape[0])


KERNEL_SETTINGS = dict(max_iter=1, check_termination=1, adaptive_rho=0, eps_abs=1e-12, eps_rel=1e-12)
EPS_SWEEP = (1e-4, 7.0, 1e6)          # the verdicts differ along it: nothing passes at 1e-4, the sums and norms pass one by one above (|A'dy| / |dy| of the
                                      # one-row dy is the planted entry, 30, or about 1 after Ruiz scaling: neither eps nor 10 eps sits on those)


# ---------------------------------------------------------------------------------------------------------------
# whole solves (tests/test_rowpart_infeasible.py, tests/test_gpu_rowpart_infeasible.py): unscaled problems dict(P, q, A, l, u)
# ---------------------------------------------------------------------------------------------------------------
def _base(seed=7, n=20, m=30):
    rng = np.random.RandomState(seed)
    A = sparse.lil_matrix((m, n))
    for i in range(m):
        A[i, i % n] = 1.0
        A[i, (3 * i + 1) % n] = 0.5
    return rng, n, m, sparse.csc_matrix(A)


def solve_problem(name):
    """-> (problem, settings).  primal: rows 0 and 1 say x0 >= 1 and x0 <= 0 and sit on rank 0 at two and at three ranks.  dual: no
    curvature along x0, x1, q pushes both down and no row through them has a lower bound.  dual_m0: P = 0, no rows.  *_inaccurate: the
    same at an iteration cap where only 10 x the tolerances pass.  feasible: the control."""
    inf = dict(eps_prim_inf=1e-4, eps_dual_inf=1e-4)
    if name.endswith("empty_rank"):
        # three singleton rows and one dense last row, as R.edge_problem("dense_last_row"): at two ranks shard_rows gives rank 1 NO rows, in
        # a problem with m_total > 0.  primal: rows 0 and 1 say x0 >= 1 and x0 <= 0.  dual: no curvature along x7, q pushes it down, and
        # the only row through it, the dense one, has no lower bound.
        rng, n = np.random.RandomState(31), 200
        cols = np.array([0, 0, 100]) if name.startswith("primal") else np.array([0, 50, 100])
        A = sparse.vstack([sparse.csc_matrix((np.ones(3), (np.arange(3), cols)), shape=(3, n)), sparse.csc_matrix(np.ones((1, n)))], format="csc")
        d, q = 1.0 + rng.rand(n), rng.randn(n)
        if name.startswith("primal"):
            l, u = np.array([1.0, -1e30, -0.1, 1.0]), np.array([1e30, 0.0, 0.1, 2.0])
        else:
            d[7], q[7] = 0.0, 1.0
            l, u = np.array([-0.1, -0.1, -0.1, -1e30]), np.array([0.1, 0.1, 0.1, 2.0])
        return dict(P=sparse.csc_matrix(sparse.diags(d)), q=q, A=A, l=l, u=u), dict(inf)
    rng, n, m, A2 = _base()
    P = sparse.csc_matrix(sparse.diags(1.0 + rng.rand(n)))
    if name.startswith("primal"):
        A = sparse.lil_matrix(A2)
        A[0, :] = 0; A[1, :] = 0; A[0, 0] = 1.0; A[1, 0] = 1.0
        l, u = -np.ones(m), np.ones(m)
        l[0], u[0], l[1], u[1], l[5], u[5] = 1.0, 1e30, -1e30, 0.0, -1e30, 1e30
        pb = dict(P=P, q=rng.randn(n), A=sparse.csc_matrix(A), l=l, u=u)
        return pb, dict(inf, **(PRIMAL_INACCURATE if name.endswith("inaccurate") else {}))
    if name.startswith("dual_m0"):
        return dict(P=sparse.csc_matrix((n, n)), q=rng.randn(n), A=sparse.csc_matrix((0, n)), l=np.zeros(0), u=np.zeros(0)), dict(inf)
    if name.startswith("dual"):
        d = 1.0 + rng.rand(n); d[0] = d[1] = 0.0
        q = rng.randn(n); q[0], q[1] = 1.0, 0.5
        l, u = -np.ones(m), np.ones(m)
        l[np.asarray((A2[:, [0, 1]] != 0).sum(axis=1)).ravel() > 0] = -1e30
        pb = dict(P=sparse.csc_matrix(sparse.diags(d)), q=q, A=A2, l=l, u=u)
        return pb, dict(inf, **(DUAL_INACCURATE if name.endswith("inaccurate") else {}))
    if name == "feasible":
        return dict(P=P, q=rng.randn(n), A=A2, l=-np.ones(m), u=np.ones(m)), dict(inf, eps_abs=1e-5, eps_rel=1e-5)
    raise KeyError(name)


PRIMAL_INACCURATE = dict(max_iter=27)      # the oracle answers `inaccurate` for every cap from 24 to 30, and from 15 to 18
DUAL_INACCURATE = dict(max_iter=16)
SOLVE_NAMES = ("primal", "dual", "dual_m0", "primal_inaccurate", "dual_inaccurate", "feasible", "primal_empty_rank", "dual_empty_rank")


def off(kw):
    return {k: v for k, v in kw.items() if k not in ("eps_prim_inf", "eps_dual_inf")}


def sequence():
    """infeasible -> update(l, u) to a feasible problem -> solve -> update(q) -> warm solve -> update_rho (a refused one first) -> solve -> warm_start -> solve; before the first update, bounds with
    l > u on the LAST row (one rank only) that must change nothing.  -> (problem, settings, list of (call, kwargs))."""
    pb, kw = solve_problem("primal")
    rng = np.random.RandomState(17)
    m, n = pb["A"].shape
    l2, u2 = pb["l"].copy(), pb["u"].copy()
    l2[0], u2[0] = -1.0, 1e30                      # x0 >= -1: feasible with x0 <= 0; row 0 stays an inequality
    u2[7] = l2[7] = 0.25                           # and one row becomes an equality: a class change, on one rank only
    lbad, ubad = l2.copy(), u2.copy()
    lbad[m - 1], ubad[m - 1] = 1.0, -1.0
    steps = [("solve", {}), ("update", dict(l=lbad, u=ubad)), ("update", dict(l=l2, u=u2)), ("solve", {}),
             ("update", dict(q=pb["q"] + 0.3 * rng.randn(n))), ("solve", {}), ("update_rho", dict(rho=-1.0)), ("update_rho", dict(rho=0.4)), ("solve", {}),
             ("warm_start", dict(x=0.1 * rng.randn(n), y=0.1 * rng.randn(m))), ("solve", {})]
    return pb, dict(kw, eps_abs=1e-5, eps_rel=1e-5), steps
