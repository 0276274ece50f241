"""Plain numpy reference of what the single-QP engine's scaling, residual, certificate and update kernels compute, and the
seeded cases they are tested on (tests/test_engine_reference.py on the CPU, tests/test_gpu_engine_kernels.py on the device).
Nothing here touches the library.  Sums are taken in np.longdouble (64-bit mantissa on x86) -- every float64 product is exact
there -- and every returned value comes with a bound on what float64 rounding may do to the device's value, U = 2**-52:

  max-norm fields   (L + 4) U S    L: longest contributing row, S: largest sum_j |a_ij| |v_j| + |other terms| over the rows
  summed fields     (N + L + 4) U sum|terms|    N: number of summed terms
  Ruiz outputs      R U relative, R = float64 roundings on the quantity's path through the kernels (ruiz_roundings)
"""
import numpy as np
import scipy.linalg as sla
from scipy import sparse
from scipy.sparse import linalg as spla

LD = np.longdouble
U = 2.0 ** -52
INF_BOUND = 1e26          # a scaled bound beyond it counts as infinite (strict comparison)
MIN_SCALING, MAX_SCALING = 1e-4, 1e4


def _clip(v):
    v = np.array(v, dtype=LD)
    v = np.where(v < LD(MIN_SCALING), LD(1.0), v)
    return np.where(v > LD(MAX_SCALING), LD(MAX_SCALING), v)


def _margin(v, skip_exact):
    """Smallest relative distance of the values from the two clip thresholds (exact hits left out where the values are inputs)."""
    v = np.atleast_1d(np.array(v, dtype=LD))
    out = np.inf
    for t in (MIN_SCALING, MAX_SCALING):
        d = np.abs(v / LD(t) - 1)
        if skip_exact:
            d = d[v != LD(t)]
        if d.size:
            out = min(out, float(d.min()))
    return out


def _coo(M):
    M = sparse.csc_matrix(M)
    M.sort_indices()
    col = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    return M.indices.astype(np.int64), col, M.data


def ruiz(Pu, A, q, l, u, passes):
    """`passes` sweeps of Ruiz equilibration with cost normalisation on (triu(P), A, q, l, u), as the solver's set-up defines it:
    per sweep  d = 1/sqrt(clip(column norms of [P; A])), e = 1/sqrt(clip(row norms of A)), P <- dPd, A <- eAd, q <- dq, D <- dD, E <- eE,
    then c_t = 1/clip(max(mean column norm of P, clip(|q|_inf))), P <- c_t P, q <- c_t q, c <- c_t c; at the end l <- E l, u <- E u.
    clip(v): v < 1e-4 -> 1, v > 1e4 -> 1e4.  Returns a dict of D, E, c, q, l, u, Px, Ax (CSC order) in long double, `margin` (the
    smallest relative distance of a clipped quantity from a threshold; first-sweep matrix norms that sit exactly on one are inputs
    and left out, and so is a c_t that is the clipped |q|_inf itself) `R`, the rounding counts of ruiz_roundings for a serial mean, and `R_device`, those for the device's reduction."""
    n, m = Pu.shape[0], A.shape[0]
    pr, pc, px = _coo(Pu)
    ar, ac, ax = _coo(A)
    px, ax = px.astype(LD), ax.astype(LD)
    q = np.asarray(q, dtype=LD).copy()
    D, E, c = np.ones(n, dtype=LD), np.ones(m, dtype=LD), LD(1.0)
    margin = np.inf

    def p_norms():
        v = np.zeros(n, dtype=LD)
        np.maximum.at(v, pc, np.abs(px))
        np.maximum.at(v, pr, np.abs(px))
        return v

    for p in range(passes):
        dn, en = p_norms(), np.zeros(m, dtype=LD)
        np.maximum.at(dn, ac, np.abs(ax))
        np.maximum.at(en, ar, np.abs(ax))
        margin = min(margin, _margin(dn, p == 0), _margin(en, p == 0))
        dn, en = 1 / np.sqrt(_clip(dn)), 1 / np.sqrt(_clip(en))
        px = px * dn[pr] * dn[pc]
        ax = ax * en[ar] * dn[ac]
        q = q * dn
        D, E = D * dn, E * en
        mean = p_norms().sum() / LD(n)
        qn = np.abs(q).max()
        ct = np.maximum(mean, _clip(qn))
        margin = min(margin, _margin(qn, False), _margin(ct, False) if mean > _clip(qn) else np.inf)
        ct = 1 / _clip(ct)
        px, q, c = px * ct, q * ct, c * ct
    return dict(D=D, E=E, c=c, q=q, l=np.asarray(l, dtype=LD) * E, u=np.asarray(u, dtype=LD) * E, Px=px, Ax=ax, margin=margin,
                R=ruiz_roundings(n, passes), R_device=ruiz_roundings(n, passes, device_sum_adds(n)))


def ruiz_roundings(n, passes, sum_adds=None):
    """float64 roundings on the path of each output through k_ruiz_norms / k_ruiz_apply / k_ruiz_cost_* / k_ruiz_finish, in units
    of U.  Each sweep's norms are maxima of stored entries -- exact selections -- and are taken as that sweep's inputs.  `sum_adds`
    is the number of additions on the path of any one term of the mean column norm: n - 1 for a serial sum (the default), the
    depth of the reduction for the device (device_sum_adds).  Per sweep, with s = sum_adds:
      d, e factors   sqrt + reciprocal = 2
      D, E           factor (2) + accumulating product = 3
      A entry        two products + two factors = 6
      c_t            s additions of the mean + division + reciprocal = s + 2
      P entry        two products + two factors + c_t + its product = s + 9
      q              factor + product + c_t + its product = s + 6
      c              c_t + accumulating product = s + 3
    and at the end l, u: E + 1.  No sweep: everything is returned as it was given (0)."""
    p, s = passes, (n - 1 if sum_adds is None else sum_adds)
    return dict(D=3 * p, E=3 * p, c=(s + 3) * p, q=(s + 6) * p, l=3 * p + (1 if p else 0), u=3 * p + (1 if p else 0), Px=(s + 9) * p, Ax=6 * p)


def device_sum_adds(n):
    """Additions on one term's path through k_ruiz_cost_norms / k_ruiz_cost_scalar: a grid of g = min(1024, ceil(n / 4)) workgroups
    of four wavefronts, one column per wavefront and turn (ceil(n / 4g) serial additions), the workgroup's tree (6 shuffle levels
    + 2), then one workgroup over the g partials (ceil(g / 256) serial additions + the same tree)."""
    g = max(1, min(1024, (n + 3) // 4))
    return -(-n // (4 * g)) + 8 + -(-g // 256) + 8


# ---------------------------------------------------------------------------------------------------------------
# residual and certificate scalars
# ---------------------------------------------------------------------------------------------------------------
class Problem:
    """(triu(P), A, q, l, u) with the long-double operators the references below share; D, E (None: no scaling)."""

    def __init__(self, Pu, A, q, l, u, D=None, E=None):
        Pu, A = sparse.csc_matrix(Pu), sparse.csc_matrix(A)
        self.n, self.m = Pu.shape[0], A.shape[0]
        self.Pu = Pu
        P = (Pu + sparse.triu(Pu, 1, format="csc").T).tocsr()
        self.P, self.A = P.astype(LD), sparse.csr_matrix(A).astype(LD)
        self.AT = self.A.T.tocsr()
        self.Pa, self.Aa, self.ATa = abs(self.P), abs(self.A), abs(self.AT)
        self.q, self.l, self.u = (np.asarray(v, dtype=LD) for v in (q, l, u))
        self.scaled = D is not None
        self.D = np.ones(self.n, dtype=LD) if D is None else np.asarray(D, dtype=LD)
        self.E = np.ones(self.m, dtype=LD) if E is None else np.asarray(E, dtype=LD)
        self.Dinv, self.Einv = 1 / self.D, 1 / self.E
        lenA = np.diff(self.A.indptr)
        self.LA = int(lenA.max()) if self.m and lenA.size else 0
        self.LM = int((np.diff(P.indptr) + np.diff(self.AT.indptr)).max())
        self.inf_u, self.inf_l = self.u > INF_BOUND, self.l < -INF_BOUND

    def project_dy(self, dy):
        """delta_y on the polar of the recession cone of [l, u]: 0 on a free row, min(dy, 0) where only u is infinite, max(dy, 0)
        where only l is."""
        dy = np.asarray(dy, dtype=float)
        out = dy.copy()
        both, up, lo = self.inf_u & self.inf_l, self.inf_u & ~self.inf_l, ~self.inf_u & self.inf_l
        out[both] = 0.0
        out[up] = np.minimum(dy[up], 0.0)
        out[lo] = np.maximum(dy[lo], 0.0)
        return out


def _mx(v):
    return float(np.abs(v).max()) if np.size(v) else 0.0


def residual_scalars(pb, x, y, z, dx, dy):
    """Every field that one residual evaluation fills, from the iterates given: (values, bars, projected delta_y)."""
    x, y, z, dx = (np.asarray(v, dtype=LD) for v in (x, y, z, dx))
    n, m = pb.n, pb.m
    val, bar = {}, {}

    def mxf(name, v, S, L, scale):
        """max-norm field pair name_s / name_u: v the vector, S its rows' absolute sums, scale the unscaling vector"""
        val[name + "_s"], bar[name + "_s"] = _mx(v), (L + 4) * U * _mx(S)
        val[name + "_u"], bar[name + "_u"] = _mx(scale * v), (L + 4) * U * _mx(scale * S)

    ax, axa = pb.A @ x, pb.Aa @ np.abs(x)
    if m == 0:
        ax, axa = np.zeros(0, dtype=LD), np.zeros(0, dtype=LD)
    mxf("pri_res", ax - z, axa + np.abs(z), pb.LA, pb.Einv)
    mxf("z", z, np.abs(z), 0, pb.Einv)
    mxf("Ax", ax, axa, pb.LA, pb.Einv)
    px, pxa = pb.P @ x, pb.Pa @ np.abs(x)
    aty, atya = (pb.AT @ y, pb.ATa @ np.abs(y)) if m else (np.zeros(n, dtype=LD), np.zeros(n, dtype=LD))
    mxf("dua_res", pb.q + px + aty, np.abs(pb.q) + pxa + atya, pb.LM, pb.Dinv)
    mxf("q", pb.q, np.abs(pb.q), 0, pb.Dinv)
    mxf("Aty", aty, atya, pb.LM, pb.Dinv)
    mxf("Px", px, pxa, pb.LM, pb.Dinv)
    terms, ta = x * (LD(0.5) * px + pb.q), np.abs(x) * (LD(0.5) * pxa + np.abs(pb.q))
    val["obj_scaled"], bar["obj_scaled"] = float(terms.sum()), (n + pb.LM + 4) * U * float(ta.sum())
    dyp = pb.project_dy(dy)
    dl = dyp.astype(LD)
    mxf("dy_norm", dl, np.abs(dl), 0, pb.E)
    # u' max(dy, 0) + l' min(dy, 0): an infinite bound meets a zero there
    t = pb.u * np.maximum(dl, 0) + pb.l * np.minimum(dl, 0)
    val["dy_lhs"], bar["dy_lhs"] = float(t.sum()), (m + 4) * U * float(np.abs(pb.u * np.maximum(dl, 0)).sum() + np.abs(pb.l * np.minimum(dl, 0)).sum())
    mxf("dx_norm", dx, np.abs(dx), 0, pb.D)
    val["q_dx"], bar["q_dx"] = float((pb.q * dx).sum()), (n + 4) * U * float(np.abs(pb.q * dx).sum())
    return val, bar, dyp


def certificate_scalars(pb, dx, dyp, eps_dx, unscaled):
    """Second stage of the infeasibility tests: ||A' dy_proj||, ||P dx|| (max norms; the _u pair divided by D when `unscaled` and
    the problem is scaled, equal to the _s pair otherwise), the number of rows with a finite u and (A dx)_i > eps_dx or a finite l
    and (A dx)_i < -eps_dx ((A dx)_i divided by E_i under the same condition), and `gap`: the smallest
    (| |A dx|_i - eps_dx | - that row's rounding bound) over the rows with a finite bound (> 0: every row's side is decided)."""
    dx, dl = np.asarray(dx, dtype=LD), np.asarray(dyp, dtype=LD)
    sc = bool(unscaled) and pb.scaled
    di = pb.Dinv if sc else np.ones(pb.n, dtype=LD)
    ei = pb.Einv if sc else np.ones(pb.m, dtype=LD)
    val, bar = {}, {}
    atdy, atdya = (pb.AT @ dl, pb.ATa @ np.abs(dl)) if pb.m else (np.zeros(pb.n, dtype=LD), np.zeros(pb.n, dtype=LD))
    pdx, pdxa = pb.P @ dx, pb.Pa @ np.abs(dx)
    for name, v, S in (("Atdy", atdy, atdya), ("Pdx", pdx, pdxa)):
        val[name + "_s"], bar[name + "_s"] = _mx(v), (pb.LM + 4) * U * _mx(S)
        val[name + "_u"], bar[name + "_u"] = _mx(di * v), (pb.LM + 4) * U * _mx(di * S)
    if pb.m == 0:
        return val, bar, 0, np.inf
    adx, adxa = ei * (pb.A @ dx), ei * (pb.Aa @ np.abs(dx))
    eps = LD(eps_dx)
    fin_u, fin_l = pb.u < INF_BOUND, pb.l > -INF_BOUND
    count = int(((fin_u & (adx > eps)) | (fin_l & (adx < -eps))).sum())
    rowbar = (np.diff(pb.A.indptr) + 4) * U * adxa
    near = np.where(fin_u, np.abs(adx - eps), np.inf)
    near = np.minimum(near, np.where(fin_l, np.abs(adx + eps), np.inf))
    gap = float((near - rowbar).min())
    return val, bar, count, gap


# ---------------------------------------------------------------------------------------------------------------
# one ADMM step
# ---------------------------------------------------------------------------------------------------------------
class _SparseKKT:
    """x~ of K x~ = r for the large cases: sparse LU of the quasi-definite [[P + sigma I, A'], [A, -1/rho]] in float64."""

    def __init__(self, pb, sigma, rho):
        n, m = pb.n, pb.m
        P = pb.P.astype(float)
        self.n = n
        kkt = sparse.bmat([[P + sigma * sparse.eye(n), pb.A.astype(float).T], [pb.A.astype(float), -sparse.diags(1.0 / rho)]], format="csc")
        self.lu = spla.splu(kkt)
        self.pad = np.zeros(m)

    def solve(self, r):
        return self.lu.solve(np.concatenate([np.asarray(r, dtype=float), self.pad]))[: self.n]

    def lam_min(self):
        op = spla.LinearOperator((self.n, self.n), matvec=self.solve, dtype=float)
        w = spla.eigsh(op, k=1, which="LA", tol=1e-6, return_eigenvectors=False)     # largest of K^-1
        return 1.0 / float(w[0])


class _DenseKKT:
    def __init__(self, pb, sigma, rho):
        A = pb.A.astype(float)
        self.K = (pb.P.astype(float) + sigma * sparse.eye(pb.n) + (A.T @ sparse.diags(rho) @ A if pb.m else 0)).toarray()
        self.lu = sla.lu_factor(self.K, check_finite=False)

    def solve(self, r):
        return sla.lu_solve(self.lu, np.asarray(r, dtype=float), check_finite=False)

    def lam_min(self):
        return float(np.linalg.eigvalsh(self.K)[0])


DENSE_MAX = 3000


def admm_step(pb, sigma, alpha, rho, x, z, y, reuse=None):
    """One ADMM iteration from (x, z, y):  K x~ = sigma x - q + A'(rho z - y), K = P + sigma I + A' rho A (a float64 LU solve --
    dense up to DENSE_MAX variables, sparse above -- with one refinement step whose residual is formed in long double),
    `reuse`: a dict the caller keeps while pb's matrices, rho and sigma are unchanged; the factorisation and lam_min are stored in
    it by the first call and taken from it by the later ones (the same objects: the results do not change).
    z~ = A x~;  x+ = alpha x~ + (1 - alpha) x;  z+ = clip(alpha z~ + (1 - alpha) z + y / rho, l, u);
    y+ = y + rho (alpha z~ + (1 - alpha) z - z+).  Returns a dict of the long-double x_tilde, x, z, y, dx, dy, v (the unclipped z+),
    lam_min of K, norm_b (2-norm of the right-hand side), plain_err (2-norm error of the unrefined float64 solve) and the rounding
    parts of the bars: rnd_x, rnd_z, rnd_y (what the update formulas themselves may round, per element) and a1 (||A_i||_1)."""
    n, m = pb.n, pb.m
    x, z, y = (np.asarray(v, dtype=LD) for v in (x, z, y))
    rho = np.asarray(rho, dtype=float)
    rl, sg, al = rho.astype(LD), LD(sigma), LD(alpha)
    if reuse is not None and "kkt" in reuse:
        kkt, lam_min = reuse["kkt"], reuse["lam_min"]
    else:
        kkt = (_DenseKKT if n <= DENSE_MAX else _SparseKKT)(pb, float(sigma), rho)
        lam_min = kkt.lam_min()
        if reuse is not None:
            reuse["kkt"], reuse["lam_min"] = kkt, lam_min

    def K(v):
        out = pb.P @ v + sg * v
        return out + pb.AT @ (rl * (pb.A @ v)) if m else out

    b = sg * x - pb.q
    if m:
        b = b + pb.AT @ (rl * z - y)
    plain = kkt.solve(b.astype(float)).astype(LD)
    xt = plain + kkt.solve((b - K(plain)).astype(float)).astype(LD)
    zt = pb.A @ xt if m else np.zeros(0, dtype=LD)
    zta = pb.Aa @ np.abs(xt) if m else np.zeros(0, dtype=LD)
    xn = al * xt + (1 - al) * x
    w = al * zt + (1 - al) * z
    v = w + y / rl
    zn = np.minimum(np.maximum(v, pb.l), pb.u)
    dy = rl * (w - zn)
    rowlen = np.diff(pb.A.indptr) if m else np.zeros(0)
    rnd_z = U * ((rowlen + 4) * np.abs(al) * zta + 4 * (np.abs((1 - al) * z) + np.abs(y / rl)))
    return dict(x_tilde=xt, x=xn, z=zn, y=y + dy, dx=xn - x, dy=dy, v=v, lam_min=lam_min,
                norm_b=float(np.sqrt((b * b).sum())), plain_err=float(np.sqrt(((plain - xt) ** 2).sum())),
                norm_xt=float(np.sqrt((xt * xt).sum())),
                rnd_x=4 * U * (np.abs(al * xt) + np.abs((1 - al) * x)), rnd_z=rnd_z,
                rnd_y=rl * rnd_z + 4 * U * (np.abs(y) + rl * (np.abs(w) + np.abs(zn))),
                a1=np.asarray(pb.Aa.sum(axis=1)).ravel() if m else np.zeros(0, dtype=LD))


def step_bars(st, alpha, rho, direct, pcg_eps_rel):
    """Bars of x+, z+, y+ per element from the bar on ||x~_dev - x~||_2:
         PCG forms     pcg_eps_rel ||b||_2 / lam_min(K) + 50 U ||x~||_2      (||K^-1 r|| <= ||r|| / lam_min at the stop ||r|| <= eps ||b||)
         direct forms  10 x the 2-norm error of the unrefined float64 LU solve of the same system + 50 U ||x~||_2
       times alpha for x, alpha ||A_i||_1 for z, rho_i times that for y, each plus the rounding of its own update formula."""
    assert st["lam_min"] > 0.0, st["lam_min"]
    bxt = (10.0 * st["plain_err"] if direct else pcg_eps_rel * st["norm_b"] / st["lam_min"]) + 50 * U * st["norm_xt"]
    bz = abs(alpha) * st["a1"].astype(float) * bxt + st["rnd_z"].astype(float)
    return dict(x_tilde=bxt, x=abs(alpha) * bxt + st["rnd_x"].astype(float), z=bz,
                y=np.asarray(rho, float) * abs(alpha) * st["a1"].astype(float) * bxt + st["rnd_y"].astype(float))


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
RHO = 0.1
SIGMA = 1e-6
CASES = ("tiny1", "tiny3", "m0", "offtile", "empty", "long", "huge", "scales", "scales_p0", "bounds")
SMALL = ("tiny1", "tiny3", "m0", "offtile", "scales", "scales_p0", "bounds")     # run on the launch-per-step kernels and with the defaults
SEEDS = dict(tiny1=1, tiny3=2, m0=3, offtile=4, empty=5, long=6, huge=7, scales=8, scales_p0=9, bounds=10)
INF = 1e30


def _tridiag(n, rng, skip=()):
    """triu of an SPD tridiagonal P (diagonal 2..3, off-diagonal -0.5: every variable coupled, eigenvalues >= 1) without the
    rows and columns of `skip`."""
    keep = np.ones(n, bool)
    keep[list(skip)] = False
    d = np.where(keep, rng.uniform(2.0, 3.0, n), 0.0)
    o = np.where(keep[:-1] & keep[1:], -0.5, 0.0) if n > 1 else np.zeros(0)
    P = sparse.diags([d, o], [0, 1], shape=(n, n), format="csc")
    P.eliminate_zeros()
    return P


def _rows_to_csc(rows, m, n):
    if not rows:
        return sparse.csc_matrix((m, n))
    ri = np.concatenate([np.full(len(c), i) for i, c, _ in rows])
    ci = np.concatenate([np.asarray(c) for _, c, _ in rows])
    vi = np.concatenate([np.asarray(v, float) for _, _, v in rows])
    return sparse.csc_matrix((vi, (ri, ci)), shape=(m, n))


def _short_rows(rng, rows_idx, n, lo=2, hi=6, cols=None):
    out = []
    pool = np.arange(n) if cols is None else np.asarray(cols)
    for i in rows_idx:
        k = min(int(rng.integers(lo, hi + 1)), pool.size)
        out.append((i, rng.choice(pool, k, replace=False), rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)))
    return out


def _peaked_row(i, cols, rng, offset, peak):
    """Row i over `cols` with entries of about 1 / sqrt(length) and +-peak at in-row offset `offset` (columns ascending)."""
    cols = np.sort(np.asarray(cols))
    v = np.clip(rng.standard_normal(cols.size), -3.0, 3.0) / np.sqrt(cols.size)
    v[offset] = peak * rng.choice([-1.0, 1.0])
    return (i, cols, v)


def peak_offset(case, which, row):
    """In-row offset of the largest |entry| of a row as the device stores it: which = "A": row of A; "P": the P part of row `row`
    of M = [P | A']; "M": the whole row of M."""
    A = sparse.csr_matrix(case["A"]); A.sort_indices()
    if which == "A":
        return int(np.abs(A[row].data).argmax())
    Pu = sparse.csc_matrix(case["Pu"])
    P = (Pu + sparse.triu(Pu, 1).T).tocsr(); P.sort_indices()
    AT = sparse.csr_matrix(A.T); AT.sort_indices()
    v = np.abs(P[row].data) if which == "P" else np.concatenate([np.abs(P[row].data), np.abs(AT[row].data)])
    return int(v.argmax())


def make_case(name):
    """dict(Pu, A, q, l, u, rho, special_rows, special_cols): the raw problem of one case of the table in
    tests/test_gpu_engine_kernels.py, from its seed in SEEDS."""
    rng = np.random.default_rng(SEEDS[name])
    special_rows, special_cols, peaks = [], [], []
    if name == "tiny1":
        n, m = 1, 1
        Pu, rows = sparse.csc_matrix([[2.0]]), [(0, [0], [1.5])]
    elif name == "tiny3":
        n, m = 3, 2
        Pu, rows = _tridiag(3, rng), [(0, [0, 2], [1.0, -2.0]), (1, [1, 2], [0.5, 1.0])]
    elif name == "m0":
        n, m = 20, 0
        Pu, rows = _tridiag(n, rng), []
    elif name == "offtile":
        n, m = 257, 300
        Pu, rows = _tridiag(n, rng), _short_rows(rng, range(m), n)
    elif name == "empty":
        n, m = 300, 2100
        dead = [3, 77, 150, 151, 299]                              # no entry in P or A
        live = np.setdiff1d(np.arange(n), dead)
        Pu = _tridiag(n, rng, skip=dead)
        rows = _short_rows(rng, list(range(0, 10)) + list(range(2071, m)), n, cols=live)     # rows 10..2070 empty
        special_cols, special_rows = dead, [9, 10, 2070, 2071]
    elif name == "long":
        n, m = 600, 40
        P = sparse.lil_matrix(_tridiag(n, rng))
        P[0, 2:n] = 0.01 * rng.choice([-1.0, 1.0], n - 2)          # one dense row of P: 600 entries of M in row 0
        P[0, 0] = 10.0
        Pu = sparse.csc_matrix(P)
        rows = _short_rows(rng, range(3, m), n)
        # the largest entry of each long row at a chosen offset in the row (columns ascending, as the device stores it): lane 63 of a
        # wavefront's first turn, lane 0 of its last turn, and the last element of a row whose length is no multiple of 64
        for i, k, off in ((0, 512, 63), (1, 513, 512), (2, 511, 510)):
            rows.append(_peaked_row(i, np.concatenate([[0], 1 + rng.choice(n - 1, k - 1, replace=False)]), rng, off, 3.0))
        # column 0 has an entry in every row of A: row 0 of M = 600 entries of P, then 40 of A'; the largest of them, A[39, 0],
        # sits at offset 639 = 9 x 64 + 63.  The largest of the P part is P[0, 63] (offset 63; P[63, 63] = 40 keeps P definite).
        rows = [(i, np.concatenate([[0], cc[cc != 0]]), np.concatenate([[v[cc == 0][0] if (cc == 0).any() else 0.3], v[cc != 0]]))
                for i, cc, v in ((i, np.asarray(cc), np.asarray(v, float)) for i, cc, v in rows)]
        rows = [(i, cc, np.where((cc == 0) & (i == 39), 50.0, v)) for i, cc, v in rows]
        P = sparse.lil_matrix(Pu)
        P[0, 0], P[0, 63], P[63, 63] = 4.0, 6.0, 40.0
        Pu = sparse.csc_matrix(P)
        special_rows, special_cols = [0, 1, 2, 39], [0, 63]
        peaks = [("A", 0, 63), ("A", 1, 512), ("A", 2, 510), ("M", 0, 639), ("P", 0, 63)]
    elif name == "huge":
        n, m = 8200, 12
        Pu = _tridiag(n, rng)
        rows = _short_rows(rng, range(2, m), n)
        for i, k, off in ((0, 8192, 63), (1, 8191, 8190)):
            rows.append(_peaked_row(i, rng.choice(n, k, replace=False), rng, off, 1.0))
        special_rows = [0, 1]
        peaks = [("A", 0, 63), ("A", 1, 8190)]
    elif name in ("scales", "scales_p0"):
        n, m = 40, 60
        Pu = _tridiag(n, rng) if name == "scales" else sparse.csc_matrix((n, n))
        # columns 0..9 of A empty apart from the rows below; the other rows live on columns 10..39 with entries in [0.5, 2]
        rows = _short_rows(rng, range(8, m), n, cols=np.arange(10, n))
        for i, (col, v) in enumerate(((0, 1e-6), (1, 1e-4), (2, 1e4), (3, 1e7), (4, 0.5e-4), (5, 2e4))):
            rows.append((i, [col], [v]))                            # a row and a column whose norm is exactly v
        rows += [(6, [6, 12], [1e-6, 1.0]), (7, [7, 13], [1e7, 1.0])]
        if name == "scales":                                        # columns 0..7 couple through P: lift their P entries out of the way
            Pu = sparse.lil_matrix(Pu)
            Pu[:8, :] = 0.0
            Pu = sparse.csc_matrix(Pu)
            Pu.eliminate_zeros()
        special_rows, special_cols = list(range(8)), list(range(8))
    elif name == "bounds":
        n, m = 40, 60
        Pu, rows = _tridiag(n, rng), _short_rows(rng, range(2, m), n)
        # rows 0, 1: empty (v = (1 - alpha) z + y / rho lands exactly on a bound from z = y = 0); row 5: norm 1e4, so that its E of
        # the first sweep is 1e-2
        rows[3] = (5, rows[3][1], rows[3][2] * 1e4 / np.abs(rows[3][2]).max())
        special_rows = [0, 1, 5]
    else:
        raise KeyError(name)
    A = _rows_to_csc(rows, m, n)
    A.sort_indices()
    q = rng.standard_normal(n)
    l, u = -rng.uniform(0.1, 1.0, m), rng.uniform(0.1, 1.0, m)
    if name == "scales":
        q[5] = 1e7
    if name == "scales_p0":
        q = q * 1e-6 / np.abs(q).max()
    if name == "bounds":
        kind = np.arange(m) % 6                # 0 both finite, 1 l only, 2 u only, 3 free, 4 equality, 5 large finite
        l[(kind == 2) | (kind == 3)] = -INF
        u[(kind == 1) | (kind == 3)] = INF
        eq = kind == 4
        u[eq] = l[eq]
        big = np.flatnonzero(kind == 5)[1:]                      # (row 5 is the 1e27 row below)
        l[big[0]], u[big[0]] = -1e25, 1e25
        l[big[1]], u[big[1]] = -1e26, 1e26                       # exactly on INF_BOUND: finite (strict comparison)
        l[big[2]], u[big[2]] = -1e26, INF
        l[big[3]], u[big[3]] = -INF, 1e26
        l[5], u[5] = -1e27, 1e27                                 # infinite as given; E = 1e-2 makes it 1e25
        l[0], u[0] = 0.0, 1.0
        l[1], u[1] = -1.0, 0.0
    elif m >= 6:
        l[m // 3], u[m // 2] = -INF, INF
        u[m - 1] = l[m - 1]
    rho = np.full(m, RHO)
    rho[l == u] = 1e3 * RHO
    rho[rng.random(m) < 0.25] = 1e3 * RHO
    return dict(name=name, n=n, m=m, Pu=sparse.csc_matrix(sparse.triu(Pu, format="csc")), A=A, q=q, l=l, u=u, rho=rho,
                special_rows=special_rows, special_cols=special_cols, peaks=peaks)


def iterates(case, salt=0):
    """Seeded x, y and an independent z for a case; a fifth of y is exactly zero (delta_y = 0 on a row that is not clamped)."""
    rng = np.random.default_rng(1000 + 17 * SEEDS[case["name"]] + salt)
    n, m = case["n"], case["m"]
    x, y, z = rng.standard_normal(n), rng.standard_normal(m) * 0.05, rng.standard_normal(m)
    y[rng.random(m) < 0.2] = 0.0
    if case["name"] == "bounds":
        y[:2], z[:2] = 0.0, 0.0
    return x, y, z


def sample(case, count=32):
    """Columns and rows whose device copies are read out: all of them up to 64, else a seeded sample with the special ones."""
    rng = np.random.default_rng(77 + SEEDS[case["name"]])
    out = []
    for size, special in ((case["n"], case["special_cols"]), (case["m"], case["special_rows"])):
        if size <= 64:
            out.append(np.arange(size))
        else:
            out.append(np.unique(np.concatenate([np.asarray(special, int), rng.choice(size, count - len(special), replace=False)])))
    return out


def eps_pair(pb, dx, unscaled):
    """Two thresholds for the A dx test, one just above and one just below the median |A dx|_i of the rows with a finite bound:
    the geometric means of that row's |A dx| and its neighbours' in sorted order (twice and half the value where it has none)."""
    sc = bool(unscaled) and pb.scaled
    adx = np.abs((pb.Einv if sc else 1) * (pb.A @ np.asarray(dx, dtype=LD))).astype(float)
    s = np.sort(adx[np.asarray((pb.u < INF_BOUND) | (pb.l > -INF_BOUND))])
    s = s[s > 0]
    k = s.size // 2
    above = np.sqrt(s[k] * s[k + 1]) if k + 1 < s.size else 2.0 * s[k]
    below = np.sqrt(s[k] * s[k - 1]) if k >= 1 else 0.5 * s[k]
    return float(above), float(below)


def scaled_problem(case, passes):
    """The case after `passes` Ruiz sweeps of the reference, as a Problem (float64 copies of the long-double data), and the
    ruiz() dict."""
    r = ruiz(case["Pu"], case["A"], case["q"], case["l"], case["u"], passes)
    Pu, A = case["Pu"].copy(), case["A"].copy()
    Pu.data, A.data = r["Px"].astype(float), r["Ax"].astype(float)
    f = lambda k: r[k].astype(float)
    pb = Problem(Pu, A, f("q"), f("l"), f("u"), f("D") if passes else None, f("E") if passes else None)
    return pb, r


def bound_margin(lu):
    """Smallest relative distance of a scaled bound from +-INF_BOUND (a bound exactly on it is an input and left out)."""
    a = np.abs(np.asarray(lu, dtype=LD))
    a = a[a != LD(INF_BOUND)]
    return float(np.abs(a / LD(INF_BOUND) - 1).min()) if a.size else np.inf
