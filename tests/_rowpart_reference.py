"""Plain numpy model of what include/osqp_amd_rowpart.h promises for one rank -- rho per row, the Jacobi inverse, the right-hand
side, K = P + sigma I + A' rho A, update_x / update_z / update_y, the fifteen check scalars, the info fields and both termination
tests -- and the seeded cases the row-partitioned kernels are tested on (tests/test_rowpart_reference.py on the CPU,
tests/test_gpu_rowpart_kernels.py on the device).  Nothing here touches the library.  It is fed with the *scaled* problem
dict(P (triu), q, A, l, u, D, E, c) directly, so that bounds can sit exactly on the thresholds of the code.

Values are np.longdouble (64-bit mantissa on x86: every product of two float64 is exact there); each comes with a bound on what
float64 rounding may do to the device's value, U = 2**-52:

  sums, dot products   (N + 6) U sum|terms|      N: number of summed terms -- any order of summation, fused or not; the 6 covers the
                                                 roundings inside a term (rho a a: 2) and the few terms added outside the sum
  element-wise         4 U sum|terms|            update_x, the argument of the projection
  maxima of products   the largest element bound: a maximum moves by no more than its arguments do
  rho per row          exact: a selection between 1e-6, rho and the one float64 product 1e3 rho
"""
import numpy as np
from scipy import sparse

LD = np.longdouble
U = 2.0 ** -52
RHO_MIN, RHO_MAX, RHO_TOL, RHO_EQ = 1e-6, 1e6, 1e-4, 1e3
INF_BOUND = 1e26
DIV_TOL = 1e-30
SC_NAMES = ("pri_u", "z_u", "Ax_u", "pri_s", "z_s", "Ax_s", "dua_u", "dua_s", "q_u", "q_s", "Aty_u", "Aty_s", "Px_u", "Px_s", "obj")
DEFAULTS = dict(rho=0.1, sigma=1e-6, alpha=1.6, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000, check_termination=25,
                adaptive_rho=1, adaptive_rho_interval=0, adaptive_rho_tolerance=5.0, scaled_termination=0,
                pcg_eps_rel=1e-9, pcg_max_iter=0)


def clip_rho(rho):
    return min(max(float(rho), RHO_MIN), RHO_MAX)


def row_class(l, u):
    """-1 free, 1 equality, 0 inequality; float64 arithmetic and strict comparisons, as set_rho_vec."""
    l, u = np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64)
    free = (l < -INF_BOUND) & (u > INF_BOUND)
    with np.errstate(invalid="ignore", over="ignore"):
        eq = ~free & ((u - l) < RHO_TOL)
    return np.where(free, -1, np.where(eq, 1, 0))


def rho_vec(l, u, rho):
    """rho per row, bit for bit (rho: the setting; it is clipped to [1e-6, 1e6] first)."""
    rho = np.float64(clip_rho(rho))
    c = row_class(l, u)
    return np.where(c == -1, np.float64(RHO_MIN), np.where(c == 1, np.float64(RHO_EQ) * rho, rho))


def eps_pcg(st, has_eq):
    e = min(st["eps_abs"] or st["eps_rel"], st["eps_rel"] or st["eps_abs"])
    v = max(1e-13, min(st["pcg_eps_rel"], 1e-5 * e))
    return max(1e-13, 1e-3 * v) if has_eq else v


def _mv(r, c, a, v, nout):
    """out[r] += a v[c] in long double, and the same with absolute values."""
    val, ab = np.zeros(nout, dtype=LD), np.zeros(nout, dtype=LD)
    t = a * v[c]
    np.add.at(val, r, t)
    np.add.at(ab, r, np.abs(t))
    return val, ab


class Model:
    def __init__(self, scaled, **settings):
        st = dict(DEFAULTS)
        for k, v in settings.items():
            if k not in st:
                raise ValueError(k)
            st[k] = v
        self.st = st
        Pu, A = sparse.coo_matrix(sparse.triu(sparse.csc_matrix(scaled["P"]))), sparse.coo_matrix(scaled["A"])
        self.n, self.m = n, m = Pu.shape[0], A.shape[0]
        off = Pu.row != Pu.col
        self.pr = np.concatenate([Pu.row, Pu.col[off]]).astype(np.int64)
        self.pc = np.concatenate([Pu.col, Pu.row[off]]).astype(np.int64)
        self.pv = np.concatenate([Pu.data, Pu.data[off]]).astype(LD)
        self.ar, self.ac, self.av = A.row.astype(np.int64), A.col.astype(np.int64), A.data.astype(LD)
        self.q, self.l, self.u = (np.asarray(scaled[k], dtype=np.float64) for k in "qlu")
        self.D, self.E, self.c = np.asarray(scaled["D"], dtype=np.float64), np.asarray(scaled["E"], dtype=np.float64), float(scaled["c"])
        self.Dinv, self.Einv = 1.0 / self.D, 1.0 / self.E            # float64 reciprocals: the handle stores exactly these
        self.scaled_data = bool(np.any(self.D != 1.0) or np.any(self.E != 1.0) or self.c != 1.0)
        self.cls = row_class(self.l, self.u)
        self.has_eq = bool((self.cls == 1).any())
        self.LP = np.bincount(self.pr, minlength=n)                  # entries per row of P, per row and per column of A
        self.LAr, self.LAc = np.bincount(self.ar, minlength=m), np.bincount(self.ac, minlength=n)
        self.eps_pcg = eps_pcg(st, self.has_eq)

    # ---- operators -------------------------------------------------------------------------------------------------
    def A_mul(self, x):
        return _mv(self.ar, self.ac, self.av, np.asarray(x, dtype=LD), self.m)

    def At_mul(self, w):
        return _mv(self.ac, self.ar, self.av, np.asarray(w, dtype=LD), self.n)

    def P_mul(self, x):
        return _mv(self.pr, self.pc, self.pv, np.asarray(x, dtype=LD), self.n)

    def minv(self, rv):
        """1 / (P_jj + sigma + sum_i rho_i A_ij^2) and its bound."""
        rv, sigma = np.asarray(rv, dtype=LD), LD(self.st["sigma"])
        d, ab = np.zeros(self.n, dtype=LD), np.zeros(self.n, dtype=LD)
        dg = self.pr == self.pc
        np.add.at(d, self.pr[dg], self.pv[dg]); np.add.at(ab, self.pr[dg], np.abs(self.pv[dg]))
        t = rv[self.ar] * self.av * self.av
        np.add.at(d, self.ac, t); np.add.at(ab, self.ac, t)
        d, ab = d + sigma, ab + sigma
        val = 1 / d
        return val, np.abs(val) * ((self.LAc + 8) * U * ab / np.abs(d) + U)

    def rhs(self, x, z, y, rv):
        """b = sigma x - q + A'(rho z - y) and its bound."""
        x, z, y, rv = (np.asarray(v, dtype=LD) for v in (x, z, y, rv))
        sigma = LD(self.st["sigma"])
        aw, ab = _mv(self.ac, self.ar, self.av, rv * z - y, self.n)
        _, ab = _mv(self.ac, self.ar, np.abs(self.av), np.abs(rv * z) + np.abs(y), self.n)
        return sigma * x - self.q + aw, (self.LAc + 8) * U * (np.abs(sigma * x) + np.abs(self.q) + ab)

    def K_mul(self, v, rv):
        """K v and the bound of a float64 evaluation of it (A v, times rho, A' of that, + P v + sigma v)."""
        v, rv, sigma = np.asarray(v, dtype=LD), np.asarray(rv, dtype=LD), LD(self.st["sigma"])
        pv, pab = self.P_mul(v)
        av, aab = self.A_mul(v)
        t, tab = self.At_mul(rv * av)
        _, tab = _mv(self.ac, self.ar, np.abs(self.av), rv * aab, self.n)
        La = int(self.LAr.max()) if self.m else 0
        return pv + sigma * v + t, (self.LP + self.LAc + La + 8) * U * (pab + np.abs(sigma * v) + tab)

    def K_dense(self, rv):
        n, m = self.n, self.m
        K = np.zeros((n, n), dtype=LD)
        np.add.at(K, (self.pr, self.pc), self.pv)
        K[np.arange(n), np.arange(n)] += LD(self.st["sigma"])
        if m and m * n * n <= 10 ** 8:
            Ad = np.zeros((m, n), dtype=LD)
            np.add.at(Ad, (self.ar, self.ac), self.av)
            K += Ad.T @ (np.asarray(rv, dtype=LD)[:, None] * Ad)
        elif m:                 # many short rows: the products of each row's entries, pair by pair
            o = np.argsort(self.ar, kind="stable")
            r, c, a = self.ar[o], self.ac[o], self.av[o]
            pos = np.arange(r.size) - np.concatenate([[0], np.cumsum(self.LAr)])[r]
            L = int(self.LAr.max())
            cols, vals = np.zeros((m, L), dtype=np.int64), np.zeros((m, L), dtype=LD)
            cols[r, pos], vals[r, pos] = c, a
            w = np.asarray(rv, dtype=LD)
            for i in range(L):
                for j in range(L):
                    np.add.at(K, (cols[:, i], cols[:, j]), w * vals[:, i] * vals[:, j])
        return K

    # ---- one ADMM iteration, given x~ --------------------------------------------------------------------------------
    def step(self, xt, x, z, y, rv, zt=None):
        """update_x / update_z / update_y from x~ (and z~ = A x~: computed here unless given).  Returns dict name -> (value, bound)
        for x, z, y, and `arg`: the argument of the projection with its bound (a row whose argument is further than that from both
        of its bounds lands where the reference says)."""
        al = LD(self.st["alpha"])
        xt, x, z, y, rv = (np.asarray(v, dtype=LD) for v in (xt, x, z, y, rv))
        if zt is None:
            zt, zab = self.A_mul(xt)
            zt_b = (self.LAr + 4) * U * zab
        else:
            zt, zt_b = np.asarray(zt, dtype=LD), np.zeros(self.m, dtype=LD)
        xn = al * xt + (1 - al) * x
        xn_b = 4 * U * (np.abs(al * xt) + np.abs((1 - al) * x))
        v = al * zt + (1 - al) * z
        v_b = np.abs(al) * zt_b + 4 * U * (np.abs(al * zt) + np.abs((1 - al) * z))
        arg = v + y / rv
        arg_b = v_b + 4 * U * (np.abs(v) + np.abs(y / rv))
        zn = np.minimum(np.maximum(arg, self.l), self.u)
        yn = y + rv * (v - zn)
        yn_b = rv * (v_b + arg_b) + 4 * U * (np.abs(y) + rv * (np.abs(v) + np.abs(zn)))
        return dict(x=(xn, xn_b), z=(zn, arg_b), y=(yn, yn_b), arg=(arg, arg_b), zt=(zt, zt_b))

    # ---- the fifteen scalars, info, termination --------------------------------------------------------------------
    def scalars(self, x, y, z):
        """The fifteen scalars of a termination check (SC_NAMES) from x, y, z, and their bounds."""
        x, y, z = (np.asarray(v, dtype=LD) for v in (x, y, z))
        n, m = self.n, self.m
        val, bnd = np.zeros(15, dtype=LD), np.zeros(15, dtype=LD)

        def put(ks, ku, v, b, s):
            # |v|_inf at ks and |s v|_inf at ku; b: the bound of v element by element (the product with s rounds once more)
            if v.size:
                val[ks], bnd[ks] = np.abs(v).max(), b.max()
                val[ku], bnd[ku] = np.abs(s * v).max(), (np.abs(s) * b + 2 * U * np.abs(s * v)).max()
        if m:
            ax, aab = self.A_mul(x)
            ax_b = (self.LAr + 4) * U * aab
            put(3, 0, ax - z, ax_b + 2 * U * (np.abs(ax) + np.abs(z)), self.Einv)
            put(4, 1, z, np.zeros(m, dtype=LD), self.Einv)
            put(5, 2, ax, ax_b, self.Einv)
        px, pab = self.P_mul(x)
        px_b = (self.LP + 4) * U * pab
        if m:
            aty, tab = self.At_mul(y)
            aty_b = (self.LAc + 4) * U * tab
        else:
            aty, tab, aty_b = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
        d = px + self.q + aty
        d_b = px_b + aty_b + 4 * U * (np.abs(px) + np.abs(self.q) + np.abs(aty))
        put(7, 6, d, d_b, self.Dinv); put(9, 8, self.q.astype(LD), np.zeros(n, dtype=LD), self.Dinv)
        put(11, 10, aty, aty_b, self.Dinv); put(13, 12, px, px_b, self.Dinv)
        t = x * (LD(0.5) * px + self.q)
        val[14] = t.sum()
        bnd[14] = (n + int(self.LP.max()) + 8) * U * (np.abs(x) * (LD(0.5) * pab + np.abs(self.q))).sum()
        return val, bnd

    def unscaled_termination(self):
        return self.scaled_data and not self.st["scaled_termination"]

    def info(self, sc, rho):
        """pri_res, dua_res, obj_val, rho_estimate from the fifteen scalars."""
        s, un = dict(zip(SC_NAMES, sc)), self.unscaled_termination()
        pri = 0 * sc[0] if self.m == 0 else (s["pri_u"] if un else s["pri_s"])
        dua = s["dua_u"] / self.c if un else s["dua_s"]
        return dict(pri_res=pri, dua_res=dua, obj_val=s["obj"] / self.c, rho_estimate=self.rho_estimate(sc, rho))

    def rho_estimate(self, sc, rho):
        s = dict(zip(SC_NAMES, sc))
        pri = (s["pri_s"] if self.m else 0 * sc[0]) / (max(s["z_s"], s["Ax_s"]) + DIV_TOL)
        dua = s["dua_s"] / (max(s["q_s"], s["Aty_s"], s["Px_s"]) + DIV_TOL)
        return min(max(rho * np.sqrt(pri / dua), RHO_MIN), RHO_MAX)

    def terminated(self, sc, approximate=False):
        s, st, un = dict(zip(SC_NAMES, sc)), self.st, self.unscaled_termination()
        k = 10.0 if approximate else 1.0
        ea, er = k * st["eps_abs"], k * st["eps_rel"]
        i = self.info(sc, 1.0)
        prim_ok = self.m == 0 or i["pri_res"] < ea + er * (max(s["z_u"], s["Ax_u"]) if un else max(s["z_s"], s["Ax_s"]))
        nrm = max(s["q_u"], s["Aty_u"], s["Px_u"]) / self.c if un else max(s["q_s"], s["Aty_s"], s["Px_s"])
        return bool(prim_ok and i["dua_res"] < ea + er * nrm)

    def status(self, sc):
        return "solved" if self.terminated(sc) else ("solved inaccurate" if self.terminated(sc, True) else "maximum iterations reached")

    # ---- the whole loop, with an exact dense solve in place of PCG -----------------------------------------------------
    def new_state(self):
        n, m = self.n, self.m
        return dict(x=np.zeros(n, dtype=LD), xt=np.zeros(n, dtype=LD), z=np.zeros(m, dtype=LD), y=np.zeros(m, dtype=LD),
                    rho=None, rho_updates=0, chol=None)

    def solve(self, state=None):
        from types import SimpleNamespace
        st = self.st
        s = state if state is not None else self.new_state()
        if s["rho"] is None:
            s["rho"] = clip_rho(st["rho"])
        interval = st["adaptive_rho_interval"] or (4 * st["check_termination"] if st["check_termination"] else 100)
        status, it, checked, sc = None, 0, False, None
        for it in range(1, st["max_iter"] + 1):
            rv = rho_vec(self.l, self.u, s["rho"])
            if s["chol"] is None:
                s["chol"] = cholesky(self.K_dense(rv))
            b, _ = self.rhs(s["x"], s["z"], s["y"], rv)
            s["xt"] = chol_solve(s["chol"], b)
            r = self.step(s["xt"], s["x"], s["z"], s["y"], rv)
            s["x"], s["z"], s["y"] = r["x"][0], r["z"][0], r["y"][0]
            checked = bool(st["check_termination"]) and it % st["check_termination"] == 0
            if checked:
                sc, _ = self.scalars(s["x"], s["y"], s["z"])
                if self.terminated(sc):
                    status = "solved"
                    break
            if st["adaptive_rho"] and it % interval == 0:
                if not checked:
                    sc, _ = self.scalars(s["x"], s["y"], s["z"])
                new = float(self.rho_estimate(sc, s["rho"]))
                if new > s["rho"] * st["adaptive_rho_tolerance"] or new < s["rho"] / st["adaptive_rho_tolerance"]:
                    s["rho"], s["chol"] = clip_rho(new), None
                    s["rho_updates"] += 1
        if not checked:
            sc, _ = self.scalars(s["x"], s["y"], s["z"])
        if status is None:
            status = self.status(sc)
        i = self.info(sc, s["rho"])
        info = SimpleNamespace(status=status, iter=it, rho_updates=s["rho_updates"], **{k: float(v) for k, v in i.items()})
        return SimpleNamespace(x=(self.D * s["x"]).astype(np.float64), y=(self.E * s["y"] / self.c).astype(np.float64), info=info, state=s)


def cholesky(K):
    """Lower Cholesky factor in long double; raises when K is not positive definite."""
    K = np.array(K, dtype=LD)
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        d = K[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite at %d" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def chol_solve(L, b):
    n = L.shape[0]
    y = np.zeros(n, dtype=LD)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def dominant(model):
    """True when P + sigma I is strictly diagonally dominant with a positive diagonal: K = that + a Gram matrix is then positive
    definite (for the cases that are too large for a dense factor)."""
    d, off = np.zeros(model.n, dtype=LD), np.zeros(model.n, dtype=LD)
    dg = model.pr == model.pc
    np.add.at(d, model.pr[dg], model.pv[dg])
    np.add.at(off, model.pr[~dg], np.abs(model.pv[~dg]))
    return bool(np.all(d + LD(model.st["sigma"]) > off))


# ---------------------------------------------------------------------------------------------------------------
# the seeded cases
# ---------------------------------------------------------------------------------------------------------------
SIZES = ((1, 256), (255, 1), (256, 257), (257, 255), (32768, 32769), (32769, 32768))      # (n, m): every size once as n and once as m
PLANT_AT = (0, 63, 64, 255, 256, -1)


def banded(n, m, seed, scaled=False, band=True, per_row=2):
    """P: diagonal in [1, 2] with 0.1 on the first super-diagonal (diagonally dominant); A: `per_row` entries per row in distinct columns
    that move along with the row; rows by turns narrow (|bound| 0.01: the first projection lands on l or on u), wide (lands inside),
    free (beyond +-1e26) and equality.  scaled: D, E in [0.5, 2], c = 0.7."""
    rng = np.random.RandomState(seed)
    d = 1.0 + rng.rand(n)
    P = sparse.diags(d)
    if band and n > 1:
        P = P + sparse.diags(np.full(n - 1, 0.1), 1)
    k = min(per_row, n)
    rows = np.repeat(np.arange(m), k)
    cols = ((np.arange(m)[:, None] * k + np.arange(k)[None, :]) % n).ravel()
    vals = (rng.uniform(0.5, 1.5, m * k) * rng.choice([-1.0, 1.0], m * k))
    A = sparse.csc_matrix((vals, (rows, cols)), shape=(m, n))
    q = rng.randn(n)
    kind = np.arange(m) % 4
    l = np.select([kind == 0, kind == 1, kind == 2], [-0.01, -50.0, -1e30], 0.05)
    u = np.select([kind == 0, kind == 1, kind == 2], [0.01, 50.0, 1e30], 0.05)
    if scaled:
        D, E, c = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, m), 0.7
    else:
        D, E, c = np.ones(n), np.ones(m), 1.0
    return dict(P=sparse.triu(P, format="csc"), q=q, A=A, l=l.astype(float), u=u.astype(float), D=D, E=E, c=c)


def class_case():
    """Bounds on the thresholds of set_rho_vec (all comparisons strict), and the three kinds of column.  Returns the scaled dict and
    the classes claimed, row by row."""
    below, above = np.nextafter(-1e26, -np.inf), np.nextafter(1e26, np.inf)
    rows = [(-1e26, 1e30, 0),                       # l exactly -1e26: not free
            (-1e30, 1e26, 0),                       # u exactly 1e26: not free
            (below, above, -1),                     # one ulp beyond both: free
            (below, 1e26, 0),
            (0.0, 1e-4, 0),                         # u - l exactly 1e-4: inequality
            (0.0, np.nextafter(1e-4, 0.0), 1),      # one ulp below: equality
            (-0.5e-4, 0.5e-4, 0),                   # exact difference again, around zero
            (1.0, 1.0, 1),
            (-1e30, 1e30, -1),
            (-1.0, 2.0, 0)]
    m, n = len(rows), 6
    # columns: 0, 1 diagonal of P and entries of A; 2 entries of A and no diagonal of P stored; 3 diagonal of P only; 4 entirely empty; 5 as 0
    P = sparse.csc_matrix((np.array([1.5, 2.0, 0.75, 1.25]), (np.array([0, 1, 3, 5]), np.array([0, 1, 3, 5]))), shape=(n, n))
    ar = np.repeat(np.arange(m), 2)
    ac = np.array([[0, 2], [1, 2], [0, 5], [2, 5], [0, 1], [1, 2], [2, 5], [0, 5], [1, 5], [0, 2]]).ravel()
    av = np.random.RandomState(11).uniform(0.5, 1.5, 2 * m) * np.where(np.arange(2 * m) % 3 == 0, -1.0, 1.0)
    A = sparse.csc_matrix((av, (ar, ac)), shape=(m, n))
    q = np.array([0.3, -0.2, 0.1, 0.4, 1e-7, -0.6])
    sc = dict(P=P, q=q, A=A, l=np.array([r[0] for r in rows]), u=np.array([r[1] for r in rows]), D=np.ones(n), E=np.ones(m), c=1.0)
    return sc, np.array([r[2] for r in rows])


def dense_column_case(k, n=300, seed=21):
    """A with k rows whose column 0 is dense (row 0 of [P | A'] then holds exactly k entries: nothing of P is stored in column 0)
    and one more entry per row; diagonal P elsewhere."""
    rng = np.random.RandomState(seed + k)
    d = 1.0 + rng.rand(n); d[0] = 0.0
    P = sparse.csc_matrix(sparse.diags(d)); P.eliminate_zeros()
    rows = np.repeat(np.arange(k), 2)
    cols = np.stack([np.zeros(k, dtype=int), 1 + np.arange(k) % (n - 1)], axis=1).ravel()
    vals = rng.uniform(0.5, 1.5, 2 * k) * rng.choice([-1.0, 1.0], 2 * k)
    A = sparse.csc_matrix((vals, (rows, cols)), shape=(k, n))
    kind = np.arange(k) % 3
    l = np.select([kind == 0, kind == 1], [-0.01, -50.0], -1e30)
    u = np.select([kind == 0, kind == 1], [0.01, 50.0], 1e30)
    return dict(P=sparse.triu(P, format="csc"), q=rng.randn(n), A=A, l=l.astype(float), u=u.astype(float), D=np.ones(n), E=np.ones(k), c=1.0)


def planted(n, m, at, seed, scaled):
    """A banded case whose largest |q_j| sits at column `at` and whose largest |z_i| (so also the largest |A x - z|) at row `at`, both
    with a negative sign (at = -1: the last index).  Row `at` has u = -1000 and no lower bound: the first projection lands on u.
    scaled: D and E are smallest there, so the unscaled maxima sit at the same index."""
    sc = banded(n, m, seed, scaled=scaled)
    j, i = at % n, at % m
    q, l, u, D, E = (sc[k].copy() for k in ("q", "l", "u", "D", "E"))
    q[j] = -(np.abs(q).max() * 4 + 1.0)
    l[i], u[i] = -1e30, -1000.0
    if scaled:
        D[j], E[i] = 0.5, 0.5
    sc.update(q=q, l=l, u=u, D=D, E=E)
    return sc


def m0_case(n=257, seed=5):
    sc = banded(n, 0, seed)
    return sc


def zero_q_case(n=300, m=200, seed=8):
    """q = 0 and 0 strictly inside every pair of bounds: b = 0 at every iteration."""
    sc = banded(n, m, seed)
    kind = np.arange(m) % 3
    sc.update(q=np.zeros(n), l=np.select([kind == 0, kind == 1], [-0.01, -50.0], -1e30).astype(float),
              u=np.select([kind == 0, kind == 1], [0.01, 50.0], 1e30).astype(float))
    return sc


def slow_pcg_case(n=400, seed=9):
    """P = tridiag(-1, 2.0001, -1)-like (still diagonally dominant), few rows: Jacobi-PCG needs far more than four iterations."""
    rng = np.random.RandomState(seed)
    P = sparse.diags(np.full(n, 2.0001)) + sparse.diags(np.full(n - 1, -1.0), 1)
    m = 20
    A = sparse.csc_matrix((np.ones(m), (np.arange(m), np.arange(m) * (n // m))), shape=(m, n))
    return dict(P=sparse.triu(P, format="csc"), q=rng.randn(n), A=A, l=-np.ones(m), u=np.ones(m), D=np.ones(n), E=np.ones(m), c=1.0)


def diagonal_K_case(n=300, seed=10):
    """P diagonal and every row of A a single entry in a column of its own: K is diagonal and the Jacobi-PCG ends after ONE iteration,
    so three of the first group's four are issued past convergence."""
    rng = np.random.RandomState(seed)
    m = n // 2
    P = sparse.diags(1.0 + rng.rand(n))
    A = sparse.csc_matrix((rng.uniform(0.5, 1.5, m), (np.arange(m), 2 * np.arange(m))), shape=(m, n))
    return dict(P=sparse.triu(P, format="csc"), q=rng.randn(n), A=A, l=-0.3 * np.ones(m), u=0.3 * np.ones(m), D=np.ones(n), E=np.ones(m), c=1.0)


def nonconvex_case(n=64):
    """Diagonal P with one entry -0.5 and q = e_7 there alone: K = P + sigma I has a negative eigenvalue and the first p'Kp is
    q_7^2 / (-0.5 + sigma) < 0."""
    d = np.ones(n); d[7] = -0.5
    q = np.zeros(n); q[7] = 1.0
    return dict(P=sparse.csc_matrix(sparse.diags(d)), q=q, A=sparse.csc_matrix((0, n)), l=np.zeros(0), u=np.zeros(0), D=np.ones(n), E=np.ones(0), c=1.0)


# ---- two-rank edges (tests/test_rowpart.py): unscaled problems dict(P, q, A, l, u) for the oracle and for both variants ----
def edge_problem(name):
    rng = np.random.RandomState(31)
    if name == "dense_last_row":         # three singleton rows and one dense last row: shard_rows gives rank 1 no rows
        n = 200
        A = sparse.vstack([sparse.csc_matrix((np.ones(3), (np.arange(3), np.array([0, 50, 100]))), shape=(3, n)),
                           sparse.csc_matrix(np.ones((1, n)))], format="csc")
        return dict(P=sparse.csc_matrix(sparse.diags(1.0 + rng.rand(n))), q=rng.randn(n), A=A,
                    l=np.array([-0.1, -0.1, -0.1, 1.0]), u=np.array([0.1, 0.1, 0.1, 1.0 + 1.0]))
    if name == "eq_on_rank1":            # equality rows only in the second half of the rows
        n, m = 40, 60
        A = sparse.random(m, n, density=0.15, random_state=rng, format="csc") + sparse.vstack([sparse.eye(n), sparse.eye(m - n, n)], format="csc")
        l, u = -np.ones(m), np.ones(m)
        l[50:] = u[50:] = 0.1 * rng.randn(10)
        return dict(P=sparse.csc_matrix(sparse.diags(1.0 + rng.rand(n))), q=rng.randn(n), A=sparse.csc_matrix(A), l=l, u=u)
    if name == "m0":
        n = 30
        B = sparse.random(n, n, density=0.1, random_state=rng)
        P = sparse.triu(B.T @ B + sparse.eye(n), format="csc")
        return dict(P=P, q=rng.randn(n), A=sparse.csc_matrix((0, n)), l=np.zeros(0), u=np.zeros(0))
    if name == "n2_diag":                # world = 3: shard_triu gives nnz [1, 1, 0]
        return dict(P=sparse.csc_matrix(sparse.diags([1.0, 2.0])), q=np.array([1.0, -1.0]),
                    A=sparse.csc_matrix(np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]])), l=np.array([0.2, -0.5, -0.5]), u=np.array([0.2, 0.5, 0.5]))
    raise KeyError(name)


EDGE_WORLD2 = ("dense_last_row", "eq_on_rank1", "m0")
EDGE_WORLD3 = ("n2_diag",)
EDGE_SETTINGS = dict(eps_abs=1e-5, eps_rel=1e-5)
