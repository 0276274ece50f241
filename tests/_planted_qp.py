"""QPs whose solution and active set are chosen, for the tests of the polish / adjoint / tangent route
(k_bp_active, k_bp_form, k_bp_invert, kkt_solve_refined, then k_bp_polish, k_ba_adjoint or k_bt_tangent).  Plain
numpy and scipy; it knows nothing of the library.

Generator (seeded; the patterns are shared by a batch, the values are per member):
  P   shape_family's diagonally dominant construction (tests/_batch_parity.py); member b holds f_b P, f_b in [0.5, 2].
  A   row i has a dominant entry of magnitude in [1, 2] and random sign in column i % n and up to two more entries in
      [-0.2, 0.2]; member b holds s_b A, s_b = 10^U(-1, 1).  (One factor per member: with a factor of its own for every
      row, sigma_min / sigma_max of a few hundred active rows falls to about 3e-3, below the 1e-2 that
      test_planted_qp_host.py demands of every case.)
  active rows   at most one per variable, among rows j, j + n, j + 2n, ...: the active rows are then a row subset of a
      diagonally dominant matrix and independent by construction.
  planting   x* standard normal, act in {-1, 0, +1}^m, |y*| in [0.5, 2] on the active rows (negative at a lower
      bound) and 0 elsewhere, q = -(P x* + A' y*); an active row sits at A x* (an equality row, a row whose other
      bound is infinite, or one whose other bound is 0.5 .. 1 away), an inactive row is free, one-sided or two-sided
      with gaps in [0.5, 1].

Truth: M [x; nu] = [-q; b_act], M = [P, Ar'; Ar, 0], rows ordered lows first, then upps; float64 LU, then
iterative refinement with the residual in long double until it stops falling (Route.solve_true).  The adjoint and
tangent truths are the formulas of _adjoint_reference.py and _tangent_reference.py over the same refined solve.

Yardstick: a float64 model of the device route -- the explicit inverse of [P + delta I, Ar'; Ar, -delta I], then
exactly k refinement steps against M -- on scaled data (P~ = c D P D, A~ = E A D, q~ = c D q, l~ = E l, u~ = E u;
D = E = 1, c = 1 for unscaled data), unscaled afterwards: with T = diag(D, E_act),
    M~ = T [c P, Ar'; Ar, 0] T,   so   M [x; nu] = [g1; g2]   <=>   [x; c nu] = T M~^-1 T [c g1; g2].
Polish also projects (z, y) on the normal cone in the scaled space, as polish.c does.

The wrong-pivot verdict: the case "wrongpivot" (VERDICT_CASES, not in CASES) has one member whose KKT inversion must
meet the pivot 0.0 on the device -- see _build -- and `gj_verdict`, a float64 model of the device's Gauss-Jordan sweep
on the matrix `device_kkt` forms, says which pivot that is (tests/test_planted_verdict_host.py,
tests/test_gpu_batch_pivot_verdict.py).

Bar (one function, `bar`): err <= 10 err_model + 1e-14 max|truth| per output array; the factor and the floor are
the project's (check_member_kinv, Engine.check) and cover another summation order.  Two-sided where asked
(k in {0, 1}): also err >= err_model / 10 -- there the error is the deterministic regularisation error."""
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla
from scipy import sparse

LD = np.longdouble
POLISH = ("x", "y", "obj")
ADJOINT = ("dq", "dl", "du", "dPx", "dAx")
TANGENT = ("dx", "dy")
NDIR = 2


# ------------------------------------------------------------------------------------------------ generator
def _p_pattern(rng, n, empty=False, dense_row=None, no_p=(), pair=None):
    """triu(P), CSC, sorted.  dense_row: that row of the full P couples to every variable that has a P row at all.
    no_p: variables whose row and column of P are empty, the diagonal included (P stays positive semidefinite).
    pair = (j0, j1), j0 < j1: the two variables are coupled to each other and to no other variable -- rows and columns
    j0, j1 of P hold (j0, j0), (j0, j1), (j1, j1) alone."""
    if empty:
        return sparse.csc_matrix((n, n))
    off = sparse.triu(sparse.random(n, n, density=min(1.0, 3.0 / n), random_state=rng, format="csc"), 1)
    off.data = rng.uniform(-0.3, 0.3, off.nnz)
    F = off.toarray()
    if dense_row is not None:
        r = dense_row
        F[r, r + 1:] = rng.uniform(-0.03, 0.03, n - r - 1)
        F[:r, r] = rng.uniform(-0.03, 0.03, r)
    F = F + F.T
    no_p = np.asarray(no_p, np.int64)
    F[no_p, :] = 0.0; F[:, no_p] = 0.0
    if pair is not None:
        j0, j1 = pair
        assert 0 <= j0 < j1 < n
        F[[j0, j1], :] = 0.0; F[:, [j0, j1]] = 0.0
        F[j0, j1] = F[j1, j0] = 0.3
    d = 1.0 + np.abs(F).sum(axis=1) + rng.uniform(0, 2, n)
    d[no_p] = 0.0
    F[np.arange(n), np.arange(n)] = d
    P = sparse.csc_matrix(np.triu(F))
    P.sort_indices()
    return P


def _a_pattern(rng, n, m, dense_rows=(), empty_col=None):
    """A, CSC, sorted.  dense_rows: rows with an entry in every column (but empty_col), the off-dominant ones small
    enough to keep the row dominant.  empty_col: a column without entries; the row that would have its dominant
    entry there has it in the next column instead (the cases never make that row active)."""
    rows, cols, vals = [], [], []
    for i in range(m):
        j = i % n
        if j == empty_col:
            j = (j + 1) % n
        rows.append(i); cols.append(j); vals.append(rng.choice([-1.0, 1.0]) * rng.uniform(1.0, 2.0))
        if i in dense_rows:
            extra = [c for c in range(n) if c != j and c != empty_col]
            v = rng.uniform(-1.0, 1.0, len(extra)) * 0.4 / max(1, len(extra))
        else:
            k = int(rng.integers(0, 3))
            extra = [int(c) for c in rng.choice(n, min(n, k + 2), replace=False) if c != j and c != empty_col][:k]
            v = rng.uniform(-0.2, 0.2, len(extra))
        rows += [i] * len(extra); cols += extra; vals += list(v)
    A = sparse.csc_matrix((vals, (rows, cols)), shape=(m, n))
    A.sort_indices()
    return A


def choose_rows(rng, n, m, count, lo=0, hi=None, must=(), never=()):
    """`count` active rows in [lo, hi), at most one per variable (row i belongs to variable i % n), `must` among them."""
    hi = m if hi is None else hi
    rows = [int(r) for r in must]
    used = {r % n for r in rows}
    assert len(used) == len(rows) and len(rows) <= count
    for r in rng.permutation(np.arange(lo, hi)):
        if len(rows) == count:
            break
        if r % n not in used and r not in never:
            rows.append(int(r)); used.add(int(r) % n)
    assert len(rows) == count, (count, len(rows))
    return np.array(sorted(rows), np.int64)


def _plant(rng, P, A, rows, sign, kinds=None):
    """One member on its own values P, A: (q, l, u, x, y, act).  rows: its active rows; sign: "mixed", "low" or "upp";
    kinds: per active row 0 equality, 1 other bound infinite, 2 other bound 0.5 .. 1 away (None: in turn, in a random
    order of the rows, signs alternating every three so that equality rows of both signs occur)."""
    m, n = A.shape
    Pf = (P + sparse.triu(P, 1).T).tocsr()
    x = rng.standard_normal(n)
    act = np.zeros(m, np.int64)
    order = rng.permutation(len(rows))
    kind = np.zeros(m, np.int64)
    for k, t in enumerate(order):
        r = rows[t]
        s = {"low": -1, "upp": 1}.get(sign) or (1 if (k // 3) % 2 == 0 else -1)
        act[r] = s
        kind[r] = k % 3 if kinds is None else kinds[t]
    y = np.where(act != 0, act * rng.uniform(0.5, 2.0, m), 0.0)
    q = -(Pf @ x + A.T @ y)
    ax = A @ x
    l = ax - rng.uniform(0.5, 1.0, m); u = ax + rng.uniform(0.5, 1.0, m)
    ik = 0
    for i in range(m):
        if act[i] == 0:                     # inactive: two-sided, free, one-sided in turn
            c = ik % 4; ik += 1
            if c == 1:
                l[i], u[i] = -np.inf, np.inf
            elif c == 2:
                l[i] = -np.inf
            elif c == 3:
                u[i] = np.inf
            continue
        if act[i] < 0:
            l[i] = ax[i]
            if kind[i] == 0: u[i] = ax[i]
            elif kind[i] == 1: u[i] = np.inf
        else:
            u[i] = ax[i]
            if kind[i] == 0: l[i] = ax[i]
            elif kind[i] == 1: l[i] = -np.inf
    return q, l, u, x, y, act


def pair_slots(P, pair):
    """The slots of (j0, j0), (j0, j1), (j1, j1) in the values of triu(P) (CSC, sorted)."""
    j0, j1 = pair
    at = lambda i, j: int(P.indptr[j] + np.searchsorted(P.indices[P.indptr[j]:P.indptr[j + 1]], i))
    slots = np.array([at(j0, j0), at(j0, j1), at(j1, j1)], np.int64)
    assert np.array_equal(P.indices[slots], [j0, j0, j1])
    return slots


def _assemble(name, engines, seed, n, m, members, p_kw=None, a_kw=None, settings=None, singular=None):
    """members: per member (rows or a function of the rng giving them, sign[, kinds]).  singular: the member whose
    pair of P (p_kw["pair"]) holds [[1, 1], [1, 1]] -- set before its q is planted, so the planted point solves it."""
    rng = np.random.default_rng(seed)
    P = _p_pattern(rng, n, **(p_kw or {}))
    A = _a_pattern(rng, n, m, **(a_kw or {}))
    B = len(members)
    pair = (p_kw or {}).get("pair")
    Px_all = np.empty((B, P.nnz)); Ax_all = np.empty((B, A.nnz))
    Q = np.empty((B, n)); L = np.empty((B, m)); U = np.empty((B, m))
    X = np.empty((B, n)); Y = np.empty((B, m)); act = np.empty((B, m), np.int64)
    for b, spec in enumerate(members):
        rows, sign = spec[0], spec[1]
        rows = rows(rng) if callable(rows) else np.asarray(rows, np.int64)
        Px_all[b] = rng.uniform(0.5, 2.0) * P.data
        Ax_all[b] = 10.0 ** rng.uniform(-1.0, 1.0) * A.data
        if b == singular:
            Px_all[b][pair_slots(P, pair)] = 1.0
        Pb = sparse.csc_matrix((Px_all[b], P.indices, P.indptr), shape=(n, n))
        Ab = sparse.csc_matrix((Ax_all[b], A.indices, A.indptr), shape=(m, n))
        Q[b], L[b], U[b], X[b], Y[b], act[b] = _plant(rng, Pb, Ab, rows, sign, spec[2] if len(spec) > 2 else None)
    grng = np.random.default_rng(seed + 4242)
    draw = lambda *s: grng.standard_normal(s)
    inc = SimpleNamespace(gx=draw(B, n), gy=draw(B, m), dQ=draw(B, NDIR, n), dL=draw(B, NDIR, m), dU=draw(B, NDIR, m),
                          dPx=draw(B, NDIR, P.nnz), dAx=draw(B, NDIR, A.nnz))
    return SimpleNamespace(name=name, engines=engines, n=n, m=m, B=B, P=P, A=A, Px_all=Px_all, Ax_all=Ax_all, Q=Q, L=L, U=U,
                           x=X, y=Y, act=act, inc=inc, settings=dict(settings or {}), pair=pair, singular=singular)


BOTH, STREAMED = ("auto", "streamed"), ("streamed",)
CASES = ("one", "pad", "pad_exact", "scan", "scan2", "rows", "lp", "lds64k", "max")
ENGINES = dict(one=BOTH, pad=BOTH, pad_exact=BOTH, scan=BOTH, scan2=STREAMED, rows=STREAMED, lp=BOTH, lds64k=STREAMED,
               max=STREAMED)          # (n <= 128: the tiled engine too)
ROWS_DENSE_A, ROWS_EMPTY_COL, ROWS_NO_P = (3, 17), 150, (5, 7, 200)
# Cases with a member whose KKT inversion meets a pivot of the wrong sign: not in CASES, whose every member is served.
VERDICT_CASES = ("wrongpivot",)
ENGINES["wrongpivot"] = BOTH
PAIR = (9, 23)                         # j0 < j1, the decoupled pair of "wrongpivot"
VERDICT_DELTA = 2.0 ** -60             # > 0, and below half an ulp of 1.0: 1.0 + delta == 1.0
_cases = {}


def _build(name, variant):
    s = 1000 * variant
    pick = lambda n, m, count, **kw: (lambda rng: choose_rows(rng, n, m, count, **kw))
    if name == "one":        # none active; one low; one upp; an equality row
        return _assemble(name, BOTH, 11 + s, 1, 5, [([], "mixed"), ([2], "low", [1]), ([4], "upp", [2]), ([1], "mixed", [0])])
    if name == "pad":        # NPOL = 96 with four different identity paddings
        counts = (0, 24, 25, 40) if variant == 0 else (40, 7, 0, 31)
        return _assemble(name, BOTH, 12 + s, 40, 56, [(pick(40, 56, c), "mixed") for c in counts])
    if name == "pad_exact":  # member 0: N == NPOL == 64, no padding at all
        return _assemble(name, BOTH, 13 + s, 40, 56, [(pick(40, 56, 24), "mixed"), (pick(40, 56, 8), "mixed")])
    if name == "scan":       # k_bp_active's 256-wide scan: across its edge; only beyond it, all upps; only the first 64, all lows
        n, m = 64, 257
        return _assemble(name, BOTH, 14 + s, n, m, [(pick(n, m, 30, must=(255, 256)), "mixed"),
                                                    (pick(n, m, 1, lo=256), "upp"), (pick(n, m, 20, hi=64), "low")])
    if name == "scan2":      # the same across 256 and across 512
        n, m = 128, 513
        return _assemble(name, STREAMED, 15 + s, n, m, [(pick(n, m, 50, must=(255, 256)), "mixed"),
                                                        (pick(n, m, 50, must=(511, 512)), "mixed"),
                                                        (pick(n, m, 40, lo=256, must=(512,)), "upp"),
                                                        (pick(n, m, 40, hi=128), "low")])
    if name == "rows":       # rows of P and A longer than k_bp_form's 256 threads; an empty column; no P diagonal
        # (row 0 of the full P has 297 entries, not 300: a variable without a P diagonal can have no other entry of
        # P either, or P would be indefinite)
        n, m = 300, 310
        never = (ROWS_EMPTY_COL,)
        must = ROWS_DENSE_A + ROWS_NO_P
        return _assemble(name, STREAMED, 16 + s, n, m, [(pick(n, m, 120, must=must, never=never), "mixed"),
                                                        (pick(n, m, 9, must=must + (309,), never=never), "mixed")],
                         p_kw=dict(dense_row=0, no_p=ROWS_NO_P), a_kw=dict(dense_rows=ROWS_DENSE_A, empty_col=ROWS_EMPTY_COL))
    if name == "lp":         # P stored empty, n active rows: three vertices
        n, m = 24, 48
        return _assemble(name, BOTH, 17 + s, n, m, [(pick(n, m, n), "mixed")] * 3, p_kw=dict(empty=True))
    if name == "lds64k":     # NPOL = 1216, k_bp_polish's LDS 67 840 B
        return _assemble(name, STREAMED, 18 + s, 600, 600, [(np.arange(600), "mixed"), ([], "mixed")])
    if name == "max":        # N == NPOL == 1408, every row of the KKT matrix a real one; m at the streamed engine's limit
        n, m = 704, 1129     # (n = 1024, N = 2048 passed too but spends 9 s in the three inversions: DESIGN section 4)
        return _assemble(name, STREAMED, 19 + s, n, m, [(pick(n, m, n), "mixed")])
    if name == "wrongpivot":
        # One member's P holds [[1, 1], [1, 1]] on the pair PAIR, which P couples to nothing else.  Without scaling and
        # with delta below half an ulp of 1 the device forms these very bits, pivot j0 is 1 and leaves
        # K[j1][j1] = fma(-1, 1 * (1 / 1), 1) = 0 exactly: pivot j1 is 0.0, the wrong sign (gj_verdict).  P is positive
        # semidefinite and the active rows j0, j1 -- their dominant entries sit in those columns -- pin x_j0 - x_j1, so
        # the QP is convex with a unique solution.  NPOL = 96 with four different paddings; variant 1 moves the
        # singular pair from member 1 to member 2.
        n, m = 40, 56
        counts = (5, 24, 25, 40) if variant == 0 else (40, 7, 25, 31)
        return _assemble(name, BOTH, 20 + s, n, m, [(pick(n, m, c, must=PAIR), "mixed") for c in counts],
                         p_kw=dict(pair=PAIR), settings=dict(scaling=0, delta=VERDICT_DELTA), singular=1 if variant == 0 else 2)
    raise KeyError(name)


def case(name, variant=0):
    """The case (built once, never modified).  variant 1: a second planted problem on the same shapes (for `pad` with
    other active sets); the update test moves a handle of variant 0 to its values, which sit on the same patterns."""
    key = (name, variant)
    if key not in _cases:
        c = _build(name, variant)
        if variant:                           # same patterns as variant 0: only then can a handle be updated to it
            c0 = case(name)
            c = _rebase(c, c0)
        _cases[key] = c
    return _cases[key]


def _rebase(c, c0):
    """A second problem on the patterns of c0: other values, other active sets (c's), planted anew."""
    rng = np.random.default_rng(977 + c.B)
    P, A, n, m = c0.P, c0.A, c0.n, c0.m
    out = SimpleNamespace(**vars(c))
    out.P, out.A = P, A
    out.Px_all = np.empty_like(c0.Px_all); out.Ax_all = np.empty_like(c0.Ax_all)
    out.Q = np.empty_like(c0.Q); out.L = np.empty_like(c0.L); out.U = np.empty_like(c0.U)
    out.x = np.empty_like(c0.x); out.y = np.empty_like(c0.y); out.act = np.empty_like(c0.act)
    for b in range(c0.B):
        out.Px_all[b] = rng.uniform(0.5, 2.0) * P.data
        out.Ax_all[b] = 10.0 ** rng.uniform(-1.0, 1.0) * A.data
        if b == c.singular:
            out.Px_all[b][pair_slots(P, c.pair)] = 1.0
        Pb = sparse.csc_matrix((out.Px_all[b], P.indices, P.indptr), shape=(n, n))
        Ab = sparse.csc_matrix((out.Ax_all[b], A.indices, A.indptr), shape=(m, n))
        rows = np.flatnonzero(c.act[b])
        out.Q[b], out.L[b], out.U[b], out.x[b], out.y[b], out.act[b] = _plant(rng, Pb, Ab, rows, "mixed")
    g = np.random.default_rng(5151)
    draw = lambda *s: g.standard_normal(s)
    out.inc = SimpleNamespace(gx=draw(c0.B, n), gy=draw(c0.B, m), dQ=draw(c0.B, NDIR, n), dL=draw(c0.B, NDIR, m),
                              dU=draw(c0.B, NDIR, m), dPx=draw(c0.B, NDIR, P.nnz), dAx=draw(c0.B, NDIR, A.nnz))
    return out


# ------------------------------------------------------------------------------------------------ one member
def member(c, b, Pv=None, Av=None, q=None, l=None, u=None):
    """Member b of a case as dense data: Pf (full symmetric), Ad, q, l, u, the planted act and the row order of M
    (lows first, then upps).  Pv / Av / q / l / u: other values on the same patterns (the scaled data of a handle)."""
    n, m = c.n, c.m
    Pu = sparse.csc_matrix((c.Px_all[b] if Pv is None else np.asarray(Pv, float), c.P.indices, c.P.indptr), shape=(n, n))
    Ac = sparse.csc_matrix((c.Ax_all[b] if Av is None else np.asarray(Av, float), c.A.indices, c.A.indptr), shape=(m, n))
    act = c.act[b]
    low, upp = np.flatnonzero(act < 0), np.flatnonzero(act > 0)
    return SimpleNamespace(n=n, m=m, Pu=Pu, Ac=Ac, Pf=(Pu + sparse.triu(Pu, 1).T).toarray(), Ad=Ac.toarray().reshape(m, n),
                           q=c.Q[b] if q is None else q, l=c.L[b] if l is None else l, u=c.U[b] if u is None else u,
                           act=act, low=low, upp=upp, rows=np.concatenate([low, upp]).astype(np.int64),
                           Pi=Pu.indices, Pj=np.repeat(np.arange(n), np.diff(Pu.indptr)),
                           Ai=Ac.indices, Aj=np.repeat(np.arange(n), np.diff(Ac.indptr)))


class Route:
    """M = [P, Ar'; Ar, 0] of a member on its planted rows, with the two solves."""

    def __init__(self, mem):
        n, k = mem.n, mem.rows.size
        Ar = mem.Ad[mem.rows]
        M = np.zeros((n + k, n + k))
        M[:n, :n] = mem.Pf; M[:n, n:] = Ar.T; M[n:, :n] = Ar
        self.n, self.k, self.M, self.Ar = n, k, M, Ar
        self._lu = self._Ml = None
        self._inv = {}

    # the three pieces of solve_true that depend on how M is stored (tests/_kkt_instance_cases.py holds M sparse at n = 8192)
    def _factor(self):
        if self._lu is None:
            self._lu = sla.lu_factor(self.M, check_finite=False)
            self._Ml = self.M.astype(LD)

    def _lu_solve(self, v):
        return sla.lu_solve(self._lu, v, check_finite=False)

    def _residual(self, gl, x):
        return gl - self._Ml @ x

    def solve_true(self, g):
        """float64 LU, then refinement with the residual in long double until it stops falling; the best iterate."""
        self._factor()
        gl = np.asarray(g, LD)
        x = self._lu_solve(np.asarray(g, float)).astype(LD)
        best, xbest = np.inf, x
        for _ in range(12):
            r = self._residual(gl, x)
            nr = float(np.abs(r).max()) if r.size else 0.0
            if not nr < best:
                break
            best, xbest = nr, x
            if nr == 0.0:
                break
            x = x + self._lu_solve(r.astype(float)).astype(LD)
        return xbest.astype(float)

    def residual_ld(self, x, g):
        """g - M x in long double."""
        if self._Ml is None:
            self._Ml = self.M.astype(LD)
        return np.asarray(g, LD) - self._Ml @ np.asarray(x, LD)

    def solve_model(self, g, k, delta):
        """The explicit float64 inverse of the delta-regularised matrix, then exactly k refinement steps against M."""
        if delta not in self._inv:
            Mr = self.M.copy()
            i = np.arange(self.n + self.k)
            Mr[i, i] += np.where(i < self.n, delta, -delta)
            self._inv[delta] = np.linalg.inv(Mr)
        Minv = self._inv[delta]
        s = Minv @ g
        for _ in range(k):
            s = s + Minv @ (g - self.M @ s)
        return s


def _obj(mem, x):
    return float(0.5 * x @ (mem.Pf @ x) + mem.q @ x)


def true_polish(mem, route):
    s = route.solve_true(np.concatenate([-mem.q, mem.l[mem.low], mem.u[mem.upp]]))
    x = s[:mem.n]
    y = np.zeros(mem.m); y[mem.rows] = s[mem.n:]
    return SimpleNamespace(x=x, y=y, obj=np.array([_obj(mem, x)]))


def adjoint_from(mem, x, y, gx, gy, solve):
    """_adjoint_reference.py's formulas over solve(g) = M^-1 g."""
    n, m = mem.n, mem.m
    r = solve(np.concatenate([gx, gy[mem.rows]]))
    rx, rnu = r[:n], r[n:]
    rnu_full = np.zeros(m); rnu_full[mem.rows] = rnu
    nu_full = np.where(mem.act != 0, y, 0.0)
    dl = np.zeros(m); du = np.zeros(m)
    dl[mem.low] = rnu[:mem.low.size]; du[mem.upp] = rnu[mem.low.size:]
    Ai, Aj, Pi, Pj = mem.Ai, mem.Aj, mem.Pi, mem.Pj
    dAx = np.where(mem.act[Ai] != 0, -(nu_full[Ai] * rx[Aj] + rnu_full[Ai] * x[Aj]), 0.0)
    dPx = np.where(Pi == Pj, -rx[Pi] * x[Pi], -(rx[Pi] * x[Pj] + rx[Pj] * x[Pi]))
    return SimpleNamespace(dq=-rx, dl=dl, du=du, dPx=dPx, dAx=dAx)


def tangent_from(mem, x, y, inc, solve):
    """_tangent_reference.py's formulas over solve(g) = M^-1 g, for the NDIR directions inc.dQ[d], ...: dx, dy [NDIR, .].
    A member that holds its matrices sparse (mem.sparse, tests/_kkt_instance_cases.py at n = 8192) keeps dP, dA sparse."""
    n, m = mem.n, mem.m
    dx = np.zeros((NDIR, n)); dy = np.zeros((NDIR, m))
    y_act = np.where(mem.act != 0, y, 0.0)
    keep = getattr(mem, "sparse", False)
    for d in range(NDIR):
        dPu = sparse.csc_matrix((inc.dPx[d], mem.Pu.indices, mem.Pu.indptr), shape=(n, n))
        dP = dPu + sparse.triu(dPu, 1).T
        dA = sparse.csc_matrix((inc.dAx[d], mem.Ac.indices, mem.Ac.indptr), shape=(m, n))
        dP, dA = (dP.tocsr(), dA.tocsr()) if keep else (dP.toarray(), dA.toarray().reshape(m, n))
        db = np.concatenate([inc.dL[d][mem.low], inc.dU[d][mem.upp]])
        g = np.concatenate([-(inc.dQ[d] + dP @ x + dA.T @ y_act), db - (dA @ x)[mem.rows]])
        r = solve(g)
        dx[d] = r[:n]; dy[d, mem.rows] = r[n:]
    return SimpleNamespace(dx=dx, dy=dy)


def member_inc(c, b):
    i = c.inc
    return SimpleNamespace(gx=i.gx[b], gy=i.gy[b], dQ=i.dQ[b], dL=i.dL[b], dU=i.dU[b], dPx=i.dPx[b], dAx=i.dAx[b])


_truths = {}


def truth(c, b):
    """Every output of member b from the refined solve (computed once per case and member, never modified)."""
    key = (c.name, id(c), b)
    if key not in _truths:
        mem = member(c, b)
        route = Route(mem)
        pol = true_polish(mem, route)
        inc = member_inc(c, b)
        adj = adjoint_from(mem, pol.x, pol.y, inc.gx, inc.gy, route.solve_true)
        tan = tangent_from(mem, pol.x, pol.y, inc, route.solve_true)
        ax = mem.Ad @ pol.x
        scale_pri = float(np.abs(ax).max()) if mem.m else 0.0
        scale_dua = float(max(np.abs(mem.Pf @ pol.x).max(), np.abs(mem.Ad.T @ pol.y).max() if mem.m else 0.0, np.abs(mem.q).max()))
        _truths[key] = SimpleNamespace(mem=mem, route=route, **vars(pol), **vars(adj), **vars(tan),
                                       scale_pri=scale_pri, scale_dua=scale_dua)
    return _truths[key]


def model(c, b, k, delta=1e-6, ws=None, point=None):
    """Every output of member b from the float64 model of the device route with k refinement steps.  ws: the scaled
    data of a handle (dict with D, E, c, Pv, Av: BatchOSQP.member_workspace); None: unscaled data (D = E = 1, c = 1).
    Also pri / dua (unscaled residuals) and pri_s / dua_s (residuals of the scaled problem).  point: (x, y) at which
    the adjoint and the tangent are taken in place of the model's own polished point (a handle whose polish was
    rejected holds the ADMM iterate)."""
    n, m = c.n, c.m
    raw = member(c, b)
    if ws is None:
        D, E, cs, sm = np.ones(n), np.ones(m), 1.0, raw
    else:
        D, E, cs = np.asarray(ws["D"], float), np.asarray(ws["E"], float).reshape(m), float(ws["c"])
        sm = member(c, b, Pv=ws["Pv"], Av=ws["Av"], q=cs * D * raw.q, l=E * raw.l, u=E * raw.u)
    route = Route(sm)
    rows = sm.rows
    T = np.concatenate([D, E[rows]])
    # polish, in the scaled space, with the projection of polish.c
    s = route.solve_model(np.concatenate([-sm.q, sm.l[sm.low], sm.u[sm.upp]]), k, delta)
    xs = s[:n]
    nu = np.zeros(m); nu[rows] = s[n:]
    axs = sm.Ad @ xs
    t = axs + nu
    zs = np.minimum(np.maximum(t, sm.l), sm.u)
    ys = t - zs
    x, y = D * xs, E * ys / cs
    dr_s = sm.Pf @ xs + sm.q + sm.Ad.T @ ys
    pr_s = axs - zs
    amax = lambda v: float(np.abs(v).max()) if v.size else 0.0
    out = SimpleNamespace(x=x, y=y, obj=np.array([_obj(raw, x)]), pri_s=amax(pr_s), dua_s=amax(dr_s),
                          pri=amax(pr_s / E), dua=amax(dr_s / D) / cs, scale_pri_s=amax(axs),
                          scale_dua_s=max(amax(sm.Pf @ xs), amax(sm.Ad.T @ ys), amax(sm.q)))

    def solve(g):                             # M^-1 g through the scaled route
        g = np.asarray(g, float)
        w = route.solve_model(T * np.concatenate([cs * g[:n], g[n:]]), k, delta) * T
        w[n:] /= cs
        return w
    inc = member_inc(c, b)
    px, py = (x, y) if point is None else point
    for part in (adjoint_from(raw, px, py, inc.gx, inc.gy, solve), tangent_from(raw, px, py, inc, solve)):
        for name, v in vars(part).items():
            setattr(out, name, v)
    return out


def truth_at(c, b, x, y):
    """The adjoint and tangent outputs of member b with the refined solve, taken at the point (x, y)."""
    t = truth(c, b)
    inc = member_inc(c, b)
    out = SimpleNamespace()
    for part in (adjoint_from(t.mem, x, y, inc.gx, inc.gy, t.route.solve_true), tangent_from(t.mem, x, y, inc, t.route.solve_true)):
        for name, v in vars(part).items():
            setattr(out, name, v)
    return out


def accepts(pri, dua, pri0, dua0):
    """The acceptance rule of polish (polish.c:301-311) for polished residuals pri, dua after ADMM's pri0, dua0."""
    return bool((pri < pri0 and dua < dua0) or (pri < pri0 and dua0 < 1e-10) or (dua < dua0 and pri0 < 1e-10))


def device_kkt(mem, delta):
    """[P + delta I, Ar'; Ar, -delta I] of a member as k_bp_form forms it: the planted rows, lows first."""
    M = Route(mem).M.copy()
    i = np.arange(M.shape[0])
    M[i, i] = np.where(i < mem.n, M[i, i] + delta, 0.0 - delta)
    return M


def gj_verdict(K, n):
    """A float64 model of gj_sweep (batch_streamed.h) as k_bp_invert runs it: Gauss-Jordan in place in the natural
    order, no pivoting, and the quasi-definite verdict -- pivot k must be > 0 for k < n and < 0 beyond; zero and NaN
    are wrong.  Returns the first wrong pivot as (k, value), or None.  (The device fuses the update of an entry into
    one fma; here the product is rounded first.  Where the update is exact -- the singular pair -- both give the same
    bits; elsewhere the verdict rests on pivots far from zero.)"""
    K = np.array(K, float)
    N = K.shape[0]
    for k in range(N):
        akk = K[k, k]
        if not (akk > 0.0 if k < n else akk < 0.0):
            return k, float(akk)
        piv = 1.0 / akk
        rk = K[k] * piv
        ck = K[:, k].copy()
        K -= np.outer(ck, rk)
        K[:, k] = 0.0 - ck * piv
        K[k] = rk
        K[k, k] = piv
    return None


# ------------------------------------------------------------------------------------------------ the bar
def err(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max()) if b.size else 0.0


def bar(err_model, truth_value):
    t = np.asarray(truth_value, float)
    return 10.0 * err_model + 1e-14 * (float(np.abs(t).max()) if t.size else 0.0)


def check(tag, got, tru, mod, names, two_sided=False, worst=None):
    """Every array `names` of `got` against `tru` under the bar that `mod` sets.  worst: dict name -> largest err / bar
    seen so far (updated).  Raises AssertionError naming every array that misses."""
    bad = []
    for name in names:
        g, t, mo = np.asarray(getattr(got, name), float), getattr(tru, name), getattr(mod, name)
        assert g.shape == np.shape(t), tag + (name, g.shape, np.shape(t))
        e, em = err(g, t), err(mo, t)
        limit = bar(em, t)
        ratio = e / limit if limit > 0 else (0.0 if e == 0 else np.inf)
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), ratio)
        if not e <= limit:
            bad.append((name, "err %.3e > bar %.3e (model %.3e)" % (e, limit, em)))
        if two_sided and not e >= em / 10.0:
            bad.append((name, "err %.3e < model %.3e / 10" % (e, em)))
    assert not bad, tag + tuple(bad)


def residual_bars(tru, mod, scaled=False):
    """(bar of pri_res, bar of dua_res): the bar with the model's residual as err_model and, as max|truth|, the largest
    term of the residual at the truth (|A x|; |P x|, |A' y|, |q|)."""
    if scaled:                                # residuals of the scaled problem: its terms set the floor
        return 10.0 * mod.pri_s + 1e-14 * mod.scale_pri_s, 10.0 * mod.dua_s + 1e-14 * mod.scale_dua_s
    return 10.0 * mod.pri + 1e-14 * tru.scale_pri, 10.0 * mod.dua + 1e-14 * tru.scale_dua
