"""Cases of OSQP.verify (osqp_amd_verify, osqp_amd/csrc/verify.h): tests/test_gpu_verify.py runs them on the device,
tests/test_verify_cases_host.py proves on the CPU what the device tests lean on.  Problems, given points and tolerances are
built once and never modified.  (tests/_verify_cases.py holds the cases of BatchOSQP.verify.)

The kernels take one wavefront per row of A and per column (a row of the symmetric P and a column of A), ROWS of them per
workgroup and sweep, at most CAP workgroups, and hand a row or column with more than LONG entries to a whole workgroup.
These constants are the kernels' own (hipver_info, read from the library without a device); the sizes that depend on them
are computed from them here and asserted in the tests.

  n1m0, n1m1, n300m0                     the smallest problems, and no constraints at all
  e63 .. e257                            n one below, at and above 64 and 256, m = 2 n + 1
  trip                                   n = m = CAP * ROWS + 1: exactly one row and one column take a second trip of the sweep
  structure, structure_noP,              n = 40: an empty row and an empty column of A, a column of P with nothing on the
  structure_diagP                        diagonal, stored zeros in P and A; then nnzP = 0; then a diagonal-only P
  lengths                                n = 1500, m = 700: rows of A, columns of A and rows of the symmetric P with 63, 64, 65,
                                         127, 128, 129, LONG - 1, LONG and LONG + 1 entries (an arrow-shaped P, dense rows and dense
                                         columns of A, cut to length)
  inf_zero, inf_nonzero                  infinite bounds under zero and under nonzero multipliers
  nan_<v>, osqpnan_<v>                   an IEEE NaN / the number OSQP_NAN in each of x, y, dx, dy
  pinf_true, pinf_spoiled, pinf_zero     two contradictory rows planted in a random problem; dy their certificate, a spoiled one, 0
  dinf_true, dinf_spoiled, dinf_zero     a variable without curvature or constraints and q_j < 0; dx its direction, a spoiled one, 0
  loose                                  tolerances so wide that `optimal` holds
  random                                 a random sparse QP, n = 2000, m = 4000

Every P is such that K = P + sigma I + A' rho A is positive definite (setup's convexity probe passes); verify itself asks
nothing of the kind."""
import ctypes as C
import functools

import numpy as np
from scipy import sparse

OSQP_NAN = float(0x7FC00000)
EPS_INF = (1e-4, 1e-4)            # the default eps_prim_inf, eps_dual_inf
DEFAULT_EPS = (1e-3, 1e-3)        # the default eps_abs, eps_rel
LENGTHS_BASE = (63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def constants():
    """dict(NT, ROWS, CAP, LONG) from hipver_info."""
    import osqp_amd
    f = osqp_amd.lib().hipver_info
    f.restype, f.argtypes = C.c_int, [C.POINTER(C.c_int)]
    out = (C.c_int * 4)()
    assert f(out) == 0
    return dict(NT=out[0], ROWS=out[1], CAP=out[2], LONG=out[3])


def lengths():
    L = constants()["LONG"]
    return LENGTHS_BASE + (L - 1, L, L + 1)


def grid(n, m):
    k = constants()
    return min(k["CAP"], max(1, -(-max(n, m) // k["ROWS"])))


def _qp(n, m, seed, per_row=4, per_col=3):
    """A random sparse QP: P diagonally dominant with per_col off-diagonals a column, A with per_row entries a row; ranges,
    equalities and one-sided rows; a random point with exact zeros in y and no multiplier on an infinite bound."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for j in range(n):
        k = min(per_col, j)
        if k:
            rows.append(rng.choice(j, k, replace=False)); cols.append(np.full(k, j))
    if rows:
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        off = sparse.csc_matrix((rng.uniform(-0.1, 0.1, rows.size), (rows, cols)), shape=(n, n))
    else:
        off = sparse.csc_matrix((n, n))
    P = (off + sparse.diags(rng.uniform(1.0, 2.0, n))).tocsc()
    if m:
        k = min(per_row, n)
        ar = np.repeat(np.arange(m), k)
        ac = np.concatenate([rng.choice(n, k, replace=False) for _ in range(m)])
        A = sparse.csc_matrix((rng.standard_normal(ar.size), (ar, ac)), shape=(m, n))
    else:
        A = sparse.csc_matrix((0, n))
    return _finish(P, A, rng)


def _finish(P, A, rng, keep_zeros=False):
    n, m = A.shape[1], A.shape[0]
    P = sparse.triu(P, format="csc") if not keep_zeros else P
    A = sparse.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    x0 = rng.standard_normal(n)
    ax = A @ x0
    l, u = ax - rng.uniform(0.1, 1.0, m), ax + rng.uniform(0.1, 1.0, m)
    kind = rng.integers(0, 5, m)                     # 0, 1: a range; 2: an equality; 3: no upper bound; 4: no lower bound
    l[kind == 2] = u[kind == 2] = ax[kind == 2]
    u[kind == 3] = 1e30; l[kind == 4] = -1e30
    q = rng.standard_normal(n)
    x = rng.standard_normal(n); y = rng.standard_normal(m) * 10.0 ** rng.uniform(-1, 1, m)
    y[rng.random(m) < 0.3] = 0.0
    y = np.where(((y > 0) & (u > 1e26)) | ((y < 0) & (l < -1e26)), 0.0, y)
    dx, dy = rng.standard_normal(n), rng.standard_normal(m)
    return dict(P=P, A=A, q=q, l=l, u=u, x=x, y=y, dx=dx, dy=dy, eps=None)


def _structure(kind):
    """n = 40, m = 30.  Row 7 and column 39 of A are empty; column 38 of triu(P) holds one off-diagonal entry and no diagonal
    (row 1 of A, the single entry 5 on it, keeps K positive definite); P and A each store two zeros.  kind "noP": no entry in P;
    "diagP": the diagonal alone."""
    rng = np.random.default_rng(4100)
    n, m = 40, 30
    c = _qp(n, m, 4101)
    A = c["A"].tolil()
    A[7, :] = 0.0; A[:, 39] = 0.0; A[1, :] = 0.0; A[1, 38] = 5.0
    A = A.tocsc(); A.eliminate_zeros(); A.sort_indices()
    free = np.flatnonzero(A.indices != 1)            # (row 1's entry stays)
    A.data[free[[3, -2]]] = 0.0                      # stored zeros: still entries of the pattern
    if kind == "noP":
        P = sparse.csc_matrix((n, n))
    elif kind == "diagP":
        P = sparse.diags(rng.uniform(1.0, 2.0, n)).tocsc()
    else:
        P = sparse.triu(c["P"]).tolil()
        P[:, 38] = 0.0; P[38, :] = 0.0; P[0, 38] = 0.05
        P = P.tocsc(); P.eliminate_zeros(); P.sort_indices()
        assert P[38, 38] == 0 and P[:, 38].nnz == 1
        P.data[[1, P.nnz - 3]] = 0.0
        assert P.nnz == len(P.data) and np.count_nonzero(P.data) == P.nnz - 2
    assert A[7, :].nnz == 0 and A[:, 39].nnz == 0 and np.count_nonzero(A.data) == A.nnz - 2
    return _finish(P, A, rng, keep_zeros=True)


def _lengths():
    """n = 1500, m = 700.  Row r of A, column r of A and row r of the symmetric P (r = 0 .. 8) have lengths()[r] entries each: the
    dense rows of A lie on columns 20 .., its dense columns on rows 20 .., the arrow of P on (r, 20 ..) beside its diagonal.  The
    other rows of A (560 ..) hold four entries each on columns 600 ...  The given x and y are such that the longest row and the
    longest column of A attain |A x|oo and |A'y|oo, so that an entry lost from either shows."""
    rng = np.random.default_rng(4200)
    n, m, Ls = 1500, 700, lengths()
    assert max(Ls) <= m - 20 and max(Ls) + 20 <= 600
    ar, ac, pr, pc = [], [], [], []
    for r, L in enumerate(Ls):
        ar.append(np.full(L, r)); ac.append(20 + np.arange(L))                 # row r of A
        ar.append(20 + np.arange(L)); ac.append(np.full(L, r))                 # column r of A
        pr.append(np.full(L - 1, r)); pc.append(20 + np.arange(L - 1))         # row r of P: the diagonal and L - 1 more
    for i in range(560, m):
        ar.append(np.full(4, i)); ac.append(600 + rng.choice(n - 600, 4, replace=False))
    ar, ac, pr, pc = (np.concatenate(v) for v in (ar, ac, pr, pc))
    A = sparse.csc_matrix((rng.uniform(0.5, 1.5, ar.size) * rng.choice([-1.0, 1.0], ar.size), (ar, ac)), shape=(m, n))
    P = sparse.csc_matrix((rng.uniform(-1e-3, 1e-3, pr.size), (pr, pc)), shape=(n, n)) + sparse.diags(rng.uniform(2.0, 3.0, n))
    c = _finish(P.tocsc(), A, rng)
    # the longest row and the longest column of A attain |A x|oo and |A'y|oo: x and y take the signs of their entries there
    row, col = c["A"].tocsr()[len(Ls) - 1], c["A"][:, len(Ls) - 1]
    x, y = c["x"].copy(), c["y"].copy()
    x[row.indices] = np.abs(x[row.indices]) * np.sign(row.data)
    y[col.indices] = np.abs(y[col.indices]) * np.sign(col.data)
    y = np.where(((y > 0) & (c["u"] > 1e26)) | ((y < 0) & (c["l"] < -1e26)), 0.0, y)
    last = col.indices[-1]                           # the column's last entry counts: a range there, and a multiplier
    l, u = c["l"].copy(), c["u"].copy()
    l[last], u[last], y[last] = -3.0, 3.0, np.sign(col.data[-1])
    return dict(c, x=x, y=y, l=l, u=u)


def _planted_pinf(kind):
    """Rows 3 and 4 of a random problem made the same row with the bounds [1, 2] and [-2, -1]: dy = -e_3 + e_4 gives
    u'dy+ + l'dy- = -2 and A'dy = 0 exactly."""
    c = _qp(70, 141, 4300)
    A = c["A"].tolil(); A[4, :] = A[3, :]
    A = A.tocsc(); A.sort_indices()
    l, u = c["l"].copy(), c["u"].copy()
    l[3], u[3], l[4], u[4] = 1.0, 2.0, -2.0, -1.0
    dy = np.zeros(141)
    if kind != "zero":
        dy[3], dy[4] = -1.0, (1.0 if kind == "true" else 0.5)
    return dict(c, A=A, l=l, u=u, dy=dy)


def _planted_dinf(kind):
    """Variable 9 of a random problem without curvature and without constraints, q_9 = -1: dx = e_9 gives q'dx = -1, P dx = 0,
    A dx = 0.  The spoiled direction adds 0.3 e_10, which has curvature."""
    c = _qp(70, 141, 4400)
    P = c["P"].tolil(); P[9, :] = 0.0; P[:, 9] = 0.0
    P = P.tocsc(); P.eliminate_zeros(); P.sort_indices()
    A = c["A"].tolil(); A[:, 9] = 0.0
    A = A.tocsc(); A.eliminate_zeros(); A.sort_indices()
    q = c["q"].copy(); q[9] = -1.0
    dx = np.zeros(70)
    if kind != "zero":
        dx[9] = 1.0
        if kind == "spoiled":
            dx[10] = 0.3
    return dict(c, P=P, A=A, q=q, dx=dx)


def _planted_value(base, vec, value):
    c = dict(case(base))
    v = c[vec].copy()
    v[len(v) // 3] = value
    c[vec] = v
    return c


EDGE_N = (63, 64, 65, 255, 256, 257)
NAMES = (["n1m0", "n1m1", "n300m0"] + ["e%d" % n for n in EDGE_N] + ["trip", "structure", "structure_noP", "structure_diagP", "lengths",
         "inf_zero", "inf_nonzero"] + ["%s_%s" % (k, v) for k in ("nan", "osqpnan") for v in ("x", "y", "dx", "dy")] +
         ["pinf_true", "pinf_spoiled", "pinf_zero", "dinf_true", "dinf_spoiled", "dinf_zero", "loose", "random"])


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(P (triu, CSC), A (CSC), q, l, u, x, y, dx, dy, eps: (eps_abs, eps_rel) or None = the defaults)."""
    if name in ("n1m0", "n1m1", "n300m0"):
        n, m = {"n1m0": (1, 0), "n1m1": (1, 1), "n300m0": (300, 0)}[name]
        return _qp(n, m, 4000 + n + m)
    if name[0] == "e" and name[1:].isdigit():
        n = int(name[1:])
        return _qp(n, 2 * n + 1, 4000 + n)
    if name == "trip":
        k = constants()
        n = k["CAP"] * k["ROWS"] + 1
        return _qp(n, n, 4500, per_row=3, per_col=2)
    if name.startswith("structure"):
        return _structure(name.partition("_")[2])
    if name == "lengths":
        return _lengths()
    if name in ("inf_zero", "inf_nonzero"):
        c = _qp(65, 131, 4600)
        if name == "inf_zero":
            assert np.any(c["u"] > 1e26) and np.any(c["l"] < -1e26)
            return c
        y = c["y"].copy()
        y[np.flatnonzero(c["u"] > 1e26)[0]] = 0.7; y[np.flatnonzero(c["l"] < -1e26)[0]] = -0.2
        return dict(c, y=y)
    if name.startswith("nan_") or name.startswith("osqpnan_"):
        kind, _, vec = name.partition("_")
        return _planted_value("e65", vec, np.nan if kind == "nan" else OSQP_NAN)
    if name.startswith("pinf_"):
        return _planted_pinf(name[5:])
    if name.startswith("dinf_"):
        return _planted_dinf(name[5:])
    if name == "loose":
        return dict(_qp(65, 131, 4700), eps=(50.0, 0.5))
    if name == "random":
        return _qp(2000, 4000, 4800)
    raise KeyError(name)


def eps_of(c):
    return c["eps"] or DEFAULT_EPS


@functools.lru_cache(maxsize=None)
def reference(name):
    """The sparse long-double reference of the case (computed once, shared)."""
    return reference_of(case(name))


def reference_of(c, **kw):
    """... of a case dict, or of one with some of its entries replaced."""
    from _verify_sparse_reference import reference as ref
    P, A, e = c["P"], c["A"], eps_of(c)
    n, m = A.shape[1], A.shape[0]
    return ref(n, m, P.indptr, P.indices, P.data, A.indptr, A.indices, A.data, c["q"], c["l"], c["u"], c["x"], c["y"], c["dx"], c["dy"],
               e[0], e[1], EPS_INF[0], EPS_INF[1], **kw)


UPDATES = ("lin_cost", "bounds", "lower_bound", "upper_bound", "P", "A", "P_A")
PARTS = dict(lin_cost="q", bounds="lu", lower_bound="l", upper_bound="u", P="P", A="A", P_A="PA")      # what each touches


def update_data(c, what, partial=False, seed=0):
    """(the keyword arguments of OSQP.update, the case after it) for the update entry `what` of UPDATES on the case c.  partial:
    P / A values for every third slot through an index list.  Bounds widen (l <= u stays); matrix values move by up to 10 %
    (P stays diagonally dominant)."""
    rng = np.random.default_rng(4900 + UPDATES.index(what) + 10 * seed)
    n, m = c["A"].shape[1], c["A"].shape[0]
    kw, new = {}, dict(c)
    parts = PARTS[what]
    if "q" in parts:
        kw["q"] = new["q"] = c["q"] + rng.standard_normal(n)
    if "l" in parts:
        kw["l"] = new["l"] = np.maximum(c["l"] - rng.uniform(0.05, 0.5, m), -1e30)
    if "u" in parts:
        kw["u"] = new["u"] = np.minimum(c["u"] + rng.uniform(0.05, 0.5, m), 1e30)
    for M in "PA":
        if M in parts:
            old = c[M]
            idx = np.arange(0, old.nnz, 3) if partial else np.arange(old.nnz)
            vals = old.data[idx] * rng.uniform(0.9, 1.1, idx.size)
            mat = old.copy(); mat.data[idx] = vals
            new[M] = mat
            kw[M + "x"] = vals
            if partial:
                kw[M + "x_idx"] = idx
    return kw, new


def handle(c, **settings):
    """OSQP().setup on the case's problem (P as its stored triangle: stored zeros stay entries)."""
    import osqp_amd
    m = c["A"].shape[0]
    return osqp_amd.OSQP().setup(P=c["P"], q=c["q"], A=c["A"] if m else None, l=c["l"] if m else None, u=c["u"] if m else None, **settings)
