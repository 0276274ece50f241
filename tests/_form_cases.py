"""Seeded cases that put every linear-solve form of the single-QP engine (hipeng_resident_info [9]: 0 launch-per-step PCG,
1 resident PCG, 2 block-resident PCG, 3 block-direct, 4 dense-direct) through whole ADMM steps from extrapolated start vectors
and straight after each host call; a Python restatement of the two direct forms' host-side classification (engine.hip:
blocks_eligible / blocks_coupled_eligible, dense_direct_host.h: the dense rows and the B2 set); the host calls as data
(OPS, ORDERS, op_changes); and a float64 model of the step the device takes from the start vector it holds, with the one-place
defects the step bars must not forgive.  tests/test_form_cases_host.py checks all of it on the CPU,
tests/test_gpu_form_steps.py runs the cases on the device.  Nothing here touches the library.

make(name) returns the keys of _pcg_cases.make (name: the seed key of _engine_reference.iterates) and
  case     the name in NAMES
  env      the environment the engine is created in (OSQP_AMD_EXTRAP_SCHED is added by the test)
  claims   form; info: the slots of hipeng_resident_info the case is about ([2] E, [3] workgroups / blocks / dense unknowns,
           [15] coupling rows / B2 unknowns; form 2's grid is the device's own and is read from _pcg_cases.br_probe there);
           layout: slots of hipeng_pcg_layout; gone: {variable: row} of the engine-eliminated slacks; bars: "pcg", "direct",
           "direct_elim" or "direct_inv" (f4_b2_nd0 alone: inverse_residual_error in place of the LU solve's error); large: an n = 8192 case (4 steps, three host calls); symv / vd / fin_dots / plain_rhs: the route
           inside the form, which the device does not report -- the case is built so that the route's own rule selects it
           (dense_direct_host.h: nnz(A) >= 2e5; engine.hip build_blockdirect: every huge row folded) or the switch forces it.
"""
import functools

import numpy as np
import scipy.linalg as sla
from scipy import sparse
from scipy.sparse import linalg as spla

from tests import _direct_problems as DP
from tests import _elim_cases as EC
from tests import _engine_reference as R
from tests import _pcg_cases as PC

LD, U = R.LD, R.U
RHO, RHO_MIN, EQ, INF = DP.RHO, DP.RHO_MIN, DP.EQ, R.INF
PCG_EPS = PC.PCG_EPS
ALPHA = 1.6
COND_CAP = 1e4
DD_DENSE_ROW, DD_NBR, DD_NB, CPL_MAX = 32, 8, 128, 512

STEPS = dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=0)
BLOCKRES = dict(OSQP_AMD_BLOCK_DIRECT=0, OSQP_AMD_DENSE_DIRECT=0)
BD_ENV = dict(OSQP_AMD_BLOCK_DIRECT=1)
DD_ENV = dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=2)
BD_BLOCKS = [32, 33, 64, 127, 128]

NAMES = ("f0_blocks", "f0_long_split",
         "f1_e8_pipe1", "f1_e8_pipe0", "f1_e20_pipe1", "f1_e20_pipe0",
         "f2_nh0", "f2_nh1",
         "f3_plain", "f3_kc1", "f3_kc17", "f3_kc17_plainrhs", "f3_huge1", "f3_huge4", "f3_huge4_nofin", "f3_huge5",
         "f4_b2", "f4_b2_nd0", "f4_slack_pyy0", "f4_slack_pyy03", "f4_symv384", "f4_symv1152", "f4_vd")
# one case per form for the default 5 / 12 schedule and for the host calls, and the three more the host calls run on
PER_FORM = ("f0_blocks", "f1_e20_pipe1", "f2_nh0", "f3_kc1", "f4_b2")
HOST_CALL_CASES = PER_FORM + ("f3_kc17", "f4_slack_pyy0", "f4_symv384")
SEEDS = {name: 501 + k for k, name in enumerate(NAMES)}
R.SEEDS.update(SEEDS)


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
def _raw(name, seed, Pu, A, rho, claims, env):
    """q, l, u for a (triu(P), A, rho) of tests/_direct_problems.py: the rows with rho = 1e3 RHO are equalities, those with RHO_MIN
    free, the others ranges around zero."""
    rng = np.random.default_rng(seed)
    n, m = Pu.shape[0], A.shape[0]
    q = rng.standard_normal(n)
    l, u = -rng.uniform(0.1, 1.0, m), rng.uniform(0.1, 1.0, m)
    eq, free = rho == EQ * RHO, rho == RHO_MIN
    u[eq] = l[eq]
    l[free], u[free] = -INF, INF
    Pu, A = sparse.csc_matrix(Pu), sparse.csc_matrix(A)
    Pu.sort_indices()
    A.sort_indices()
    return dict(name=name, case=name, n=n, m=m, Pu=Pu, A=A, q=q, l=l, u=u, rho=np.asarray(rho, float), env=dict(env), claims=claims)


def _from(base, name, env, claims):
    c = dict(base)
    c.update(case=name, env=dict(env), claims=claims)
    return c


SHARED = {"f3_kc17_plainrhs": "f3_kc17", "f3_huge4_nofin": "f3_huge4"}       # the same problem under another switch: one reference serves both


def _bd(name, blocks, env, kc=0, nhuge=0, **more):
    base = SHARED.get(name, name)
    Pu, A, rho = DP.bd_problem(blocks, seed=SEEDS[base], kc=kc, nhuge=nhuge)
    if nhuge:                                        # Ruiz lifts a huge row's entries to about 1: an equality's rho on it would put cond(K) above the cap
        rho[-nhuge:] = RHO
        if nhuge > 1:
            rho[-1] = RHO_MIN
    form_kc = kc if kc else (nhuge if nhuge > PC.MAX_HUGE_FOLD else 0)
    claims = dict(form=3, info={3: len(blocks), 15: form_kc}, bars="direct", large=sum(blocks) >= 8192, huge=nhuge,
                  fin_dots=int(0 < nhuge <= PC.MAX_HUGE_FOLD), plain_rhs=0)
    claims.update(more)
    c = _raw(base, SEEDS[base], Pu, A, rho, claims, dict(BD_ENV, **env))
    c["case"] = name
    return c


def _dd(name, na, env=None, symv=0, vd=0, **kw):
    nb, ns = len(kw.get("b2_nbrs", ())), kw.get("nslack", 0)
    Pu, A, rho = DP.dd_problem(na, seed=SEEDS[name], **kw)
    m = A.shape[0]
    gone = {na + nb + s: m - ns + s for s in range(ns)}
    if ns:                                           # no free row on a slack: with P_yy = 0 its K_yy would be sigma + 1e-6 a^2, cond(K) 5e8
        rho[m - ns:] = np.where(rho[m - ns:] == RHO_MIN, RHO, rho[m - ns:])
        if kw.get("pyy", 0.0) == 0.0:                # ... and K_yy = sigma + rho a^2 alone: equalities (A x + s = b), which keeps cond(K) below the cap
            rho[m - ns:] = EQ * RHO
    if vd:                                           # 400 dense rows: a third of them at 1e3 RHO would put cond(K) at 3e4
        rho[:kw["nd"]] = np.where(rho[:kw["nd"]] == EQ * RHO, RHO, rho[:kw["nd"]])
    in_b2 = sum(1 for k in kw.get("b2_nbrs", ()) if k <= DD_NBR)
    claims = dict(form=4, info={3: na + nb - in_b2, 15: in_b2}, bars="direct_elim" if ns else "direct", large=False, gone=gone,
                  symv=symv, vd=vd, nd=kw.get("nd", max(1, na // 64)) if kw.get("row_len", 40) >= DD_DENSE_ROW else 0)
    return _raw(name, SEEDS[name], Pu, A, rho, claims, dict(DD_ENV, **(env or {})))


@functools.lru_cache(maxsize=None)
def make(name):
    if name == "f0_blocks":
        b = PC.make("blocks_mixed")
        return _from(b, name, STEPS, dict(form=0, info={1: 0, 2: 0, 3: 0}, layout=dict(dense=8, dense_rows=608, split=0), bars="pcg", large=False))
    if name == "f0_long_split":
        b = R.make_case("long")
        return _from(b, name, dict(STEPS, OSQP_AMD_SPLIT=1), dict(form=0, info={1: 0, 2: 0, 3: 0}, layout=dict(dense=0, long=2, split=1), bars="pcg", large=False))
    if name.startswith("f1_"):
        E, pipe = int(name[4:name.index("_pipe")]), int(name[-1])
        b = PC.make("res_e%d" % E)
        nwg = b["claims"]["nwg"]
        env = dict(OSQP_AMD_DENSE_DIRECT=0, OSQP_AMD_RESIDENT_MIN_N=1, OSQP_AMD_RESIDENT_NWG=nwg, OSQP_AMD_RESIDENT_PIPE=pipe)
        return _from(b, name, env, dict(form=1, info={1: 1, 2: E, 3: nwg}, bars="pcg", large=False, E=E, nwg=nwg))
    if name == "f2_nh0":
        return _from(PC.br_probe(), name, BLOCKRES, dict(form=2, info={1: 1, 2: 64}, layout=dict(dense=2, dense_rows=64, huge=0, folded=0), bars="pcg", large=False))
    if name == "f2_nh1":
        b = PC._blocks_with_rows(name, np.random.default_rng(SEEDS[name]), [128] * 64, 1)
        return _from(b, name, BLOCKRES, dict(form=2, info={1: 1, 2: 64}, layout=dict(dense=64, dense_rows=8192, huge=1, folded=1), bars="pcg", large=True))
    if name == "f3_plain":
        return _bd(name, BD_BLOCKS, {})
    if name == "f3_kc1":
        return _bd(name, BD_BLOCKS, {}, kc=1)
    if name == "f3_kc17":
        return _bd(name, BD_BLOCKS, {}, kc=17)
    if name == "f3_kc17_plainrhs":
        return _bd(name, BD_BLOCKS, dict(OSQP_AMD_BLOCK_PLAIN=1), kc=17, plain_rhs=1)
    if name in ("f3_huge1", "f3_huge4", "f3_huge5"):
        return _bd(name, [128] * 64, {}, nhuge=int(name[-1]))
    if name == "f3_huge4_nofin":
        return _bd(name, [128] * 64, dict(OSQP_AMD_BLOCK_FIN_DOTS=0), nhuge=4, fin_dots=0)
    if name == "f4_b2":
        return _dd(name, 100, b2_nbrs=(0, 3, 8))
    if name == "f4_b2_nd0":
        c = _dd(name, 100, b2_nbrs=(0, 3, 8), nd=0)
        c["claims"]["bars"] = "direct_inv"           # (misses the LU-based direct bar with no defect found: inverse_residual_error)
        return c
    if name.startswith("f4_slack_pyy"):
        return _dd(name, 100, nslack=10, pyy=0.0 if name.endswith("pyy0") else 0.3)
    if name in ("f4_symv384", "f4_symv1152"):
        return _dd(name, int(name[7:]), env=dict(OSQP_AMD_DENSE_SYMV=1), symv=1)
    if name == "f4_vd":
        return _dd(name, 512, vd=1, nd=400, row_len=512)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# the direct forms' host-side classification, restated
# ---------------------------------------------------------------------------------------------------------------
def bd_structure(c):
    """build_blockdirect from (triu(P), A): dict(blocks: dense diagonal blocks when they tile 0..n, else 0; kc: coupling rows of the
    coupled form, 0 in the plain form (every row one entry, but for at most four huge rows, all folded); folded; eligible)."""
    dense = PC.dense_blocks(c["Pu"])
    tiles, nxt = True, 0
    for c0, b, _ in dense:
        tiles, nxt = tiles and c0 == nxt, c0 + b
    tiles = tiles and nxt == c["n"]
    lenA = np.diff(sparse.csr_matrix(c["A"]).indptr)
    huge = np.flatnonzero(lenA >= PC.HUGE_ROW)
    folded = huge if huge.size <= PC.MAX_HUGE_FOLD else huge[:0]
    rest = np.setdiff1d(np.arange(c["m"]), folded)
    plain = tiles and folded.size == huge.size and bool(np.all(lenA[rest] == 1))
    crows = np.flatnonzero(lenA >= 2)
    coupled = tiles and not plain and 0 < crows.size <= CPL_MAX
    return dict(blocks=len(dense) if tiles else 0, kc=int(crows.size) if coupled else 0, folded=int(folded.size), eligible=bool(plain or coupled),
                fin_dots=int(folded.size > 0 and folded.size == huge.size))


def dd_structure(c):
    """build_dense_direct from (triu(P), A): dict(na dense unknowns, nap, nb2 unknowns that leave by the sparse Schur complement, nd
    dense rows (>= 32 entries on variables that are not eliminated), nnzA, vd: the one-gather start-up is live)."""
    Pu, Ac, Ar = sparse.csc_matrix(c["Pu"]), sparse.csc_matrix(c["A"]), sparse.csr_matrix(c["A"])
    n, m = c["n"], c["m"]
    erow, _ = EC.eliminated(Pu, Ac)
    gone = erow >= 0
    isdense, indense = np.zeros(m, bool), np.zeros(n, bool)
    for i in range(m):
        cols = Ar.indices[Ar.indptr[i]:Ar.indptr[i + 1]]
        if int((~gone[cols]).sum()) >= DD_DENSE_ROW:
            isdense[i] = True
            indense[cols] = True
    coupled = np.zeros(n, bool)
    pcol = np.repeat(np.arange(n), np.diff(Pu.indptr))
    off = Pu.indices != pcol
    coupled[Pu.indices[off]] = True
    coupled[pcol[off]] = True
    blocked, chosen = np.zeros(n, bool), np.zeros(n, bool)
    for j in range(n):
        if gone[j] or indense[j] or coupled[j] or blocked[j]:
            continue
        nb, ok = [], True
        for i in Ac.indices[Ac.indptr[j]:Ac.indptr[j + 1]]:
            for v in Ar.indices[Ar.indptr[i]:Ar.indptr[i + 1]]:
                if v == j or gone[v]:
                    continue
                if chosen[v]:
                    ok = False
                    break
                if v not in nb:
                    nb.append(int(v))
                    if len(nb) > DD_NBR:
                        ok = False
                        break
            if not ok:
                break
        if ok:
            chosen[j] = True
            blocked[nb] = True
    na = int((~gone & ~chosen).sum())
    return dict(na=na, nap=-(-na // DD_NB) * DD_NB, nb2=int(chosen.sum()), nd=int(isdense.sum()), nnzA=int(Ac.nnz), vd=int(Ac.nnz >= 2e5),
                gone={int(j): int(erow[j]) for j in np.flatnonzero(gone)})


# ---------------------------------------------------------------------------------------------------------------
# the data an engine holds, and the host calls as data
# ---------------------------------------------------------------------------------------------------------------
def scaled(c, passes=10):
    """`cur` of the case after the reference's Ruiz sweeps (float64 copies), for the CPU tests; the GPU tests build theirs from what
    hipeng_ruiz_scale returned."""
    r = R.ruiz(c["Pu"], c["A"], c["q"], c["l"], c["u"], passes)
    f = lambda k: r[k].astype(float)
    return dict(Px=f("Px"), Ax=f("Ax"), q=f("q"), l=f("l"), u=f("u"), rho=c["rho"].copy(), sigma=R.SIGMA, D=f("D"), E=f("E"))


def matrices(c, cur):
    Pu, A = c["Pu"].copy(), c["A"].copy()
    Pu.data, A.data = cur["Px"].copy(), cur["Ax"].copy()
    return Pu, A


def problem(c, cur):
    Pu, A = matrices(c, cur)
    return R.Problem(Pu, A, cur["q"], cur["l"], cur["u"], cur["D"], cur["E"])


OPS = ("q", "bounds", "bounds+rho", "rho", "matrices", "changed", "sigma", "cold", "kkt", "warm_x", "warm_y", "set_z")
LARGE_OPS = ("q", "rho", "matrices")
# In both orders a call that changes rho or A is followed, one step later, by one that leaves the start vector alone (rho -> q,
# matrices -> bounds; bounds+rho -> sigma, matrices -> q): the step after the second call starts from the vector that the first
# step after the reset extrapolated.
ORDERS = (("q", "changed", "rho", "q", "matrices", "bounds", "cold", "kkt", "sigma", "bounds+rho", "warm_x", "warm_y", "set_z"),
          ("sigma", "kkt", "set_z", "bounds+rho", "sigma", "warm_y", "cold", "matrices", "q", "warm_x", "rho", "changed", "bounds"))


LARGE_ORDERS = (("q", "rho", "q", "matrices"), ("matrices", "q", "rho"))


def orders(c):
    """The two orders of host calls a case runs: every call of OPS, or LARGE_OPS on the n = 8192 cases."""
    assert all(set(o) == set(OPS) for o in ORDERS) and all(set(o) == set(LARGE_OPS) for o in LARGE_ORDERS)
    return LARGE_ORDERS if c["claims"]["large"] else ORDERS


def op_changes(op, c, cur, xyz, rng):
    """What the host call `op` changes: (data: the new values of the keys of `cur` it replaces, iterates: None, ("cold",),
    ("kkt", b, (x, y, z)), ("x", x), ("y", y) or ("z", z)).  Magnitudes are chosen so that each one-place defect of defects()
    misses the step bars by more than 10 x (tests/test_form_cases_host.py)."""
    n, m = c["n"], c["m"]
    x, y, z = xyz
    if op == "q":
        return dict(q=cur["q"] * rng.uniform(0.5, 1.5, n) + 0.1 * rng.standard_normal(n)), None
    if op == "bounds":                               # values only: every finite bound moves, an equality stays one
        l, u = cur["l"].copy(), cur["u"].copy()
        eq, fin = l == u, (np.abs(l) < 1e20) & (np.abs(u) < 1e20)
        s = rng.uniform(-0.3, 0.3, m)
        l[eq], u[eq] = l[eq] + s[eq], l[eq] + s[eq]
        rg = fin & ~eq
        l[rg], u[rg] = l[rg] - rng.uniform(0.05, 0.3, m)[rg], u[rg] + rng.uniform(0.05, 0.3, m)[rg]
        return dict(l=l, u=u), None
    if op == "bounds+rho":                           # an equality row becomes a range and the reverse, each with the rho of its new class
        l, u, rho = cur["l"].copy(), cur["u"].copy(), cur["rho"].copy()
        eq = np.flatnonzero(l == u)
        rg = np.flatnonzero((l < u) & (np.abs(l) < 1e20) & (np.abs(u) < 1e20))
        i, j = int(eq[0]), int(rg[0])
        l[i], u[i], rho[i] = l[i] - 0.3, u[i] + 0.2, RHO
        u[j], rho[j] = l[j], EQ * RHO
        return dict(l=l, u=u, rho=rho), None
    if op == "rho":
        rho = 10.0 ** rng.uniform(-3.0, 3.0, m)
        rho[0], rho[-1] = 1e-3, 1e3
        return dict(rho=rho), None
    if op == "matrices":                             # _changed_matrices of tests/test_gpu_pcg_edges.py, on the values held now
        s = np.sqrt(rng.choice([0.9, 1.1], n))
        Pu, A = sparse.csc_matrix(c["Pu"]), sparse.csc_matrix(c["A"])
        pcol = np.repeat(np.arange(n), np.diff(Pu.indptr))
        return dict(Px=cur["Px"] * s[Pu.indices] * s[pcol], Ax=cur["Ax"] * rng.choice([0.9, 1.1], A.nnz)), None
    if op == "changed":
        return {}, None
    if op == "sigma":
        return dict(sigma={1e-6: 1e-3, 1e-3: 1e-5}.get(cur["sigma"], 1e-3)), None
    if op == "cold":
        return {}, ("cold",)
    if op == "kkt":
        return {}, ("kkt", rng.standard_normal(n + m), (rng.standard_normal(n), 0.05 * rng.standard_normal(m), rng.standard_normal(m)))
    if op == "warm_x":
        return {}, ("x", x + 0.3 * rng.standard_normal(n))
    if op == "warm_y":
        return {}, ("y", y + 0.05 * rng.standard_normal(m))
    if op == "set_z":
        return {}, ("z", z + 0.3 * rng.standard_normal(m))
    raise KeyError(op)


# ---------------------------------------------------------------------------------------------------------------
# float64 model of the device's step
# ---------------------------------------------------------------------------------------------------------------
class _Op:
    """P, A as float64 CSR and a solver of K = P + sigma I + A' rho A (dense LU up to 3000 variables, else a sparse LU of the
    quasi-definite form)."""

    def __init__(self, c, cur):
        Pu, A = matrices(c, cur)
        self.P = (Pu + sparse.triu(Pu, 1, format="csc").T).tocsr()
        self.A = sparse.csr_matrix(A)
        self.AT = self.A.T.tocsr()
        self.rho, self.sigma, self.n = cur["rho"], cur["sigma"], c["n"]
        self._lu = None

    def solve(self, r):
        n = self.n
        if self._lu is None:
            if n <= R.DENSE_MAX:
                K = (self.P + self.sigma * sparse.eye(n) + self.AT @ sparse.diags(self.rho) @ self.A).toarray()
                self._lu = sla.lu_factor(K, check_finite=False)
            else:
                self._lu = spla.splu(sparse.bmat([[self.P + self.sigma * sparse.eye(n), self.AT], [self.A, -sparse.diags(1.0 / self.rho)]], format="csc"))
        if n <= R.DENSE_MAX:
            return sla.lu_solve(self._lu, r, check_finite=False)
        pad = np.zeros(self.A.shape[0])
        v = self._lu.solve(np.concatenate([r, pad]))[:n]          # (one refinement step: the model is exact algebra, not the bar's yardstick)
        return v + self._lu.solve(np.concatenate([r - (self.P @ v + self.sigma * v + self.AT @ (self.rho * (self.A @ v))), pad]))[:n]


def cond_K(c, cur):
    """cond_2 of K = P + sigma I + A' rho A: dense eigenvalues up to 3000 variables; above, Lanczos for the largest eigenvalue of K and
    of K^-1 (through the sparse LU of the quasi-definite form, as _engine_reference does for lam_min)."""
    op = _Op(c, cur)
    n = c["n"]
    if n <= R.DENSE_MAX:
        w = np.linalg.eigvalsh((op.P + op.sigma * sparse.eye(n) + op.AT @ sparse.diags(op.rho) @ op.A).toarray())
        return float(w[-1] / w[0])
    K = spla.LinearOperator((n, n), matvec=lambda v: op.P @ v + op.sigma * v + op.AT @ (op.rho * (op.A @ v)), dtype=float)
    Ki = spla.LinearOperator((n, n), matvec=op.solve, dtype=float)
    hi = spla.eigsh(K, k=1, which="LA", tol=1e-6, return_eigenvectors=False)[0]
    lo = spla.eigsh(Ki, k=1, which="LA", tol=1e-6, return_eigenvectors=False)[0]
    return float(hi * lo)


def inverse_residual_error(c, cur, st, x, z, y, vn):
    """2-norm error of x~ = v_n + K^-1 r when the float64 explicit inverse of K (LAPACK) multiplies the float64 residual
    r = b - K v_n of the start vector [v_n | rho A v_n] the engine holds, against the refined x~ of the reference step `st`: what
    the direct forms' arithmetic costs when nothing is wrong.  With a start vector extrapolated while the iterates still jump,
    ||r|| is several times ||b|| (theta = 1 at the third solve: 6 x), and this error several times that of an LU solve of K x~ = b,
    the yardstick of _engine_reference.step_bars(direct=True).  Computed from the reference alone."""
    op = _Op(c, cur)
    n = c["n"]
    K = (op.P + op.sigma * sparse.eye(n) + op.AT @ sparse.diags(op.rho) @ op.A).toarray()
    b = cur["sigma"] * np.asarray(x, float) - cur["q"] + op.AT @ (cur["rho"] * np.asarray(z, float) - np.asarray(y, float))
    vn = np.asarray(vn, float)
    r = b - K @ vn
    xt = vn + np.linalg.inv(K) @ r
    d = xt.astype(LD) - st["x_tilde"]
    return float(np.sqrt((d * d).sum()))


def theta(hist, sched):
    return 0.0 if hist < sched[0] else (0.5 if hist < sched[1] else 1.0)


class Sim:
    """What the engine holds, in float64: the data `cur`, the iterates x, z, y, x~ and z~ of the last solve (va, zt), the start
    vector (vn, vm) of the next one (vx), the previous [x~ | rho z~] (on, om: vold) and the count of solves since the start
    vector's history was reset (hist_r).  The step it models (k_pcg_init, the solve, k_admm_finalize):
        b = sigma x - q + A'(rho z - y);  r = b - (P + sigma I) vn - A' vm;  x~ = vn + K^-1 r;  z~ = A x~
        x+ = alpha x~ + (1 - alpha) x;  z+ = clip(alpha z~ + (1 - alpha) z + y / rho);  y+ = y + rho (alpha z~ + (1 - alpha) z - z+)
        next start vector [x~ | rho z~] + theta (that - the previous one), theta from the schedule at hist_r.
    An exact K^-1 makes x~ independent of a start vector with vm = rho A vn; the defects below are the ways in which it is not."""

    def __init__(self, c, cur, sched=(1, 2), alpha=ALPHA):
        self.c, self.cur, self.sched, self.alpha = c, dict(cur), sched, alpha
        self.op = _Op(c, self.cur)
        n, m = c["n"], c["m"]
        self.x, self.y, self.z, self.xt, self.zt = np.zeros(n), np.zeros(m), np.zeros(m), np.zeros(n), np.zeros(m)
        self.reset()

    def reset(self):
        """reset_start after k_refresh_m: the start vector and the previous vector are [x~ | rho z~] of the data held now."""
        self.vn, self.vm = self.xt.copy(), self.cur["rho"] * self.zt
        self.on, self.om = self.vn.copy(), self.vm.copy()
        self.hist, self.ext = 0, None

    def set_iterates(self, x=None, y=None, z=None):
        if y is not None:
            self.y = np.array(y, float)
        if x is not None:
            self.x = np.array(x, float)
            self.xt = self.x.copy()
            self.z = self.op.A @ self.x
            self.zt = self.z.copy()
        if z is not None:
            self.z = np.array(z, float)
        self.reset()

    def apply(self, op, data, it, stale_vold=False):
        """The host call: returns the snapshot of what was held before it (for defects()).  stale_vold: the planted defect of a
        reset_start that leaves the previous vector (vold) as it was."""
        old = dict(cur=dict(self.cur), op=self.op, zt=self.zt.copy(), vn=self.vn.copy(), vm=self.vm.copy(), on=self.on.copy(), om=self.om.copy(),
                   xt=self.xt.copy(), hist=self.hist)
        self.cur.update(data)
        if any(k in data for k in ("Px", "Ax", "rho", "sigma")):
            self.op = _Op(self.c, self.cur)
        if "Ax" in data or op == "changed":
            self.zt = self.op.A @ self.xt
        eliminated = bool(self.c["claims"].get("gone"))
        if any(k in data for k in ("Px", "Ax", "rho")) or op == "changed" or ("sigma" in data and eliminated):
            self.reset()
        if it is not None:
            if it[0] == "cold":
                n, m = self.c["n"], self.c["m"]
                self.x, self.y, self.z, self.xt, self.zt = np.zeros(n), np.zeros(m), np.zeros(m), np.zeros(n), np.zeros(m)
                self.reset()
            elif it[0] == "kkt":
                self.set_iterates(*[it[2][k] for k in (0, 1, 2)])
            else:
                self.set_iterates(**{it[0]: it[1]})
        if stale_vold:
            self.on, self.om = old["on"], old["om"]
        return old

    def solve_step(self, q=None, lu=None, Kop=None, vn=None, vm=None, without_vn=False):
        """(x+, z+, y+, x~, z~) of the step from what is held, with the named pieces replaced."""
        cur, op, al = self.cur, self.op, self.alpha
        rho = cur["rho"]
        vn, vm = self.vn if vn is None else vn, self.vm if vm is None else vm
        b = cur["sigma"] * self.x - (cur["q"] if q is None else q) + op.AT @ (rho * self.z - self.y)
        r = b - (op.P @ vn + cur["sigma"] * vn) - op.AT @ vm
        xt = (0.0 if without_vn else vn) + (op if Kop is None else Kop).solve(r)
        zt = op.A @ xt
        l, u = (cur["l"], cur["u"]) if lu is None else lu
        w = al * zt + (1 - al) * self.z
        zn = np.minimum(np.maximum(w + self.y / rho, l), u)
        return al * xt + (1 - al) * self.x, zn, self.y + rho * (w - zn), xt, zt

    def step(self):
        x, z, y, xt, zt = self.solve_step()
        self.hist += 1
        th = theta(self.hist, self.sched)
        rz = self.cur["rho"] * zt
        self.vn, self.vm = xt + th * (xt - self.on), rz + th * (rz - self.om)
        self.ext = (rz, self.om, th)
        self.on, self.om = xt, rz
        self.x, self.z, self.y, self.xt, self.zt = x, z, y, xt, zt
        return x, z, y

    def defects(self, old):
        """{label: (x+, z+, y+)} of the one-place defects that the host call just applied could leave behind; a defect whose wrong
        piece equals the right one after this call (the old q after a call that did not touch q) cannot show and is left out."""
        cur, o = self.cur, old["cur"]
        out = {}
        differs = lambda a, b: a.shape != b.shape or bool(np.any(a != b))
        if differs(cur["q"], o["q"]):
            out["old q in b"] = self.solve_step(q=o["q"])
        if differs(cur["l"], o["l"]) or differs(cur["u"], o["u"]):
            out["old l, u in the clip"] = self.solve_step(lu=(o["l"], o["u"]))
        for key, label in ((("rho",), "old rho in K^-1"), (("Px", "Ax"), "old P, A in K^-1"), (("sigma",), "old sigma in K^-1")):
            if any(differs(np.atleast_1d(cur[k]), np.atleast_1d(o[k])) for k in key):
                mix = dict(cur)
                mix.update({k: o[k] for k in key})
                out[label] = self.solve_step(Kop=_Op(self.c, mix))
        if differs(cur["rho"], o["rho"]):
            out["old rho in v_m"] = self.solve_step(vm=o["rho"] * self.zt)
        if differs(cur["Ax"], o["Ax"]):
            out["old A in v_m"] = self.solve_step(vm=cur["rho"] * (old["op"].A @ self.xt))
        if differs(self.zt, old["zt"]):
            out["z~ from before the call"] = self.solve_step(vm=cur["rho"] * old["zt"])
        if self.hist == old["hist"] and self.ext is not None and self.ext[2] == 1.0:      # no reset: the start vector is the extrapolated one
            rz, om, _ = self.ext
            out["v_n with theta 1, v_m with 0.5"] = self.solve_step(vm=rz + 0.5 * (rz - om))
        if np.any(self.vn != 0.0):
            out["x~ = K^-1 r without v_n"] = self.solve_step(without_vn=True)
        return {k: v[:3] for k, v in out.items()}
