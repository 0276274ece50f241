"""Planted QPs on the structured problems of the per-form linear-solve tests, for the KKT instance that polish and the solution
derivatives build (kkt_instance in osqp_host.c): a second engine on (P~, A~[active rows]) with rho = 1 / d on every row, sigma = d,
d = max(delta, 1e-3), which chooses its linear-solve form from (P, A_red) on its own.  tests/test_kkt_instance_cases_host.py proves
the cases on the CPU, tests/test_gpu_kkt_instance_forms.py runs them on the device.  Plain numpy and scipy; nothing here touches
the library.

A case keeps the pattern and the values of (P, A) of its builder (_direct_problems.bd_problem / dd_problem, _pcg_cases.make,
br_probe and _blocks_with_rows, _engine_reference.make_case) and replaces q, l, u by planted ones (_planted_qp._plant: x* standard
normal, |y*| in [0.5, 2] on the active rows with the sign of the bound, gaps of 0.5 .. 1 elsewhere, kinds in turn).  It is shaped
like a one-member case of _planted_qp.py (B = 1), so member(), _planted_qp.member_inc and _single_sens_reference.member_qp serve it.

Active rows are independent by construction: `pick` accepts a row only if it holds a column that no row accepted before it
touches (a triangular structure), and `peels` checks the same of a finished set in any order.

  env       the environment the handle is set up in: the switches of _form_cases (both engines read them)
  settings  OSQP settings next to polish = 1
  claims    what the instance is, from the host restatements applied to (P, A[active rows]) -- instance_claims():
            form (hipeng_resident_info [9]), info {slot: value}, layout {name: value} (hipeng_pcg_layout), elim
            (hipeng_elim_count).  `main` holds the same of (P, A), `differs` the keys in which the case says the two differ.
            The resident kernel's E has no host restatement: form only, the test prints the slot.

Truth: _planted_qp.Route / true_polish / adjoint_from / tangent_from.  At n = 8192 the member holds its matrices sparse and
SparseRoute factors M by a sparse LU and forms the refinement residual in long double from the COO triplets; the stop rule is
Route.solve_true's.

Conditioning: COND[name] is cond_2(P~ + d I + A~r' A~r / d) on the oracle's scaled data, the matrix a PCG form of the instance
iterates on; COND_CAP is the largest value of the same quantity over the members tests/test_gpu_single_sens.py already runs on the
PCG paths (PLANTED_MEMBERS and RANDOM_QP of _single_sens_reference.py).  Every case on a PCG form (0, 1, 2) lies at or below the
cap.  The host test recomputes both."""
import functools
from types import SimpleNamespace

import numpy as np
from scipy import sparse
from scipy.sparse import linalg as spla

import _planted_qp as pq
from tests import _direct_problems as DP
from tests import _elim_cases as EC
from tests import _engine_reference as R
from tests import _form_cases as FC
from tests import _pcg_cases as PC

LD = np.longdouble
MAX_PARTS, TB = 1024, 256                  # engine_device.h: the grid cap of k_sens_grad / k_sens_tan_rhs, threads per workgroup
SPARSE_ABOVE = 3000                        # members above this n hold their matrices sparse
F1_ENV = lambda nwg: dict(OSQP_AMD_DENSE_DIRECT=0, OSQP_AMD_RESIDENT_MIN_N=1, OSQP_AMD_RESIDENT_NWG=nwg, OSQP_AMD_RESIDENT_PIPE=1)

NAMES = ("ki_f0_blocks", "ki_f0_long_on", "ki_f0_long_off", "ki_f1_e8", "ki_f1_e20", "ki_f2_nh0", "ki_f3_plain", "ki_f3_kc16",
         "ki_f3_kc17", "ki_f3_kc0", "ki_f3_huge1", "ki_f0_huge1", "ki_f4_b2", "ki_f4_slack", "ki_mred0", "ki_all_eq")
LARGE = ("ki_f3_huge1", "ki_f0_huge1")
SEEDS = {name: 901 + k for k, name in enumerate(NAMES)}
KC_MAIN = 33                               # coupling rows of the main problem of ki_f3_kc*
HUGE_MAIN = 33                             # huge rows of the main problem of ki_f3_huge1: nnz(A) > MAX_PARTS * TB

# cond_2(P~ + d I + A~r' A~r / d), d = 1e-3, on the oracle's scaled data (tests/test_kkt_instance_cases_host.py recomputes them)
COND_CAP = 1.266e5                         # the largest over PLANTED_MEMBERS and RANDOM_QP: ("rows", 0)
COND = {"ki_f0_blocks": 1.261e5, "ki_f0_long_on": 1.042e4, "ki_f0_long_off": 8.893e3, "ki_f1_e8": 8.337e4, "ki_f1_e20": 8.260e4,
        "ki_f2_nh0": 1.247e4, "ki_f3_plain": 1.044e4, "ki_f3_kc16": 2.970e4, "ki_f3_kc17": 3.531e4, "ki_f3_kc0": 1.088e4,
        "ki_f3_huge1": 1.012e5, "ki_f0_huge1": 6.836e4, "ki_f4_b2": 6.596e5, "ki_f4_slack": 2.454e5, "ki_mred0": 2.790e1,
        "ki_all_eq": 3.257e5}          # (the direct forms 3 and 4 are not bound by the cap)


# ---------------------------------------------------------------------------------------------------------------
# independent rows by construction
# ---------------------------------------------------------------------------------------------------------------
def pick(A, candidates, count=None, touched=()):
    """Rows of `candidates`, in that order, each accepted only if it holds a column that no accepted row (and no column of
    `touched`) touches: row k of the result has an entry where rows 0 .. k-1 have none, so they are independent.  Stops at
    `count` rows (None: as many as the order gives)."""
    A = sparse.csr_matrix(A)
    used = np.zeros(A.shape[1], bool)
    used[np.asarray(touched, int)] = True
    out = []
    for i in candidates:
        if count is not None and len(out) == count:
            break
        cols = A.indices[A.indptr[i]:A.indptr[i + 1]]
        if cols.size and not used[cols].all():
            out.append(int(i))
            used[cols] = True
    assert count is None or len(out) == count, (count, len(out))
    return out


def peels(A, rows):
    """Can the rows be removed one at a time, each holding a column that no remaining row touches?  Then they are independent."""
    S = sparse.csr_matrix(A)[np.asarray(rows, int)]
    S = sparse.csr_matrix((np.ones(S.nnz), S.indices, S.indptr), shape=S.shape)
    left = np.ones(S.shape[0], bool)
    while left.any():
        cnt = np.asarray(S[left].sum(axis=0)).ravel()
        alone = sparse.csr_matrix(S @ sparse.diags((cnt == 1).astype(float)))
        free = left & (np.diff(alone.indptr) > 0) & (np.asarray(alone.sum(axis=1)).ravel() > 0)
        if not free.any():
            return False
        left &= ~free
    return True


# ---------------------------------------------------------------------------------------------------------------
# the host restatements, applied to the instance
# ---------------------------------------------------------------------------------------------------------------
def _as_case(Pu, A):
    Pu, A = sparse.csc_matrix(Pu), sparse.csc_matrix(A)
    return dict(Pu=Pu, A=A, n=Pu.shape[0], m=A.shape[0])


# the engine's defaults of the switches the rule below reads (tests/test_engine_switches_host.py holds them to the engine's table)
SWITCH_DEFAULTS = dict(OSQP_AMD_RESIDENT=1, OSQP_AMD_RESIDENT_BLOCKS=1, OSQP_AMD_BLOCK_DIRECT=1, OSQP_AMD_ELIM=1, OSQP_AMD_DENSE_DIRECT=1,
                       OSQP_AMD_DENSE_SMALL=1024, OSQP_AMD_RESIDENT_MIN_N=256)


def instance_claims(Pu, A, env):
    """Form, info slots, layout slots and eliminated count of an engine created on (triu(P), A) under `env`, in the order of
    hipeng_create: block-direct, block-resident, the elimination, dense-direct for at most OSQP_AMD_DENSE_SMALL (1024) dense
    unknowns, the resident PCG, dense-direct where it pays (OSQP_AMD_DENSE_DIRECT=2: whenever it fits), else the launch-per-step
    kernels.  The restatements are _form_cases.bd_structure / dd_structure, _pcg_cases.structure and _elim_cases.eliminated.
    Whether the resident plan holds K is the device's own (hipeng_resident_plan): where the rule reaches it, form 1 is claimed."""
    c = _as_case(Pu, A)
    n, m = c["n"], c["m"]
    on = lambda k: int(env.get(k, SWITCH_DEFAULTS[k]))
    res, blocks = on("OSQP_AMD_RESIDENT") != 0, on("OSQP_AMD_RESIDENT") != 0 and on("OSQP_AMD_RESIDENT_BLOCKS") != 0
    bd = FC.bd_structure(c)
    st = PC.structure(c)
    layout = dict(dense=len(st["dense"]), dense_rows=st["dense_rows"], long=len(st["long"]), huge=len(st["huge"]), folded=st["folded"])
    plain = bd["blocks"] > 0 and bd["eligible"] and bd["kc"] == 0
    if blocks and on("OSQP_AMD_BLOCK_DIRECT") != 0 and bd["eligible"]:
        return dict(form=3, info={3: bd["blocks"], 15: bd["kc"]}, layout=layout, elim=0)
    if blocks and plain:
        return dict(form=2, info={2: 64}, layout=layout, elim=0)
    erow, _ = EC.eliminated(c["Pu"], c["A"]) if on("OSQP_AMD_ELIM") != 0 else (np.full(n, -1), None)
    elim = int((erow >= 0).sum())
    dd = FC.dd_structure(c) if m and on("OSQP_AMD_DENSE_DIRECT") != 0 else None
    d4 = lambda: dict(form=4, info={3: dd["na"], 15: dd["nb2"]}, layout=layout, elim=elim, nd=dd["nd"])
    if dd is not None and 0 < dd["na"] <= on("OSQP_AMD_DENSE_SMALL"):
        return d4()
    if res and on("OSQP_AMD_RESIDENT_MIN_N") <= n <= 15616 and not st["huge"]:
        return dict(form=1, info={}, layout=layout, elim=elim)
    if dd is not None and on("OSQP_AMD_DENSE_DIRECT") == 2 and 0 < dd["na"] <= 8192:
        return d4()
    return dict(form=0, info={1: 0, 2: 0, 3: 0}, layout=layout, elim=elim)


# ---------------------------------------------------------------------------------------------------------------
# planting
# ---------------------------------------------------------------------------------------------------------------
def _planted(name, Pu, A, rows, env, settings=None, equalities=(), differs=(), about=""):
    """The case: (P, A) as given, q, l, u planted on the active rows `rows` (`equalities` among them are equality rows, the
    others take the kinds in turn)."""
    rng = np.random.default_rng(SEEDS[name])
    P, A = sparse.csc_matrix(Pu), sparse.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    n, m = P.shape[0], A.shape[0]
    rows = np.array(sorted(int(r) for r in rows), np.int64)
    assert np.unique(rows).size == rows.size and set(equalities) <= set(rows.tolist())
    kinds = None
    if len(equalities):
        kinds, k = [], 0
        for r in rows:
            kinds.append(0 if r in equalities else k % 3)
            k += r not in equalities
    q, l, u, x, y, act = pq._plant(rng, P, A, rows, "mixed", kinds)
    g = np.random.default_rng(SEEDS[name] + 4242)
    draw = lambda *s: g.standard_normal(s)
    inc = SimpleNamespace(gx=draw(1, n), gy=draw(1, m), dQ=draw(1, pq.NDIR, n), dL=draw(1, pq.NDIR, m), dU=draw(1, pq.NDIR, m),
                          dPx=draw(1, pq.NDIR, P.nnz), dAx=draw(1, pq.NDIR, A.nnz))
    Ar = sparse.csr_matrix(A)[rows]
    return SimpleNamespace(name=name, n=n, m=m, B=1, P=P, A=A, Px_all=P.data[None, :].copy(), Ax_all=A.data[None, :].copy(),
                           Q=q[None], L=l[None], U=u[None], x=x[None], y=y[None], act=act[None], inc=inc, rows=rows,
                           env=dict(env), settings=dict(settings or {}), large=name in LARGE, about=about, differs=tuple(differs),
                           claims=instance_claims(P, Ar, env), main=instance_claims(P, A, env))


def _third(rng, items):
    items = list(items)
    return [items[k] for k in sorted(rng.permutation(len(items))[: max(1, len(items) // 3)])]


@functools.lru_cache(maxsize=None)
def make(name):
    rng = np.random.default_rng(SEEDS[name] + 7)
    if name == "ki_f0_blocks":
        # blocks_mixed: 2-3-entry rows over a permutation of the variables (disjoint supports), then four single-entry rows per block
        b = PC.make("blocks_mixed")
        lenA = np.diff(sparse.csr_matrix(b["A"]).indptr)
        multi, single = np.flatnonzero(lenA > 1), np.flatnonzero(lenA == 1)
        rows = pick(b["A"], list(multi[::3]) + list(single), count=len(multi[::3]) + 12)
        return _planted(name, b["Pu"], b["A"], rows, FC.STEPS, about="dense blocks of P kept, about a third of the rows active")
    if name in ("ki_f0_long_on", "ki_f0_long_off"):
        # "long": rows 0, 1 of A hold 512 and 513 entries; every row holds column 0, so that column is spent from the start
        b = R.make_case("long")
        short = [int(i) for i in rng.permutation(np.arange(3, 39))]
        rows = pick(b["A"], ([0] if name.endswith("_on") else []) + short, count=13, touched=[0])
        # scaling = 0: the case's A[39, 0] = 50 and P[63, 63] = 40 make Ruiz shrink the cost to c = 1.5e-2 and D to 0.14, P~ falls
        # below d on part of the null space of the active rows, the refinement contracts by 0.6 a step and the route model itself
        # ends 7e-7 from the truth after its 15 steps (cond 3.8e6, above the cap); on the raw data it takes 4 steps (cond 1e4)
        return _planted(name, b["Pu"], b["A"], rows, dict(FC.STEPS, OSQP_AMD_SPLIT=1), settings=dict(scaling=0), differs=() if name.endswith("_on") else ("long",),
                        about="the long row 0 of A active (instance layout long >= 1)" if name.endswith("_on")
                        else "no long row active: instance layout long == 0, the main engine still has two")
    if name in ("ki_f1_e8", "ki_f1_e20"):
        b = PC.make("res_e%s" % name[7:])
        rows = pick(b["A"], rng.permutation(b["m"]), count=b["m"] // 3)
        return _planted(name, b["Pu"], b["A"], rows, F1_ENV(b["claims"]["nwg"]), about="resident PCG, E = %s in the main engine" % name[7:])
    if name == "ki_f2_nh0":
        b = PC.br_probe()
        return _planted(name, b["Pu"], b["A"], _third(rng, range(b["m"])), FC.BLOCKRES, about="block-resident, rows inside blocks active")
    if name == "ki_f3_plain":
        Pu, A, _ = DP.bd_problem(FC.BD_BLOCKS, seed=SEEDS[name])
        return _planted(name, Pu, A, _third(rng, range(A.shape[0])), FC.BD_ENV, about="only single-block rows, a third of them active")
    if name in ("ki_f3_kc16", "ki_f3_kc17", "ki_f3_kc0"):
        # one main problem for the three: a single-entry row per variable, then KC_MAIN coupling rows of 2-6 entries
        Pu, A, _ = DP.bd_problem(FC.BD_BLOCKS, seed=SEEDS["ki_f3_kc16"], kc=KC_MAIN)
        n = Pu.shape[0]
        kc = int(name[8:])
        crng = np.random.default_rng(SEEDS["ki_f3_kc16"] + 7)
        cpl = pick(A, [int(i) for i in n + crng.permutation(KC_MAIN)], count=kc) if kc else []
        Ar = sparse.csr_matrix(A)
        spent = np.unique(np.concatenate([Ar.indices[Ar.indptr[i]:Ar.indptr[i + 1]] for i in cpl])) if cpl else np.zeros(0, int)
        singles = _third(crng, np.setdiff1d(np.arange(n), spent))        # (row j is the single-entry row of variable j)
        return _planted(name, Pu, A, cpl + singles, FC.BD_ENV, differs=("kc",),
                        about="%d of the main problem's %d coupling rows active: instance info[15] = %d" % (kc, KC_MAIN, kc))
    if name in LARGE:
        # dense blocks of 128, a box row per variable, then huge rows over every variable; the first huge row is an active equality
        nh = HUGE_MAIN if name == "ki_f3_huge1" else 1
        b = PC._blocks_with_rows(name, np.random.default_rng(SEEDS[name]), [128] * 64, nh)
        n = b["n"]
        rows = _third(rng, range(n)) + [n]
        env = FC.BD_ENV if name == "ki_f3_huge1" else FC.STEPS
        return _planted(name, b["Pu"], b["A"], rows, env, equalities=(n,), differs=("kc",) if nh > 1 else (),
                        about="n = 8192, one huge equality row active" + (", %d more in the main problem: nnz(A) > MAX_PARTS * 256" % (nh - 1) if nh > 1 else
                                                                         ", folded into k_cg_B on the launch-per-step kernels"))
    if name == "ki_f4_b2":
        # 100 core variables, 3 dense rows (0..2), 25 short rows (3..27), then two rows each for four more variables with 0, 3, 8 and
        # 12 core neighbours (rows 28..35).  Active: dense row 0 alone of the dense ones; both rows of the 3-neighbour variable; one
        # row of the 8-neighbour variable (the instance eliminates it); neither row of the other two.
        Pu, A, _ = DP.dd_problem(100, seed=SEEDS[name], nd=3, b2_nbrs=(0, 3, 8, 12))
        rows = pick(A, [30, 31, 32, 0] + [int(i) for i in 3 + rng.permutation(25)], count=14)
        return _planted(name, Pu, A, rows, FC.DD_ENV, differs=("na", "nd", "elim"),
                        about="dense-direct with B2 neighbours; one of three dense rows active, a B2 variable of the main engine eliminated")
    if name == "ki_f4_slack":
        # 10 slacks with P_yy = 0 stored, each in a row of its own (rows m-10 .. m-1): all ten rows active equalities
        Pu, A, _ = DP.dd_problem(100, seed=SEEDS[name], nslack=10, pyy=0.0)
        m = A.shape[0]
        slack = list(range(m - 10, m))
        rows = pick(A, slack + [int(i) for i in 1 + rng.permutation(m - 11)], count=18)
        return _planted(name, Pu, A, rows, FC.DD_ENV, equalities=tuple(slack), about="nslack = 10, pyy = 0: every slack row an active equality, the instance eliminates the ten too")
    if name == "ki_mred0":
        Pu, A, _ = DP.dd_problem(100, seed=SEEDS[name])
        return _planted(name, Pu, A, [], {}, differs=("form",), about="no row active: an instance with m = 0")
    if name == "ki_all_eq":
        Pu, A, _ = DP.dd_problem(100, seed=SEEDS[name], nd=2, nshort=20)
        m = A.shape[0]
        return _planted(name, Pu, A, range(m), FC.DD_ENV, equalities=tuple(range(m)), about="m <= n, every row an active equality: the instance's A is A")
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# the truth
# ---------------------------------------------------------------------------------------------------------------
class SparseRoute(pq.Route):
    """Route with M held sparse: a sparse LU, and the refinement residual g - M x accumulated in long double from the COO
    triplets of M.  solve_true itself -- the stop rule -- is Route's."""

    def __init__(self, mem):
        n, k = mem.n, mem.rows.size
        Ar = sparse.csr_matrix(mem.Ad)[mem.rows]
        M = sparse.bmat([[sparse.csr_matrix(mem.Pf), Ar.T], [Ar, None]], format="coo") if k else sparse.coo_matrix(mem.Pf)
        self.n, self.k, self.M, self.Ar = n, k, M.tocsc(), Ar
        self._row, self._col, self._val = M.row, M.col, M.data.astype(LD)
        self._lu = self._Ml = None
        self._inv = {}

    def _factor(self):
        if self._lu is None:
            self._lu = spla.splu(self.M)

    def _lu_solve(self, v):
        return self._lu.solve(np.asarray(v, float))

    def _residual(self, gl, x):
        r = np.array(gl, LD)
        np.subtract.at(r, self._row, self._val * np.asarray(x, LD)[self._col])
        return r

    def residual_ld(self, x, g):
        return self._residual(np.asarray(g, LD), x)


def member(c, Pv=None, Av=None, act=None):
    """The case's one member as _planted_qp.member gives it; above SPARSE_ABOVE variables with Pf and Ad as CSR (mem.sparse).
    Pv / Av: other values on the same patterns; act: another active set (a row dropped)."""
    if act is not None:
        c = SimpleNamespace(**{**vars(c), "act": np.asarray(act, np.int64)[None]})
    if c.n <= SPARSE_ABOVE:
        mem = pq.member(c, 0, Pv=Pv, Av=Av)
        mem.sparse = False
        return mem
    n, m = c.n, c.m
    Pu = sparse.csc_matrix((c.Px_all[0] if Pv is None else np.asarray(Pv, float), c.P.indices, c.P.indptr), shape=(n, n))
    Ac = sparse.csc_matrix((c.Ax_all[0] if Av is None else np.asarray(Av, float), c.A.indices, c.A.indptr), shape=(m, n))
    a = c.act[0]
    low, upp = np.flatnonzero(a < 0), np.flatnonzero(a > 0)
    return SimpleNamespace(n=n, m=m, Pu=Pu, Ac=Ac, Pf=sparse.csr_matrix(Pu + sparse.triu(Pu, 1).T), Ad=sparse.csr_matrix(Ac), q=c.Q[0], l=c.L[0],
                           u=c.U[0], act=a, low=low, upp=upp, rows=np.concatenate([low, upp]).astype(np.int64), sparse=True,
                           Pi=Pu.indices, Pj=np.repeat(np.arange(n), np.diff(Pu.indptr)), Ai=Ac.indices, Aj=np.repeat(np.arange(n), np.diff(Ac.indptr)))


def outputs(c, mem):
    """Every output of the member from the refined solve: x, y, obj, dq, dl, du, dPx, dAx, dx, dy, with mem and route."""
    route = SparseRoute(mem) if mem.sparse else pq.Route(mem)
    pol = pq.true_polish(mem, route)
    inc = pq.member_inc(c, 0)
    adj = pq.adjoint_from(mem, pol.x, pol.y, inc.gx, inc.gy, route.solve_true)
    tan = pq.tangent_from(mem, pol.x, pol.y, inc, route.solve_true)
    return SimpleNamespace(mem=mem, route=route, **vars(pol), **vars(adj), **vars(tan))


_truths = {}


def truth(name):
    """The truth of the case (computed once, never modified)."""
    if name not in _truths:
        c = make(name)
        _truths[name] = outputs(c, member(c))
    return _truths[name]


OUTPUTS = pq.POLISH + pq.ADJOINT + pq.TANGENT


def mutations(c):
    """(label, member) of the three one-place changes the parity bar must not forgive: a relative change of 1e-4 to the diagonal
    value of P at the largest |x*_j|, the same to the entry of an active row of A with the largest |a_ij x*_j|, and one active row
    dropped (the one with the largest |y*| among those whose variables all have curvature in P).  Without active rows, the first alone."""
    x, y, a = c.x[0], c.y[0], c.act[0]
    Pj = np.repeat(np.arange(c.n), np.diff(c.P.indptr))
    diag = np.flatnonzero(c.P.indices == Pj)
    k = int(diag[np.abs(c.P.data[diag] * x[Pj[diag]]).argmax()])
    Pv = c.Px_all[0].copy(); Pv[k] *= 1.0 + 1e-4
    out = [("P[%d,%d] * (1 + 1e-4)" % (Pj[k], Pj[k]), member(c, Pv=Pv))]
    if a.any():
        Aj = np.repeat(np.arange(c.n), np.diff(c.A.indptr))
        w = np.where(a[c.A.indices] != 0, np.abs(c.A.data * x[Aj]), -1.0)
        k = int(w.argmax())
        Av = c.Ax_all[0].copy(); Av[k] *= 1.0 + 1e-4
        out.append(("A[%d,%d] * (1 + 1e-4)" % (c.A.indices[k], Aj[k]), member(c, Av=Av)))
        # (not a row that carries a variable without curvature in P, a slack with P_yy = 0: without it M is singular)
        flat = abs(sparse.csr_matrix(c.A)) @ (c.P.diagonal() == 0.0).astype(float) > 0
        i = int(np.abs(np.where((a != 0) & ~flat, y, 0.0)).argmax())
        a2 = a.copy(); a2[i] = 0
        out.append(("row %d dropped" % i, member(c, act=a2)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# conditioning
# ---------------------------------------------------------------------------------------------------------------
def cond_reduced(Pfs, Ars, delta=1e-3):
    """cond_2 of P~ + d I + A~r' A~r / d.  Dense eigenvalues up to SPARSE_ABOVE variables; above, Lanczos for the largest
    eigenvalue of the matrix and of its inverse (through a sparse LU of [P~ + d I, A~r'; A~r, -d I])."""
    n, k = Pfs.shape[0], Ars.shape[0]
    if n <= SPARSE_ABOVE:
        Pd = Pfs.toarray() if sparse.issparse(Pfs) else np.asarray(Pfs)
        Ad = Ars.toarray().reshape(k, n) if sparse.issparse(Ars) else np.asarray(Ars).reshape(k, n)
        w = np.linalg.eigvalsh(Pd + delta * np.eye(n) + Ad.T @ Ad / delta)
        return float(w[-1] / w[0])
    Pfs, Ars = sparse.csr_matrix(Pfs), sparse.csr_matrix(Ars)
    AT = Ars.T.tocsr()
    K = spla.LinearOperator((n, n), matvec=lambda v: Pfs @ v + delta * v + AT @ (Ars @ v) / delta, dtype=float)
    lu = spla.splu(sparse.bmat([[Pfs + delta * sparse.eye(n), AT], [Ars, -delta * sparse.eye(k)]], format="csc"))
    Ki = spla.LinearOperator((n, n), matvec=lambda v: lu.solve(np.concatenate([v, np.zeros(k)]))[:n], dtype=float)
    hi = spla.eigsh(K, k=1, which="LA", tol=1e-6, return_eigenvectors=False)[0]
    lo = spla.eigsh(Ki, k=1, which="LA", tol=1e-6, return_eigenvectors=False)[0]
    return float(hi * lo)
