"""Cases of tests/test_gpu_batch_common_sessions.py -- a common-K handle's life against the long-double reference, the
refinement verdict after a subset solve, a pack while a verdict is open, the geometry of a pack -- proved on the CPU by
tests/test_common_session_cases_host.py.

A session is a list of steps played on a handle and on `CommonReference` alike:
  ("solve", members or None)   ("update", dict(Q=, L=, U=))   ("update_rho", value)   ("warm_start", X, Y)

"general"   `adaptive_family(33, 66, 70, 100.0)` under ADAPTIVE with scaled_termination = 1, Q as it comes: q^ of the batch
            is not q^ of any of the listed sets, so no handle set up on a subset has the batch's scaling.
"cut"       `common_family(17, 37, 130, 1054)` under FIXED with max_iter = 40: members stop unsolved and are continued by
            later, different subsets; one warm_start(X, Y) with given values in the middle.  "cut-cold" is its twin with
            the setting warm_start = 0: a solve of all members but one, then a subset solve that restarts the listed
            members from zero; then warm_start(X, Y), which turns the setting on, and two subset solves that continue.
verdict     VERDICT_*: a block-diagonal model whose members S keep the ill-conditioned block at exactly zero.
"probing"   a block model under adaptive rho with adaptive_rho_interval = 24, max_iter = 45 and a stated refine_tol: the
            probes of iterations 1 to 4 leave the verdict off, K is inverted at 24, and the check point 25 -- with the
            pack it triggers -- falls inside the four iterations probed next, which turn the verdict on.
geometry    GEOMETRY: wave batches (members of `common_family(17, 37, ., 1054)`, some made easy as `wave_case` does) whose
            first pack has a chosen shape."""
import numpy as np
from scipy import sparse

from _common_cases import ADAPTIVE, FIXED, adaptive_family, common_family
from _common_members_cases import WAVE_M, WAVE_N, WAVE_SEED

# ---- sessions ------------------------------------------------------------------------------------------------------------
GENERAL_B = 70
GENERAL_S1 = np.arange(0, GENERAL_B, 3)
GENERAL_S2 = np.arange(20, GENERAL_B)
GENERAL_SHIFT_SEED = 7
CUT_B = 130
CUT_WARM_SEED = 11
CUT_COLD_OUT = (127,)       # from a cold start member 127 misses the exact test at iteration 40 by 3.7e-4: it is never listed


def _general():
    P, A, Q, L, U, _ = adaptive_family(33, 66, GENERAL_B, 100.0)
    rng = np.random.default_rng(GENERAL_SHIFT_SEED)
    # the bounds move with the member's feasible point (x0 + d): every row keeps its width, hence its class
    shift = (A @ (0.1 * rng.standard_normal((GENERAL_B, 33))).T).T
    rest = np.setdiff1d(np.arange(GENERAL_B), GENERAL_S1)
    steps = [("solve", GENERAL_S1), ("solve", GENERAL_S2), ("update", dict(Q=Q * 1.25, L=L + shift, U=U + shift)),
             ("solve", GENERAL_S1), ("update_rho", 0.3), ("solve", rest), ("solve", None)]
    return (P, A, Q, L, U), dict(ADAPTIVE, scaled_termination=1), steps


def _cut(cold=False):
    P, A, Q, L, U, X0 = common_family(WAVE_N, WAVE_M, CUT_B, WAVE_SEED)
    kw = dict(FIXED, max_iter=40)
    rng = np.random.default_rng(CUT_WARM_SEED)
    X = 0.5 * X0
    Y = 0.1 * rng.standard_normal((CUT_B, WAVE_M)) * (L == U)          # multipliers on the equality rows only
    third = np.arange(0, CUT_B, 3)
    if cold:
        # (the warm_start call turns the setting on, as osqp_warm_start does: the last solve continues its members)
        evens = np.arange(0, CUT_B, 2)
        return (P, A, Q, L, U), dict(kw, warm_start=0), [("solve", np.setdiff1d(np.arange(CUT_B), CUT_COLD_OUT)), ("solve", evens),
                                                         ("warm_start", X, Y), ("solve", third), ("solve", evens)]
    steps = [("solve", np.arange(0, CUT_B, 2)), ("solve", np.arange(30, 100)), ("warm_start", X, Y), ("solve", third),
             ("solve", np.setdiff1d(np.arange(CUT_B), third)), ("solve", None)]
    return (P, A, Q, L, U), kw, steps


def session_case(name):
    """((P, A, Q, L, U), settings, steps) of a named session."""
    return {"general": _general, "cut": _cut, "cut-cold": lambda: _cut(True), "probing": _probing}[name]()


def play(obj, step):
    """One step on a handle or on a reference; a solve returns its result."""
    if step[0] == "solve":
        return obj.solve() if step[1] is None else obj.solve(members=step[1])
    if step[0] == "update":
        assert not obj.update(**step[1])
    elif step[0] == "update_rho":
        assert not obj.update_rho(step[1])
    else:
        assert not obj.warm_start(step[1], step[2])
    return None


_RUNS = {}


def session_reference(orc, name, dtype=np.longdouble):
    """(the reference after the session, [(step index, result) of every solve]); computed once per process and shared --
    callers leave both unchanged."""
    from _common_reference import reference_for
    if (name, dtype) not in _RUNS:
        (P, A, Q, L, U), kw, steps = session_case(name)
        ref = reference_for(orc, P, A, Q, L, U, dtype=dtype, **kw)
        out = []
        for k, step in enumerate(steps):
            r = play(ref, step)
            if r is not None:
                out.append((k, r))
        _RUNS[name, dtype] = (ref, out)
    return _RUNS[name, dtype]


# ---- a pack while a verdict is open --------------------------------------------------------------------------------------
PROBING_B = 70
PROBING_EASY = np.arange(1, PROBING_B, 2)
PROBING_SEED = 3
PROBING_RHO0 = 1e-6
PROBING_REFINE_TOL = 1e-12         # OSQP_AMD_BATCH_REFINE_TOL of this case, read at setup
PROBING_SETTINGS = dict(ADAPTIVE, adaptive_rho_interval=24, scaled_termination=1, scaling=0, rho=PROBING_RHO0, max_iter=45)


def _probing():
    """The block model of the verdict case with block 2 at P ~ 1e-5 and equality rows ten times larger, solved from
    rho = 1e-6 with adaptive_rho_interval = 24 and max_iter = 45.  With the first rho the 1e3 rho rows weigh little and
    K^-1 is accurate; the move at 24 raises rho twenty-fold and the probes of iterations 25 to 28 -- the only other
    window before max_iter -- find residuals some 500 times larger.  Every odd member is easy (q scaled by 1e-4, its
    equality rows at 0) and ends at the check point 25, where the rule packs."""
    rng = np.random.default_rng(PROBING_SEED)
    n1, n2, neq, B = 6, 6, 2, PROBING_B
    n, m = n1 + n2, n1 + neq
    M = rng.standard_normal((n2, n2))
    P2 = 1e-5 * (M @ M.T / n2 + np.eye(n2))
    P = sparse.triu(sparse.block_diag([sparse.diags(rng.uniform(0.5, 2.0, n1)), P2], format="csc"), format="csc")
    Aeq = 10.0 * rng.standard_normal((neq, n2))
    A = sparse.vstack([sparse.hstack([sparse.identity(n1), sparse.csc_matrix((n1, n2))]),
                       sparse.hstack([sparse.csc_matrix((neq, n1)), sparse.csc_matrix(Aeq)])], format="csc")
    Q = rng.standard_normal((B, n)) * 20.0
    Q[:, n1:] *= 1e-5
    L = np.empty((B, m)); U = np.empty((B, m))
    L[:, :n1], U[:, :n1] = -1.0, 1.0
    X2 = rng.standard_normal((B, n2))
    L[:, n1:] = U[:, n1:] = X2 @ Aeq.T
    Q[PROBING_EASY] *= 1e-4
    L[PROBING_EASY, n1:] = U[PROBING_EASY, n1:] = 0.0
    return (P, A, Q, L, U), dict(PROBING_SETTINGS), [("solve", None)]


# ---- the verdict case ----------------------------------------------------------------------------------------------------
VERDICT_B, VERDICT_N1, VERDICT_N2, VERDICT_EQ = 8, 6, 6, 2
VERDICT_S = np.array([0, 2, 3, 6])
VERDICT_SEED = 3
VERDICT_SETTINGS = dict(FIXED, scaling=0, max_iter=300)
REFINE_TOL = 1e-14                                         # the engine's default (OSQP_AMD_BATCH_REFINE_TOL unset)


def verdict_case():
    """(P, A, Q, L, U).  Block 1: diagonal P, one unit box row per variable -- K is diagonal there.  Block 2: a small P,
    VERDICT_EQ dense equality rows and no box rows, so K's second block has eigenvalues from |P2| ~ 1e-3 up to
    1e3 rho |a|^2.  Members of VERDICT_S have q = 0 in block 2 and their equality rows at 0: block 2 stays exactly 0."""
    rng = np.random.default_rng(VERDICT_SEED)
    n1, n2, B = VERDICT_N1, VERDICT_N2, VERDICT_B
    n = n1 + n2
    M = rng.standard_normal((n2, n2))
    P2 = 1e-3 * (M @ M.T / n2 + np.eye(n2))
    P = sparse.block_diag([sparse.diags(rng.uniform(0.5, 2.0, n1)), P2], format="csc")
    P = sparse.triu(P, format="csc")
    Aeq = rng.standard_normal((VERDICT_EQ, n2))
    A = sparse.vstack([sparse.hstack([sparse.identity(n1), sparse.csc_matrix((n1, n2))]),
                       sparse.hstack([sparse.csc_matrix((VERDICT_EQ, n1)), sparse.csc_matrix(Aeq)])], format="csc")
    m = n1 + VERDICT_EQ
    Q = rng.standard_normal((B, n)) * 2.0
    L = np.empty((B, m)); U = np.empty((B, m))
    L[:, :n1], U[:, :n1] = -1.0, 1.0
    X2 = rng.standard_normal((B, n2))
    L[:, n1:] = U[:, n1:] = X2 @ Aeq.T
    Q[VERDICT_S, n1:] = 0.0
    L[VERDICT_S, n1:] = U[VERDICT_S, n1:] = 0.0
    return P, A, Q, L, U


def gauss_jordan_inverse(K):
    """K^-1 in float64 by Gauss-Jordan without pivoting, as the engine inverts (zero multipliers skipped: exact zeros stay)."""
    n = K.shape[0]
    W = np.hstack([np.array(K, dtype=np.float64), np.eye(n)])
    for k in range(n):
        W[k] = W[k] / W[k, k]
        for i in range(n):
            if i != k and W[i, k] != 0.0:
                W[i] = W[i] - W[i, k] * W[k]
    return W[:, n:]


def probe_replay(Pf, Ad, q, l, u, ctype, rho, sigma=1e-6, alpha=1.6, iters=4, windows=((1, 4),), moves=None):
    """[iters, B] the ratio |R - K X~|_inf / |R|_inf k_bc_probe would take in each of the first `iters` iterations of a
    cold solve on scaled data (q, l, u [B, .], one class per row), replayed in float64: K^-1 by Gauss-Jordan without
    pivoting, the residual through the operator P X~ + sigma X~ + A'(rho .* A X~), the refinement step applied in the
    iterations of `windows` (first, last; as the engine does while it probes) and nowhere else -- the run of a verdict
    that stays off.  moves: {iteration: rho adopted after it}, K re-formed and re-inverted there.  The engine's steps in
    numpy's summation order.  Also returns cond(K) of every K and whether every K^-1 kept K's zero pattern exactly."""
    m, n = Ad.shape
    B = q.shape[0]
    x = np.zeros((B, n)); z = np.zeros((B, m)); y = np.zeros((B, m))
    out = np.zeros((iters, B))
    conds, kept = [], True

    def form(rho):
        rv = np.where(ctype == -1, 1e-6, np.where(ctype == 1, 1e3 * rho, rho))
        K = Pf + sigma * np.eye(n) + Ad.T @ (rv[:, None] * Ad)
        Kinv = gauss_jordan_inverse(K)
        conds.append(float(np.linalg.cond(K)))
        return rv, Kinv, bool(np.all(Kinv[K == 0.0] == 0.0))

    rv, Kinv, ok = form(rho)
    kept = kept and ok
    for it in range(1, iters + 1):
        R = sigma * x - q + (rv * z - y) @ Ad
        xt = R @ Kinv.T
        Rr = R - (xt @ Pf + sigma * xt + (rv * (xt @ Ad.T)) @ Ad)
        out[it - 1] = np.abs(Rr).max(axis=1) / np.abs(R).max(axis=1)
        if any(a <= it <= b for a, b in windows):
            xt = xt + Rr @ Kinv.T
        zt = xt @ Ad.T
        v = alpha * zt + (1 - alpha) * z
        zn = np.clip(v + y / rv, l, u)
        x = alpha * xt + (1 - alpha) * x
        y = y + rv * (v - zn)
        z = zn
        if moves and it in moves:
            rv, Kinv, ok = form(moves[it])
            kept = kept and ok
    return out, conds, kept


def probe_ratios(P, A, Q, L, U, rho=0.1, sigma=1e-6, alpha=1.6, iters=4):
    """`probe_replay` of the first `iters` iterations for unscaled data (scaling = 0) whose rows are equalities or
    two-sided inequalities: (ratios, cond(K), zero pattern kept)."""
    Pf = (P + sparse.triu(P, 1).T).toarray(); Ad = A.toarray()
    out, conds, kept = probe_replay(Pf, Ad, Q, L, U, np.where(L[0] == U[0], 1, 0), rho, sigma, alpha, iters)
    return out, conds[0], kept


_VERDICT = {}


def verdict_reference(orc, dtype=np.longdouble):
    """The long-double run of the whole verdict batch (a full cold solve: with a fixed rho and no scaling a member's run
    does not depend on who is solved with it); dtype=np.float64: the plain-double run of the conditioning check."""
    from _common_reference import reference_for
    if dtype not in _VERDICT:
        P, A, Q, L, U = verdict_case()
        ref = reference_for(orc, P, A, Q, L, U, dtype=dtype, **VERDICT_SETTINGS)
        _VERDICT[dtype] = (ref, ref.solve())
    return _VERDICT[dtype]


# ---- pack geometry -------------------------------------------------------------------------------------------------------
# name: (B, hard positions, family members left out).  Position c of the batch holds the c-th member of
# `common_family(17, 37, ., 1054)` that is not left out; the positions outside `hard` are made easy (q = 0, bounds around
# 0: they end at iteration 25 and q^ is that of the hard ones).  A family member is left out when, in this batch, it
# would end at iteration 25 where the case needs it running, or would come within MARGIN_CHECK of a threshold.
GEOMETRY = {
    "shift-1": (65, (1, 65), (13, 48, 49, 53, 54, 68)),                                   # those six would end at 25
    "shift-1-chunk": (321, (1, 321), (49, 54, 68, 122, 140, 152, 168, 203, 213, 234)),    # likewise
    "back": (600, (300, 600), (412, 497)),             # 6.9e-4 and 1.1e-3 from a threshold at iterations 50 and 75
    "to-256": (330, (0, 268), (210, 223)),             # 1.1e-3 and 6.2e-4 from a threshold at iterations 25 and 50
    "to-257": (330, (0, 269), (210, 223)),
}
# what the host test proves of each: (columns the first pack leaves, packs, columns at the end)
GEOMETRY_PROVED = {"shift-1": (64, 1, 64), "shift-1-chunk": (320, 2, 62), "back": (294, 3, 17), "to-256": (256, 2, 42),
                   "to-257": (257, 2, 42)}


def geometry_case(name):
    """(P, A, Q, L, U, hard positions)."""
    B, (h0, h1), out = GEOMETRY[name]
    F = B + len(out)
    P, A, Q, L, U, X0 = common_family(WAVE_N, WAVE_M, F, WAVE_SEED)
    keep = np.setdiff1d(np.arange(F), out)
    Q, L, U, X0 = Q[keep], L[keep], U[keep], X0[keep]
    hard = np.arange(h0, h1)
    for b in np.setdiff1d(np.arange(B), hard):
        ax = A @ X0[b]
        Q[b] = 0.0
        L[b] = L[b] - ax
        U[b] = U[b] - ax
    return P, A, Q, L, U, hard


_GEOMETRY_RUNS = {}


def geometry_reference(orc, name, dtype=np.longdouble):
    from _common_reference import reference_for
    if (name, dtype) not in _GEOMETRY_RUNS:
        P, A, Q, L, U, _ = geometry_case(name)
        ref = reference_for(orc, P, A, Q, L, U, dtype=dtype, **FIXED)
        _GEOMETRY_RUNS[name, dtype] = (ref, ref.solve())
    return _GEOMETRY_RUNS[name, dtype]


def first_pack_src(iters):
    """`src` of the first pack: the columns still running after the first check point at which the rule packs."""
    from _common_members_cases import GROUP
    iters = np.asarray(iters)
    C = iters.size
    for it in sorted(set(iters.tolist())):
        run = np.flatnonzero(iters > it)
        if run.size and -(-run.size // GROUP) < -(-C // GROUP):
            return it, run
    return None, None
