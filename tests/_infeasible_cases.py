"""Cases and references for the infeasibility code of the batch engines (osqp_amd/csrc/batch_admm.h: the cheap halves of
both tests in update_info, the pinf / dinf branches of check_termination, the no-solution branch of store_solution), which
the tiled engine reaches through k_batch_solve, the streamed one through k_bs_loop and the common-K one through k_bc_check.
No GPU here: tests/test_infeasible_cases_host.py runs all of it against the oracle, tests/test_gpu_batch_infeasible.py
against the engines.

The family.  planted_family builds eight members on one P, A (table in its docstring); every verdict is planted by hand,
at an index the caller chooses, so the deciding row and the deciding variable can sit in the first or in a later trip of
every loop of the kernel.

The certificate reference.  is_primal_infeasible / is_dual_infeasible (src/auxil.c:361-512) decide on the scaled
iterates dy~, dx~ of the scaled problem P~ = c D P D, q~ = c D q, A~ = E A D, l~ = E l, u~ = E u.  With
`unscaled` = (scaling and not scaled_termination) they unscale every quantity before comparing, and check_termination
(auxil.c:762-780) hands out w = E dy~ and d = D dx~.  In exact arithmetic that is the test on the raw problem:

    norm           |E dy~|_inf                                           = |w|_inf
    ineq_lhs       u~'max(dy~, 0) + l~'min(dy~, 0) = sum (E_i u_i)(w_i / E_i)+ ...   = u'w+ + l'w-      (E_i > 0 keeps the signs)
    |Dinv A~'dy~|  Dinv D A' E dy~                                       = |A'w|_inf
    norm           |D dx~|_inf                                           = |d|_inf
    q~'dx~         c q'D Dinv d = c q'd        against c eps |d|:   q'd < eps |d|
    |Dinv P~ dx~|  c Dinv D P D Dinv d = c |P d|   against c eps |d|:   |P d|_inf < eps |d|
    Einv A~ dx~    Einv E A D Dinv d           = A d                     row by row against +-eps |d|

so each criterion `< eps * norm` holds on (P, q, A, l, u) with the certificate that is returned, and store_solution's
division by the infinity norm (auxil.c:545-555) changes neither side's sign nor the ratio.  The projection on the polar of
the recession cone is sign-preserving under E too: w_i = 0 on a free row, w_i <= 0 where only u_i is infinite, w_i >= 0
where only l_i is.  With scaling = 0 nothing is scaled and the same holds trivially.  With scaling > 0 and
scaled_termination = 1 nothing is unscaled: the certificates ARE dy~ and dx~ and the criteria hold, as written, on the
scaled problem (cost scaling 1: q~'dx~ < eps |dx~|, |P~ dx~| < eps |dx~|) -- certificate_reference is then given that
problem (scaled_problem, from the D, E, c and scaled values of BatchOSQP.member_workspace or of the oracle's workspace).

Bars.  As in tests/_verify_reference.py: a float64 sum of k products is within gamma_k * sum |t_i| of the exact one, and
the bar of a sum is (k + C) * 2^-53 * sum |t_i|.  Here C = 16: the four units of _verify_reference.py (a second product
rounding, one more operation on the finished entry, the second order of gamma_k, the long-double reference's own error)
and the twelve roundings a term meets on its way through the scaled space (three for a scaled matrix value, two for each
scaled vector entry, the reciprocals of D, E and c, two unscalings -- `SCALED` there) -- the kernel decided on dy~, dx~ in
that space, and the entries of the certificate it returns went through E (or D), 1 / max and one more product, which the
same count covers.  A criterion a < b is `satisfied` when a < b + bar(a) + bar(b): what the kernel found true in float64
cannot be false by more than that in exact arithmetic.  The sign and zero conditions are exact: fmin, fmax and a
product with a positive number do not round a zero or a sign away."""
from types import SimpleNamespace

import numpy as np
from scipy import sparse

from _batch_parity import shape_family

LD = np.longdouble
U53 = 2.0 ** -53
C_BAR = 16
OSQP_INFTY = 1e30
OSQP_NAN = float(0x7FC00000)
BINF = 1e26                      # OSQP_INFTY * MIN_SCALING
STATUSES = [1, -4, -4, 1, -3, -3, -3, -4]                     # the table of planted_family
EPS_INF = 1e-4                   # eps_prim_inf = eps_dual_inf, the defaults

# name -> (n, m, seed, v, r0, r1, rr, rf).  Every shape but "20x30" is planted at the end: the deciding variable is the
# last one and the deciding rows the last four.  (128, 259): the tiled maximum and the second trip of the two-lanes-per-row
# loops at 512 threads; (520, 1043): the second trip of the one-lane-per-entry certificate loops.  With these seeds
# test_every_decision_is_robust (tests/test_infeasible_cases_host.py) holds for every member under every setting but
# check_termination = 1, where three shapes take the next seed at which it does (RESEEDED: with a check at every
# iteration one of the eight runs passed within 6e-4 of a threshold -- 20x30 member 4's rho estimate at iteration 32,
# 64x131 member 3's primal residual at 32, 128x259 member 2's row 109 of A dx at 13).
CASES = {
    "20x30": (20, 30, 55, 5, 0, 1, 2, 3),
    "6x9": (6, 9, 3, 5, 7, 8, 6, 5),
    "64x131": (64, 131, 5, 63, 129, 130, 128, 127),
    "128x259": (128, 259, 9, 127, 257, 258, 256, 255),
    "129x261": (129, 261, 11, 128, 259, 260, 258, 257),
    "520x1043": (520, 1043, 13, 519, 1041, 1042, 1040, 1039),
}
RESEEDED = {("20x30", "check_every"): 56, ("64x131", "check_every"): 7, ("128x259", "check_every"): 10}
TILED = ("20x30", "6x9", "64x131", "128x259")                 # n <= 128
LIVE = ("64x131", "129x261")
SETTINGS = {
    "default": dict(),
    "scaled_term": dict(scaled_termination=1),
    "unscaled": dict(scaling=0),
    "unscaled_scaled_term": dict(scaling=0, scaled_termination=1),
    "fixed_rho": dict(adaptive_rho=0),
    "check_every": dict(check_termination=1),
}
MAX_ITER = 4000
M0_N = (1, 2, 65)
M0_Q = (1.5, 0.0, -0.7)
M0_STATUSES = [-4, 1, -4]
# max_iter -> {member: status} on the "128x259" family with default settings: the middle of the window of max_iter in which
# the member's exact test still fails and the tenfold one passes (member 2: 58..99, 4: 26..32, 5: 26..34, 6: 9..12;
# tests/test_infeasible_cases_host.py re-derives them)
INACCURATE = {80: {2: 4}, 29: {4: 3}, 30: {5: 3}, 10: {6: 3}}
INACCURATE_CASE = "128x259"


def kw_of(setting, **more):
    return dict(SETTINGS[setting], max_iter=MAX_ITER, **more)


def space(kw):
    """"raw": the certificate is in the raw space (scaling = 0, or unscaled by E / D); "scaled": it stays in the scaled one."""
    return "scaled" if kw.get("scaling", 10) and kw.get("scaled_termination", 0) else "raw"


_cache = {}


def planted_family(n, m, seed, v, r0, r1, rr, rf):
    """B = 8 members on one P, A.  From shape_family(n, m, 8, seed): row and column v of P and column v of A are zeroed;
    row r1 is a copy of row r0; row rr is the single entry 2.0 in column v; row rf is empty.  Every bound is (A x0) -+ 0.5,
    rows rr and rf are free, q_v = 0; then

      member  planted                                              verdict
      0       nothing                                              solved
      1       q_v = 1.5                                            dual infeasible; the ray meets only a free row
      2       q_v = 1.5, u_rr = ax_rr + 1, l_rr = -inf             dual infeasible; A dx != 0, allowed by the infinite side
      3       q_v = 1.5, l_rr = ax_rr - 1, u_rr = +inf             solved; the same ray is forbidden
      4       r0 in [ax + 5, ax + 6], r1 in [ax - 6, ax - 5]       primal infeasible, two-sided
      5       r0 >= ax + 5 (u = +inf), r1 <= ax - 5 (l = -inf)     primal infeasible, one-sided
      6       r0 == ax + 3, r1 == ax - 3                           primal infeasible, equalities
      7       as member 4, and q_v = -0.7                          dual infeasible too; primal infeasible is asked first

    -> P (upper triangle), A, Q, L, U, ax."""
    key = (n, m, seed, v, r0, r1, rr, rf)
    if key not in _cache:
        P, A, Q, _, _, x0 = shape_family(n, m, 8, seed)
        Pd = P.tolil(); Pd[v, :] = 0.0; Pd[:, v] = 0.0
        P = sparse.triu(Pd.tocsc(), format="csc"); P.eliminate_zeros()
        Al = A.tolil(); Al[:, v] = 0.0
        if Al[r0, :].nnz == 0:
            Al[r0, 0 if v else 1] = 1.0
        Al[r1, :] = Al[r0, :]
        Al[rr, :] = 0.0; Al[rr, v] = 2.0
        Al[rf, :] = 0.0
        A = Al.tocsc(); A.eliminate_zeros(); A.sort_indices()
        ax = A @ x0
        L = np.tile(ax - 0.5, (8, 1)); U = np.tile(ax + 0.5, (8, 1))
        L[:, [rr, rf]] = -np.inf; U[:, [rr, rf]] = np.inf
        Q = Q.copy(); Q[:, v] = 0.0
        Q[[1, 2, 3], v] = 1.5
        L[2, rr], U[2, rr] = -np.inf, ax[rr] + 1.0
        L[3, rr], U[3, rr] = ax[rr] - 1.0, np.inf
        for b in (4, 7):
            L[b, r0], U[b, r0] = ax[r0] + 5.0, ax[r0] + 6.0
            L[b, r1], U[b, r1] = ax[r1] - 6.0, ax[r1] - 5.0
        L[5, r0], U[5, r0] = ax[r0] + 5.0, np.inf
        L[5, r1], U[5, r1] = -np.inf, ax[r1] - 5.0
        L[6, r0] = U[6, r0] = ax[r0] + 3.0
        L[6, r1] = U[6, r1] = ax[r1] - 3.0
        Q[7, v] = -0.7
        for a in (Q, L, U, ax):
            a.setflags(write=False)
        _cache[key] = (P, A, Q, L, U, ax)
    return _cache[key]


def family(name, setting="default"):
    n, m, seed, *where = CASES[name]
    return planted_family(n, m, RESEEDED.get((name, setting), seed), *where)


def live_updates(name):
    """The two updates of the live-handle tests on family `name` (its seed of the default settings), every row keeping its class:
    bounds: members 4, 5, 6 become feasible (4: the common box again; 5: r0 >= ax - 0.5, r1 <= ax + 0.5, still one-sided;
    6: r0 == r1 == ax, still equalities) and member 0 takes member 4's contradictory boxes -> statuses BOUNDS_STATUSES;
    cost (on the first problem): member 1's q_v becomes 0 and member 0's 1.5 -> statuses COST_STATUSES.
    -> (L2, U2, Q2)."""
    n, m, seed, v, r0, r1, rr, rf = CASES[name]
    P, A, Q, L, U, ax = family(name)
    L2, U2, Q2 = L.copy(), U.copy(), Q.copy()
    L2[0], U2[0] = L[4], U[4]
    L2[4], U2[4] = L[0], U[0]
    L2[5, r0], L2[5, r1], U2[5, r0], U2[5, r1] = ax[r0] - 0.5, -np.inf, np.inf, ax[r1] + 0.5
    L2[6, r0] = U2[6, r0] = ax[r0]
    L2[6, r1] = U2[6, r1] = ax[r1]
    Q2[1, v], Q2[0, v] = 0.0, 1.5
    return L2, U2, Q2


BOUNDS_STATUSES = [-3, -4, -4, 1, 1, 1, 1, -4]        # member 7 keeps its boxes and its q_v
COST_STATUSES = [-4, 1, -4, 1, -3, -3, -3, -4]


def m0_family(n):
    """P = diag(1, ..., 1, 0), no rows; q_{n-1} = 1.5, 0, -0.7 in the three members: dual infeasible, solved, dual
    infeasible, with certificate entry n - 1 equal to -1 / +1."""
    d = np.ones(n); d[-1] = 0.0
    P = sparse.csc_matrix(sparse.diags(d)); P.eliminate_zeros()
    A = sparse.csc_matrix((0, n))
    Q = np.tile(np.random.default_rng(100 + n).standard_normal(n), (3, 1))
    Q[:, -1] = M0_Q
    return P, A, Q, np.zeros((3, 0)), np.zeros((3, 0))


# ---------------------------------------------------------------------------------------------------------------
# the certificate reference
# ---------------------------------------------------------------------------------------------------------------
def _dense(P, A, n):
    Pu = sparse.triu(sparse.csc_matrix(P), format="csc")
    Pf = (Pu + sparse.triu(Pu, 1).T).toarray().astype(LD)
    SP = ((abs(Pu) + abs(sparse.triu(Pu, 1).T)) != 0).toarray()
    Ac = sparse.csc_matrix(A)
    Ad = Ac.toarray().astype(LD).reshape(Ac.shape[0], n)
    SA = (Ac != 0).toarray().reshape(Ac.shape[0], n)
    return Pf, SP, Ad, SA


def _bar(k, s):
    return (np.asarray(k, LD) + C_BAR) * U53 * np.asarray(s, LD)


def _mx(v):
    return np.max(v) if np.size(v) else LD(0)


def scaled_problem(ws, P, A, q, l, u):
    """The scaled problem of a member from D, E, c and the scaled matrix values (a dict with D, E, c, Pv, Av as
    BatchOSQP.member_workspace and _batch_parity.oracle_ws return it; the patterns are those of triu(P) and A)."""
    Pu = sparse.triu(sparse.csc_matrix(P), format="csc"); Pu.sort_indices()
    Ac = sparse.csc_matrix(A); Ac.sort_indices()
    Ps = sparse.csc_matrix((ws["Pv"], Pu.indices, Pu.indptr), shape=Pu.shape)
    As = sparse.csc_matrix((ws["Av"], Ac.indices, Ac.indptr), shape=Ac.shape)
    l = np.maximum(np.asarray(l, float), -OSQP_INFTY); u = np.minimum(np.asarray(u, float), OSQP_INFTY)
    return Ps, As, ws["c"] * ws["D"] * np.asarray(q, float), ws["E"] * l, ws["E"] * u


def certificate_reference(P, A, q, l, u, cert, kind, eps=EPS_INF, tenfold=False):
    """The quantities is_primal_infeasible (kind "primal", cert = w [m]) or is_dual_infeasible (kind "dual", cert = d [n])
    compare, in long double from the problem as given, each with its rounding bar.

    -> namespace: norm, norm_bar (|cert|_inf against 1);
                  criteria: [(name, value, limit, bar)] -- the reference asks value < limit (for a row of A d: <=);
                  excess: {name: (value - limit) / bar}, satisfied while <= 1;
                  exact: {name: bool} the sign and zero conditions of the projection (primal only).
    eps is eps_prim_inf / eps_dual_inf, times 10 with tenfold (the `inaccurate` statuses)."""
    cert = np.asarray(cert, np.float64)
    n = sparse.csc_matrix(P).shape[0]
    Pf, SP, Ad, SA = _dense(P, A, n)
    m = Ad.shape[0]
    l = np.maximum(np.asarray(l, np.float64).reshape(m), -OSQP_INFTY); u = np.minimum(np.asarray(u, np.float64).reshape(m), OSQP_INFTY)
    uinf, linf = u > BINF, l < -BINF
    e = LD(eps) * (10 if tenfold else 1)
    c = cert.astype(LD)
    out = SimpleNamespace(criteria=[], exact={}, kind=kind)
    nd = _mx(np.abs(c))
    out.norm, out.norm_bar = float(nd), 4 * U53            # s * (1 / max): the reciprocal and the product round once each
    lim, b_lim = e * nd, 2 * U53 * e * nd
    if kind == "primal":
        assert cert.shape == (m,)
        out.exact["zero on free rows"] = bool(np.all(cert[uinf & linf] == 0.0))
        out.exact["w <= 0 where u = +inf"] = bool(np.all(cert[uinf] <= 0.0))
        out.exact["w >= 0 where l = -inf"] = bool(np.all(cert[linf] >= 0.0))
        aA = np.abs(Ad)
        atw, s_atw, k = Ad.T @ c, aA.T @ np.abs(c), SA.sum(0)
        out.criteria.append(("|A'w|", _mx(np.abs(atw)), lim, _mx(_bar(k, s_atw)) + b_lim))
        # an infinite bound meets a zero of w+ / w- (the conditions above); where it does not, the term is +-1e30 |w_i|, as
        # the reference forms it, and the criterion fails by as much
        wp, wm = np.maximum(c, 0), np.minimum(c, 0)
        lhs = LD(u.astype(LD) @ wp + l.astype(LD) @ wm)
        s_lhs = np.abs(u).astype(LD) @ wp + np.abs(l).astype(LD) @ (-wm)
        out.criteria.append(("u'w+ + l'w-", lhs, lim, _bar(2 * m, s_lhs) + b_lim))
    else:
        assert cert.shape == (n,)
        q = np.asarray(q, np.float64).reshape(n).astype(LD)
        out.criteria.append(("q'd", q @ c, lim, _bar(n, np.abs(q) @ np.abs(c)) + b_lim))
        pd, s_pd = Pf @ c, np.abs(Pf) @ np.abs(c)
        out.criteria.append(("|P d|", _mx(np.abs(pd)), lim, _mx(_bar(SP.sum(1), s_pd)) + b_lim))
        if m:
            ad, b_ad = Ad @ c, _bar(SA.sum(1), np.abs(Ad) @ np.abs(c)) + b_lim
            for name, rows, sign in (("(A d)_i, u_i finite", ~uinf, 1), ("-(A d)_i, l_i finite", ~linf, -1)):
                if rows.any():
                    # the row that fails by most, in bars (bars differ by row); all rows pass: the one closest to failing
                    ex = (sign * ad[rows] - lim) / b_ad[rows]
                    i = int(np.argmax(ex))
                    out.criteria.append((name, (sign * ad[rows])[i], lim, b_ad[rows][i]))
    out.excess = {name: float((val - limit) / bar) for name, val, limit, bar in out.criteria}
    return out


def reference_failures(ref, margin=1.0):
    """What of a certificate_reference is not satisfied: criteria in excess of `margin` bars, a norm off 1 by more than
    `margin` bars, exact conditions that are false."""
    bad = ["%s: excess %.3g bars" % (k, v) for k, v in ref.excess.items() if not v <= margin]
    if not abs(ref.norm - 1.0) <= margin * ref.norm_bar:
        bad.append("norm: %.17g, %.3g bars from 1" % (ref.norm, abs(ref.norm - 1.0) / ref.norm_bar))
    return bad + [k for k, ok in ref.exact.items() if not ok]


def assert_certificate(P, A, q, l, u, cert, kind, what, tenfold=False):
    ref = certificate_reference(P, A, q, l, u, cert, kind, tenfold=tenfold)
    bad = reference_failures(ref)
    assert not bad, (what, kind, bad)
    return ref


# ---------------------------------------------------------------------------------------------------------------
# every comparison of a run, in long double
# ---------------------------------------------------------------------------------------------------------------
def decisions(so, ws, kw):
    """Steps the oracle `so` (set up, not yet solved; ws = _batch_parity.oracle_ws(so)) one iteration at a time as
    osqp_solve does (osqp.c:354-581) and recomputes in long double, from the oracle's iterates, every pair check_termination
    (auxil.c:681-786) and adapt_rho (auxil.c:13-74) compare -- only those the short-circuit order reaches.
    -> (status, iter, rho_updates, pairs): pairs = [(iteration, name, a, b)] for a comparison of a with b."""
    import ctypes as C
    st = so.settings()
    n, m = so.n, so.m
    w = so.work
    unscaled = bool(st.scaling and not st.scaled_termination)
    Pu = sparse.csc_matrix(ws["Pu"]); Pf = (Pu + sparse.triu(Pu, 1).T).toarray().astype(LD)
    Ad = sparse.csc_matrix(ws["A"]).toarray().astype(LD).reshape(m, n)
    D, E, c = ws["D"].astype(LD), ws["E"].astype(LD), LD(ws["c"])
    Di, Ei, ci = (1 / D, 1 / E, 1 / c) if unscaled else (np.ones(n, LD), np.ones(m, LD), LD(1))
    Dn, En, csc = (D, E, c) if unscaled else (np.ones(n, LD), np.ones(m, LD), LD(1))
    q = so._vec(w.data.contents.q, n).astype(LD)
    l, u = so._vec(w.data.contents.l, m), so._vec(w.data.contents.u, m)
    uinf, linf = u > BINF, l < -BINF
    l, u = l.astype(LD), u.astype(LD)
    interval = st.adaptive_rho_interval or (4 * st.check_termination if st.check_termination else 100)
    pairs, rho_updates, state = [], 0, {}
    vec = lambda p, k: so._vec(p, k).astype(LD)

    def norms():
        x, z, y = vec(w.x, n), vec(w.z, m), vec(w.y, m)
        ax, px, aty = Ad @ x, Pf @ x, Ad.T @ y
        state.update(pri_s=_mx(np.abs(ax - z)), nz_s=_mx(np.abs(z)), nax_s=_mx(np.abs(ax)),
                     dua_s=_mx(np.abs(px + q + aty)), nq_s=_mx(np.abs(q)), naty_s=_mx(np.abs(aty)), npx_s=_mx(np.abs(px)),
                     pri=_mx(np.abs(Ei * (ax - z))), nz=_mx(np.abs(Ei * z)), nax=_mx(np.abs(Ei * ax)),
                     dua=ci * _mx(np.abs(Di * (px + q + aty))), nq=ci * _mx(np.abs(Di * q)), naty=ci * _mx(np.abs(Di * aty)),
                     npx=ci * _mx(np.abs(Di * px)))

    def check(it, approximate):
        s = state
        f = 10 if approximate else 1
        ea, er, epi, edi = (LD(v) * f for v in (st.eps_abs, st.eps_rel, st.eps_prim_inf, st.eps_dual_inf))
        tag = "approximate " if approximate else ""

        def lt(name, a, b):
            pairs.append((it, tag + name, float(a), float(b)))
            return bool(a < b)
        prim_ok = dual_ok = pinf = dinf = False
        if m == 0:
            prim_ok = True
        elif lt("pri_res < eps_pri", s["pri"], ea + er * max(s["nz"], s["nax"])):
            prim_ok = True
        else:
            dy = vec(w.delta_y, m)
            dy = np.where(uinf, np.where(linf, 0, np.minimum(dy, 0)), np.where(linf, np.maximum(dy, 0), dy))
            nd = _mx(np.abs(En * dy))
            if lt("1e-30 < |dy|", LD(1e-30), nd):
                lhs = u @ np.maximum(dy, 0) + l @ np.minimum(dy, 0)
                if lt("lhs < eps |dy|", lhs, epi * nd):
                    pinf = lt("|A'dy| < eps |dy|", _mx(np.abs(Di * (Ad.T @ dy))), epi * nd)
        if lt("dua_res < eps_dua", s["dua"], ea + er * max(s["nq"], s["naty"], s["npx"])):
            dual_ok = True
        else:
            dx = vec(w.delta_x, n)
            ndx = _mx(np.abs(Dn * dx))
            if lt("1e-30 < |dx|", LD(1e-30), ndx):
                if lt("q'dx < c eps |dx|", q @ dx, csc * edi * ndx):
                    if lt("|P dx| < c eps |dx|", _mx(np.abs(Di * (Pf @ dx))), csc * edi * ndx):
                        adx = Ei * (Ad @ dx)
                        viol = False
                        for i in range(m):           # every row a finite side lets decide
                            if not uinf[i]:
                                viol |= lt("(A dx)_%d > eps |dx|" % i, edi * ndx, adx[i])
                            if not linf[i]:
                                viol |= lt("(A dx)_%d < -eps |dx|" % i, adx[i], -edi * ndx)
                        dinf = not viol
        if prim_ok and dual_ok:
            return 2 if approximate else 1
        if pinf:
            return 3 if approximate else -3
        if dinf:
            return 4 if approximate else -4
        return 0

    status, it, checked = 0, 0, False
    while it < st.max_iter:
        it += 1
        so.iterate()
        checked = bool(st.check_termination and it % st.check_termination == 0)
        adapt = bool(st.adaptive_rho and it % interval == 0)
        if checked or adapt:
            norms()
        if checked:
            status = check(it, False)
            if status:
                break
        if adapt:
            s, rho = state, LD(st.rho)
            pr = (s["pri_s"] if m else LD(0)) / (max(s["nz_s"], s["nax_s"]) + LD(1e-30))
            du = s["dua_s"] / (max(s["nq_s"], s["naty_s"], s["npx_s"]) + LD(1e-30))
            rn = min(max(rho * np.sqrt(pr / du), LD(1e-6)), LD(1e6))
            tol = LD(st.adaptive_rho_tolerance)
            pairs.append((it, "rho_new > tol rho", float(rn), float(rho * tol)))
            pairs.append((it, "rho_new < rho / tol", float(rn), float(rho / tol)))
            if rn > rho * tol or rn < rho / tol:
                assert so.update_rho(float(rn)) == 0
                st = so.settings()
                rho_updates += 1
    if not status:
        if not checked:
            norms()
            status = check(it, False)
        if not status:
            status = check(it, True) or -2
    return status, it, rho_updates, pairs


def margin(pairs):
    """The smallest relative distance |a - b| / max(|a|, |b|) of the pairs (a == b == 0 counts as 0: on the threshold),
    and the pair it belongs to."""
    best = (np.inf, None)
    for p in pairs:
        a, b = p[2], p[3]
        d = abs(a - b) / max(abs(a), abs(b)) if (a or b) else 0.0
        if d < best[0]:
            best = (d, p)
    return best


def coupled_variants(name):
    """Two single problems on family `name` whose certificate spans two DIFFERENT scaling factors -- in the family itself
    rows r0 and r1 are equal, so E_r0 = E_r1, and the ray is one variable, so a certificate with E or D applied once too
    often is, after the division by its norm, still a certificate there.
    primal: member 4 with row r1 = 3 x row r0 (and its box 3 x as far): w_r0 + 3 w_r1 = 0 holds for E dy~ only.
    dual: member 1 with variable v - 1 emptied like v, q_{v-1} = 0.4, and row rf the equality x_v - 3 x_{v-1} = 0: the ray
    has d_v = 3 d_{v-1}, which holds for D dx~ only.
    -> ((P, A, q, l, u), (P, A, q, l, u))"""
    n, m, seed, v, r0, r1, rr, rf = CASES[name]
    P, A, Q, L, U, ax = family(name)
    Al = A.tolil(); Al[r1, :] = 3.0 * Al[r0, :]
    l, u = L[4].copy(), U[4].copy()
    l[r1], u[r1] = 3.0 * (ax[r0] - 6.0), 3.0 * (ax[r0] - 5.0)
    primal = (P, Al.tocsc(), Q[4], l, u)
    Pd = P.tolil(); Pd[v - 1, :] = 0.0; Pd[:, v - 1] = 0.0
    P2 = sparse.triu(Pd.tocsc(), format="csc"); P2.eliminate_zeros()
    Al = A.tolil(); Al[:, v - 1] = 0.0; Al[rf, v] = 1.0; Al[rf, v - 1] = -3.0
    A2 = Al.tocsc(); A2.eliminate_zeros()
    q = Q[1].copy(); q[v - 1] = 0.4
    l, u = L[1].copy(), U[1].copy()
    l[rf] = u[rf] = 0.0
    return primal, (P2, A2, q, l, u)
