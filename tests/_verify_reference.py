"""The 16 slots of BatchOSQP.verify (osqp_amd_batch_verify, osqp_amd/csrc/batch_verify.h) restated in numpy long double
from the raw P, q, A, l, u and the unscaled point, with the rounding bound ("bar") of every slot and the distance of
every verdict from its threshold.  Nothing here comes from the code under test.

Every quantity the kernel forms is a sum of k terms t_1 .. t_k (products of given float64 numbers), or a maximum over
such sums.  In float64 -- u = 2^-53, products and additions rounded one by one, in any order and with or without fused
multiply-adds -- a computed sum s^ of k such terms satisfies

    |s^ - s| <= gamma_k * sum |t_i|,   gamma_k = k u / (1 - k u)       (Higham, Accuracy and Stability, 3.1-3.4):

a term passes through its own product (one rounding; a product of three factors: two) and at most k - 1 additions.  The
bar of a sum is therefore

    bar = (k + C) * 2^-53 * sum |t_i|,   C = 4.

C covers, one unit each: the second product rounding of a three-factor term (x_j P_jk x_k, y_i A_ik x_k); one more
rounded operation on the finished entry (a - z, (px + q) + aty, obj - dual_obj, eps_abs + eps_rel * norm); the second
order of gamma_k (k u < 1e-12 here, so gamma_k < (k + 1) u by a wide margin); and the long-double reference's own error
(k * 2^-64 * sum |t_i| < u * sum |t_i| for k < 2048).  A fused multiply-add only removes roundings.  Maximum, absolute
value, clamp and the comparisons are exact and 1-Lipschitz, so the bar of a maximum over entries is the largest bar of
an entry: the final max adds nothing.  Multiplying by 0.5 is exact.

    reference(...) -> namespace: val [16] float64, bar [16] float64, sums {name: (value, sum |terms|, k)} for every sum,
                      margin {"optimal" | "prim_inf" | "dual_inf": the verdict's distance from flipping, in bars}.

A verdict is a conjunction of comparisons a < b (or a > b).  The margin of a comparison is |a - b| / (bar a + bar b).  A
true verdict flips when any of its comparisons does: its margin is the smallest of them.  A false verdict flips only when
every false comparison does: its margin is the largest among the false ones."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
C = 4
# The solve forms obj, pri_res and dua_res from the same terms in its scaled space: P~ = c D P D, q~ = c D q, A~ = E A D,
# x~ = D^-1 x, y~ = c E^-1 y, and the result unscaled by D^-1, E^-1, c^-1.  Exactly, every term is the raw one; in
# float64 a term meets at most 12 more roundings (three for a scaled matrix value, two for each scaled vector entry, the
# reciprocals of D, E and c, the two unscalings), so the solve's value is within (k + C + 12) u sum |t_i| of the exact
# one, and (k + 16) / (k + 4) <= 4: within SCALED bars of the reference.
SCALED = 4
OSQP_INFTY = 1e30
OSQP_NAN = float(0x7FC00000)
BINF = 1e26                      # OSQP_INFTY * MIN_SCALING
DIVISION_TOL = 1.0 / OSQP_INFTY
FIELDS = ["obj", "pri_res", "dua_res", "norm_ax", "norm_z", "norm_px", "norm_aty", "norm_q", "eps_pri", "eps_dua", "comp",
          "dual_obj", "gap", "optimal", "prim_inf", "dual_inf"]


def dense(n, m, Pp, Pi, Px, Ap, Ai, Ax):
    """(P full symmetric [n, n], its pattern as 0/1, A [m, n], its pattern) in long double from the CSC arrays of triu(P)
    and A; a stored zero counts as an entry of the pattern (the kernel adds it)."""
    P = np.zeros((n, n), LD); SP = np.zeros((n, n)); A = np.zeros((m, n), LD); SA = np.zeros((m, n))
    for j in range(n):
        for k in range(Pp[j], Pp[j + 1]):
            i = Pi[k]
            P[i, j] += LD(Px[k]); SP[i, j] = 1
            if i != j:
                P[j, i] += LD(Px[k]); SP[j, i] = 1
        for k in range(Ap[j], Ap[j + 1]):
            A[Ai[k], j] += LD(Ax[k]); SA[Ai[k], j] = 1
    return P, SP, A, SA


def _isnan(v):
    v = np.asarray(v, np.float64)
    return bool(np.any(np.isnan(v) | (v == OSQP_NAN)))


def _bar(k, s):
    return (np.asarray(k, LD) + C) * U * np.asarray(s, LD)


def _mx(v):
    return np.max(v) if np.size(v) else LD(0)


def _compare(a, bar_a, b, bar_b, less=True):
    """(a < b or a > b, its margin in bars)"""
    holds = bool(a < b) if less else bool(a > b)
    d = float(bar_a + bar_b)
    return holds, (float(abs(a - b)) / d if d > 0 else np.inf) if a != b else 0.0


def _verdict(comparisons):
    if not comparisons:
        return False, np.inf
    if all(h for h, _ in comparisons):
        return True, min(g for _, g in comparisons)
    return False, max(g for h, g in comparisons if not h)


def reference(n, m, Pp, Pi, Px, Ap, Ai, Ax, q, l, u, x, y, dx, dy, eps_abs, eps_rel, eps_pinf, eps_dinf, drop=None):
    """drop = (i, j), i < j, an entry of triu(P): the planted defect of a kernel that applies the stored triangle as one
    half only -- P_ji is left out."""
    P, SP, A, SA = dense(n, m, Pp, Pi, Px, Ap, Ai, Ax)
    if drop is not None:
        P[drop[1], drop[0]] = 0
    f = lambda v, k: np.asarray(v, np.float64).reshape(k).astype(LD)
    q, x, dx = f(q, n), f(x, n), f(dx, n)
    l, u, y, dy = f(l, m), f(u, m), f(y, m), f(dy, m)
    val, bar, sums, margin = np.zeros(16, LD), np.zeros(16, LD), {}, {}
    aP, aA, kP, kA, kAt = np.abs(P), np.abs(A), SP.sum(1), SA.sum(1), SA.sum(0)
    uinf, linf = u > BINF, l < -BINF

    # ---- slots 0-13 ----------------------------------------------------------------------------------------------------
    xs, ys = np.where(np.isnan(x), 0, x), np.where(np.isnan(y), 0, y)       # (a NaN point: the slots are overwritten below)
    ax, s_ax = A @ xs, aA @ np.abs(xs)
    z = np.minimum(np.maximum(ax, l), u)
    px, s_px = P @ xs, aP @ np.abs(xs)
    aty, s_aty = A.T @ ys, aA.T @ np.abs(ys)
    b_ax, b_px, b_aty = _bar(kA, s_ax), _bar(kP, s_px), _bar(kAt, s_aty)
    yp, ym = np.maximum(ys, 0), np.maximum(-ys, 0)
    on_inf = bool(np.any((yp != 0) & uinf) or np.any((ym != 0) & linf))
    xpx_terms = LD(0.5) * (np.abs(xs) @ aP @ np.abs(xs))
    k_xpx = SP.sum()
    sums["obj"] = (LD(0.5) * (xs @ px) + q @ xs, xpx_terms + np.abs(q) @ np.abs(xs), k_xpx + n)
    fu, fl = np.where(uinf, 0, u), np.where(linf, 0, l)
    sums["dual_obj"] = (-LD(0.5) * (xs @ px) - (fu @ yp - fl @ ym), xpx_terms + np.abs(fu) @ yp + np.abs(fl) @ ym, k_xpx + 2 * m)
    val[0], bar[0] = sums["obj"][0], _bar(sums["obj"][2], sums["obj"][1])
    val[1], bar[1] = _mx(np.abs(ax - z)), _mx(b_ax)
    dua, s_dua, k_dua = px + q + aty, s_px + np.abs(q) + s_aty, kP + kAt + 1
    val[2], bar[2] = _mx(np.abs(dua)), _mx(_bar(k_dua, s_dua))
    val[3], bar[3] = _mx(np.abs(ax)), _mx(b_ax)
    val[4], bar[4] = _mx(np.abs(z)), _mx(b_ax)
    val[5], bar[5] = _mx(np.abs(px)), _mx(b_px)
    val[6], bar[6] = _mx(np.abs(aty)), _mx(b_aty)
    val[7], bar[7] = _mx(np.abs(q)), 0
    val[8] = LD(eps_abs) + LD(eps_rel) * max(val[3], val[4])
    bar[8] = LD(eps_rel) * max(bar[3], bar[4]) + C * U * val[8]
    val[9] = LD(eps_abs) + LD(eps_rel) * max(val[5], val[6], val[7])
    bar[9] = LD(eps_rel) * max(bar[5], bar[6]) + C * U * val[9]
    if on_inf:
        val[10], val[11], val[12] = OSQP_INFTY, -OSQP_INFTY, OSQP_INFTY
    else:
        # yp_i (u_i - z_i) = yp_i u_i - sum_k yp_i A_ik x_k where z_i = (A x)_i, and less where z_i is clamped: k_i + 1 terms
        tu, tl = yp * (fu - z), ym * (z - fl)
        val[10] = max(_mx(tu), _mx(tl), LD(0))
        bar[10] = max(_mx(_bar(kA + 1, yp * (np.abs(fu) + s_ax))), _mx(_bar(kA + 1, ym * (np.abs(fl) + s_ax))), LD(0))
        val[11], bar[11] = sums["dual_obj"][0], _bar(sums["dual_obj"][2], sums["dual_obj"][1])
        val[12] = val[0] - val[11]
        bar[12] = _bar(sums["obj"][2] + sums["dual_obj"][2], sums["obj"][1] + sums["dual_obj"][1])
    opt, margin["optimal"] = _verdict([_compare(val[1], bar[1], val[8], bar[8]), _compare(val[2], bar[2], val[9], bar[9])])
    val[13] = 1.0 if opt else 0.0
    if _isnan(x) or _isnan(y):
        val[:13], bar[:13], val[13], margin["optimal"] = OSQP_NAN, 0, 0.0, np.inf

    # ---- slot 14: is_primal_infeasible (auxil.c:361-424) with E = I ------------------------------------------------------
    margin["prim_inf"] = np.inf
    if not _isnan(dy):
        d = np.where(uinf, np.where(linf, 0, np.minimum(dy, 0)), np.where(linf, np.maximum(dy, 0), dy))
        nd = _mx(np.abs(d))
        if nd > DIVISION_TOL:
            thr, b_thr = LD(eps_pinf) * nd, U * LD(eps_pinf) * nd
            sums["ineq_lhs"] = (u @ np.maximum(d, 0) + l @ np.minimum(d, 0), np.abs(u) @ np.maximum(d, 0) + np.abs(l) @ np.maximum(-d, 0), 2 * m)
            atd, s_atd = A.T @ d, aA.T @ np.abs(d)
            ok, margin["prim_inf"] = _verdict([
                _compare(sums["ineq_lhs"][0], _bar(2 * m, sums["ineq_lhs"][1]), thr, b_thr),
                _compare(_mx(np.abs(atd)), _mx(_bar(kAt, s_atd)), thr, b_thr)])
            val[14] = 1.0 if ok else 0.0

    # ---- slot 15: is_dual_infeasible (auxil.c:426-512) with D = E = I, c = 1 ---------------------------------------------
    margin["dual_inf"] = np.inf
    if not _isnan(dx):
        nd = _mx(np.abs(dx))
        if nd > DIVISION_TOL:
            thr, b_thr = LD(eps_dinf) * nd, U * LD(eps_dinf) * nd
            sums["q_dx"] = (q @ dx, np.abs(q) @ np.abs(dx), n)
            pd, s_pd = P @ dx, aP @ np.abs(dx)
            ad, b_ad = A @ dx, _bar(kA, aA @ np.abs(dx))
            rows = [_compare(sums["q_dx"][0], _bar(n, sums["q_dx"][1]), thr, b_thr),
                    _compare(_mx(np.abs(pd)), _mx(_bar(kP, s_pd)), thr, b_thr)]
            for i in range(m):           # a row passes when NOT (finite u and adx > thr) and NOT (finite l and adx < -thr)
                if u[i] < BINF:
                    h, g = _compare(ad[i], b_ad[i], thr, b_thr, less=False)
                    rows.append((not h, g))
                if l[i] > -BINF:
                    h, g = _compare(ad[i], b_ad[i], -thr, b_thr)
                    rows.append((not h, g))
            ok, margin["dual_inf"] = _verdict(rows)
            val[15] = 1.0 if ok else 0.0
    return SimpleNamespace(val=val.astype(np.float64), bar=bar.astype(np.float64), sums=sums, margin=margin)


def batch_reference(P, A, Q, L, Uu, X, Y, DX, DY, eps_abs, eps_rel, eps_pinf, eps_dinf, Px_all=None, Ax_all=None, members=None):
    """reference() for every member (or the listed ones) of a batch on the pattern of triu(P) and A (scipy CSC): the
    records [R, 16], the bars [R, 16], and the three margins [R] each.  X, Y, DX, DY are [R, .]: row r belongs to the r-th
    member of the call."""
    from scipy import sparse
    Pu = sparse.triu(P, format="csc"); Pu.sort_indices()
    Ac = sparse.csc_matrix(A); Ac.sort_indices()
    n, m = Pu.shape[0], Ac.shape[0]
    mem = range(Q.shape[0]) if members is None else list(members)
    out = [reference(n, m, Pu.indptr, Pu.indices, Pu.data if Px_all is None else Px_all[b], Ac.indptr, Ac.indices,
                     Ac.data if Ax_all is None else Ax_all[b], Q[b], L[b], Uu[b], X[r], Y[r], DX[r], DY[r], eps_abs, eps_rel,
                     eps_pinf, eps_dinf) for r, b in enumerate(mem)]
    return SimpleNamespace(val=np.array([o.val for o in out]), bar=np.array([o.bar for o in out]),
                           margin={k: np.array([o.margin[k] for o in out]) for k in ("optimal", "prim_inf", "dual_inf")},
                           members=out)


def assert_matches(V, ref, what=""):
    """The device records V [R, 16] against batch_reference: every float slot within its bar, every verdict equal."""
    V = np.asarray(V)
    assert V.shape == ref.val.shape, (what, V.shape, ref.val.shape)
    err = np.abs(V[:, :13] - ref.val[:, :13])
    bad = np.argwhere(~(err <= ref.bar[:, :13]))
    assert bad.size == 0, (what, [(int(r), FIELDS[k], float(V[r, k]), float(ref.val[r, k]), float(err[r, k]), float(ref.bar[r, k]))
                                  for r, k in bad[:6]])
    assert np.array_equal(V[:, 13:], ref.val[:, 13:]), (what, V[:, 13:].tolist(), ref.val[:, 13:].tolist())
