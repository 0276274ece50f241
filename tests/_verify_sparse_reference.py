"""tests/_verify_reference.reference restated with sparse long-double arithmetic, for OSQP.verify (osqp_amd_verify,
osqp_amd/csrc/verify.h) on problems too large for dense matrices: the same 16 values, the same bars, the same verdict
margins, from the CSC arrays of triu(P) and A.  Nothing here comes from the code under test.

The bar of a sum of k terms keeps its formula, (k + C) * 2^-53 * sum |t_i|, for any order of summation (see
_verify_reference), so it binds the wavefront and workgroup sums of k_ver_point as it binds k_batch_verify.  One of the
four units of C = 4 there is the long-double side's own error, k * 2^-64 * sum |t_i| = (k / 2048) * 2^-53 * sum |t_i|,
which fits one unit only while k <= 2048.  Here that unit grows with the row:

    C(k) = 3 + max(1, ceil(k / 2048)),

4 for k <= 2048 -- the dense reference's bars, bit for bit -- and never more than 4 + ceil(k / 2048).

    reference(..., skip_row=None, skip_col=None) -> the namespace of _verify_reference.reference.

drop = (i, j) is the dense reference's planted defect (the lower half P_ji left out); drop_at = (r, c) leaves out the one
entry at row r, column c of the symmetric P, whichever half it is in.  skip_row = i / skip_col = j plant
the defect of a sweep that never reaches row i of A / column j: the row's (column's) entry of A x (P x, A'y, q) is left
out of every maximum and sum taken over the rows (columns)."""
from types import SimpleNamespace

import numpy as np

from _verify_reference import LD, U, C, OSQP_INFTY, BINF, DIVISION_TOL, _isnan, _mx, _compare, _verdict


def _bar(k, s):
    k = np.asarray(k, LD)
    return (k + 3 + np.maximum(1, np.ceil(k / 2048))) * U * np.asarray(s, LD)


class _Mat:
    """A sparse matrix as triplets in long double: products with a vector, with absolute values, and entries per row."""

    def __init__(self, shape, rows, cols, vals):
        self.shape, self.r, self.c = shape, np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        self.v = np.asarray(vals, np.float64).astype(LD)

    def _dot(self, vals, x, by_col):
        out = np.zeros(self.shape[1 if by_col else 0], LD)
        np.add.at(out, self.c if by_col else self.r, vals * x[self.r if by_col else self.c])
        return out

    def dot(self, x):
        return self._dot(self.v, x, False)

    def absdot(self, x):
        return self._dot(np.abs(self.v), np.abs(x), False)

    def tdot(self, y):
        return self._dot(self.v, y, True)

    def abstdot(self, y):
        return self._dot(np.abs(self.v), np.abs(y), True)

    def per_row(self):
        return np.bincount(self.r, minlength=self.shape[0]).astype(np.float64)

    def per_col(self):
        return np.bincount(self.c, minlength=self.shape[1]).astype(np.float64)


def matrices(n, m, Pp, Pi, Px, Ap, Ai, Ax, drop=None, drop_at=None):
    """(P full symmetric, A) as _Mat; a stored zero is an entry (the kernel adds it)."""
    Pp, Ap = np.asarray(Pp, np.int64), np.asarray(Ap, np.int64)
    nnzP, nnzA = int(Pp[n]), int(Ap[n])
    pr, pv = np.asarray(Pi, np.int64)[:nnzP], np.asarray(Px, np.float64)[:nnzP]
    pc = np.repeat(np.arange(n), np.diff(Pp))
    off = pr != pc
    up, lo = pv.copy(), pv[off].copy()
    if drop is not None:
        lo[(pr[off] == drop[0]) & (pc[off] == drop[1])] = 0.0
    if drop_at is not None:
        up[(pr == drop_at[0]) & (pc == drop_at[1])] = 0.0
        lo[(pc[off] == drop_at[0]) & (pr[off] == drop_at[1])] = 0.0
    P = _Mat((n, n), np.concatenate([pr, pc[off]]), np.concatenate([pc, pr[off]]), np.concatenate([up, lo]))
    A = _Mat((m, n), np.asarray(Ai, np.int64)[:nnzA], np.repeat(np.arange(n), np.diff(Ap)), np.asarray(Ax, np.float64)[:nnzA])
    return P, A


def reference(n, m, Pp, Pi, Px, Ap, Ai, Ax, q, l, u, x, y, dx, dy, eps_abs, eps_rel, eps_pinf, eps_dinf, drop=None,
              drop_at=None, skip_row=None, skip_col=None):
    P, A = matrices(n, m, Pp, Pi, Px, Ap, Ai, Ax, drop, drop_at)
    f = lambda v, k: np.asarray(v, np.float64).reshape(-1)[:k].astype(LD)
    q, x, dx = f(q, n), f(x, n), f(dx, n)
    l, u, y, dy = f(l, m), f(u, m), f(y, m), f(dy, m)
    rows, cols = np.ones(m, bool), np.ones(n, bool)          # what the sweeps reach
    if skip_row is not None:
        rows[skip_row] = False
    if skip_col is not None:
        cols[skip_col] = False
    val, bar, sums, margin = np.zeros(16, LD), np.zeros(16, LD), {}, {}
    kP, kA, kAt = P.per_row(), A.per_row(), A.per_col()
    uinf, linf = u > BINF, l < -BINF

    # ---- slots 0-13 ----------------------------------------------------------------------------------------------------
    xs, ys = np.where(np.isnan(x), 0, x), np.where(np.isnan(y), 0, y)
    ax, s_ax = A.dot(xs), A.absdot(xs)
    z = np.minimum(np.maximum(ax, l), u)
    px, s_px = P.dot(xs), P.absdot(xs)
    aty, s_aty = A.tdot(ys), A.abstdot(ys)
    b_ax, b_px, b_aty = _bar(kA, s_ax), _bar(kP, s_px), _bar(kAt, s_aty)
    yp, ym = np.maximum(ys, 0), np.maximum(-ys, 0)
    on_inf = bool(np.any((yp != 0) & uinf & rows) or np.any((ym != 0) & linf & rows))
    xc, qc = np.where(cols, xs, 0), np.where(cols, q, 0)     # the terms of the sums over the columns
    xpx_terms = LD(0.5) * (np.abs(xc) @ s_px)
    k_xpx = kP[cols].sum()
    sums["obj"] = (LD(0.5) * (xc @ px) + qc @ xs, xpx_terms + np.abs(qc) @ np.abs(xs), k_xpx + n)
    fu, fl = np.where(uinf | ~rows, 0, u), np.where(linf | ~rows, 0, l)
    sums["dual_obj"] = (-LD(0.5) * (xc @ px) - (fu @ yp - fl @ ym), xpx_terms + np.abs(fu) @ yp + np.abs(fl) @ ym, k_xpx + 2 * m)
    val[0], bar[0] = sums["obj"][0], _bar(sums["obj"][2], sums["obj"][1])
    val[1], bar[1] = _mx(np.abs(ax - z)[rows]), _mx(b_ax[rows])
    dua, s_dua, k_dua = px + q + aty, s_px + np.abs(q) + s_aty, kP + kAt + 1
    val[2], bar[2] = _mx(np.abs(dua)[cols]), _mx(_bar(k_dua, s_dua)[cols])
    val[3], bar[3] = _mx(np.abs(ax)[rows]), _mx(b_ax[rows])
    val[4], bar[4] = _mx(np.abs(z)[rows]), _mx(b_ax[rows])
    val[5], bar[5] = _mx(np.abs(px)[cols]), _mx(b_px[cols])
    val[6], bar[6] = _mx(np.abs(aty)[cols]), _mx(b_aty[cols])
    val[7], bar[7] = _mx(np.abs(q)[cols]), 0
    val[8] = LD(eps_abs) + LD(eps_rel) * max(val[3], val[4])
    bar[8] = LD(eps_rel) * max(bar[3], bar[4]) + C * U * val[8]
    val[9] = LD(eps_abs) + LD(eps_rel) * max(val[5], val[6], val[7])
    bar[9] = LD(eps_rel) * max(bar[5], bar[6]) + C * U * val[9]
    if on_inf:
        val[10], val[11], val[12] = OSQP_INFTY, -OSQP_INFTY, OSQP_INFTY
    else:
        ypr, ymr = np.where(rows, yp, 0), np.where(rows, ym, 0)
        fuz, flz = np.where(uinf, 0, u), np.where(linf, 0, l)
        tu, tl = ypr * (fuz - z), ymr * (z - flz)
        val[10] = max(_mx(tu), _mx(tl), LD(0))
        bar[10] = max(_mx(_bar(kA + 1, ypr * (np.abs(fuz) + s_ax))), _mx(_bar(kA + 1, ymr * (np.abs(flz) + s_ax))), LD(0))
        val[11], bar[11] = sums["dual_obj"][0], _bar(sums["dual_obj"][2], sums["dual_obj"][1])
        val[12] = val[0] - val[11]
        bar[12] = _bar(sums["obj"][2] + sums["dual_obj"][2], sums["obj"][1] + sums["dual_obj"][1])
    opt, margin["optimal"] = _verdict([_compare(val[1], bar[1], val[8], bar[8]), _compare(val[2], bar[2], val[9], bar[9])])
    val[13] = 1.0 if opt else 0.0
    if _isnan(x) or _isnan(y):
        val[:13], bar[:13], val[13], margin["optimal"] = float(0x7FC00000), 0, 0.0, np.inf

    # ---- slot 14: is_primal_infeasible (auxil.c:361-424) with E = I ------------------------------------------------------
    margin["prim_inf"] = np.inf
    if not _isnan(dy):
        d = np.where(uinf, np.where(linf, 0, np.minimum(dy, 0)), np.where(linf, np.maximum(dy, 0), dy))
        dr = np.where(rows, d, 0)
        nd = _mx(np.abs(dr))
        if nd > DIVISION_TOL:
            thr, b_thr = LD(eps_pinf) * nd, U * LD(eps_pinf) * nd
            sums["ineq_lhs"] = (u @ np.maximum(dr, 0) + l @ np.minimum(dr, 0), np.abs(u) @ np.maximum(dr, 0) + np.abs(l) @ np.maximum(-dr, 0), 2 * m)
            atd, s_atd = A.tdot(d), A.abstdot(d)
            ok, margin["prim_inf"] = _verdict([
                _compare(sums["ineq_lhs"][0], _bar(2 * m, sums["ineq_lhs"][1]), thr, b_thr),
                _compare(_mx(np.abs(atd)[cols]), _mx(_bar(kAt, s_atd)[cols]), thr, b_thr)])
            val[14] = 1.0 if ok else 0.0

    # ---- slot 15: is_dual_infeasible (auxil.c:426-512) with D = E = I, c = 1 ---------------------------------------------
    margin["dual_inf"] = np.inf
    if not _isnan(dx):
        nd = _mx(np.abs(dx)[cols])
        if nd > DIVISION_TOL:
            thr, b_thr = LD(eps_dinf) * nd, U * LD(eps_dinf) * nd
            dc = np.where(cols, dx, 0)
            sums["q_dx"] = (q @ dc, np.abs(q) @ np.abs(dc), n)
            pd, s_pd = P.dot(dx), P.absdot(dx)
            ad, b_ad = A.dot(dx), _bar(kA, A.absdot(dx))
            tests = [_compare(sums["q_dx"][0], _bar(n, sums["q_dx"][1]), thr, b_thr),
                     _compare(_mx(np.abs(pd)[cols]), _mx(_bar(kP, s_pd)[cols]), thr, b_thr)]
            for i in np.flatnonzero(rows):
                if u[i] < BINF:
                    h, g = _compare(ad[i], b_ad[i], thr, b_thr, less=False)
                    tests.append((not h, g))
                if l[i] > -BINF:
                    h, g = _compare(ad[i], b_ad[i], -thr, b_thr)
                    tests.append((not h, g))
            ok, margin["dual_inf"] = _verdict(tests)
            val[15] = 1.0 if ok else 0.0
    return SimpleNamespace(val=val.astype(np.float64), bar=bar.astype(np.float64), sums=sums, margin=margin)


def assert_matches(V, ref, what=""):
    """One device record V [16] against reference(): every float slot within its bar, every verdict equal."""
    from _verify_reference import FIELDS
    V = np.asarray(V, np.float64)
    assert V.shape == (16,), (what, V.shape)
    err = np.abs(V[:13] - ref.val[:13])
    bad = [(FIELDS[k], float(V[k]), float(ref.val[k]), float(err[k]), float(ref.bar[k])) for k in range(13) if not err[k] <= ref.bar[k]]
    assert not bad, (what, bad)
    assert np.array_equal(V[13:], ref.val[13:]), (what, V[13:].tolist(), ref.val[13:].tolist())
