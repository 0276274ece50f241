"""numpy restatement of the common-K engine's shared-KKT route (osqp_amd/csrc/batch_common_kkt.h), no GPU.

The regularised solve by block elimination on scaled data,
    H = (P~ + delta I)^-1,  Wt = A~ H,  S = Ar H Ar' + delta I,
    [P~ + delta I, Ar'; Ar, -delta I] [x; nu] = [g1; g2]  <=>  t = H g1;  nu = S^-1 (Ar t - g2);  x = t - Wt[rows]' nu,
followed by exactly k refinement steps against the unregularised M = [P~, Ar'; Ar, 0].  Two versions: the float64 model
of the device route (every product in float64, the two inverses by np.linalg.inv), and the truth of the pieces H, Wt and
S^-1 in long double (_batch_parity.kinv_reference: numpy's inverse plus one Newton-Schulz step in long double).

BlockRoute is _planted_qp.Route with solve_model replaced, so block_model(c, b, k, ...) is _planted_qp.model with the
block route in place of the full one: the same scaling conventions (M [x; nu] = [g1; g2] <=> [x; c nu] = T M~^-1 T
[c g1; g2]), the same projection, the same adjoint and tangent formulas.

DEFECTS: one-place mistakes of the route, for test_common_kkt_reference_host.py to show that the bars tell them."""
import numpy as np

import _planted_qp as pq
from _batch_parity import kinv_reference

LD = np.longdouble
DEFECTS = ("delta_S", "delta_H", "stale_wt", "plus", "drop_g2", "step")


class BlockRoute(pq.Route):
    def __init__(self, mem, defect=None):
        super().__init__(mem)
        self.defect = defect
        self._blk = {}

    def pieces(self, delta):
        """(H, Wt on the active rows, S^-1) in float64, with the defect if one is set."""
        if delta not in self._blk:
            n, k, d = self.n, self.k, self.defect
            H = np.linalg.inv(self.M[:n, :n] + (0.0 if d == "delta_H" else delta) * np.eye(n))
            Wt = self.Ar @ H
            S = Wt @ self.Ar.T + (0.0 if d == "delta_S" else delta) * np.eye(k)
            Sinv = np.linalg.inv(S) if k else np.zeros((0, 0))
            if d == "stale_wt" and k:                # a row that belongs to another A: here, its own read backwards
                Wt = Wt.copy(); Wt[0] = Wt[0][::-1] * 2.0
            self._blk[delta] = (H, Wt, Sinv)
        return self._blk[delta]

    def apply(self, g, delta):
        H, Wt, Sinv = self.pieces(delta)
        n, d = self.n, self.defect
        t = H @ g[:n]
        nu = Sinv @ (self.Ar @ t - (0.0 if d == "drop_g2" else g[n:]))
        x = t + Wt.T @ nu if d == "plus" else t - Wt.T @ nu
        return np.concatenate([x, nu])

    def solve_model(self, g, k, delta):
        g = np.asarray(g, float)
        if self.defect == "step":                    # one refinement step too few
            k = k - 1
        s = self.apply(g, delta)
        for _ in range(max(k, 0)):
            s = s + self.apply(g - self.M @ s, delta)
        if self.defect == "step" and k < 0:          # (at k = 0 there is no step to leave out: one too many instead)
            s = s + self.apply(g - self.M @ s, delta)
        return s


def block_model(c, b, k, delta=1e-6, ws=None, point=None, defect=None):
    """_planted_qp.model(c, b, k, delta, ws, point) through the block route."""
    full = pq.Route
    pq.Route = lambda mem: BlockRoute(mem, defect)
    try:
        return pq.model(c, b, k, delta, ws, point)
    finally:
        pq.Route = full


def scaled_dense(P, A, ws):
    """(P~ full symmetric, A~) dense, from the handle's or the oracle's scaled values on the patterns of triu(P), A."""
    from scipy import sparse
    n, m = P.shape[0], A.shape[0]
    Pu = sparse.csc_matrix((np.asarray(ws["Pv"], float), P.indices, P.indptr), shape=(n, n))
    Ac = sparse.csc_matrix((np.asarray(ws["Av"], float), A.indices, A.indptr), shape=(m, n))
    return (Pu + sparse.triu(Pu, 1).T).toarray(), Ac.toarray().reshape(m, n)


def pieces_truth(Ps, As, rows, delta=1e-6):
    """Long-double truth of the pieces and numpy's own error against it: dict name -> (truth as float64, err_numpy).
    H and S^-1 as kinv_reference gives them; Wt = A~ H in long double.  rows: the member's active rows in the order of
    the device (lows first, then upps), or None for H and Wt alone."""
    n = Ps.shape[0]
    H_np, H_ld = kinv_reference(Ps + delta * np.eye(n))
    err = lambda a, t: float(np.abs(a.astype(LD) - t).max()) if t.size else 0.0
    out = dict(H=(H_ld.astype(float), err(H_np, H_ld)))
    Wt_ld = As.astype(LD) @ H_ld
    out["Wt"] = (Wt_ld.astype(float), err(As @ H_np, Wt_ld))
    if rows is not None and len(rows):
        Ar = As[rows]
        S = (Ar.astype(LD) @ H_ld @ Ar.astype(LD).T + LD(delta) * np.eye(len(rows), dtype=LD))
        S_np, S_ld = kinv_reference(S.astype(float))
        # (S itself is formed in long double and rounded once: its float64 image is what numpy inverts)
        out["Sinv"] = (S_ld.astype(float), err(S_np, S_ld))
    return out


def piece_bar(truth, err_np):
    """check_member_kinv's bar: ten times numpy's error plus 1e-14 of the largest entry."""
    return 10.0 * err_np + 1e-14 * (float(np.abs(truth).max()) if truth.size else 0.0)


# ---------------------------------------------------------------------------------------------- the family cases
# (n, m, B, seed) of common_family(n, m, B, seed): no rows, hence neither Wt nor S; the smallest with rows; off every
# 16 / 32 tile; NP = 64; NP = 160 with m past k_bp_active's 256-wide pass.  test_common_kkt_reference_host.py shows that
# at these seeds the oracle's own diagnostics excuse at most half of the solved members and leave two (one where the
# family leaves one).
FAMILY = [(1, 0, 3, 1001), (1, 1, 3, 1002), (17, 37, 5, 1054), (33, 66, 5, 2000), (129, 258, 4, 2004)]
FAMILY_KW = dict(adaptive_rho=0, scaled_termination=1, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000)
_family = {}


def family(shape):
    from _common_cases import common_family, mixed_family
    if shape not in _family:
        if shape == "mixed":
            _family[shape] = mixed_family()
        else:
            n, m, B, seed = shape
            _family[shape] = common_family(n, m, B, seed)[:5]
    return _family[shape]


def family_references(orc, shape):
    """Per member of the family: the pre-scaled oracle run with polish = 1, unscaled (x, y, obj, status_val,
    status_polish), and _adjoint_reference / _tangent_reference at that point for the draws of
    _tangent_reference.draws (gx, gy for the adjoint; dq, dl, du, dPx, dAx for the tangent).  Computed once, never
    modified.  Returns (ws of the common oracle, draws, [namespace per member])."""
    from _adjoint_reference import adjoint_reference
    from _batch_parity import oracle_ws
    from _common_cases import common_oracle, prescaled_oracle, unscale
    from _tangent_reference import draws, tangent_reference
    key = ("refs", shape)
    if key not in _family:
        P, A, Q, L, U = family(shape)
        B, n = Q.shape
        m = A.shape[0]
        ws = oracle_ws(common_oracle(orc, P, A, Q, L, U, **FAMILY_KW))
        Pu = sparse_triu(P)
        dr = draws((n, m, B, 1000 + n + m if shape == "mixed" else shape[3]), Pu.nnz, A.nnz)
        out = []
        for b in range(B):
            ro = prescaled_oracle(orc, ws, Q, L, U, b, polish=1, **FAMILY_KW).solve()
            x, y, obj = unscale(ws, ro)
            one = pq.SimpleNamespace(x=x, y=y, obj=obj, status_val=ro.info.status_val, status_polish=ro.info.status_polish,
                                     iter=ro.info.iter, adj=None, tan=None)
            if ro.info.status_val == 1:
                one.adj = adjoint_reference(P, A, L[b], U[b], x, y, dr.gx[b], dr.gy[b])
                one.tan = tangent_reference(P, A, x, y, dr.dq[b], dr.dl[b], dr.du[b], dr.dPx[b], dr.dAx[b])
            out.append(one)
        _family[key] = (ws, dr, out)
    return _family[key]


def sparse_triu(P):
    from scipy import sparse
    Pu = sparse.triu(sparse.csc_matrix(P), format="csc"); Pu.sort_indices()
    return Pu


def excuse(ref):
    """test_gpu_batch_adjoint.py's rule on the reference's own diagnostics ('' = the member is compared)."""
    why = []
    if ref.margin < 1e-6:
        why.append("complementarity margin %.1e" % ref.margin)
    if ref.sv_ratio < 1e-8:
        why.append("active rows dependent (%.1e)" % ref.sv_ratio)
    if ref.route_err > 1e-7:
        why.append("route model error %.1e" % ref.route_err)
    return ", ".join(why)
