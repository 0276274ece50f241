"""Cases and reference of `BatchOSQP.update_model` (osqp_amd_batch_common_update_model): new values for the shared model of
a live common-K handle.

ModelReference is _common_reference.CommonReference -- the batch loop in long double -- with the one call added, as the
header states it: P, A, q, l, u, D, E, c become those of the new scaled space (the scale_data of setup on the new raw
values and q^ over the raw Q the handle holds now); x, z, y (scaled), rho and the row classes stay; rho_updates restarts
and the status is unsolved again; K is re-formed with the rho in force.  `defect` plants one of five one-place mistakes
of that call; tests/test_common_model_cases_host.py shows that each of them misses the bars of the GPU tests by more
than ten times on a named case.

The new values are moved as test_gpu_batch_updates.new_values moves them (the diagonal of P by 1.3 - 1.9, the rest of P
by 0.5 - 1.0, A by 0.5 - 1.8), so D and E really move.

MODEL_CASES: name -> (n, m, qscale, B, seed, factor on Q given by an `update` before the first solve, crossing row).
Every case runs setup -> [update(Q = factor Q)] -> solve (max_iter = 20: nobody has finished, rho has moved) ->
update_model -> solve, with adaptive_rho_interval = 10.  The handle keeps its max_iter, so the second solve makes 20
iterations as well.
  "M33", "M129"   the adaptive families of _common_cases.ADAPTIVE_CASES.  (129, 258) with seed 1396, not the family's own
                  1387: with that one, and with six of the twelve seeds after it, a member's second solve ends on an
                  approximate primal-infeasibility certificate -- twenty iterations after new matrix values the step of y
                  is still large --, which the reference does not model (split_solve_fires; the host test shows it on
                  the oracle)
  "M33-65"        B = 65: the second workgroup of the element-wise kernels and a second column tile of the GEMM
  "M33-q"         update(Q = 3 Q) after setup: q^ at the call is that of 3 Q, not setup's
  "M33-cross"     one inequality row has, in every member, the width 1e-4 / sqrt(E_old E_new): an equality row on the
                  scaled bounds of setup, an inequality row under the new E -- the call keeps it an equality row
"""
import numpy as np
from scipy import sparse

from _batch_parity import oracle_ws
from _common_cases import ADAPTIVE, common_family, common_oracle, prescaled, row_classes
from _common_reference import CommonReference
from test_gpu_batch_updates import new_values, with_values

DEFECTS = ("stale_qhat", "reclassify", "zero_iterates", "reset_rho", "keep_rho_updates")

MODEL_CASES = {
    "M33": (33, 66, 100.0, 5, 1099, None, False),
    "M129": (129, 258, 100.0, 5, 1396, None, False),
    "M33-65": (33, 66, 100.0, 65, 1099, None, False),
    "M33-q": (33, 66, 100.0, 5, 1099, 3.0, False),
    "M33-cross": (33, 66, 100.0, 5, 1099, None, True),
}
MODEL_KW = dict(ADAPTIVE, scaled_termination=1, max_iter=20)
LAYER_SHAPE = (17, 37, 4, 1054)      # (n, m, B, seed) of the layer test: _common_kkt_layer_worker's family
# the case on which each defect has to show (test_common_model_cases_host.py)
DEFECT_CASE = dict(stale_qhat="M33-q", reclassify="M33-cross", zero_iterates="M33", reset_rho="M33", keep_rho_updates="M33")


def sorted_model(P, A):
    """triu(P) and A in CSC with sorted indices: the order of the value arrays."""
    Pu = sparse.triu(sparse.csc_matrix(P), format="csc"); Pu.sort_indices()
    A = sparse.csc_matrix(A); A.sort_indices()
    return Pu, A


def moved_model(P, A, seed):
    """(Pu, A, Pu', A', Px', Ax'): the model with sorted indices, and new_values' move of it."""
    Pu, A = sorted_model(P, A)
    Px, Ax = new_values(Pu, A, seed, False)
    return Pu, A, with_values(Pu, Px), with_values(A, Ax), Px, Ax


# The fresh-handle comparison: (n, m, B), what the call updates, with the shared pieces.  Every shape of
# _common_cases.CASES with full arrays; index subsets, P alone and A alone at (17, 37); a handle without the pieces at
# (33, 66); (300, 600): k_bc_qhat's second workgroup and the pivots' second column block; B = 65: the second workgroup
# over members.
BITS = [((1, 0, 5), "full", True), ((1, 1, 5), "full", True), ((17, 37, 5), "full", True), ((17, 37, 5), "idx", True),
        ((17, 37, 5), "P", True), ((17, 37, 5), "A", True), ((33, 66, 5), "full", False), ((33, 66, 5), "idx", False),
        ((33, 66, 65), "full", True), ((129, 258, 5), "idx", True), ((300, 600, 5), "full", True)]


def bits_case(shape, mode):
    """A case of BITS: the model the handle is set up on (Pu, A with `start` values), the arguments of update_model that
    bring it to the moved model (P2, A2) whatever the mode -- the slots the call leaves alone hold their new values from
    the start --, and Q, L, U of common_family on the MOVED model, so that its feasible points are those of the model the
    solves run on."""
    from _batch_parity import shape_family
    n, m, B = shape
    seed = 1000 + n + m
    Pu, A, P2, A2, Px, Ax = moved_model(*shape_family(n, m, 1, seed)[:2], seed + 1)
    _, _, Q, L, U, _ = common_family(n, m, B, seed, PA=(P2, A2))
    startP, startA, kw = Px.copy(), Ax.copy(), {}
    if mode == "idx":                                    # every other slot of P, every third of A, in descending order
        iP, iA = np.arange(0, Pu.nnz, 2)[::-1].copy(), np.arange(0, A.nnz, 3)[::-1].copy()
        startP[iP], startA[iA] = Pu.data[iP], A.data[iA]
        kw = dict(Px=Px[iP], Px_idx=iP)
        if A.nnz:
            kw.update(Ax=Ax[iA], Ax_idx=iA)
    if mode in ("full", "P"):
        startP = Pu.data.copy(); kw["Px"] = Px
    if mode in ("full", "A") and A.nnz:
        startA = A.data.copy(); kw["Ax"] = Ax
    return dict(P0=with_values(Pu, startP), A0=with_values(A, startA), kw=kw, P2=P2, A2=A2, Px=Px, Ax=Ax, Q=Q, L=L, U=U)


def qhat_test_q(Q):
    """The larger Q that test_qhat_follows_update gives through `update` before the call: 3 Q, every other column 6 Q."""
    Q2 = 3.0 * Q
    Q2[:, ::2] *= 2.0
    return Q2


def model_case(orc, name):
    """Everything a named case needs: Pu, A, Q (as set up), Q2 (as held at the call; Q itself without an update), L, U,
    Px', Ax', P', A', the settings, ws_old / ws_new (the oracle's common scaled spaces before and after the call) and
    ws_stale (the new values scaled with setup's q^)."""
    n, m, qscale, B, seed, qfactor, cross = MODEL_CASES[name]
    P, A, Q, L, U, _ = common_family(n, m, B, seed)
    Q = Q * qscale
    Pu, A, P2, A2, Px, Ax = moved_model(P, A, seed + 1)
    Q2 = Q if qfactor is None else Q * qfactor
    kw = dict(MODEL_KW)
    spaces = lambda L_, U_: (oracle_ws(common_oracle(orc, Pu, A, Q, L_, U_, **kw)), oracle_ws(common_oracle(orc, P2, A2, Q2, L_, U_, **kw)))
    row = None
    if cross:
        w0, w1 = spaces(L, U)
        # an inequality row, two-sided in every member, whose E moves by more than 20 % either way
        ratio = w1["E"] / w0["E"]
        two = np.all(np.isfinite(L) & np.isfinite(U), axis=0) & (w0["ctype"] == 0)
        cand = np.flatnonzero(two & (ratio > 1.2))
        assert cand.size, "no row for the crossing case"
        row = int(cand[np.argmax(ratio[cand])])
        width = 1e-4 / np.sqrt(w0["E"][row] * w1["E"][row])
        L, U = L.copy(), U.copy()
        mid = 0.5 * (L[:, row] + U[:, row])
        L[:, row], U[:, row] = mid - 0.5 * width, mid + 0.5 * width
    ws_old, ws_new = spaces(L, U)
    ws_stale = oracle_ws(common_oracle(orc, P2, A2, Q, L, U, **kw))
    return dict(name=name, Pu=Pu, A=A, Q=Q, Q2=Q2, L=L, U=U, Px=Px, Ax=Ax, P2=P2, A2=A2, kw=kw, ws_old=ws_old, ws_new=ws_new,
                ws_stale=ws_stale, row=row, B=B)


def classes_under(ws, L, U):
    """row_classes of every member on the bounds scaled with ws's E: [B, m]."""
    return np.array([row_classes(L[b], U[b], ws["E"]) for b in range(L.shape[0])])


class ModelReference(CommonReference):
    def update_model(self, ws_new, Q, L, U, defect=None, ws_stale=None):
        """The call, with the handle's raw Q, L, U as they stand.  defect: one of DEFECTS (stale_qhat takes ws_stale, the
        new values scaled with an outdated q^)."""
        assert defect is None or defect in DEFECTS, defect
        LD, B = self.ld, self.B
        ws = ws_stale if defect == "stale_qhat" else ws_new
        self.ws = ws
        self.P = (ws["Pu"] + sparse.triu(ws["Pu"], 1).T).toarray().astype(LD)
        self.A = ws["A"].toarray().astype(LD)
        data = [prescaled(ws, Q, L, U, b) for b in range(B)]
        self.q = np.array([d[1] for d in data], dtype=LD).reshape(B, self.n)
        self.l = np.array([d[3] for d in data], dtype=LD).reshape(B, self.m)
        self.u = np.array([d[4] for d in data], dtype=LD).reshape(B, self.m)
        self.D, self.E, self.c = ws["D"].astype(LD), ws["E"].astype(LD), LD(ws["c"])
        if defect == "reclassify":
            self.ctype = row_classes(L[0], U[0], ws["E"])
        if defect == "zero_iterates":
            self.x[:] = 0; self.z[:] = 0; self.y[:] = 0
        if defect != "keep_rho_updates":
            self.rho_updates[:] = 0
        self.status[:] = 0
        self._set_rho(ws["rho"] if defect == "reset_rho" else self.rho)


def _fires(ref, dx, dy, eps_pinf, eps_dinf):
    """The two infeasibility tests of the approximate check_termination (auxil.c:320-470, 709-800) with
    scaled_termination = 1, per member, on the last step dx, dy of the scaled iterates: [B] bool, True where either
    fires.  As there, a test is made only where the residual of its side misses its tolerance."""
    s = ref._info()
    ea, er = 10 * ref.st["eps_abs"], 10 * ref.st["eps_rel"]
    INF = 1e30 * 1e-4                                     # OSQP_INFTY * MIN_SCALING
    out = np.zeros(ref.B, bool)
    for b in range(ref.B):
        prim_ok = ref.m == 0 or s.pri[b] < ea + er * max(s.nz[b], s.nax[b])
        dual_ok = s.dua[b] < ea + er * max(s.nq[b], s.naty[b], s.npx[b])
        ny = np.abs(dy[b]).max(initial=0)
        if not prim_ok and ny > eps_pinf:
            up = np.where(ref.u[b] < INF, ref.u[b] * np.maximum(dy[b], 0), 0).sum()
            lo = np.where(ref.l[b] > -INF, ref.l[b] * np.minimum(dy[b], 0), 0).sum()
            if up + lo < -eps_pinf * ny and np.abs(dy[b] @ ref.A).max() < eps_pinf * ny:
                out[b] = True
        nx = np.abs(dx[b]).max(initial=0)
        if not dual_ok and nx > eps_dinf and ref.q[b] @ dx[b] < -eps_dinf * nx and np.abs(ref.P @ dx[b]).max() < eps_dinf * nx:
            adx = ref.A @ dx[b]
            ok = np.where(ref.u[b] < INF, adx < eps_dinf * nx, True) & np.where(ref.l[b] > -INF, adx > -eps_dinf * nx, True)
            out[b] |= bool(ok.all())
    return out


def split_solve_fires(ref, factors=(0.5, 1.0, 2.0)):
    """CommonReference models no infeasibility certificate, and at max_iter = 20 the approximate tests (eps x 10) are made
    on a run in mid-flight.  Runs ref's next solve of 20 iterations as 19 + 1 -- checks and adaptations change no
    iterate, so the iterates are those of the run of 20 -- and says whether either test fires for any member on the step
    of iteration 20, at the given multiples of the approximate eps (1e-3).  The adaptation due at iteration 20 is not
    made by the split run: the caller sets rho."""
    ref.st["max_iter"] = 19
    ref.solve()
    x, y = ref.x.copy(), ref.y.copy()
    ref.st["max_iter"] = 1
    ref.solve()
    ref.st["max_iter"] = 20
    return any(_fires(ref, ref.x - x, ref.y - y, f * 1e-3, f * 1e-3).any() for f in factors)


def certificates_fire(orc, name):
    """split_solve_fires for the two solves of a named case: [first solve, second solve]."""
    c, _, _, rho = model_reference(orc, name)
    ref = ModelReference(c["ws_old"], c["Q2"], c["L"], c["U"], **c["kw"])
    first = split_solve_fires(ref)
    ref._set_rho(rho)
    ref.update_model(c["ws_new"], c["Q2"], c["L"], c["U"])
    return [first, split_solve_fires(ref)]


_RUNS = {}


def model_reference(orc, name, defect=None):
    """(case, reference after its run, [result of the first solve, result of the second], rho at the call) of a named
    case; computed once per process and shared -- callers leave all of it unchanged."""
    if (name, defect) not in _RUNS:
        c = model_case(orc, name)
        st = {k: v for k, v in c["kw"].items()}
        ref = ModelReference(c["ws_old"], c["Q2"], c["L"], c["U"], **st)
        r1 = ref.solve()
        rho = float(ref.rho)
        ref.update_model(c["ws_new"], c["Q2"], c["L"], c["U"], defect=defect, ws_stale=c["ws_stale"])
        r2 = ref.solve()
        _RUNS[name, defect] = (c, ref, [r1, r2], rho)
    return _RUNS[name, defect]
