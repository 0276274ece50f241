"""Cases of tests/test_gpu_batch_update_members.py and tests/test_update_members_cases_host.py: the member-list forms
of the matrix and rho updates (osqp_amd_batch_update_matrices_members[_dev], osqp_amd_batch_update_rho_members;
`update_matrices(members=)`, `update_rho(members=)` of osqp_amd/batch.py).

Shapes, the smallest at which the kernels differ: the tiled engine at n = 12 (tile 4), 65 (tile 8, off the tile) and the
MPC shape n = 120; the streamed engine at n = 40 and 150; m = 2 n, B = 5.  Problems and new values come from the
module-level generators of tests/test_gpu_batch_updates.py (`problem`, `new_values`), every member with new values of its
own, so that a compact row that lands on the wrong member solves another problem.

Lists: the first member, the last, two scattered ones, all but one, all B (the whole-batch twin) and a boolean mask.

Seeds: chosen on the CPU with the oracle alone (tests/test_update_members_cases_host.py runs the check): for every
member of every case the oracle's sequence setup, solve, update(Px, Ax), solve ends on the same iteration count,
rho_updates and status when the new values move by 1e-15 relative (three draws), both solves end `solved`, in every
list some listed member's rho moves in the first solve, the new values move D by more than 1e-3, and the member's
second solution differs by more than 1e-4 from the one with the old values, from the one with its new P alone and from
the ones with any other member's new values."""
import numpy as np

from test_gpu_batch_updates import new_values, problem, with_values

B = 5
KW = dict(adaptive_rho_interval=10)
# (engine, kind, n)
CASES = [("auto", "family", 12), ("auto", "family", 65), ("auto", "mpc", 120), ("streamed", "family", 40),
         ("streamed", "family", 150)]
IDS = ["%s-%s-%d" % c for c in CASES]
SEEDS = {("auto", "family", 12): 983, ("auto", "family", 65): 766, ("auto", "mpc", 120): 827,
         ("streamed", "family", 40): 742, ("streamed", "family", 150): 862}
LISTS = dict(first=[0], last=[B - 1], two=[1, 3], but_one=[0, 1, 2, 4], all=list(range(B)),
             mask=np.array([True, False, True, True, False]))
# How far A moves towards new_values' A.  The family's rows leave little room around the point x0 they were built to hold
# (1.4 n two-sided and equality rows in n variables): with the full move 588 of 600 members of the larger shapes end
# primal infeasible in the oracle (40 seeds each, profiles/batch_update_members_cases_full_step.txt) and no seed leaves
# all five solved, and an infeasible member's x is not compared.  P moves in full everywhere.
A_MOVE = {("auto", "family", 65): 0.02, ("streamed", "family", 40): 0.02, ("streamed", "family", 150): 0.02}
RHO = np.array([0.7, 0.03, 2.5, 0.4, 0.2])     # member b's new rho in the update_rho(members=) tests
PARITY = 1e-6             # the bar of tests/_batch_parity.assert_parity on x and y
_cases = {}


def members_of(S):
    """The indices a list or a mask names."""
    S = np.asarray(S)
    return np.flatnonzero(S) if S.dtype == np.bool_ else S.astype(np.int64)


def case_data(case):
    """(Pu, A, Q, L, U, Pn [B, nnzP], An [B, nnzA]) of a case: the problem and every member's new values (built once,
    never modified)."""
    if case not in _cases:
        _, kind, n = case
        seed = SEEDS[case]
        Pu, A, Q, L, U, _ = problem(kind, n, seed, nB=B)
        Pn, An = new_values(Pu, A, seed + 2, True, nB=B)
        An = A.data + A_MOVE.get(case, 1.0) * (An - A.data)
        for a in (Pu.data, A.data, Q, L, U, Pn, An):
            a.setflags(write=False)
        _cases[case] = (Pu, A, Q, L, U, Pn, An)
    return _cases[case]


def oracle_sequence(orc, case, b, Px=None, Ax=None, kw=KW, first=None, q=None, rho=None):
    """Member b's oracle run: setup, solve, update(Px, Ax) where given, update_rho(rho) where given, solve.  Returns
    (first results, second results, the oracle).  q: another linear cost than the case's."""
    from _batch_parity import oracle
    Pu, A, Q, L, U, _, _ = case_data(case)
    so = oracle(orc, Pu, Q[b] if q is None else q, A, L[b], U[b], **kw)
    r1 = so.solve()
    r1 = (r1.info.iter, r1.info.rho_updates, r1.info.status_val, np.array(r1.x), np.array(r1.y))
    if first is not None:
        first(so)
    upd = {k: v for k, v in (("Px", Px), ("Ax", Ax)) if v is not None}
    if upd:
        assert so.update(**upd) == 0
    if rho is not None:
        assert so.update_rho(float(rho)) == 0
    return r1, so.solve(), so


def seed_report(orc, case, draws=3):
    """What the seed of a case is chosen by, per member b, from oracle runs alone: `robust` (the sequence with the new
    values moved by 1e-15 relative ends on the same iteration count, rho_updates and status in both solves, `draws`
    draws), `rho_moved` (rho_updates of the first solve), `D_moved` (largest relative change of D through the update),
    `matters` (the smallest distance, as tests/_batch_parity.rel measures it on x and y, between the member's second
    solution and the one with the old values, with its new P and the old A, or with another member's new values),
    `idle_robust` and `rho_robust` (the sequences of a member that is not listed -- setup, solve, solve -- and of one
    that gets RHO[b] -- setup, solve, update_rho, solve -- end where they end when q moves by 1e-15 relative)."""
    from _batch_parity import oracle_ws, rel
    Pn, An = case_data(case)[5:]
    out = []
    for b in range(B):
        D = []
        r1, r2, so = oracle_sequence(orc, case, b, Pn[b], An[b], first=lambda so: D.append(oracle_ws(so)["D"].copy()))
        D.append(oracle_ws(so)["D"])
        end = lambda r: (r.info.iter, r.info.rho_updates, r.info.status_val)
        rng = np.random.default_rng(1000 * SEEDS[case] + b)
        robust = True
        for _ in range(draws):
            wP = Pn[b] * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], Pn[b].size))
            wA = An[b] * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], An[b].size))
            q1, q2, _ = oracle_sequence(orc, case, b, wP, wA)
            robust = robust and q1[:3] == r1[:3] and end(q2) == end(r2)
        Q = case_data(case)[2]
        idle, rho = oracle_sequence(orc, case, b), oracle_sequence(orc, case, b, rho=RHO[b])
        idle_robust = rho_robust = True
        for _ in range(draws):
            wq = Q[b] * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], Q[b].size))
            for ref, kw in ((idle, {}), (rho, dict(rho=RHO[b]))):
                q1, q2, _ = oracle_sequence(orc, case, b, q=wq, **kw)
                same = q1[:3] == ref[0][:3] and end(q2) == end(ref[1])
                idle_robust, rho_robust = (idle_robust and same, rho_robust) if not kw else (idle_robust, rho_robust and same)
        others = [oracle_sequence(orc, case, b)[1], oracle_sequence(orc, case, b, Pn[b])[1]] + [oracle_sequence(orc, case, b, Pn[o], An[o])[1] for o in range(B) if o != b]
        dist = min(max(rel(o.x, r2.x), rel(o.y, r2.y)) for o in others)
        out.append(dict(robust=robust, rho_moved=int(r1[1]), D_moved=float((np.abs(D[1] - D[0]) / np.abs(D[0])).max()),
                        matters=float(dist), status=(r1[2], r2.info.status_val), idle_robust=idle_robust,
                        rho_robust=rho_robust, rho_status=rho[1].info.status_val))
    return out


def twin_arrays(setup_values, S, new, idx=None):
    """The [B, k] array of the whole-batch call that says what a member call says: the rows of the listed members S
    hold `new` ([k], written to each of them, or compact [count, k]), the others repeat the values the handle holds
    (setup_values: [nnz] shared or [B, nnz]), at the slots idx where an index list is given."""
    cur = np.broadcast_to(setup_values, (B, setup_values.shape[-1]))
    out = np.array(cur if idx is None else cur[:, idx])
    out[members_of(S)] = new
    return out


__all__ = ["B", "KW", "CASES", "IDS", "LISTS", "PARITY", "members_of", "case_data", "oracle_sequence", "twin_arrays",
           "with_values"]
