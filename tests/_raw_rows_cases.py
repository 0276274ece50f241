"""Cases of tests/test_gpu_batch_raw_rows.py and of its host companion tests/test_batch_raw_rows_host.py: per engine the
problem of tests/_members_cases.py, new q, l, u for the members of the list `three`, new values of A for the batch, and
the oracle of every member on the new data and the new values.

The oracle: on the tiled and the streamed engine the member's own run, set up on (P, q, A', l, u).  The common-K
engine shares one scaling over the batch, so there it is the yardstick of tests/_common_cases.py: the run on the
member's data pre-scaled with the common D, E, c of (P, q^, A'), brought back to the member's own units."""
from types import SimpleNamespace

import numpy as np
from scipy import sparse

from _batch_parity import oracle, oracle_ws
from _common_cases import common_oracle, prescaled_oracle, unscale
from _members_cases import B, FIXED_RHO, LISTS, new_rows, problem, whole

S = np.asarray(LISTS["three"])
_cases = {}


def case(engine):
    """P, A, Q, L, U of setup; rows: the compact new Q, L, U of the members S; full: the [B, .] arrays that say the same;
    The rows are new_rows' "Q", "L" and "U" rows brought together: the bounds move outward, so every member stays
    feasible.  Its "QLU" rows shift l and u of every row by a step of the row's own, and equality rows that share their
    columns (m = 2 n, up to three entries per row) then contradict each other: the oracle ends primal infeasible on
    listed members of the streamed and the common-K case, whatever the seed.
    Ax2, A2: the new values of A in CSC order and the matrix that holds them -- Ax times one seeded factor in [0.8, 1.2]
    for the whole matrix: every member stays feasible (its x0 divided by the factor), which a factor per entry does not
    keep on the equality rows."""
    if engine not in _cases:
        P, A, Q, L, U = problem(engine)
        cur = dict(Q=Q, L=L, U=U)
        rows = {k: new_rows(engine, cur, S, k, 41 + i)[k] for i, k in enumerate("QLU")}
        Ac = sparse.csc_matrix(A)
        Ac.sort_indices()
        Ax2 = Ac.data * np.random.default_rng(43).uniform(0.8, 1.2)
        A2 = sparse.csc_matrix((Ax2, Ac.indices, Ac.indptr), shape=Ac.shape)
        _cases[engine] = SimpleNamespace(pb=(P, A, Q, L, U), rows=rows, full=whole(cur, S, rows), Ax2=Ax2, A2=A2)
    return _cases[engine]


def oracle_runs(orc, engine):
    """Every member's expected results on the new data and the new values, as assert_parity takes them."""
    c = case(engine)
    P = c.pb[0]
    Q, L, U = c.full["Q"], c.full["L"], c.full["U"]
    kw = FIXED_RHO[engine]
    if engine != "common":
        return [oracle(orc, P, Q[b], c.A2, L[b], U[b], **kw).solve() for b in range(B)]
    ws = oracle_ws(common_oracle(orc, P, c.A2, Q, L, U, **kw))
    out = []
    for b in range(B):
        ro = prescaled_oracle(orc, ws, Q, L, U, b, **kw).solve()
        x, y, obj = unscale(ws, ro)
        out.append(SimpleNamespace(x=x, y=y, info=SimpleNamespace(status_val=ro.info.status_val, iter=ro.info.iter,
                                                                  rho_updates=ro.info.rho_updates, obj_val=obj)))
    return out
