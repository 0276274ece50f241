"""Cases of the per-call limits of a batch solve (`BatchOSQP.solve(max_iter=, time_limit=)`,
osqp_amd_batch_solve_limited): for each engine the smallest shape at which its code path exists, built from the
generators the other batch tests use, and the settings of the three kinds of test.

  budget    termination checked every CHECK iterations, rho adapted every 10: the iteration caps of KS sit at 1, around
            a check, on a rho adaptation and past convergence;
  expired   eps_abs = eps_rel = EPS on a cold start with check_termination = 0, so that the clock is first looked at in
            iteration INTERVAL.  tests/test_batch_limits_cases_host.py proves on the CPU oracle that no member passes the
            exact test in its first INTERVAL iterations, which makes "every member ends at INTERVAL" a fair assertion;
            rho is adapted in that very iteration, so a streamed member has a rebuild due when the clock stops it.
            The setup's cap is EXPIRED_MAX_ITER: without checks the streamed engine's plain solve that follows runs to
            the cap, and its verdicts -- the rho estimate, the approximate test -- have to stay away from residuals at
            the level of the K^-1 solve's error (1e-11 here), where they are noise that differs from the oracle's.
            Measured: after 30 more iterations every streamed member's residuals are above 2e-7;
  between   EPS again, checks every CHECK iterations: hundreds of iterations, so that half the time stops some members.

The common-K engine is compared with the reference run on the member's pre-scaled data (tests/_common_cases.py), which
has no batch rho: its oracle comparisons run with a fixed rho."""
from _batch_parity import oracle, oracle_ws, shape_family
from _common_cases import FIXED, common_family, common_oracle, prescaled_oracle, unscale

INTERVAL = 25          # BATCH_CLOCK_INTERVAL of batch_admm.h: the reference's default check interval
CHECK = 5              # check_termination of the budget and in-between cases
EPS = 1e-9
MAX_ITER = 4000        # the setup's cap (the default)
EXPIRED_MAX_ITER = 30  # ... of the expired cases: one more rho adaptation in the plain solve that follows

SHAPES = {             # engine= of setup, n, m, B, seed
    "tile4": ("auto", 12, 24, 6, 1201),
    "tile8": ("auto", 70, 30, 5, 1202),
    "streamed": ("streamed", 40, 60, 6, 1203),
    "common": ("common", 40, 60, 70, 1204),        # two groups of 64 columns, so a pack can happen
}
ADAPT = dict(adaptive_rho_interval=10)
BUDGET = {k: dict(ADAPT, check_termination=CHECK) for k in ("tile4", "tile8", "streamed")}
BUDGET["common"] = dict(FIXED, check_termination=CHECK)
BUDGET_COMMON_ADAPTIVE = dict(ADAPT, check_termination=CHECK)     # identities only: no per-member reference
TINY = dict(eps_abs=EPS, eps_rel=EPS, check_termination=0, max_iter=EXPIRED_MAX_ITER)
EXPIRED = {k: dict(TINY, adaptive_rho_interval=INTERVAL) for k in ("tile4", "tile8", "streamed")}
EXPIRED["common"] = dict(FIXED, **TINY)
BETWEEN = {k: dict(BUDGET[k], eps_abs=EPS, eps_rel=EPS) for k in SHAPES}
# the caps of a budget test: 1, around a check, a rho adaptation (10), and past every member's convergence (None: the
# test takes the largest iteration count of the plain solve plus 7)
KS = [1, CHECK - 1, CHECK, CHECK + 1, 10, None]


def problem(name):
    engine, n, m, B, seed = SHAPES[name]
    fam = common_family if engine == "common" else shape_family
    P, A, Q, L, U, _ = fam(n, m, B, seed)
    return engine, P, A, Q, L, U


def member_oracles(orc, name, kw, members=None):
    """{member: (oracle handle after setup, unscale)}: the member's own reference run -- for the common-K engine the
    run on its pre-scaled data -- and the map of its result to the member's x, y, obj."""
    engine, P, A, Q, L, U = problem(name)
    out = {}
    ws = oracle_ws(common_oracle(orc, P, A, Q, L, U, **kw)) if engine == "common" else None
    for b in (range(Q.shape[0]) if members is None else members):
        if engine == "common":
            out[b] = (prescaled_oracle(orc, ws, Q, L, U, b, **kw), lambda ro, ws=ws: unscale(ws, ro))
        else:
            out[b] = (oracle(orc, P, Q[b], A, L[b], U[b], **kw), lambda ro: (ro.x, ro.y, ro.info.obj_val))
    return out
