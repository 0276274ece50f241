"""GPU tests of the infeasibility code of the batch engines (osqp_amd/csrc/batch_admm.h: the projection of delta_y and the
cheap halves of both tests in update_info, the pinf / dinf branches of check_termination, the no-solution branch of
store_solution) through the three kernels that reach it: k_batch_solve (tiled, NP = 64 and 128), k_bs_loop (streamed) and
k_bc_check (common-K), on the planted families of tests/_infeasible_cases.py -- the deciding variable and rows in the last
places, one-sided and free rows that decide, every setting that turns `unscaled` off, m = 0, the `inaccurate` statuses,
and a live handle whose members change sides.

Bars.  `_batch_parity.assert_parity` against the member's oracle run (status, iterations, rho updates equal; x, y to
1e-6, the objective to 1e-8 for members with a point); certificates to 1e-5 of the largest entry against the oracle's,
the bar the other batch tests use; and `_infeasible_cases.certificate_reference`: the criteria of is_primal_infeasible /
is_dual_infeasible recomputed in long double from the raw problem (from the member's scaled problem where the
certificate stays scaled) with the rounding bars written there, and the sign and zero conditions exactly.
tests/test_infeasible_cases_host.py shows on the CPU that the oracle gives the planted verdicts, that no comparison of any
of these runs lies within 1e-3 of its threshold, and that the reference rejects planted defects.

The common-K engine takes one class per row and forms one scaling and one rho for its batch, so the eight members (whose
rows rr, r0, r1 differ in class, and whose q differ) are no batch of its own with a reference run to compare with: there
every member is a batch of one, which the engine solves as the reference solves the member
(tests/test_gpu_batch_common.py::test_identical_members).  The position tests run it on the members that share their
classes, with scaling = 0 and a fixed rho."""
from types import SimpleNamespace

import numpy as np
import pytest

import _infeasible_cases as ic
from _batch_parity import assert_parity, oracle, rel

pytestmark = pytest.mark.gpu

ENGINES = ("tiled", "streamed", "common")
SERVED = [(e, name) for e in ENGINES for name in ic.CASES if e != "tiled" or name in ic.TILED]
KIND = {-3: "primal", 3: "primal", -4: "dual", 4: "dual"}
FIELDS = ("x", "y", "status_val", "iter", "rho_updates", "obj_val", "prim_inf_cert", "dual_inf_cert", "info_raw")
_oracle_runs = {}


def _setup(engine, P, A, Q, L, U, kw):
    """One handle on the engine asked for -- and on no other: the tiled kernel at NP = 64 ("tile4") up to n = 64 and at
    NP = 128 ("tile8") above."""
    import osqp_amd
    n = Q.shape[1]
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine={"tiled": "auto"}.get(engine, engine), **kw)
    want = {"tiled": (0, 64 if n <= 64 else 128), "streamed": (1, (n + 31) // 32 * 32), "common": (2, (n + 31) // 32 * 32)}[engine]
    assert h.shape() == want, (engine, h.shape(), want)
    return h


class _Session:
    """The eight members on one engine: one handle, or on the common-K engine one handle per member.  Every call returns
    what the call on one handle of eight would: the rows stacked."""

    def __init__(self, engine, P, A, Q, L, U, kw):
        B = Q.shape[0]
        self.B = B
        self.parts = [slice(b, b + 1) for b in range(B)] if engine == "common" else [slice(0, B)]
        self.handles = [_setup(engine, P, A, Q[s], L[s], U[s], kw) for s in self.parts]

    def solve(self):
        rs = [h.solve() for h in self.handles]
        return SimpleNamespace(**{k: np.concatenate([getattr(r, k) for r in rs]) for k in FIELDS})

    def update(self, **arrays):
        for h, s in zip(self.handles, self.parts):
            assert h.update(**{k: a[s] for k, a in arrays.items()}) == 0

    def verify(self):
        vs = [h.verify() for h in self.handles]
        return SimpleNamespace(prim_inf=np.concatenate([v.prim_inf for v in vs]), dual_inf=np.concatenate([v.dual_inf for v in vs]))

    def workspace(self, b):
        return self.handles[b].member_workspace(0) if len(self.handles) > 1 else self.handles[0].member_workspace(b)

    def close(self):
        for h in self.handles:
            h.cleanup()


def _oracles(orc, key, P, A, Q, L, U, kw, then=()):
    """The members' oracle runs, computed once per case and shared by the engines: [solve, then for each update of `then`
    (a dict of per-member arrays q / l / u) update and solve] -> per member the list of results."""
    if key not in _oracle_runs:
        out = []
        for b in range(Q.shape[0]):
            so = oracle(orc, P, Q[b], A, L[b], U[b], **kw)
            runs = [so.solve()]
            for up in then:
                so.update(**{k: a[b] for k, a in up.items()})
                runs.append(so.solve())
            out.append(runs)
        _oracle_runs[key] = out
    return _oracle_runs[key]


def _check(r, ros, ses, P, A, Q, L, U, kw, what):
    """Every member of one solve against its oracle run and, where it has no solution, against the raw problem.
    -> the largest certificate difference to the oracle, relative to the largest entry."""
    worst = 0.0
    for b, ro in enumerate(ros):
        assert_parity(r, b, ro, what)
        status = ro.info.status_val
        if status not in KIND:
            continue
        tag = (what, b, status)
        assert np.all(r.x[b] == ic.OSQP_NAN) and np.all(r.y[b] == ic.OSQP_NAN), tag
        assert r.obj_val[b] == (ic.OSQP_INFTY if KIND[status] == "primal" else -ic.OSQP_INFTY), tag + (r.obj_val[b],)
        cert, want = (r.prim_inf_cert[b], ro.prim_inf_cert) if KIND[status] == "primal" else (r.dual_inf_cert[b], ro.dual_inf_cert)
        d = rel(cert, want)
        worst = max(worst, d)
        assert d < 1e-5, tag + (d,)
        pb = (P, A, Q[b], L[b], U[b]) if ic.space(kw) == "raw" else ic.scaled_problem(ses.workspace(b), P, A, Q[b], L[b], U[b])
        ic.assert_certificate(*pb, cert, KIND[status], tag, tenfold=status > 0)
    return worst


# ---- 1. every shape x setting x engine --------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(ic.SETTINGS))
@pytest.mark.parametrize("engine,name", SERVED)
def test_verdicts_and_certificates(gpu_lib, oracle_mod, engine, name, setting):
    """verify() (the raw problem and the returned certificates alone) must say prim_inf for every primal infeasible member
    and dual_inf for every dual infeasible one -- where the certificate is in the raw space.  With scaling on and
    scaled_termination = 1 the certificate is dy~ / dx~ of the scaled problem, which verify does not know: left out there."""
    P, A, Q, L, U, _ = ic.family(name, setting)
    kw = ic.kw_of(setting)
    ros = [runs[0] for runs in _oracles(oracle_mod, (name, setting), P, A, Q, L, U, kw)]
    assert [ro.info.status_val for ro in ros] == ic.STATUSES
    ses = _Session(engine, P, A, Q, L, U, kw)
    try:
        r = ses.solve()
        worst = _check(r, ros, ses, P, A, Q, L, U, kw, (engine, name, setting))
        print("certificates against the oracle: %s %s %s max %.3g" % (engine, name, setting, worst))
        if ic.space(kw) == "raw":
            v = ses.verify()
            st = np.array(ic.STATUSES)
            assert np.all(v.prim_inf[st == -3]) and np.all(v.dual_inf[st == -4]), (engine, name, setting, v.prim_inf, v.dual_inf)
    finally:
        ses.close()


# ---- 2. m = 0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(ic.SETTINGS))
@pytest.mark.parametrize("n", ic.M0_N)
@pytest.mark.parametrize("engine", ENGINES)
def test_m0(gpu_lib, oracle_mod, engine, n, setting):
    """prim_ok without a test, no A'y, an empty loop over the rows: every engine accepts m = 0."""
    P, A, Q, L, U = ic.m0_family(n)
    kw = ic.kw_of(setting)
    ros = [runs[0] for runs in _oracles(oracle_mod, ("m0", n, setting), P, A, Q, L, U, kw)]
    assert [ro.info.status_val for ro in ros] == ic.M0_STATUSES
    ses = _Session(engine, P, A, Q, L, U, kw)
    try:
        r = ses.solve()
        _check(r, ros, ses, P, A, Q, L, U, kw, (engine, "m = 0", n, setting))
        assert abs(r.dual_inf_cert[0, -1] + 1.0) <= 4 * ic.U53 and abs(r.dual_inf_cert[2, -1] - 1.0) <= 4 * ic.U53
        assert r.y.shape == (3, 0) and r.prim_inf_cert.shape == (3, 0)
    finally:
        ses.close()


# ---- 3. the inaccurate statuses ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", list(ic.INACCURATE))
@pytest.mark.parametrize("engine", ENGINES)
def test_inaccurate_verdicts(gpu_lib, oracle_mod, engine, cap):
    """max_iter inside the window where the exact test still fails and the tenfold one passes: stages 1 and 2 of admm_loop's
    stage machine with F_APPROX, the `final` tail of k_bc_check.  The certificate holds the tenfold criteria.  (verify
    takes no infeasibility tolerances, so it is not asked here.)"""
    P, A, Q, L, U, _ = ic.family(ic.INACCURATE_CASE)
    kw = dict(max_iter=cap)
    ros = [runs[0] for runs in _oracles(oracle_mod, ("cap", cap), P, A, Q, L, U, kw)]
    for b, status in ic.INACCURATE[cap].items():
        assert ros[b].info.status_val == status
    ses = _Session(engine, P, A, Q, L, U, kw)
    try:
        r = ses.solve()
        _check(r, ros, ses, P, A, Q, L, U, kw, (engine, "max_iter", cap))
        for b, status in ic.INACCURATE[cap].items():
            assert r.status_val[b] == status
    finally:
        ses.close()


# ---- 4. a live handle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["default", "fixed_rho"])
@pytest.mark.parametrize("what", ["bounds", "cost"])
@pytest.mark.parametrize("engine,name", [(e, name) for e, name in SERVED if name in ic.LIVE])
def test_live_handle(gpu_lib, oracle_mod, engine, name, what, setting):
    """solve, update, solve with warm_start on (the default): store_solution left zeros in the warm-start iterates of the
    members without a solution (the reference's cold start) and the adapted rho in place.  bounds: members 4, 5, 6 become
    feasible and member 0 primal infeasible; cost: member 1 becomes solved and member 0 dual infeasible.  Parity is against
    the oracle driven through the same calls."""
    P, A, Q, L, U, _ = ic.family(name)
    L2, U2, Q2 = ic.live_updates(name)
    kw = ic.kw_of(setting)
    up, after, want = (dict(l=L2, u=U2), (Q, L2, U2), ic.BOUNDS_STATUSES) if what == "bounds" else (dict(q=Q2), (Q2, L, U), ic.COST_STATUSES)
    runs = _oracles(oracle_mod, (name, setting, what), P, A, Q, L, U, kw, then=(up,))
    assert [ro[1].info.status_val for ro in runs] == want
    ses = _Session(engine, P, A, Q, L, U, kw)
    try:
        _check(ses.solve(), [ro[0] for ro in runs], ses, P, A, Q, L, U, kw, (engine, name, setting, "first solve"))
        ses.update(**{k.upper(): a for k, a in up.items()})
        r = ses.solve()
        _check(r, [ro[1] for ro in runs], ses, P, A, *after, kw, (engine, name, setting, "after the update of the " + what))
        v = ses.verify()
        st = np.array(want)
        assert np.all(v.prim_inf[st == -3]) and np.all(v.dual_inf[st == -4])
    finally:
        ses.close()


# ---- 5. position independence -----------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("engine", ENGINES)
def test_a_member_alone_and_inside_the_batch(gpu_lib, engine):
    """Bit for bit: member 4 (primal infeasible) and member 2 (dual infeasible) of "128x259" alone and inside their batch.
    scaling = 0, since the common engine's scaling depends on the batch; there the batch is the members that share the
    member's row classes, and rho is fixed (its rho is one for the batch)."""
    P, A, Q, L, U, _ = ic.family("128x259")
    kw = ic.kw_of("unscaled", **(dict(adaptive_rho=0) if engine == "common" else {}))
    for b, status, cert, group in ((4, -3, "prim_inf_cert", [0, 1, 4, 5, 7]), (2, -4, "dual_inf_cert", [2, 3])):
        S = np.array(group if engine == "common" else range(8))
        hs = [_setup(engine, P, A, Q[S], L[S], U[S], kw), _setup(engine, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1], kw)]
        try:
            whole, alone = (h.solve() for h in hs)
            at = int(np.flatnonzero(S == b)[0])
            assert alone.status_val[0] == status
            for k in ("info_raw", cert):
                assert np.array_equal(_bits(getattr(whole, k)[at]), _bits(getattr(alone, k)[0])), (engine, b, k)
        finally:
            for h in hs:
                h.cleanup()
