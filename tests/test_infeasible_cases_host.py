"""tests/_infeasible_cases.py on the CPU, with the oracle alone: the planted families give the verdicts of their table under
every setting, every comparison the runs make lies 1e-3 or more from its threshold (the margin
tests/test_common_reference_host.py uses for termination decisions -- three decades above the parity bar, so no engine can
honestly decide differently), the `inaccurate` windows of max_iter are where the module says, and the long-double
certificate reference accepts the oracle's certificates and rejects planted defects by 1000 bars or more."""
import numpy as np
import pytest

import _infeasible_cases as ic
from _batch_parity import oracle, oracle_ws

MARGIN = 1e-3
INFEASIBLE = {-3: "primal", 3: "primal", -4: "dual", 4: "dual"}


def _solve(orc, P, A, Q, L, U, b, **kw):
    return oracle(orc, P, Q[b], A, L[b], U[b], **kw).solve()


def _statuses(orc, P, A, Q, L, U, **kw):
    return [_solve(orc, P, A, Q, L, U, b, **kw).info.status_val for b in range(Q.shape[0])]


# ---- 1. the verdict table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(ic.SETTINGS))
@pytest.mark.parametrize("name", list(ic.CASES))
def test_the_oracle_gives_the_verdict_table(oracle_mod, name, setting):
    P, A, Q, L, U, _ = ic.family(name, setting)
    assert _statuses(oracle_mod, P, A, Q, L, U, **ic.kw_of(setting)) == ic.STATUSES


@pytest.mark.parametrize("setting", list(ic.SETTINGS))
@pytest.mark.parametrize("n", ic.M0_N)
def test_the_oracle_gives_the_m0_verdicts(oracle_mod, n, setting):
    P, A, Q, L, U = ic.m0_family(n)
    kw = ic.kw_of(setting)
    out = [_solve(oracle_mod, P, A, Q, L, U, b, **kw) for b in range(3)]
    assert [o.info.status_val for o in out] == ic.M0_STATUSES
    assert all(o.info.iter == (1 if setting == "check_every" else 25) for o in (out[0], out[2]))
    assert abs(out[0].dual_inf_cert[-1] + 1.0) <= 4 * ic.U53 and abs(out[2].dual_inf_cert[-1] - 1.0) <= 4 * ic.U53
    assert out[0].info.obj_val == -ic.OSQP_INFTY


def test_the_inaccurate_windows(oracle_mod):
    """Every max_iter from 1 to 159 that is no multiple of 25: the member's status is the `inaccurate` one all through its
    window and not just outside it.  The chosen max_iter has two neighbours or more with the same status on each side; member 6's window is
    narrower than that, so every value of it is asserted."""
    P, A, Q, L, U, _ = ic.family(ic.INACCURATE_CASE)
    windows = {2: (4, 58, 99), 4: (3, 26, 32), 5: (3, 26, 34), 6: (3, 9, 12)}
    chosen = {b: cap for cap, mem in ic.INACCURATE.items() for b in mem}
    assert {b: ic.INACCURATE[chosen[b]][b] for b in chosen} == {b: w[0] for b, w in windows.items()}
    for b, (status, lo, hi) in windows.items():
        got = {cap: _solve(oracle_mod, P, A, Q, L, U, b, max_iter=cap).info.status_val for cap in range(1, 160) if cap % 25}
        # the window is the whole run of that status around the chosen value (members 4 and 5 meet the status at a few
        # caps outside it as well: 14 to 24 and 36 to 48)
        assert all(got[cap] == status for cap in range(lo, hi + 1) if cap % 25), (b, got)
        assert all(got[cap] != status for cap in (lo - 1, hi + 1) if cap % 25), (b, got.get(lo - 1), got.get(hi + 1))
        near = [cap for cap in range(chosen[b] - 2, chosen[b] + 3)]
        if hi - lo >= 4:
            assert all(got[cap] == status for cap in near), (b, [got[cap] for cap in near])
        else:
            assert lo <= chosen[b] <= hi and all(got[cap] == status for cap in range(lo, hi + 1)), b
    for cap, mem in ic.INACCURATE.items():               # the whole batch at each chosen cap: what the GPU test compares
        st = _statuses(oracle_mod, P, A, Q, L, U, max_iter=cap)
        assert all(st[b] == s for b, s in mem.items()), (cap, st)


# ---- 2. every decision is robust -----------------------------------------------------------------------------------------
def _robust(orc, P, A, Q, L, U, what, first=None, **kw):
    """Every member's run, stepped: the long-double decisions reproduce the oracle's status, iteration count and rho
    updates, and no comparison lies within MARGIN of its threshold.  first(so, b): calls made on the handle before the
    stepped solve (a solve and an update).  -> the statuses."""
    worst, statuses = (np.inf, None), []
    for b in range(Q.shape[0]):
        so_ref, so = (oracle(orc, P, Q[b], A, L[b], U[b], **kw) for _ in range(2))
        if first:
            first(so_ref, b); first(so, b)
        ro = so_ref.solve()
        status, it, moves, pairs = ic.decisions(so, oracle_ws(so), kw)
        assert (status, it, moves) == (ro.info.status_val, ro.info.iter, ro.info.rho_updates), (what, b, status, it, moves)
        statuses.append(status)
        d, pair = ic.margin(pairs)
        assert d >= MARGIN, (what, b, d, pair)
        if d < worst[0]:
            worst = (d, (b,) + pair)
    print(what, "smallest margin %.3g at" % worst[0], worst[1])
    return statuses


@pytest.mark.parametrize("setting", list(ic.SETTINGS))
@pytest.mark.parametrize("name", list(ic.CASES))
def test_every_decision_is_robust(oracle_mod, name, setting):
    P, A, Q, L, U, _ = ic.family(name, setting)
    _robust(oracle_mod, P, A, Q, L, U, (name, setting), **ic.kw_of(setting))


@pytest.mark.parametrize("setting", list(ic.SETTINGS))
@pytest.mark.parametrize("n", ic.M0_N)
def test_every_m0_decision_is_robust(oracle_mod, n, setting):
    _robust(oracle_mod, *ic.m0_family(n), ("m = 0", n, setting), **ic.kw_of(setting))


@pytest.mark.parametrize("cap", list(ic.INACCURATE))
def test_every_decision_at_a_cut_is_robust(oracle_mod, cap):
    """The exact tests that fail at the cut and the tenfold ones that pass, for the whole batch."""
    P, A, Q, L, U, _ = ic.family(ic.INACCURATE_CASE)
    _robust(oracle_mod, P, A, Q, L, U, ("max_iter", cap), max_iter=cap)


@pytest.mark.parametrize("what", ["bounds", "cost"])
@pytest.mark.parametrize("setting", ["default", "fixed_rho"])
@pytest.mark.parametrize("name", ic.LIVE)
def test_the_live_updates_give_their_verdicts_robustly(oracle_mod, name, setting, what):
    """solve, update, solve on one oracle handle per member -- the sequence the GPU test drives: the second solve (warm, or
    from the cold start a member without a solution is left with; the adapted rho kept) gives the new verdicts, and every
    decision of it keeps the margin."""
    P, A, Q, L, U, _ = ic.family(name)
    L2, U2, Q2 = ic.live_updates(name)
    kw = ic.kw_of(setting)
    firsts = []

    def first(so, b):
        firsts.append(so.solve().info.status_val)
        so.update(**(dict(l=L2[b], u=U2[b]) if what == "bounds" else dict(q=Q2[b])))
    want = ic.BOUNDS_STATUSES if what == "bounds" else ic.COST_STATUSES
    got = _robust(oracle_mod, P, A, Q, L, U, (name, setting, what), first=first, **kw)
    assert firsts[::2] == ic.STATUSES and got == want, (firsts, got)


# ---- 3. the certificate reference ----------------------------------------------------------------------------------------
def _problem(orc, P, A, Q, L, U, b, kw):
    """(the problem the certificate's criteria hold on, the oracle's result, D, E)"""
    so = oracle(orc, P, Q[b], A, L[b], U[b], **kw)
    ws = oracle_ws(so)
    ro = so.solve()
    pb = ic.scaled_problem(ws, P, A, Q[b], L[b], U[b]) if ic.space(kw) == "scaled" else (P, A, Q[b], L[b], U[b])
    return pb, ro, ws["D"], ws["E"]


@pytest.mark.parametrize("setting", list(ic.SETTINGS))
@pytest.mark.parametrize("name", list(ic.CASES))
def test_the_reference_accepts_the_oracles_certificates(oracle_mod, name, setting):
    """In every setting, the scaled-space one included: the module's algebra is the oracle's."""
    P, A, Q, L, U, _ = ic.family(name, setting)
    kw = ic.kw_of(setting)
    for b, status in enumerate(ic.STATUSES):
        if status in INFEASIBLE:
            pb, ro, _, _ = _problem(oracle_mod, P, A, Q, L, U, b, kw)
            kind = INFEASIBLE[status]
            ref = ic.assert_certificate(*pb, ro.prim_inf_cert if kind == "primal" else ro.dual_inf_cert, kind, (name, setting, b))
            print(name, setting, b, kind, "excess in bars", {k: "%.3g" % v for k, v in ref.excess.items()})


@pytest.mark.parametrize("n", ic.M0_N)
def test_the_reference_accepts_the_m0_and_the_inaccurate_certificates(oracle_mod, n):
    P, A, Q, L, U = ic.m0_family(n)
    for setting in ic.SETTINGS:
        kw = ic.kw_of(setting)
        for b in (0, 2):
            pb, ro, _, _ = _problem(oracle_mod, P, A, Q, L, U, b, kw)
            ic.assert_certificate(*pb, ro.dual_inf_cert, "dual", ("m = 0", n, setting, b))
    P, A, Q, L, U, _ = ic.family(ic.INACCURATE_CASE)
    for cap, mem in ic.INACCURATE.items():
        for b, status in mem.items():
            pb, ro, _, _ = _problem(oracle_mod, P, A, Q, L, U, b, dict(max_iter=cap))
            cert = ro.prim_inf_cert if status == 3 else ro.dual_inf_cert
            ic.assert_certificate(*pb, cert, INFEASIBLE[status], (cap, b), tenfold=True)
            # and the exact criteria do not hold: that is why the status is the inaccurate one
            assert ic.reference_failures(ic.certificate_reference(*pb, cert, INFEASIBLE[status])), (cap, b)


@pytest.mark.parametrize("name", ["6x9", "128x259", "520x1043"])
def test_the_reference_rejects_planted_defects(oracle_mod, name):
    """Each defect fails some criterion by 1000 bars or more (a false sign or zero condition has no bar: it fails by any
    amount): a flipped sign on a deciding row, a certificate that is not normalised, E or D applied twice, and a
    delta_y that was not projected on a free row."""
    n, m, seed, v, r0, r1, rr, rf = ic.CASES[name]
    P, A, Q, L, U, _ = ic.family(name)
    kw = ic.kw_of("default")

    def fails(pb, cert, kind, what):
        ref = ic.certificate_reference(*pb, cert, kind)
        big = [k for k, e in ref.excess.items() if e >= 1000.0] + [k for k, ok in ref.exact.items() if not ok]
        if abs(ref.norm - 1.0) >= 1000.0 * ref.norm_bar:
            big.append("norm")
        print(name, what, "fails", big)
        assert big, (name, what, ref.excess, ref.norm)

    for b in (4, 5, 6):                                   # primal certificates
        pb, ro, D, E = _problem(oracle_mod, P, A, Q, L, U, b, kw)
        w = ro.prim_inf_cert
        assert not ic.reference_failures(ic.certificate_reference(*pb, w, "primal"))
        flipped = w.copy(); flipped[r0] = -flipped[r0]
        fails(pb, flipped, "primal", (b, "sign of row r0 flipped"))
        fails(pb, 1.25 * w, "primal", (b, "not normalised"))
        free = w.copy(); free[rf] = 0.3
        fails(pb, free, "primal", (b, "delta_y of a free row kept"))
    for b in (1, 2, 7):                                   # dual certificates
        pb, ro, D, E = _problem(oracle_mod, P, A, Q, L, U, b, kw)
        d = ro.dual_inf_cert
        assert not ic.reference_failures(ic.certificate_reference(*pb, d, "dual"))
        fails(pb, -d, "dual", (b, "sign flipped"))
        fails(pb, 1.25 * d, "dual", (b, "not normalised"))
    # E or D applied twice, on the variants whose certificate spans two different scaling factors (in the family itself such
    # a vector is, once divided by its norm, still a certificate -- ic.coupled_variants)
    for pb, kind, S in zip(ic.coupled_variants(name), ("primal", "dual"), ("E", "D")):
        so = oracle(oracle_mod, pb[0], pb[2], pb[1], pb[3], pb[4], **kw)
        ws, ro = oracle_ws(so), so.solve()
        assert ro.info.status_val == (-3 if kind == "primal" else -4)
        cert = ro.prim_inf_cert if kind == "primal" else ro.dual_inf_cert
        assert not ic.reference_failures(ic.certificate_reference(*pb, cert, kind))
        twice = ws[S] * cert
        fails(pb, twice / np.abs(twice).max(), kind, (S + " applied twice",))
    # member 2's ray has (A d)_rr != 0, which only the infinite lower side allows: the same certificate on member 3's
    # bounds (the sides swapped) is no certificate
    pb, ro, _, _ = _problem(oracle_mod, P, A, Q, L, U, 2, kw)
    assert abs(ro.dual_inf_cert[v]) == np.abs(ro.dual_inf_cert).max()
    fails((P, A, Q[3], L[3], U[3]), ro.dual_inf_cert, "dual", (2, "the clauses of the row test swapped"))
