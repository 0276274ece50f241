"""The case "wrongpivot" of tests/_planted_qp.py stays inside its conditions (no GPU): one member's KKT inversion must
meet a pivot of the wrong sign on the device (status -1 from k_bp_invert), every other member must be served.

The yardstick of the verdict is pq.gj_verdict, a float64 model of the device's Gauss-Jordan sweep in its natural order,
on the matrix the device forms (pq.device_kkt).  The oracle is none: its polish factors in a fill-reducing order, never
meets the zero and accepts the member.  What the oracle vouches for is the rest -- every member is a convex QP that ADMM
solves, with the planted active set -- and, for the healthy members, that the model of the device route is accepted
against ADMM's residuals, so tests/test_gpu_batch_pivot_verdict.py compares every one of them and excuses none."""
import numpy as np
import pytest

import _planted_qp as pq
from _batch_parity import oracle, oracle_ws

LD = np.longdouble
VARIANTS = (0, 1)
DELTA = pq.VERDICT_DELTA


def _case(variant):
    return pq.case("wrongpivot", variant)


def test_the_case_is_what_it_says():
    c0, c1 = _case(0), _case(1)
    assert "wrongpivot" not in pq.CASES and "wrongpivot" in pq.VERDICT_CASES
    assert (c0.singular, c1.singular) == (1, 2) and c0.pair == c1.pair == pq.PAIR
    assert c0.settings == dict(scaling=0, delta=2.0 ** -60) and 1.0 + DELTA == 1.0 and DELTA > 0.0
    assert (c0.n, c0.m, c0.B) == (40, 56, 4)
    assert c1.P is c0.P and c1.A is c0.A
    j0, j1 = pq.PAIR
    Pf = (c0.P + c0.P.T).toarray()
    for j, other in ((j0, j1), (j1, j0)):                  # the pair is coupled to nothing else
        assert set(np.flatnonzero(Pf[j])) == {j, other}
    for c in (c0, c1):
        counts = [int(np.count_nonzero(a)) for a in c.act]
        assert len(set(counts)) == c.B and (c.n + max(counts) + 31) & ~31 == 96, counts     # four different paddings
        slots = pq.pair_slots(c.P, c.pair)
        for b in range(c.B):
            assert c.act[b][j0] != 0 and c.act[b][j1] != 0                  # rows j0, j1 pin x_j0 - x_j1
            v = c.Px_all[b][slots]
            if b == c.singular:
                assert np.array_equal(v, [1.0, 1.0, 1.0])
            else:
                assert v[0] * v[2] > 4.0 * v[1] * v[1]                      # an ordinary, well-conditioned 2 x 2 block
            Pf = pq.member(c, b).Pf                                         # PSD (to eigvalsh's rounding), PD when healthy
            assert np.linalg.eigvalsh(Pf).min() >= (-c.n * 2.0 ** -52 * np.abs(Pf).max() if b == c.singular else 0.1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_modelled_verdict(variant):
    """On the matrix the device forms, the sweep meets (j1, 0.0) on the singular member and no wrong pivot elsewhere."""
    c = _case(variant)
    for b in range(c.B):
        mem = pq.member(c, b)
        K = pq.device_kkt(mem, DELTA)
        assert np.array_equal(K, K.T) and K[pq.PAIR[0], pq.PAIR[0]] == mem.Pf[pq.PAIR[0], pq.PAIR[0]]
        v = pq.gj_verdict(K, c.n)
        if b == c.singular:
            assert v is not None and v[0] == pq.PAIR[1] and v[1] == 0.0 and not np.signbit(v[1]), (variant, b, v)
        else:
            assert v is None, (variant, b, v)
            # the healthy members' inversion is not hurt by the tiny delta: cond(M) is small, and an explicit inverse of
            # the regularised matrix is one of M to rounding
            M = pq.Route(mem).M
            R = np.abs(np.linalg.inv(K) @ M - np.eye(M.shape[0])).max()
            assert R <= 1e-12, (variant, b, R)


def test_near_miss_recipes(oracle_mod):
    """The recipe needs both of its settings.  delta = 1e-6 (the default): pivot j0 is 1 + 1e-6 and leaves about 2e-6.
    scaling = 10 (the default): the device sees D P D, the pair is no multiple of [[1, 1], [1, 1]] any more.  Either
    way the sweep meets no exact zero on the singular member -- whatever verdict rounding then gives is not pinned."""
    c = _case(0)
    b = c.singular
    raw = pq.member(c, b)
    v = pq.gj_verdict(pq.device_kkt(raw, 1e-6), c.n)
    assert v is None, v
    ws = oracle_ws(oracle(oracle_mod, raw.Pu, raw.q, raw.Ac, raw.l, raw.u, scaling=10, delta=DELTA))
    assert not np.all(ws["D"] == 1.0)
    sm = pq.member(c, b, Pv=ws["Pv"], Av=ws["Av"])
    slots = pq.pair_slots(c.P, c.pair)
    p = np.asarray(ws["Pv"])[slots]
    assert not (p[0] == p[1] == p[2]), p
    v = pq.gj_verdict(pq.device_kkt(sm, DELTA), c.n)
    assert v is None or v[1] != 0.0, v
    print("scaling=10: pair", p, "verdict", v)
    # and without scaling the oracle's workspace holds the raw bits, which is what the device then sees
    ws0 = oracle_ws(oracle(oracle_mod, raw.Pu, raw.q, raw.Ac, raw.l, raw.u, **c.settings))
    assert np.array_equal(ws0["Pv"], c.Px_all[b]) and np.array_equal(ws0["Av"], c.Ax_all[b]) and ws0["c"] == 1.0


@pytest.mark.parametrize("variant", VARIANTS)
def test_truth_and_conditions(variant):
    """What tests/test_planted_qp_host.py demands of a case, of every member, the singular one included: the truth
    satisfies the KKT conditions in long double with the planted signs, |y| >= 0.1 on the active rows, every gap of an
    inactive bound >= 0.1, sigma_min / sigma_max of the active rows >= 1e-2.  cond(M) <= 1e5, the bound under which
    _batch_parity.check_member_kinv holds an explicit inverse to numpy's error."""
    c = _case(variant)
    for b in range(c.B):
        t = pq.truth(c, b)
        mem, tag = t.mem, (variant, b)
        s = np.concatenate([t.x, t.y[mem.rows]])
        g = np.concatenate([-mem.q, mem.l[mem.low], mem.u[mem.upp]])
        r = np.abs(t.route.residual_ld(s, g)).astype(float)
        lim = 2.0 ** -52 * (np.abs(t.route.M) @ np.abs(s) + np.abs(g))
        assert np.all(r <= lim), tag + (float((r / np.maximum(lim, 1e-300)).max()),)
        assert np.array_equal(np.sign(t.y).astype(np.int64), mem.act), tag
        assert pq.err(t.x, c.x[b]) <= 1e-12 * max(1.0, np.abs(c.x[b]).max()), tag
        assert pq.err(t.y, c.y[b]) <= 1e-12 * max(1.0, np.abs(c.y[b]).max()), tag
        ax = (mem.Ad.astype(LD) @ t.x.astype(LD)).astype(float)
        act = mem.act
        assert np.abs(t.y[act != 0]).min() >= 0.1, tag
        gap_l = np.where(act < 0, np.inf, ax - mem.l)
        gap_u = np.where(act > 0, np.inf, mem.u - ax)
        eq = (mem.l == mem.u)
        gap_l[eq] = np.inf; gap_u[eq] = np.inf
        assert min(gap_l.min(), gap_u.min()) >= 0.1, tag
        sv = np.linalg.svd(mem.Ad[mem.rows], compute_uv=False)
        cond = np.linalg.cond(t.route.M)
        print("wrongpivot", variant, b, "mred", mem.rows.size, "sv ratio %.3f cond(M) %.1f" % (sv.min() / sv.max(), cond))
        assert mem.rows.size <= c.n and sv.min() / sv.max() >= 1e-2, tag + (sv.min() / sv.max(),)
        assert cond <= 1e5, tag + (cond,)


@pytest.mark.parametrize("kw", [{}, dict(adaptive_rho_interval=10)], ids=["default", "interval10"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_solves_every_member(oracle_mod, variant, kw):
    """scaling = 0, default eps: OSQP_SOLVED on every member, the singular one included (K = P + sigma I + A' rho A is
    positive definite), and polish's two tests (low z - l < -y, upp u - z < y) at ADMM's point give the planted set."""
    c = _case(variant)
    for b in range(c.B):
        mem = pq.member(c, b)
        so = oracle(oracle_mod, mem.Pu, mem.q, mem.Ac, mem.l, mem.u, **c.settings, **kw)
        ro = so.solve()
        tag = (variant, b, ro.info.status_val, ro.info.iter)
        assert ro.info.status_val == 1, tag
        x, z, y = so.iterates()
        low = z - mem.l < -y
        upp = ~low & (mem.u - z < y)
        assert np.array_equal(np.where(low, -1, np.where(upp, 1, 0)), mem.act), tag
        print("wrongpivot", variant, b, kw, "iter", ro.info.iter, "pri %.2e dua %.2e" % (ro.info.pri_res, ro.info.dua_res))


@pytest.mark.parametrize("variant", VARIANTS)
def test_healthy_members_are_compared(oracle_mod, variant):
    """The model of the device route (3 refinement steps, the case's delta, unscaled data) is accepted by polish's rule
    against the oracle's ADMM residuals, and its error against the truth is finite: the GPU tests hold every healthy
    member to pq.bar with must_accept."""
    c = _case(variant)
    for b in range(c.B):
        if b == c.singular:
            continue
        mem, t = pq.member(c, b), pq.truth(c, b)
        ro = oracle(oracle_mod, mem.Pu, mem.q, mem.Ac, mem.l, mem.u, **c.settings).solve()
        mo = pq.model(c, b, 3, DELTA)
        tag = (variant, b, mo.pri, mo.dua, ro.info.pri_res, ro.info.dua_res)
        assert ro.info.status_val == 1 and pq.accepts(mo.pri, mo.dua, ro.info.pri_res, ro.info.dua_res), tag
        errs = {name: pq.err(getattr(mo, name), getattr(t, name)) for name in pq.POLISH + pq.ADJOINT + pq.TANGENT}
        assert all(np.isfinite(e) for e in errs.values()), tag + (errs,)
        # ... and small: the bar it sets is no licence
        for name, e in errs.items():
            assert e <= 1e-10 * max(1.0, float(np.abs(getattr(t, name)).max())), tag + (name, e)
