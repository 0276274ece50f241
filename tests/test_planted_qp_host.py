"""The planted cases of tests/_planted_qp.py stay inside their own conditions (no GPU): for every case and member the
truth satisfies the KKT conditions in long double with the planted signs, |y| >= 0.1 on the active rows, every gap of
an inactive bound >= 0.1, sigma_min / sigma_max of the active rows >= 1e-2, and the model of the device route loses
more than 100x of its error from 0 to 1 and from 1 to 2 refinement steps -- which is what lets the two-sided bar at
k in {0, 1} tell a step too few or too many.  The CPU oracle with polish=1 must end solved, polished, on the planted
active set and within the bar of the truth: an independent float64 implementation attains it, so nothing needs
excusing on the device."""
import numpy as np
import pytest

import _planted_qp as pq
from _adjoint_reference import active_set
from _batch_parity import oracle, oracle_ws

LD = np.longdouble


@pytest.mark.parametrize("name", pq.CASES)
def test_truth_and_conditions(oracle_mod, name):
    c = pq.case(name)
    for b in range(c.B):
        t = pq.truth(c, b)
        mem, tag = t.mem, (name, b)
        n, m = mem.n, mem.m
        # KKT in long double: stationarity and the active rows to the rounding of the float64 truth (half an ulp of every
        # term of the row, twice over for the right-hand side), the other rows strictly inside
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
        if act.any():
            assert np.abs(t.y[act != 0]).min() >= 0.1, tag
        gap_l = np.where(act < 0, np.inf, ax - mem.l)       # an active bound has no gap; the other bound of an equality row neither
        gap_u = np.where(act > 0, np.inf, mem.u - ax)
        eq = (mem.l == mem.u)
        gap_l[eq] = np.inf; gap_u[eq] = np.inf
        if m:
            assert min(gap_l.min(), gap_u.min()) >= 0.1, tag
            assert np.all(ax >= mem.l - 1e-12 * np.abs(ax)) and np.all(ax <= mem.u + 1e-12 * np.abs(ax)), tag
        if mem.rows.size:
            sv = np.linalg.svd(mem.Ad[mem.rows], compute_uv=False)
            assert mem.rows.size <= n and sv.min() / sv.max() >= 1e-2, tag + (sv.min() / sv.max(),)
        # the model's error per refinement step, over each call's outputs together and relative to their size; on the
        # scaled data of the oracle's set-up, which the device's equals to 1e-14 (check_member_kinv): the GPU tests
        # evaluate the model there
        ws = oracle_ws(oracle(oracle_mod, mem.Pu, mem.q, mem.Ac, mem.l, mem.u, **c.settings))
        e = []
        for k in range(3):
            mo = pq.model(c, b, k, ws=ws)
            e.append([max(pq.err(getattr(mo, a), getattr(t, a)) / max(np.abs(getattr(t, a)).max(), 1e-300)
                          for a in names if np.size(getattr(t, a)) and np.abs(getattr(t, a)).max() > 0)
                      for names in (pq.POLISH, pq.ADJOINT, pq.TANGENT)])
        print(name, b, "mred", mem.rows.size, "model error after 0, 1, 2 steps (polish, adjoint, tangent):",
              " | ".join(" ".join("%.1e" % v for v in row) for row in e))
        for j in range(3):
            assert e[0][j] > 100 * e[1][j] and e[1][j] > 100 * e[2][j], tag + (j, e[0][j], e[1][j], e[2][j])


def test_row_mix():
    """Every class of row occurs: active equality rows of both multiplier signs, active rows whose other bound is
    infinite (at either bound) or finite, free rows, inactive one- and two-sided rows."""
    seen = set()
    for name in pq.CASES:
        c = pq.case(name)
        for b in range(c.B):
            l, u, act = c.L[b], c.U[b], c.act[b]
            for i in range(c.m):
                fin = (np.isfinite(l[i]), np.isfinite(u[i]))
                seen.add((int(act[i]), "eq" if l[i] == u[i] else fin))
    want = {(-1, "eq"), (1, "eq"), (-1, (True, False)), (1, (False, True)), (-1, (True, True)), (1, (True, True)),
            (0, (False, False)), (0, (True, True)), (0, (True, False)), (0, (False, True))}
    assert want <= seen, want - seen
    pad = pq.case("pad")
    for b in (1, 2, 3):
        kinds = {(int(a), "eq" if lo == hi else (np.isfinite(lo), np.isfinite(hi))) for a, lo, hi in zip(pad.act[b], pad.L[b], pad.U[b])}
        assert want <= kinds, (b, want - kinds)


def test_shapes_reach_their_paths():
    """What each case is for, in numbers: NPOL and the paddings, the LDS of the three kernels, the longest rows."""
    npol = lambda c: (c.n + max(int(np.count_nonzero(c.act[b])) for b in range(c.B)) + 31) & ~31
    mred = lambda c: tuple(int(np.count_nonzero(c.act[b])) for b in range(c.B))
    bp_lds = lambda n, m, N: (8 * (3 * N + 2 * n + 5 * m + 32) + 4 * 2 * m + 15) & ~15
    ba_lds = lambda n, m, N: (8 * (4 * N + 2 * n + 2 * m) + 4 * 2 * m + 15) & ~15
    assert mred(pq.case("pad")) == (0, 24, 25, 40) and npol(pq.case("pad")) == 96
    assert mred(pq.case("pad_exact")) == (24, 8) and npol(pq.case("pad_exact")) == 64
    assert mred(pq.case("pad", 1)) != mred(pq.case("pad")) and npol(pq.case("pad", 1)) == 96
    sc = pq.case("scan")
    assert sc.act[0][255] != 0 and sc.act[0][256] != 0
    assert np.all(sc.act[1][:256] == 0) and np.all(sc.act[1] >= 0) and sc.act[1].any()
    assert np.all(sc.act[2][64:] == 0) and np.all(sc.act[2] <= 0) and sc.act[2].any()
    s2 = pq.case("scan2")
    assert all(s2.act[0][i] != 0 for i in (255, 256)) and all(s2.act[1][i] != 0 for i in (511, 512))
    assert np.all(s2.act[2][:256] == 0) and np.all(s2.act[2] >= 0) and s2.act[2][512] == 1
    assert np.all(s2.act[3][128:] == 0) and np.all(s2.act[3] <= 0) and s2.act[3].any()
    ro = pq.case("rows")
    Pf = (ro.P + ro.P.T).tocsr()
    assert np.diff(Pf.indptr).max() > 256 and np.diff(ro.A.tocsr().indptr).max() > 256
    assert np.diff(ro.A.indptr)[pq.ROWS_EMPTY_COL] == 0
    d = ro.P.diagonal()
    for j in pq.ROWS_NO_P:
        assert d[j] == 0 and Pf[j].nnz == 0 and all(ro.act[b][j] != 0 for b in range(ro.B))
    assert all(ro.act[b][i] != 0 for b in range(ro.B) for i in pq.ROWS_DENSE_A)
    lp = pq.case("lp")
    assert lp.P.nnz == 0 and mred(lp) == (24, 24, 24) and len({tuple(a) for a in lp.act}) == 3
    big = pq.case("lds64k")
    assert mred(big) == (600, 0) and npol(big) == 1216 and bp_lds(600, 600, 1216) == 67840 > 65536
    assert ba_lds(600, 600, 1216) <= 65536 < ba_lds(704, 1129, 1408)      # the adjoint and the tangent cross 64 KiB only at `max`
    mx = pq.case("max")
    assert mred(mx) == (704,) and npol(mx) == 1408 and bp_lds(704, 1129, 1408) <= 160 * 1024
    for name in pq.CASES:                     # the members of a batch have different active sets
        c = pq.case(name)
        assert len({tuple(a) for a in c.act}) == c.B, name


@pytest.mark.parametrize("name", pq.CASES)
def test_oracle_attains_the_bar(oracle_mod, name):
    c = pq.case(name)
    worst = {}
    for b in range(c.B):
        mem, t = pq.member(c, b), pq.truth(c, b)
        so = oracle(oracle_mod, mem.Pu, mem.q, mem.Ac, mem.l, mem.u, polish=1, **c.settings)
        ws = oracle_ws(so)
        ro = so.solve()
        tag = (name, b, ro.info.status_val, ro.info.status_polish, ro.info.iter)
        assert ro.info.status_val == 1 and ro.info.status_polish == 1, tag
        assert np.array_equal(active_set(ro.y)[2], mem.act), tag
        mo = pq.model(c, b, 3, ws=ws)
        got = pq.SimpleNamespace(x=ro.x, y=ro.y, obj=np.array([ro.info.obj_val]))
        pq.check(tag, got, t, mo, pq.POLISH, worst=worst)
        bp, bd = pq.residual_bars(t, mo)
        assert ro.info.pri_res <= bp and ro.info.dua_res <= bd, tag + (ro.info.pri_res, bp, ro.info.dua_res, bd)
        print(name, b, "iter", ro.info.iter, "x %.1e y %.1e" % (pq.err(ro.x, t.x), pq.err(ro.y, t.y)))
    print(name, "oracle worst err / bar:", {k: "%.2f" % v for k, v in worst.items()})
