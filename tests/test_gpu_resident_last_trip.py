"""GPU tests of the predicted last trip of k_pcg_resident (engine_pcg_resident.h) and of the row state overlaid on the registers of K.

A pipelined solve of N PCG iterations makes N + 3 vector trips: the start-up product, N iterations, one trip whose exchange only
delivers the ||r||^2 that says "converged", and the true-residual check.  When wavefront 0 predicts that the coming trip is that
wasted one it sends x - x0 instead, so that the trip's products serve the check: N + 2 trips on a hit, N + 4 on a miss, and the
iterates are the parent's bit for bit either way.  OSQP_AMD_RESIDENT_PREDICT=0 is the loop without it, OSQP_AMD_RESIDENT_PREDICT_MARGIN
scales the threshold (1e30: fires at the first chance, after the second iteration, and misses whenever N > 2).

Engines are built like test_gpu_pcg_edges.test_resident_every_E builds them: the cases res_e<E> of tests/_pcg_cases.py,
OSQP_AMD_DENSE_DIRECT=0 OSQP_AMD_RESIDENT_MIN_N=1 OSQP_AMD_RESIDENT_NWG=<claims>, pcg_eps_rel = 1e-12.  Yardstick of the steps:
_engine_reference.admm_step (long double) with _engine_reference.step_bars, none tuned on device output.

  step bars, bits   E = 8 (row state partly on kv[]), 20, 24 (unspilled only with the overlay), 64 (spilling): one ADMM step from
                    non-zero iterates with the defaults, PREDICT=0 and PREDICT_MARGIN=1e30: each within the bars, all three equal
                    in every bit, no launch gave up.
  trip counts       the same engines, 24 consecutive ADMM iterations: per solve N + 3 with PREDICT=0; N + 2 with one hit at the default
                    margin (N + 3 with neither hit nor miss where the rule did not fire: printed); N + 4 with exactly one miss
                    at margin 1e30 (until the window of 16 solves switches the predictions off); no hit or miss with
                    OSQP_AMD_RESIDENT_PIPE=0.  Every solve of these cases needs more than the 64 iterations the pipelined phase
                    allows (99 .. 177 at pcg_eps_rel = 1e-12, measured): it is cut there, checked and finished by the
                    other recurrences, which is one trip more (N + 4; N + 5 with the miss), and the rule has nothing to fire on
                    at the default margin.  N + 3 / N + 2 / N + 4 themselves are asserted per solve on the chains below, whose
                    solves stay inside the pipelined phase on `tiny3` and `m0` (27 hits in 30 solves on `m0`).
  chain             30 ADMM iterations on `tiny3`, `m0`, `offtile` (tests/_engine_reference.py) on the resident form: bits of
                    x, y, z after 3 and 30 iterations equal among the defaults, PREDICT=0 and margin 1e30; per iteration and in sum
                    trips = (N + 3) - hits + misses, the solves with N <= 2 included (nothing fires before two ||r||^2 are known;
                    `offtile`'s solves pass the cap: N + 4 as above).
  ill-conditioned   the QP of tools/resident_soak.py (test_gpu_resident._qp, seed 11, equality rows) through the solver as that tool
                    sets it up, cold starts: the iterates after 1 .. 8 ADMM iterations and of the full solve, the PCG iteration
                    counts and the failed true-residual checks equal between the defaults and PREDICT=0.
  switch-off        margin 1e30 for more solves than the window of 16: the predicted trips stop; they resume after set_rho.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _engine_reference as R
from tests import _pcg_cases as PC
from tests._hipeng import Engine

pytestmark = pytest.mark.gpu

ALPHA = 1.6
WINDOW = 16                                   # RES_PRED_WINDOW of engine_pcg_resident.h
CAP = 64                                      # iterations after which a solve leaves the pipelined phase (engine_pcg_resident.h, k_pcg_resident)
STEPS = 24                                    # consecutive ADMM iterations of the res_e<E> cases
SETTINGS = {"default": {}, "predict0": dict(OSQP_AMD_RESIDENT_PREDICT=0), "margin1e30": dict(OSQP_AMD_RESIDENT_PREDICT_MARGIN="1e30"),
            "pipe0": dict(OSQP_AMD_RESIDENT_PIPE=0)}
# n, m, equality rows of the ill-conditioned QP: tools/resident_soak.py's (900, 700, 200) scaled down.  Every size tried -- (270, 210, 60),
# (360, 280, 80), (450, 350, 100), (600, 467, 133), (900, 700, 200) -- fails true-residual checks in every cold solve (one per solve at
# the smallest, two at the others), and 270 variables are as few as a resident plan takes by default (256): the smallest it is
# (test_ill_conditioned_cold_start asserts that checks fail)
ILL = (270, 210, 60)
ILL_STEPS = 8


def trips(e):
    """hipeng_resident_trips: dict of trips, solves, hits, misses, off (for this K), switch."""
    f = e.L.hipeng_resident_trips
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 8)()
    assert f(e.h, out) == 0
    return dict(trips=out[0], solves=out[1], hits=out[2], misses=out[3], off=out[4], switch=out[5])


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _same_bits(tag, a, b):
    for k, va, vb in zip("xyz", a, b):
        diff = int((_bits(va) != _bits(vb)).sum())
        assert diff == 0, (tag, k, diff, "elements differ")


def _res_env(c, **extra):
    return dict(OSQP_AMD_DENSE_DIRECT=0, OSQP_AMD_RESIDENT_MIN_N=1, OSQP_AMD_RESIDENT_NWG=c["claims"]["nwg"], **extra)


def _open_res(c, E, setting):
    e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=_res_env(c, **SETTINGS[setting]), q=c["q"], l=c["l"], u=c["u"], alpha=ALPHA,
               pcg_eps_rel=PC.PCG_EPS, pcg_max_iter=20000)
    try:
        o = e.ruiz_scale(10)
        e.matrices_changed()
        e.set_rho(c["rho"])
        inf = e.info()
        assert (inf[9], inf[1], inf[2], inf[3]) == (1, 1, E, c["claims"]["nwg"]), (E, setting, inf[:10])
        assert e.elim() == 0
    except BaseException:
        e.close()
        raise
    return e, o


@functools.lru_cache(maxsize=None)
def _steps(E, setting):
    """STEPS ADMM iterations of case res_e<E> from the seeded iterates under one setting, one by one: (x, y, z) after the first,
    info after the first, the Ruiz output, and per iteration (N, trips, hits, misses, off)."""
    c = PC.make("res_e%d" % E)
    e, o = _open_res(c, E, setting)
    try:
        x0, y0, z0 = R.iterates(c)
        e.set_iterates(x0, y0, z0)
        rows, last, first = [], trips(e), None
        for k in range(STEPS):
            e.run_admm(1)
            now, inf = trips(e), e.info()
            assert now["solves"] == last["solves"] + 1 and (inf[7], inf[8], inf[10]) == (0, 0, 0), (E, setting, k, now, inf)
            rows.append((int(inf[6]), now["trips"] - last["trips"], now["hits"] - last["hits"], now["misses"] - last["misses"], now["off"]))
            last = now
            if k == 0:
                s8 = e.stats()
                assert (s8["admm_done"], s8["pcg_forced"], s8["neg_curvature"]) == (1, 0, 0), (E, setting, s8)
                first = (e.download(False)[:3], inf, now)
        return first[0], first[1], first[2], o, rows, last
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _reference(E):
    """The long-double step of case res_e<E> and its bars (computed once, shared, left unchanged)."""
    c = PC.make("res_e%d" % E)
    o = _steps(E, "predict0")[3]
    Pu, A = c["Pu"].copy(), c["A"].copy()
    Pu.data, A.data = o["Px"].copy(), o["Ax"].copy()
    pb = R.Problem(Pu, A, o["q"], o["l"], o["u"], o["D"], o["E"])
    x0, y0, z0 = R.iterates(c)
    st = R.admm_step(pb, R.SIGMA, ALPHA, c["rho"], x0, z0, y0)
    return st, R.step_bars(st, ALPHA, c["rho"], False, PC.PCG_EPS)


@pytest.mark.parametrize("E", [8, 20, 24, 64])
def test_step_within_bars_and_bit_identical(E):
    st, bars = _reference(E)
    runs = {s: _steps(E, s) for s in ("default", "predict0", "margin1e30")}
    for s, (xyz, inf, tr, o, _, _) in runs.items():
        assert inf[10] == 0, (E, s, "a resident launch gave up", inf)
        assert np.all(o["l"] <= xyz[2]) and np.all(xyz[2] <= o["u"])
        for k, got in zip("xyz", xyz):
            err = np.abs(got.astype(R.LD) - st[k]).astype(float)
            ratio = float((err / np.maximum(bars[k], 1e-300)).max()) if err.size else 0.0
            print(f"[last-trip] res_e{E} {s}: {k}+ max err {err.max() if err.size else 0.0:.2e} err/bar {ratio:.3e}; pcg iterations {inf[6]}, {tr}")
            assert np.all(err <= bars[k]), (E, s, k, ratio)
    for s in ("default", "margin1e30"):
        _same_bits(f"res_e{E} {s} against PREDICT=0", runs[s][0], runs["predict0"][0])


def _base_trips(n):
    """Vector trips of a solve of n PCG iterations without the predicted trip and without a failed check that counts: the start-up
    product, n iterations, the trip that learns "converged", the check = n + 3.  A solve that reaches the cap of CAP pipelined
    iterations is cut there, checked (one trip) and finished by the Chronopoulos-Gear recurrences: n + 4."""
    return n + 3 if n < CAP else n + 4


def _check_margin_1e30(tag, rows):
    """rows of (N, trips, hits, misses, off) per solve at margin 1e30: the rule fires after the second iteration -- a miss when
    N > 2 (one trip more), a hit when N == 2 (trip 3 is the one that learns "converged"), nothing when N < 2; the window of
    WINDOW solves is judged as engine_pcg_resident.h's RES_PRED_WINDOW says."""
    ws = wh = wm = 0
    is_off = False
    for k, (n, t, h, m, off) in enumerate(rows):
        eh, em = (0, 0) if is_off or n < 2 else ((1, 0) if n == 2 else (0, 1))
        assert (t, h, m) == (_base_trips(n) - eh + em, eh, em), (tag, "margin 1e30", k, n, t, h, m, is_off)
        if not is_off:
            ws, wh, wm = ws + 1, wh + eh, wm + em
            if ws == WINDOW:
                is_off, ws, wh, wm = wm > wh, 0, 0, 0
        assert off == int(is_off), (tag, "margin 1e30", k, off, is_off)


@pytest.mark.parametrize("E", [8, 20, 24, 64])
def test_trip_counts(E):
    """Per solve of STEPS consecutive ADMM iterations (the first from the seeded iterates; the first solves are longer than the cap
    of the pipelined phase, the later ones stay inside it): the counts of the module's docstring."""
    runs = {s: _steps(E, s) for s in SETTINGS}
    rows = {s: r[4] for s, r in runs.items()}
    N = [r[0] for r in rows["predict0"]]
    print(f"[last-trip] res_e{E}: pcg iterations per solve {N}")
    for s in ("default", "margin1e30"):
        assert [r[0] for r in rows[s]] == N, (E, s, "PCG iterations differ from PREDICT=0", [r[0] for r in rows[s]], N)
    inside = [k for k, n in enumerate(N) if 2 < n < CAP]
    print(f"[last-trip] res_e{E}: solves inside the pipelined phase with N > 2: {len(inside)} of {len(N)}")
    for k, (n, t, h, m, off) in enumerate(rows["predict0"]):
        assert (t, h, m, off) == (_base_trips(n), 0, 0, 0), (E, "PREDICT=0", k, n, t, h, m, off)
    assert runs["predict0"][5]["switch"] == 0 and runs["default"][5]["switch"] == 1
    fired = []
    for k, (n, t, h, m, off) in enumerate(rows["default"]):
        assert m == 0 and h in (0, 1) and t == _base_trips(n) - h, (E, "default margin", k, n, t, h, m)
        assert off == 0 and (h == 0 or 2 <= n < CAP), (E, k, n, h, off)
        fired.append(h)
    print(f"[last-trip] res_e{E}: default margin, hit (N + 2 trips) per solve {fired}: fired and hit in {sum(fired)} of {len(inside)} solves with 2 < N < 64")
    # margin 1e30: fires after the second iteration: a miss when N > 2 (N + 4, or N + 5 past the cap), a hit when N == 2; the window
    # of WINDOW solves is judged as engine_pcg_resident.h's RES_PRED_WINDOW says
    _check_margin_1e30(f"res_e{E}", rows["margin1e30"])
    for k, (n, t, h, m, off) in enumerate(rows["pipe0"]):
        assert (h, m) == (0, 0), (E, "PIPE=0", k, h, m)
    assert runs["pipe0"][1][10] == 0


def _chain(name, setting, count=30):
    """`count` ADMM iterations one by one on the resident form: iterates after 3 and `count`, per-iteration (N, trips, hits, misses)."""
    c = R.make_case(name)
    from tests import _iteration_chain_worker as W
    env = dict(W.ENVS["resident"], **SETTINGS[setting])
    e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=env, q=c["q"], l=c["l"], u=c["u"], alpha=ALPHA, pcg_eps_rel=W.PCG_EPS,
               pcg_max_iter=20000)
    try:
        e.ruiz_scale(10)
        e.matrices_changed()
        e.set_rho(c["rho"])
        inf = e.info()
        assert (inf[9], inf[1]) == (1, 1), (name, setting, "not on the resident form", inf[:10])
        e.set_iterates(*R.iterates(c))
        snaps, rows, last = {}, [], trips(e)
        for k in range(1, count + 1):
            e.run_admm(1)
            now, inf = trips(e), e.info()
            assert inf[7] == 0 and inf[8] == 0 and inf[10] == 0, (name, setting, k, inf)
            if now["solves"] > last["solves"]:                     # (a start vector that passes the stop test runs no solve)
                rows.append((k, int(inf[6]), now["trips"] - last["trips"], now["hits"] - last["hits"], now["misses"] - last["misses"], now["off"]))
            else:
                assert now == last, (name, setting, k, now, last)
            last = now
            if k in (3, count):
                snaps[k] = e.download(False)[:3]
        return snaps, rows, last
    finally:
        e.close()


@pytest.mark.parametrize("name", ["tiny3", "m0", "offtile"])
def test_chain_of_30_iterations(name):
    on, rows, tot = _chain(name, "default")
    off, rows0, tot0 = _chain(name, "predict0")
    for k in (3, 30):
        _same_bits(f"{name} after {k} iterations", on[k], off[k])
    print(f"[last-trip] chain {name}: (iteration, N, trips, hits, misses) with the defaults {rows}")
    print(f"[last-trip] chain {name}: totals with the defaults {tot}, with PREDICT=0 {tot0}")
    assert [r[:2] for r in rows] == [r[:2] for r in rows0], (name, "PCG iterations differ", rows, rows0)
    for k, n, t, h, m, _ in rows0:
        assert (t, h, m) == (_base_trips(n), 0, 0), (name, "PREDICT=0", k, n, t, h, m)
    for k, n, t, h, m, _ in rows:
        assert t == _base_trips(n) - h + m and h + m <= 1, (name, k, n, t, h, m)
        if n <= 1:
            assert h == 0 and m == 0, (name, k, "fired before two residual norms were on record", n, h, m)
    assert tot["trips"] == sum(_base_trips(r[1]) for r in rows) - tot["hits"] + tot["misses"], (name, tot, rows)
    assert tot["trips"] == tot0["trips"] - tot["hits"] + tot["misses"], (name, tot, tot0)
    # the miss path on the same chain: the same bits, and per solve what the rule says at margin 1e30
    miss, rows_m, tot_m = _chain(name, "margin1e30")
    for k in (3, 30):
        _same_bits(f"{name} after {k} iterations, margin 1e30", miss[k], off[k])
    print(f"[last-trip] chain {name}: (iteration, N, trips, hits, misses, off) at margin 1e30 {rows_m}")
    assert [r[:2] for r in rows_m] == [r[:2] for r in rows0], (name, "PCG iterations differ at margin 1e30", rows_m, rows0)
    _check_margin_1e30(f"chain {name}", [r[1:] for r in rows_m])
    assert tot_m["trips"] == tot0["trips"] - tot_m["hits"] + tot_m["misses"], (name, tot_m, tot0)


def _ill_run(size, setting, upto=ILL_STEPS):
    """The soak's QP through the solver, as tools/resident_soak.py sets it up (cold starts, constant rho): solves of 1 .. upto ADMM
    iterations and a full one, each from the cold start: (x, y, iterations, PCG iterations, failed checks so far) of each."""
    import osqp_amd
    from tests._hipeng import _env
    from tests.test_gpu_resident import _info, _qp
    n, m, eq = size
    pb = _qp(n, m, 11, eq=eq)
    with _env(OSQP_AMD_DENSE_SMALL=0, OSQP_AMD_DENSE_DIRECT=0, **SETTINGS[setting]):
        s = osqp_amd.OSQP().setup(**pb, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho=0, warm_start=0)
    inf = _info(s)
    assert inf["form"] == 1 and inf["in_use"], (size, setting, inf)
    out = []
    for k in list(range(1, upto + 1)) + [4000]:
        s.update_settings(max_iter=k)
        r = s.solve()
        inf = _info(s)
        assert inf["gave_up"] == 0 and s.stats()["resident"] == 1, inf
        out.append((np.asarray(r.x, float).copy(), np.asarray(r.y, float).copy(), int(r.info.iter), int(s.stats()["pcg_iters_total"]),
                    int(inf["checks_failed"]), int(inf["pipe_off"])))
    f = osqp_amd.lib().hipeng_resident_trips
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]
    t = (C.c_longlong * 8)()
    assert f(s.engine(), t) == 0
    return out, list(t)[:4]


def test_ill_conditioned_cold_start():
    on, t_on = _ill_run(ILL, "default")
    off, t_off = _ill_run(ILL, "predict0")
    print(f"[last-trip] ill-conditioned {ILL}: (ADMM iterations, PCG iterations, failed checks so far, pipelined phase off) per solve "
          f"{[r[2:] for r in off]}; trips / solves / hits / misses {t_on}, PREDICT=0 {t_off}")
    assert off[-1][4] > 0, (ILL, "no true-residual check failed: not the case this test is about", [r[2:] for r in off])
    assert [r[2:] for r in on] == [r[2:] for r in off], ([r[2:] for r in on], [r[2:] for r in off])
    for k, (a, b) in enumerate(zip(on, off)):
        for name, va, vb in (("x", a[0], b[0]), ("y", a[1], b[1])):
            diff = int((_bits(va) != _bits(vb)).sum())
            assert diff == 0, ("ill-conditioned", "solve", k, name, diff, "elements differ")


def test_switch_off_per_K_and_back_on():
    c = PC.make("res_e20")
    e, _ = _open_res(c, 20, "margin1e30")
    try:
        e.set_iterates(*R.iterates(c))
        seen = []
        for k in range(WINDOW + 4):
            e.run_admm(1)
            seen.append((int(e.info()[6]), trips(e)))
        print("[last-trip] switch-off: (N, counters) per solve " + "; ".join(f"{n} {t['trips']}/{t['hits']}/{t['misses']}/{t['off']}" for n, t in seen))
        at = seen[WINDOW - 1][1]
        assert at["solves"] == WINDOW and at["misses"] > at["hits"] and at["off"] == 1, at
        assert all(t["off"] == 0 for _, t in seen[: WINDOW - 1])
        end = seen[-1][1]
        assert (end["hits"], end["misses"], end["off"]) == (at["hits"], at["misses"], 1), (at, end)
        assert end["trips"] - at["trips"] == sum(_base_trips(n) for n, _ in seen[WINDOW:]), (at, end, [n for n, _ in seen[WINDOW:]])
        e.set_rho(c["rho"] * 2.0)                                    # a new K
        assert trips(e)["off"] == 0
        e.run_admm(1)
        n, after = int(e.info()[6]), trips(e)
        print(f"[last-trip] switch-off: after set_rho N = {n}, {after}")
        assert n > 2 and after["misses"] == end["misses"] + 1 and after["trips"] - end["trips"] == _base_trips(n) + 1, (n, end, after)
        assert e.info()[10] == 0 and e.info()[8] == 0
    finally:
        e.close()
