"""GPU tests of the start-up of k_pcg_resident (engine_pcg_resident.h): the entry, the start-up sums of wavefront 0, u0 taken in before the loop.

Wavefront 0 alone sums k_pcg_init's partials of ||r0||^2 and ||b||^2 (every load in flight at once, added in the order the sum has
always had) and hands tol2 and the verdict "the start vector already passes" to the other seven through LDS; all eight leave
together behind the barrier in front of the loop.  u0 is swept into LDS before that barrier (OSQP_AMD_RESIDENT_U0=0: it is exchanged
like every later vector).  Engines are built like test_gpu_resident_last_trip builds them.  Every case asserts the resident form
(info()[9] == 1), in use, no launch that gave up, and its premise about gridM through layout()[12].

  tol2 to the bit   State::tol2 of a launch equals tests/_resident_startup.py's float64 replay on the partials of ||b||^2 downloaded
                    from the device (hipeng_resident_start_peek), at gridM = 1 (`tiny3`), a few (`res_e8`), more than 64 (`res_e64`)
                    and the cap of 1024 (a banded P of 1200 rows of 129 entries: every row of M a block of its own).
                    tests/test_resident_startup_reference_host.py holds the replay against long double and shows that a sum which
                    loses the last partial of a lane is another number.  Shown once on a scratch build whose lanes stop one partial
                    short: all four cases fail on it, as they must (profiles/resident_startup_identity.txt).  Measured gridM: 1, 15,
                    610, 1024.
  step bars, bits   res_e8, res_e20, res_e24, res_e64: one ADMM step from non-zero iterates within _engine_reference.step_bars (the
                    long-double reference test_gpu_resident_last_trip computes, shared), and OSQP_AMD_RESIDENT_U0=0 equal to the
                    default in every bit of x, y and z.
  starts converged  `tiny3` and `m0` until an iteration's start vector passes the stop test: that solve has 0 PCG iterations, the
                    trip counters stand still, no launch gave up, and the iteration after it lies within its bars.
"""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy import sparse

from tests import _engine_reference as R
from tests import _iteration_chain_worker as W
from tests import _pcg_cases as PC
from tests import _resident_startup as S
from tests._hipeng import Engine
from tests.test_gpu_resident_last_trip import ALPHA, _reference, _res_env, _same_bits, trips

pytestmark = pytest.mark.gpu

CAP = 1024                                    # MAX_PARTS of engine_device.h


def peek(e):
    """hipeng_resident_start_peek: gridM, the partials of ||b||^2 as the last k_pcg_init left them, State::tol2 of the last launch."""
    f = e.L.hipeng_resident_start_peek
    f.restype, f.argtypes = C.c_longlong, [C.c_void_p, C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_double)]
    buf, tol2 = (C.c_double * CAP)(), C.c_double()
    g = f(e.h, buf, CAP, C.byref(tol2))
    assert 1 <= g <= CAP, g
    return int(g), np.array(buf[:g], dtype=np.float64), float(tol2.value)


def _on_resident(e, tag, nwg=None):
    inf = e.info()
    assert (inf[9], inf[0], inf[1], inf[10]) == (1, 1, 1, 0), (tag, "not a resident engine in use", inf[:11])
    if nwg is not None:
        assert inf[3] == nwg, (tag, inf[:11])


def _cap_case():
    """More than 1024 row blocks of M: n = 1200, P banded with half-width 64 (129 entries in an interior row, so no two of them share
    a block of 256 products; nnz(M) about 155 000 keeps the chunk at 256), diagonally dominant; four short rows of A."""
    n, m, hw = 1200, 4, 64
    rng = np.random.default_rng(4242)
    i, j = np.triu_indices(n, 1)
    keep = j - i <= hw
    i, j = i[keep], j[keep]
    v = rng.uniform(-1.0, 1.0, i.size) / (2.0 * hw)
    d = np.ones(n)
    np.add.at(d, i, np.abs(v)); np.add.at(d, j, np.abs(v))
    Pu = sparse.csc_matrix((np.concatenate([v, d]), (np.concatenate([i, np.arange(n)]), np.concatenate([j, np.arange(n)]))), shape=(n, n))
    Pu.sort_indices()
    rows = np.repeat(np.arange(m), 3)
    cols = np.array([5, 300, 900, 17, 600, 1100, 64, 65, 66, 1, 598, 1199])
    A = sparse.csc_matrix((rng.uniform(0.5, 1.0, rows.size), (rows, cols)), shape=(m, n))
    A.sort_indices()
    return dict(name="cap1024", n=n, m=m, Pu=Pu, A=A, q=rng.standard_normal(n), l=-np.ones(m), u=np.ones(m), rho=np.full(m, R.RHO),
                x=rng.standard_normal(n), y=rng.standard_normal(m) * 0.05, z=rng.standard_normal(m))


def _open(c, env):
    e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=env, q=c["q"], l=c["l"], u=c["u"], alpha=ALPHA, pcg_eps_rel=PC.PCG_EPS,
               pcg_max_iter=20000)
    try:
        o = e.ruiz_scale(10)
        e.matrices_changed()
        e.set_rho(c["rho"])
    except BaseException:
        e.close()
        raise
    return e, o


TOL2_CASES = {                                # name -> (case, environment, forced grid, premise about gridM)
    "tiny3": (lambda: R.make_case("tiny3"), lambda c: W.ENVS["resident"], lambda g: g == 1),
    "res_e8": (lambda: PC.make("res_e8"), lambda c: _res_env(c), lambda g: 2 <= g <= 63),
    "res_e64": (lambda: PC.make("res_e64"), lambda c: _res_env(c), lambda g: 64 < g < CAP),
    "cap1024": (_cap_case, lambda c: W.ENVS["resident"], lambda g: g == CAP),
}


@pytest.mark.parametrize("name", list(TOL2_CASES))
def test_tol2_to_the_bit(name):
    make, env, premise = TOL2_CASES[name]
    c = make()
    e, _ = _open(c, env(c))
    try:
        _on_resident(e, name, c["claims"]["nwg"] if "claims" in c else None)
        g12 = e.layout()[12]
        assert premise(g12), (name, "gridM is not what this case is about", g12)
        x0, y0, z0 = (c["x"], c["y"], c["z"]) if "x" in c else R.iterates(c)
        e.set_iterates(x0, y0, z0)
        for k in range(2):                    # two launches: the second sums other partials with another epoch
            before = trips(e)
            e.run_admm(1)
            _on_resident(e, name)
            g, part, tol2 = peek(e)
            assert g == g12 and part.size == g, (name, g, g12)
            want = S.tol2(part, e.prm.pcg_eps_rel, e.prm.pcg_eps_abs)
            print(f"[resident-startup] {name} launch {k}: gridM {g}, sum |part| {np.abs(part).sum():.6e}, tol2 {tol2!r}, replay {float(want)!r}, "
                  f"solves {trips(e)['solves'] - before['solves']}")
            assert np.float64(tol2).view(np.uint64) == np.float64(want).view(np.uint64), (name, k, g, tol2, float(want))
            assert tol2 > 0.0 and np.all(part >= 0.0) and part.sum() > 0.0, (name, k)
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _one_step(E, u0):
    c = PC.make("res_e%d" % E)
    e, o = _open(c, _res_env(c, **({} if u0 is None else dict(OSQP_AMD_RESIDENT_U0=u0))))
    try:
        _on_resident(e, (E, u0), c["claims"]["nwg"])
        assert e.info()[2] == E and e.elim() == 0, (E, e.info()[:11])
        g12 = e.layout()[12]
        e.set_iterates(*R.iterates(c))
        e.run_admm(1)
        _on_resident(e, (E, u0))
        inf, st = e.info(), e.stats()
        assert (inf[7], inf[8]) == (0, 0) and (st["admm_done"], st["pcg_forced"], st["neg_curvature"]) == (1, 0, 0), (E, u0, inf, st)
        return e.download(False)[:3], o, int(inf[6]), trips(e), g12
    finally:
        e.close()


@pytest.mark.parametrize("E", [8, 20, 24, 64])
def test_step_within_bars_and_u0_paths_bit_identical(E):
    st, bars = _reference(E)
    runs = {u0: _one_step(E, u0) for u0 in (None, 0)}
    g12 = runs[None][4]
    assert (2 <= g12 <= 63) if E == 8 else (64 < g12 < CAP), (E, "gridM", g12)
    for u0, (xyz, o, iters, tr, _) in runs.items():
        assert np.all(o["l"] <= xyz[2]) and np.all(xyz[2] <= o["u"])
        for k, got in zip("xyz", xyz):
            err = np.abs(got.astype(R.LD) - st[k]).astype(float)
            ratio = float((err / np.maximum(bars[k], 1e-300)).max()) if err.size else 0.0
            print(f"[resident-startup] res_e{E} U0={u0}: {k}+ max err {err.max() if err.size else 0.0:.2e} err/bar {ratio:.3e}; gridM {g12}, "
                  f"pcg iterations {iters}, {tr}")
            assert np.all(err <= bars[k]), (E, u0, k, ratio)
    # u0 exchanged instead of read: one vector trip more, the same numbers
    assert runs[0][2] == runs[None][2], (E, "PCG iterations differ between the two ways u0 arrives", runs[0][2], runs[None][2])
    _same_bits(f"res_e{E} OSQP_AMD_RESIDENT_U0=0 against the default", runs[0][0], runs[None][0])


@pytest.mark.parametrize("name", ["tiny3", "m0"])
def test_solve_that_starts_converged(name, limit=500):      # (test_gpu_iteration_chain's from_start needs 154 and 14 iterations at alpha = 1)
    c = R.make_case(name)
    e, o, pb, _ = W.open_case(c, "resident")
    try:
        _on_resident(e, name)
        assert e.layout()[12] >= 1
        last, found, total = trips(e), None, e.stats()["pcg_iters_total"]
        for k in range(1, limit + 1):
            before = e.download(False)[:3]
            e.run_admm(1)
            _on_resident(e, (name, k))
            now, st = trips(e), e.stats()
            if found is not None:             # the iteration after the one that started converged: within its bars
                x, y, z = before
                ref = R.admm_step(pb, R.SIGMA, ALPHA, c["rho"], x, z, y)
                bars = R.step_bars(ref, ALPHA, c["rho"], False, W.PCG_EPS)
                for key, got in zip("xyz", e.download(False)[:3]):
                    err = np.abs(got.astype(R.LD) - ref[key]).astype(float)
                    ratio = float((err / np.maximum(bars[key], 1e-300)).max()) if err.size else 0.0
                    print(f"[resident-startup] {name} iteration {k} (after the converged start): {key}+ err/bar {ratio:.3e}, pcg iterations {st['pcg_iters_last']}")
                    assert np.all(err <= bars[key]), (name, k, key, ratio)
                break
            if now["solves"] == last["solves"]:
                found = k
                assert now == last, (name, k, "the trip counters moved in a launch that ran no solve", now, last)
                assert (st["pcg_iters_last"], st["pcg_iters_total"] - total, st["admm_done"]) == (0, 0, 1), (name, k, total, st)
                g, part, tol2 = peek(e)
                want = S.tol2(part, e.prm.pcg_eps_rel, e.prm.pcg_eps_abs)
                assert np.float64(tol2).view(np.uint64) == np.float64(want).view(np.uint64), (name, k, tol2, float(want))
                print(f"[resident-startup] {name}: the start vector of iteration {k} passes the stop test (tol2 {tol2:.3e}); counters {now}")
            last, total = now, st["pcg_iters_total"]
        assert found is not None, (name, f"no start vector passed the stop test in {limit} iterations")
        assert found < limit, (name, found)
    finally:
        e.close()
