"""D cotangents per adjoint call and one KKT inversion per solve on the batch engines (BatchOSQP.adjoint with
[B, D, .] arrays, osqp_amd_batch_adjoint_multi, BatchOSQP.kkt_info).

Shapes, problems, incoming gradients, the reference, the excuse rule and the bars are those of
test_gpu_batch_adjoint.py, imported from there; bit equality is `same` of test_gpu_batch_device_io.py (floats by their
bit patterns).  The three cotangents of a shape: _incoming(shape), a second seeded draw, and zeros.  The reference of
the first comes from _references; that of the second is the same function (adjoint_reference on the oracle's polished
x, y, from _oracle_runs) kept under a key of its own, because _references files every explicit gradient under one
key.  tests/test_batch_adjoint_multi_host.py shows the reference linear in the cotangent.

A member whose inversion meets a pivot of the wrong sign (status -1) needs a recipe of its own: that verdict on a kept
inversion is exercised by tests/test_gpu_batch_pivot_verdict.py (test_kept_inversion) on the case "wrongpivot" of
tests/_planted_qp.py, which tests/test_planted_verdict_host.py proves on the CPU."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse

from _adjoint_reference import adjoint_reference
from _batch_parity import rel
from test_gpu_batch_adjoint import (GRADS, M0_SHAPE, STREAMED_SHAPES, TILED_SHAPES, _compare, _family, _incoming,
                                    _oracle_runs, _references)
from test_gpu_batch_device_io import same

pytestmark = pytest.mark.gpu

SMALL = (17, 37, 6, 2)
BIT_SHAPES = [(17, 37, 6, 2), (65, 40, 6, 5)]
ENGINES = ["auto", "streamed"]
FIELDS = GRADS + ("active", "status_adjoint")
_second = {}


def _cotangents(shape):
    """dX [B, 3, n], dY [B, 3, m]: _incoming(shape), a second seeded draw, zeros."""
    n, m, B, seed = shape
    dX0, dY0 = _incoming(shape)
    rng = np.random.default_rng(9090 + seed)
    dX1, dY1 = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    return np.stack([dX0, dX1, np.zeros((B, n))], axis=1), np.stack([dY0, dY1, np.zeros((B, m))], axis=1)


def _second_references(orc, shape, **kw):
    """What _references computes, for the second cotangent (computed once per shape and settings)."""
    key = (shape, tuple(sorted(kw.items())))
    if key not in _second:
        P, A, Q, L, U, _ = _family(shape)
        dX, dY = _cotangents(shape)
        runs = _oracle_runs(orc, shape, **kw)
        _second[key] = [adjoint_reference(P, A, L[b], U[b], ro.x, ro.y, dX[b, 1], dY[b, 1]) for b, ro in enumerate(runs)]
    return _second[key]


def _slice(a, d):
    """Cotangent d of a [B, D, .] result, in the form of a single-cotangent result."""
    return SimpleNamespace(active=a.active, status_adjoint=a.status_adjoint,
                           **{g: None if getattr(a, g) is None else getattr(a, g)[:, d] for g in GRADS})


def _handle(shape, engine, polish=True, **kw):
    import osqp_amd
    P, A, Q, L, U, _ = _family(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **kw)
    r = bs.solve()
    if polish:
        r = bs.polish()
    return bs, r


def _assert_same(a, b, what, fields=FIELDS):
    for k in fields:
        assert same(getattr(a, k), getattr(b, k)), (what, k)


def _check_parity(orc, shape, engine):
    bs, r = _handle(shape, engine)
    n, m, B, _ = shape
    dX, dY = _cotangents(shape)
    a = bs.adjoint(dX, dY, matrices=True)
    assert a.dq.shape == (B, 3, n) and a.dl.shape == a.du.shape == (B, 3, m) and a.active.shape == (B, m)
    assert a.dPx.shape == (B, 3, bs.Pu.nnz) and a.dAx.shape == (B, 3, bs.Ah.nnz) and a.status_adjoint.shape == (B,)
    runs = _oracle_runs(orc, shape, polish=1)
    sp = np.array([ro.info.status_polish for ro in runs])
    assert np.array_equal(r.status_polish, sp), (r.status_polish, sp)
    assert np.all(r.status_val == 1) and np.all(np.isin(a.status_adjoint, (1, -1)))
    accepted = [b for b in range(B) if sp[b] == 1]
    assert accepted
    _compare(_slice(a, 0), _references(orc, shape, polish=1), accepted, "%s %s cotangent 0" % (engine, shape))
    _compare(_slice(a, 1), _second_references(orc, shape, polish=1), accepted, "%s %s cotangent 1" % (engine, shape))
    for g in GRADS:
        assert np.all(getattr(a, g)[:, 2] == 0.0), (g, "the zero cotangent")
    bs.cleanup()


@pytest.mark.parametrize("shape", TILED_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
def test_parity_tiled(gpu_lib, oracle_mod, shape):
    _check_parity(oracle_mod, shape, "auto")


@pytest.mark.parametrize("shape", STREAMED_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
def test_parity_streamed(gpu_lib, oracle_mod, shape):
    _check_parity(oracle_mod, shape, "streamed")


@pytest.mark.parametrize("engine", ENGINES)
def test_parity_no_constraints(gpu_lib, oracle_mod, engine):
    """m = 0, as test_gpu_batch_adjoint.test_no_constraints checks it, per cotangent: dl/dq = -P^-1 dX, no row arrays."""
    bs, r = _handle(M0_SHAPE, engine)
    n, _, B, _ = M0_SHAPE
    P = _family(M0_SHAPE)[0]
    dX, dY = _cotangents(M0_SHAPE)
    a = bs.adjoint(dX, dY, matrices=True)
    Pf = (P + sparse.triu(P, 1).T).toarray()
    assert a.dq.shape == (B, 3, n) and a.dl.shape == a.du.shape == (B, 3, 0) and a.active.shape == (B, 0)
    assert a.dAx.shape == (B, 3, 0) and list(a.status_adjoint) == [1] * B
    for d, refs in ((0, _references(oracle_mod, M0_SHAPE, polish=1)), (1, _second_references(oracle_mod, M0_SHAPE, polish=1))):
        for b in range(B):
            want = -np.linalg.solve(Pf, dX[b, d])
            print("m0", engine, d, b, rel(a.dq[b, d], want), rel(a.dPx[b, d], refs[b].dPx))
            assert rel(a.dq[b, d], want) < 1e-6 and rel(a.dq[b, d], refs[b].dq) < 1e-6 and rel(a.dPx[b, d], refs[b].dPx) < 1e-6
    assert np.all(a.dq[:, 2] == 0.0) and np.all(a.dPx[:, 2] == 0.0)
    assert same(bs.adjoint(dX, None, matrices=True).dq, a.dq)
    bs.cleanup()


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "n%d_m%d" % s[:2])
@pytest.mark.parametrize("engine", ENGINES)
def test_cotangents_carry_the_single_call_bits(gpu_lib, engine, shape):
    """Slice d of a D = 3 call against adjoint(dX[:, d], dY[:, d]) on the same handle; D = 1 of the new entry against the
    existing entry; a permutation of the cotangents."""
    bs, _ = _handle(shape, engine)
    dX, dY = _cotangents(shape)
    a = bs.adjoint(dX, dY, matrices=True)
    assert np.all(a.status_adjoint == 1)
    singles = [bs.adjoint(dX[:, d], dY[:, d], matrices=True) for d in range(3)]
    for d in range(3):
        _assert_same(_slice(a, d), singles[d], ("slice", d))
    one = bs.adjoint(dX[:, :1], dY[:, :1], matrices=True)
    assert one.dq.shape == (shape[2], 1, shape[0])
    _assert_same(_slice(one, 0), singles[0], "D = 1")
    perm = [2, 0, 1]
    p = bs.adjoint(dX[:, perm], dY[:, perm], matrices=True)
    for g in GRADS:
        assert same(getattr(p, g), getattr(a, g)[:, perm]), ("permuted", g)
    assert same(p.active, a.active) and same(p.status_adjoint, a.status_adjoint)
    # without matrices=True the matrix gradients are not computed and the others do not move
    q = bs.adjoint(dX, dY)
    assert q.dPx is None and q.dAx is None
    _assert_same(q, a, "no matrices", ("dq", "dl", "du", "active", "status_adjoint"))
    bs.cleanup()


@pytest.mark.parametrize("engine", ENGINES)
def test_chunks(gpu_lib, monkeypatch, engine):
    """OSQP_AMD_BATCH_POLISH_CAP_BYTES (read at setup) set to two members' matrices, as test_gpu_batch_adjoint.test_chunks
    sets it: three chunks, the same bits, and nothing kept."""
    shape = SMALL
    dX, dY = _cotangents(shape)
    bs, _ = _handle(shape, engine)
    one = bs.adjoint(dX, dY, matrices=True)
    info = bs.kkt_info()
    assert info.kept == 1 and info.members == shape[2]
    npol = (shape[0] + int(np.count_nonzero(one.active, axis=1).max()) + 31) & ~31
    assert info.npol == npol
    monkeypatch.setenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES", str(2 * npol * npol * 8))
    bm, _ = _handle(shape, engine)
    many = bm.adjoint(dX, dY, matrices=True)
    _assert_same(one, many, "chunks")
    assert np.all(one.status_adjoint == 1)
    assert tuple(bm.kkt_info())[1:] == (0, 0, 0)
    again = bm.adjoint(dX, dY, matrices=True)            # nothing was kept: it builds again
    _assert_same(one, again, "chunks, second call")
    assert bm.kkt_info().builds == bs.kkt_info().builds + 1
    bs.cleanup(); bm.cleanup()


def _tangents(shape, nP, nA):
    n, m, B, seed = shape
    rng = np.random.default_rng(5151 + seed)
    return dict(dQ=rng.standard_normal((B, n)), dL=rng.standard_normal((B, m)), dU=rng.standard_normal((B, m)),
                dPx=rng.standard_normal((B, nP)), dAx=rng.standard_normal((B, nA)))


@pytest.mark.parametrize("engine", ENGINES)
def test_one_inversion_per_solve(gpu_lib, monkeypatch, engine):
    """adjoint, adjoint [B, 3, .], tangent and adjoint again on one solve build once; a twin set up under
    OSQP_AMD_BATCH_KKT_CACHE=0 builds four times and returns the same bits.  polish() that does work drops the inversion,
    a second polish() does not, an update withdraws the calls, a solve outdates what was kept."""
    import osqp_amd
    shape = SMALL
    P, A, Q, L, U, _ = _family(shape)
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)
    monkeypatch.setenv("OSQP_AMD_BATCH_KKT_CACHE", "0")
    t = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)
    monkeypatch.delenv("OSQP_AMD_BATCH_KKT_CACHE")
    dX3, dY3 = _cotangents(shape)
    dX, dY = dX3[:, 0], dY3[:, 0]
    tg = _tangents(shape, h.Pu.nnz, h.Ah.nnz)
    TF = ("dx", "dy", "active", "status_tangent")

    def four_calls(b):
        return [b.adjoint(dX, dY, matrices=True), b.adjoint(dX3, dY3, matrices=True), b.tangent(**tg), b.adjoint(dX, dY, matrices=True)]

    def compare(mine, twins, what):
        for k, (x, y) in enumerate(zip(mine, twins)):
            _assert_same(x, y, (what, k), TF if hasattr(x, "dx") else FIELDS)

    assert tuple(h.kkt_info()) == (0, 0, 0, 0)
    for b in (h, t):
        assert np.all(b.solve().status_val == 1)
    got, want = four_calls(h), four_calls(t)
    compare(got, want, "first solve")
    assert np.all(got[0].status_adjoint == 1) and np.all(got[2].status_tangent == 1) and np.any(got[2].dx != 0)
    hi, ti = h.kkt_info(), t.kkt_info()
    assert (hi.builds, hi.kept, hi.members) == (1, 1, shape[2]) and hi.npol % 32 == 0 and hi.npol >= shape[0]
    assert tuple(ti) == (4, 0, 0, 0)
    # polish does work: its own pass counts as a build, and the next call rebuilds at the polished point
    rh, rt = h.polish(), t.polish()
    assert same(rh.x, rt.x) and same(rh.status_polish, rt.status_polish) and np.any(rh.status_polish == 1)
    assert tuple(h.kkt_info()) == (2, 0, 0, 0)
    a_h, a_t = h.adjoint(dX, dY, matrices=True), t.adjoint(dX, dY, matrices=True)
    _assert_same(a_h, a_t, "after polish")
    assert not same(a_h.dPx, got[0].dPx)                 # (the point moved: dPx carries x)
    assert h.kkt_info()[:2] == (3, 1)
    # a second polish finds the work done: nothing is dropped, nothing is built
    assert same(h.polish().x, rh.x)
    assert h.kkt_info()[:2] == (3, 1)
    compare(four_calls(h), four_calls(t), "after polish")
    assert h.kkt_info()[:2] == (3, 1) and t.kkt_info().builds == 4 + 1 + 1 + 4
    # an update withdraws the permission to call, and with it what was kept
    for b in (h, t):
        assert b.update(Q=Q * 1.01) == 0
    assert h.kkt_info()[:2] == (3, 0)
    for call in (lambda: h.adjoint(dX, dY), lambda: h.adjoint(dX3, dY3), lambda: h.tangent(**tg)):
        with pytest.raises(RuntimeError, match=r"failed \(7\)"):
            call()
    # a solve: the next call rebuilds, on the new point
    for b in (h, t):
        b.solve()
    assert h.kkt_info()[:2] == (3, 0)
    got2, want2 = four_calls(h), four_calls(t)
    compare(got2, want2, "second solve")
    assert not same(got2[0].dPx, got[0].dPx)
    assert h.kkt_info()[:2] == (4, 1)
    h.cleanup(); t.cleanup()


@pytest.mark.parametrize("engine", ENGINES)
def test_statuses_on_a_kept_inversion(gpu_lib, engine):
    """The status-mix batch of test_gpu_batch_adjoint.test_unsolved_members_get_zeros: the calls that use the kept
    inversion report 0 and zeros for the members that did not end solved and 1 for the other, as the call that built it."""
    import osqp_amd
    from test_gpu_batch_polish import _mixed
    P, A, Q, L, U, kw = _mixed()
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **kw)
    r = bs.solve()
    assert list(r.status_val) == [1, -3, 2, -2]
    rng = np.random.default_rng(7)
    gX, gY = rng.standard_normal(Q.shape), rng.standard_normal(L.shape)
    first = bs.adjoint(gX, gY, matrices=True)
    assert tuple(bs.kkt_info())[:2] == (1, 1) and bs.kkt_info().members == 1
    second = bs.adjoint(gX, gY, matrices=True)
    gX3, gY3 = np.stack([gX, 2 * gX], axis=1), np.stack([gY, -gY], axis=1)
    multi = bs.adjoint(gX3, gY3, matrices=True)
    tan = bs.tangent(dQ=gX)
    assert tuple(bs.kkt_info())[:2] == (1, 1)
    _assert_same(first, second, "second call")
    _assert_same(_slice(multi, 0), first, "multi, cotangent 0")
    for a in (first, second, multi):
        assert list(a.status_adjoint) == [1, 0, 0, 0]
        assert np.any(a.dq[0] != 0.0)
        for b in (1, 2, 3):
            for g in FIELDS:
                assert np.all(getattr(a, g)[b] == 0), (b, g)
    assert list(tan.status_tangent) == [1, 0, 0, 0] and np.any(tan.dx[0] != 0.0) and np.all(tan.dx[1:] == 0.0)
    bs.cleanup()


@pytest.mark.parametrize("engine", ENGINES)
def test_handle_untouched(gpu_lib, engine):
    """As test_gpu_batch_adjoint.test_handle_untouched, with the new calls in between: results, member_workspace, a later
    polish()'s record and a later adjoint()."""
    shape = SMALL
    bs, r0 = _handle(shape, engine)
    B = shape[2]
    dX3, dY3 = _cotangents(shape)
    a0 = bs.adjoint(dX3[:, 0], dY3[:, 0], matrices=True)
    w0 = [bs.member_workspace(b) for b in range(B)]
    m1 = bs.adjoint(dX3, dY3, matrices=True)
    bs.kkt_info()
    m2 = bs.adjoint(dX3, dY3)
    r1 = bs.results()
    for k in ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert", "status_polish"):
        assert same(getattr(r0, k), getattr(r1, k)), k
    a1 = bs.adjoint(dX3[:, 0], dY3[:, 0], matrices=True)
    _assert_same(a0, a1, "a later adjoint")
    _assert_same(m1, m2, "multi again", ("dq", "dl", "du", "active", "status_adjoint"))
    for b in range(B):
        w1 = bs.member_workspace(b)
        for k in ("D", "E", "ctype", "Kinv", "Pv", "Av"):
            assert np.array_equal(w0[b][k], w1[k]), (b, k)
        assert w0[b]["rho"] == w1["rho"] and w0[b]["c"] == w1["c"], b
    r2 = bs.polish()                                     # polish's own record is still there
    for k in ("x", "y", "info_raw", "status_polish"):
        assert same(getattr(r0, k), getattr(r2, k)), k
    _assert_same(a0, bs.adjoint(dX3[:, 0], dY3[:, 0], matrices=True), "after the second polish")
    bs.cleanup()


def test_device_route(gpu_lib, tmp_path):
    """adjoint_into with [B, 3, .] torch CUDA tensors is bit-equal to adjoint() from host arrays of the same numbers; a
    host array among the device arrays, and outputs of another D, raise ValueError.  In a child process
    (tests/_adjoint_multi_worker.py says why)."""
    dX, dY = _cotangents(SMALL)
    np.savez(tmp_path / "in.npz", dX=dX, dY=dY)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_adjoint_multi_worker.py")
    p = subprocess.run([sys.executable, worker] + [str(v) for v in SMALL] + [str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = SimpleNamespace(**np.load(tmp_path / "out.npz"))
    for k in FIELDS + ("dq_noY", "dl_noY"):
        assert same(getattr(got, "host_" + k), getattr(got, "dev_" + k)), k
    assert got.host_dq.shape == (SMALL[2], 3, SMALL[0]) and np.all(got.host_status_adjoint == 1)
    assert list(got.raised) == [True, True, True]
    assert list(got.kkt_info[:2]) == [2, 1]              # polish's pass, then one build for the four adjoint calls


@pytest.mark.parametrize("engine", ENGINES)
def test_refusals(gpu_lib, engine):
    import ctypes as C
    import osqp_amd
    from osqp_amd import abi
    shape = SMALL
    n, m, B, _ = shape
    P, A, Q, L, U, _ = _family(shape)
    dX, dY = _cotangents(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)
    with pytest.raises(RuntimeError, match=r"failed \(7\)"):
        bs.adjoint(dX, dY)                               # no solve yet
    bs.solve()
    assert np.all(bs.adjoint(dX, dY).status_adjoint == 1)
    out = [np.zeros((B, 1, k)) for k in (n, m, m)]
    act, st = np.zeros((B, m), np.int64), np.zeros(B, np.int64)
    nf = C.cast(None, abi.c_float_p)
    for ncot in (0, -1, 65536):                          # OSQP_DATA_VALIDATION_ERROR, before anything is read
        assert bs._lib.osqp_amd_batch_adjoint_multi(bs._h, ncot, abi.fptr(dX), abi.fptr(dY), *[abi.fptr(o) for o in out],
                                                    nf, nf, abi.iptr(act), abi.iptr(st)) == 1, ncot
        assert bs._lib.osqp_amd_batch_adjoint_multi_dev(bs._h, ncot, *([None] * 9)) == 1, ncot
    assert bs._lib.osqp_amd_batch_adjoint_multi(bs._h, 1, nf, nf, *[abi.fptr(o) for o in out], nf, nf,
                                                abi.iptr(act), abi.iptr(st)) == 1       # dX is NULL
    with pytest.raises(ValueError):
        bs.adjoint(dX[:, :, :-1], dY)
    with pytest.raises(ValueError):
        bs.adjoint(dX, dY[:, :2])
    assert all(o.sum() == 0 for o in out)
    bs.cleanup()


def test_one_engine_per_member_refuses(gpu_lib):
    import osqp_amd
    shape = STREAMED_SHAPES[-1]
    P, A, Q, L, U, _ = _family(shape)
    dX, dY = _cotangents(shape)
    bs = osqp_amd.BatchOSQP().setup(P, A, Q[:2], L[:2], U[:2])
    with pytest.raises(RuntimeError, match='engine="streamed"'):
        bs.adjoint(dX[:2], dY[:2])
    with pytest.raises(RuntimeError, match="one single-QP engine per member"):
        bs.kkt_info()
    bs.cleanup()
