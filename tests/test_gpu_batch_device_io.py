"""GPU tests of the device-array route of the batch engines (include/osqp_amd_batch.h, "Device arrays in and out"):
`BatchOSQP.update`, `update_matrices` and `warm_start` given device arrays, `results_into`, `adjoint_into`, the pointer
check, and `BatchQPLayer` on CUDA tensors.

The bar everywhere is bit equality between a handle driven through host arrays and a twin, set up from the same data,
driven through device arrays holding the same numbers: both run the same arithmetic kernels on the same workspace, so
nothing weaker is warranted.  Floats are compared by their bit patterns (so a NaN would equal itself and -0.0 would
not equal 0.0), integers by value.

No torch here (the layer runs in a child process, tests/_device_layer_worker.py): device buffers are hipMalloc'd
through ctypes and wrapped in a small class with `__cuda_array_interface__`.  No entry point that copies or launches is
ever given a pointer that is not device memory; only the classifying hook sees a host address.

Shapes (n, m, B), problems from tests/_batch_parity.shape_family, whose bounds hold +-inf (so the clamp on the device
is compared with numpy's):
  tiled     (17, 37, 5)    off the tile; the whole bound check is one workgroup (185 elements)
  tiled     (64, 131, 7)   917 bound elements: four check workgroups, the last one ragged (149 of 256)
  tiled     (3, 0, 4)      m = 0
  streamed  (40, 40, 6), (150, 300, 3)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from _batch_parity import shape_family

pytestmark = pytest.mark.gpu

KW = dict(adaptive_rho_interval=10)
SHAPES = [("auto", 17, 37, 5), ("auto", 64, 131, 7), ("auto", 3, 0, 4), ("streamed", 40, 40, 6), ("streamed", 150, 300, 3)]
IDS = ["%s-%d-%d-%d" % s for s in SHAPES]
TYPESTR = {np.dtype(np.float64): "<f8", np.dtype(np.int32): "<i4"}


class Device:
    """hipMalloc'd arrays for one test, freed when it ends."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.live = []

    def empty(self, shape, dtype=np.float64):
        return DevArray(self, tuple(shape), np.dtype(dtype))

    def put(self, a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        d = self.empty(a.shape, a.dtype)
        if a.nbytes:
            assert self.hip.hipMemcpy(d.ptr, a.ctypes.data, a.nbytes, 1) == 0       # hipMemcpyHostToDevice
        return d

    def close(self):
        for p in self.live:
            self.hip.hipFree(p)
        self.live = []


class DevArray:
    def __init__(self, dev, shape, dtype):
        self.dev, self.shape, self.dtype = dev, shape, dtype
        self.nbytes = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        assert dev.hip.hipMalloc(C.byref(p), max(self.nbytes, 8)) == 0 and p.value
        self.ptr = p.value
        dev.live.append(self.ptr)
        self.__cuda_array_interface__ = dict(shape=shape, typestr=TYPESTR[dtype], data=(self.ptr, False), version=2, strides=None)

    def get(self):
        h = np.empty(self.shape, self.dtype)
        if self.nbytes:
            assert self.dev.hip.hipMemcpy(h.ctypes.data, self.ptr, self.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return h


@pytest.fixture
def dev(gpu_lib):
    d = Device()
    yield d
    d.close()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float64 and b.dtype == np.float64:
        return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    return np.array_equal(a, b)


def twins(engine, n, m, B, seed):
    """The problem and two handles set up from it: [0] is driven through host arrays, [1] through device arrays."""
    import osqp_amd
    pb = shape_family(n, m, B, seed)
    P, A, Q, L, U, _ = pb
    return pb, [osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **KW) for _ in range(2)]


def moved(Q, L, U, rng):
    """New data every member can hold: each member gets its neighbour's bounds (its row classes change, so K^-1 is
    rebuilt), a little wider; infinite bounds stay infinite."""
    return Q * rng.uniform(0.8, 1.2, Q.shape) + 0.1 * rng.standard_normal(Q.shape), np.roll(L, 1, axis=0) - 0.05, np.roll(U, 1, axis=0) + 0.07


def fetch_device(h, dev):
    """X, Y, info8, DX, DY, status_polish of a handle through results_into (m-sized ones None when m = 0)."""
    B, n, m = h.B, h.n, h.m
    X, I, DX, sp = dev.empty((B, n)), dev.empty((B, 8)), dev.empty((B, n)), dev.empty((B,), np.int32)
    Y, DY = (dev.empty((B, m)), dev.empty((B, m))) if m else (None, None)
    h.results_into(X=X, Y=Y, info=I, DX=DX, DY=DY, status_polish=sp)
    z = np.zeros((B, 0))
    return dict(x=X.get(), y=Y.get() if m else z, info_raw=I.get(), dual_inf_cert=DX.get(), prim_inf_cert=DY.get() if m else z,
                status_polish=sp.get())


def assert_same_results(r, g, what):
    for k in ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert", "status_polish"):
        assert same(getattr(r, k), g[k]), (what, k)


def solve_both(hs, dev, what):
    """One solve on each twin; the host twin's results against the device twin's, fetched on the device."""
    r = hs[0].solve()
    hs[1].solve(fetch=False)
    assert_same_results(r, fetch_device(hs[1], dev), what)
    return r


def cleanup(hs):
    for h in hs:
        h.cleanup()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_update_chain_is_bit_equal(shape, dev):
    """update(Q, L, U) -> solve -> polish -> adjoint(matrices=True) -> results: all thirteen arrays."""
    engine, n, m, B = shape
    (P, A, Q, L, U, _), hs = twins(engine, n, m, B, seed=21)
    rng = np.random.default_rng(5)
    Q2, L2, U2 = moved(Q, L, U, rng)
    if m:
        assert np.isinf(L2).any() and np.isinf(U2).any()       # the clamp has work to do
    gx, gy = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    assert hs[0].update(Q=Q2, L=L2, U=U2) == 0
    assert hs[1].update(Q=dev.put(Q2), L=dev.put(L2), U=dev.put(U2)) == 0
    hs[0].solve(fetch=False); hs[1].solve(fetch=False)
    r = hs[0].polish()
    assert hs[1].polish(fetch=False) is None
    assert_same_results(r, fetch_device(hs[1], dev), "polished")
    assert same(hs[1].results().status_polish, r.status_polish)       # results() after polish(fetch=False) reads the status
    assert (r.status_val == 1).any() and (r.status_polish != 0).any()
    a = hs[0].adjoint(gx, gy if m else None, matrices=True)
    nP, nA = hs[1].Pu.nnz, hs[1].Ah.nnz
    out = dict(dq=dev.empty((B, n)), dPx=dev.empty((B, nP)), dAx=dev.empty((B, nA)), status_adjoint=dev.empty((B,), np.int32))
    if m:
        out.update(dl=dev.empty((B, m)), du=dev.empty((B, m)), active=dev.empty((B, m), np.int32))
    else:
        out.update(dl=None, du=None, active=None)
    hs[1].adjoint_into(dev.put(gx), dev.put(gy) if m else None, **out)
    assert (a.status_adjoint == 1).any()
    for k, d in out.items():
        if d is not None:
            assert same(getattr(a, k), d.get()), k
    assert_same_results(hs[0].results(), fetch_device(hs[1], dev), "after the adjoint")
    cleanup(hs)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_update_of_a_subset_is_bit_equal(shape, dev):
    engine, n, m, B = shape
    (P, A, Q, L, U, _), hs = twins(engine, n, m, B, seed=22)
    Q2, L2, U2 = moved(Q, L, U, np.random.default_rng(6))
    for name, v in (("Q", Q2), ("L", L2), ("U", U2)):
        assert hs[0].update(**{name: v}) == 0
        assert hs[1].update(**{name: dev.put(v)}) == 0
        solve_both(hs, dev, name + " only")
    cleanup(hs)


def test_refused_update_changes_nothing(dev):
    """One l > u pair at the first element, the last one (the tail of the last check workgroup) and one in between:
    the call returns 1 and the twin that never saw it solves to the same bits -- right away, and again after a matrix
    update has re-read the raw q, l, u of both."""
    engine, n, m, B = SHAPES[1]
    (P, A, Q, L, U, _), hs = twins(engine, n, m, B, seed=23)
    solve_both(hs, dev, "first solve")
    Q2, L2, U2 = moved(Q, L, U, np.random.default_rng(7))
    for pos in (0, B * m - 1, 3 * m + 77):
        Lb, Ub = L2.copy(), U2.copy()
        Lb.flat[pos], Ub.flat[pos] = 1.0, 0.0
        assert hs[1].update(Q=dev.put(Q2), L=dev.put(Lb), U=dev.put(Ub)) == 1, pos
        solve_both(hs, dev, "after the refusal at %d" % pos)
    Ax = A.tocsc().data * np.random.default_rng(8).uniform(0.7, 1.4, A.nnz)
    assert hs[0].update_matrices(Ax=Ax) == 0 and hs[1].update_matrices(Ax=Ax) == 0
    solve_both(hs, dev, "after a matrix update")
    cleanup(hs)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_update_matrices_is_bit_equal(shape, dev):
    """Shared full Ax; per-member full Ax; per-member Px on an index subset; both matrices at once -- each followed by
    a warm solve.  A bad host index list is refused with the twin's codes, before the device array is looked at."""
    from osqp_amd import abi
    engine, n, m, B = shape
    (P, A, Q, L, U, _), hs = twins(engine, n, m, B, seed=24)
    solve_both(hs, dev, "first solve")
    nP, nA = hs[0].Pu.nnz, hs[0].Ah.nnz
    Px0, Ax0 = hs[0].Pu.x[:nP].copy(), hs[0].Ah.x[:nA].copy()
    diag = np.flatnonzero(hs[0].Pu.i[:nP] == np.repeat(np.arange(n), np.diff(hs[0].Pu.p)))
    rng = np.random.default_rng(9)
    idx = np.union1d(diag[::2], rng.choice(nP, 3, replace=False))
    grow = lambda k: np.where(np.isin(k, diag), rng.uniform(1.3, 1.9, (B, k.size)), rng.uniform(0.5, 1.0, (B, k.size)))
    variants = [("shared Ax", dict(Ax=Ax0 * rng.uniform(0.6, 1.5, nA))),
                ("per-member Ax", dict(Ax=Ax0 * rng.uniform(0.6, 1.5, (B, nA)))),
                ("per-member Px on a subset", dict(Px=Px0[idx] * grow(idx), Px_idx=idx)),
                ("both", dict(Px=Px0 * grow(np.arange(nP)), Ax=Ax0 * rng.uniform(0.6, 1.5, (B, nA))))]
    for what, kw in variants:
        on_device = {k: (v if k.endswith("idx") else dev.put(v)) for k, v in kw.items()}
        assert hs[0].update_matrices(**kw) == 0, what
        assert hs[1].update_matrices(**on_device) == 0, what
        solve_both(hs, dev, what)
    # the refusals of the C entry point itself (BatchOSQP.update_matrices raises before it gets there)
    lib, vals = hs[1]._lib, dev.put(np.ones((B, max(nP, nA) + 1)))
    null_i = C.cast(None, abi.c_int_p)
    long_list, bad = np.zeros(max(nP, nA) + 1, np.int64), np.array([0, nP + nA], np.int64)
    calls = [((vals.ptr, abi.iptr(long_list), nP + 1, 1, None, null_i, 0, 0), 1),
             ((None, null_i, 0, 0, vals.ptr, abi.iptr(long_list), nA + 1, 1), 2),
             ((vals.ptr, abi.iptr(bad), 2, 1, None, null_i, 0, 0), 1),             # OSQP_DATA_VALIDATION_ERROR
             ((None, null_i, 0, 0, vals.ptr, abi.iptr(bad), 2, 1), 1)]
    host_vals = np.ones((B, max(nP, nA) + 1))
    for args, want in calls:
        assert lib.osqp_amd_batch_update_matrices_dev(hs[1]._h, *args) == want
        host_args = tuple(abi.fptr(host_vals) if a == vals.ptr else (C.cast(None, abi.c_float_p) if a is None else a) for a in args)
        assert lib.osqp_amd_batch_update_matrices(hs[0]._h, *host_args) == want
    solve_both(hs, dev, "after the refusals")
    cleanup(hs)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]], ids=[IDS[0], IDS[4]])
def test_warm_start_is_bit_equal(shape, dev):
    engine, n, m, B = shape
    (P, A, Q, L, U, x0), hs = twins(engine, n, m, B, seed=25)
    rng = np.random.default_rng(10)
    for what in ("X", "Y", "XY"):
        kw = {}
        if "X" in what:
            kw["X"] = x0 + 0.1 * rng.standard_normal((B, n))
        if "Y" in what:
            kw["Y"] = rng.standard_normal((B, m))
        assert hs[0].warm_start(**kw) == 0
        assert hs[1].warm_start(**{k: dev.put(v) for k, v in kw.items()}) == 0
        solve_both(hs, dev, "warm start " + what)
    cleanup(hs)


def test_results_into_and_adjoint_into(dev):
    """Outputs may be left out; what was fetched is the caller's copy, which a later solve does not touch; the
    adjoint before any solve is refused with OSQP_WORKSPACE_NOT_INIT_ERROR."""
    engine, n, m, B = SHAPES[0]
    (P, A, Q, L, U, _), hs = twins(engine, n, m, B, seed=26)
    rng = np.random.default_rng(11)
    gx = dev.put(rng.standard_normal((B, n)))
    dq, dl, du = dev.empty((B, n)), dev.empty((B, m)), dev.empty((B, m))
    with pytest.raises(RuntimeError, match=r"\(7\)"):
        hs[1].adjoint_into(gx, None, dq, dl, du)
    r = solve_both(hs, dev, "first solve")
    X, sp = dev.empty((B, n)), dev.empty((B,), np.int32)
    hs[1].results_into(X=X)                                   # X alone
    hs[1].results_into(status_polish=sp)                      # no polish since the solve: not tried
    assert same(X.get(), r.x) and not sp.get().any()
    a = hs[0].adjoint(gx.get())
    hs[1].adjoint_into(gx, None, dq, dl, du)                  # no dY, no matrix gradients, no active, no status
    assert same(dq.get(), a.dq) and same(dl.get(), a.dl) and same(du.get(), a.du)
    kept = (X.get(), dq.get())
    Q2 = moved(Q, L, U, rng)[0]
    assert hs[0].update(Q=Q2) == 0 and hs[1].update(Q=dev.put(Q2)) == 0
    r2 = solve_both(hs, dev, "second solve")
    assert not same(r2.x, r.x)
    assert same(X.get(), kept[0]) and same(dq.get(), kept[1])
    cleanup(hs)


def test_pointer_check(dev):
    """The hook alone is shown a host address; it only asks the runtime about it."""
    (P, A, Q, L, U, _), hs = twins("auto", 17, 37, 2, seed=27)
    lib = hs[0]._lib
    d = dev.empty((4, 8))
    host = np.zeros(32)
    assert lib.osqp_amd_batch_check_dev_ptr(hs[0]._h, d.ptr) == 0
    assert lib.osqp_amd_batch_check_dev_ptr(hs[0]._h, d.ptr + 8 * 5) == 0          # inside the allocation
    assert lib.osqp_amd_batch_check_dev_ptr(hs[0]._h, host.ctypes.data) == 1       # OSQP_DATA_VALIDATION_ERROR
    assert lib.osqp_amd_batch_check_dev_ptr(hs[0]._h, None) == 1
    cleanup(hs)


def test_layer_on_cuda_tensors(gpu_lib, tmp_path):
    """BatchQPLayer on (17, 37, 5) with CUDA tensors against the same layer with CPU tensors: X, Y and the gradients
    for Q, L, U and Ax bit-equal, in the first call (which sets the handle up) and in two more calls on the live
    handle (which take the device entry points); the third one's loss is X.sum() + Y.sum(), whose incoming gradients
    are expanded, non-contiguous tensors.  The layer runs in a child process
    (tests/_device_layer_worker.py says why)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_device_layer_worker.py")
    out = tmp_path / "out.npz"
    p = subprocess.run([sys.executable, worker, "17", "37", "5", "3", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    g = np.load(out)
    assert list(g["routes"]) == ["device"] * 3 + ["host"] * 3
    assert bool(g["outputs_on_device"]) and bool(g["last_results_on_device"])
    for call in ("1", "2", "3"):
        for k in ("X", "Y", "dq", "dl", "du", "dAx", "status_polish", "status_adjoint"):
            assert same(g["dev_" + k + call], g["host_" + k + call]), (k, call)
        assert (g["host_status_adjoint" + call] == 1).any()
    assert not same(g["host_X1"], g["host_X2"])
