"""Cases of tests/test_gpu_batch_members.py: the member lists, the small problems per engine, the new rows a member
update brings and the whole-batch arrays that say the same, and hipMalloc'd device arrays for the _dev forms.

Shapes: B = 9 with lists at both ends, a scattered one and all of them; n off every tile (17 on the tiled engine, 40 and
33 on the streamed and the common-K engine, m = 2 n), so that a member's rows end inside a wavefront and the 256-wide
loops of the per-member kernels take one partial pass."""
import ctypes as C

import numpy as np
from scipy import sparse

from _batch_parity import shape_family
from _common_cases import FIXED, common_family

B = 9
ENGINES = ("auto", "streamed", "common")
SHAPES = dict(auto=(17, 34), streamed=(40, 80), common=(33, 66))
LISTS = dict(first=[0], last=[B - 1], three=[2, 3, 7], all=list(range(B)))
# a fixed rho: a member's solve then depends on nothing but its own data and iterates
FIXED_RHO = dict(auto=dict(adaptive_rho=0), streamed=dict(adaptive_rho=0), common=dict(FIXED))
ARRAYS = ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert")
_problems = {}


def problem(engine, m0=False, qscale=1.0, shape=None):
    """(P, A, Q, L, U) of the engine's shape, or of `shape` (built once, never modified); m0: no constraints."""
    key = (engine, m0, qscale, shape)
    if key not in _problems:
        n, m = shape or SHAPES[engine]
        seed = 500 + n
        if m0:
            P, _, Q = shape_family(n, m, B, seed)[:3]
            A = sparse.csc_matrix((0, n)); L = np.zeros((B, 0)); U = np.zeros((B, 0))
        elif engine == "common":
            P, A, Q, L, U = common_family(n, m, B, seed)[:5]
        else:
            P, A, Q, L, U = shape_family(n, m, B, seed)[:5]
        _problems[key] = (P, A, Q * qscale, L, U)
    return _problems[key]


def handle(engine, pb, **kw):
    import osqp_amd
    P, A, Q, L, U = pb
    extra = dict(shared_kkt=True) if engine == "common" else {}
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **extra, **{**FIXED_RHO[engine], **kw})


def new_rows(engine, cur, S, which, seed):
    """Compact new rows for the members S of the data `cur` (dict Q, L, U): which in "Q", "L", "U", "QLU".  Bounds move
    outward (L down, U up) or, together, by a common shift, so l <= u holds.  A lone L or U turns the equality rows of
    the listed members into inequalities -- a class change, which the tiled and the streamed engine serve per member
    (BF_REBUILD for the listed alone); the common-K engine holds one class per row, so there the equality rows stay."""
    rng = np.random.default_rng(seed)
    S = np.asarray(S)
    Q, L, U = cur["Q"][S], cur["L"][S], cur["U"][S]
    out = {}
    if "Q" in which:
        out["Q"] = Q * rng.uniform(0.8, 1.25, Q.shape) + 0.05 * rng.standard_normal(Q.shape)
    step = rng.uniform(0.01, 0.05, L.shape)
    if which == "QLU":
        out["L"], out["U"] = L + step, U + step
    else:
        keep = (L == U) if engine == "common" else np.zeros(L.shape, bool)
        if which == "L":
            out["L"] = np.where(keep, L, L - step)
        if which == "U":
            out["U"] = np.where(keep, U, U + step)
    return out


def whole(cur, S, rows):
    """The [B, .] arrays of a whole-batch update that says what update(members=S, **rows) says: the unlisted rows
    repeated from what the handle holds."""
    out = {}
    for k, v in rows.items():
        a = cur[k].copy()
        a[np.asarray(S)] = v
        out[k] = a
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(r1, r2, i1=slice(None), i2=slice(None), fields=ARRAYS, what=""):
    for k in fields:
        a, b = getattr(r1, k), getattr(r2, k)
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert np.array_equal(bits(a[i1]), bits(b[i2])), (what, k)


def same_workspace(w1, w2, what=""):
    assert w1.keys() == w2.keys()
    for k in w1:
        assert np.array_equal(bits(np.asarray(w1[k], dtype=None)), bits(np.asarray(w2[k], dtype=None))), (what, k)


# ---- device arrays ------------------------------------------------------------------------------------------------------
TYPESTR = {np.dtype(np.float64): "<f8", np.dtype(np.int32): "<i4"}


class Device:
    """hipMalloc'd arrays for one test, freed when it ends (as tests/test_gpu_batch_device_io.py makes them)."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.live = []

    def put(self, a, dtype=np.float64, rows=None):
        """a on the device; rows: the array the handle sees is the first `rows` rows of it (the others guard)."""
        a = np.ascontiguousarray(a, dtype=dtype)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0 and p.value
        self.live.append(p.value)
        if a.nbytes:
            assert self.hip.hipMemcpy(p.value, a.ctypes.data, a.nbytes, 1) == 0       # hipMemcpyHostToDevice
        return DevArray(self, p.value, a.shape, a.dtype, rows)

    def close(self):
        for p in self.live:
            self.hip.hipFree(p)
        self.live = []


class DevArray:
    def __init__(self, dev, ptr, shape, dtype, rows=None):
        self.dev, self.ptr, self.full, self.dtype = dev, ptr, shape, dtype
        seen = shape if rows is None else (rows,) + tuple(shape[1:])
        self.__cuda_array_interface__ = dict(shape=tuple(seen), typestr=TYPESTR[dtype], data=(ptr, False), version=2, strides=None)

    def get(self):
        """The whole allocation, guard rows included."""
        h = np.empty(self.full, self.dtype)
        if h.nbytes:
            assert self.dev.hip.hipMemcpy(h.ctypes.data, self.ptr, h.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return h
