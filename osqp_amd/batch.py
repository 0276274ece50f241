"""Batched solves of many small QPs with a shared sparsity pattern (MPC-style,
BASELINE config 4) -- ctypes plumbing over include/osqp_amd_batch.h.  One
workgroup per QP on the GPU; see osqp_amd/csrc/batch.hip."""
import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
from scipy import sparse

from . import _abi as abi
from ._lib import lib

BATCH_MAX_N = 128     # register-tiled K^-1 of the batch kernel (batch.hip)
STREAMED_MAX_N = 1024  # streamed-inverse engine (batch_streamed.h)
ENGINES = {"tiled": 0, "streamed": 1, "common": 2}   # OSQP_AMD_BATCH_TILED / _STREAMED / _COMMON
KktInfo = namedtuple("KktInfo", "builds kept npol members")     # BatchOSQP.kkt_info()
Columns = namedtuple("Columns", "started packs ended")          # BatchOSQP.columns()
SolveReport = namedtuple("SolveReport", "max_iter time_limit elapsed cut")   # BatchOSQP.solve_report()
INFO_FIELDS = ["iter", "status_val", "obj_val", "pri_res", "dua_res", "rho_updates", "rho_estimate", "rho"]
# the 16 slots of a record of BatchOSQP.verify (osqp_amd_batch_verify); the last three are verdicts
VERIFY_FIELDS = ["obj", "pri_res", "dua_res", "norm_ax", "norm_z", "norm_px", "norm_aty", "norm_q", "eps_pri", "eps_dua", "comp",
                 "dual_obj", "gap", "optimal", "prim_inf", "dual_inf"]


# the arguments of each osqp_amd_batch_<name> after (handle, members, count): f = float array, i = c_int array,
# v = device address, n = c_int
MEMBER_CALLS = {
    "update_members": "fff", "update_members_dev": "vvv",
    "warm_start_members": "ff", "warm_start_members_dev": "vv",
    "polish_members": "i",
    "adjoint_members": "n" + "f" * 7 + "ii", "adjoint_members_dev": "n" + "v" * 9,
    "tangent_members": "n" + "f" * 7 + "ii", "tangent_members_dev": "n" + "v" * 9,
    "get_members": "fffff", "get_members_dev": "vvvvv",
}
# ... and of every other osqp_amd_batch_<name>, in the same letters and h = the handle, H = a place for a handle or a
# device address, c = csc matrix, s = settings, d = c_float.  Device addresses travel as integers (c_void_p); index
# lists are host data in the _dev forms too.
_CALLS = {
    "setup": "Hnccfffffsn", "setup_engine": "Hnnccfffffsn", "setup_common": "Hnccfffsn", "cleanup": "h",
    "update": "hfff", "update_dev": "hvvv", "warm_start": "hff", "warm_start_dev": "hvv", "update_rho": "hfn",
    "update_matrices": "h" + "finn" * 2, "update_matrices_dev": "h" + "vinn" * 2,
    "update_matrices_members": "hin" + "finn" * 2, "update_matrices_members_dev": "hin" + "vinn" * 2, "update_rho_members": "hinfn",
    "common_update_model": "h" + "fin" * 2, "common_update_model_dev": "h" + "vin" * 2,
    "solve": "h", "solve_members": "hin", "solve_limited": "hinnd", "solve_report": "hf", "common_columns": "hi",
    "polish": "hi", "polish_status_dev": "hv", "kkt_info": "hi", "common_kkt": "hn", "common_kkt_peek": "hffniif",
    "adjoint": "h" + "f" * 7 + "ii", "adjoint_multi": "hn" + "f" * 7 + "ii", "tangent": "hn" + "f" * 7 + "ii",
    "adjoint_dev": "h" + "v" * 9, "adjoint_multi_dev": "hn" + "v" * 9, "tangent_dev": "hn" + "v" * 9,
    "get": "hfffff", "get_dev": "hvvvvv", "solved_members": "hi", "shape": "hii", "rounds": "hii",
    "member": "hnffffifffi", "device_ptrs": "hHHH", "check_dev_ptr": "hv",
    "verify": "hffffddf", "verify_dev": "hvvvvddv", "verify_members": "hinffffddf", "verify_members_dev": "hinvvvvddv",
}


def _bind(L):
    """Declares the batch entry points on the library object L, once per object (a second call does nothing)."""
    if getattr(L, "_osqp_amd_batch_bound", False):
        return
    kinds = dict(h=C.c_void_p, H=C.POINTER(C.c_void_p), v=C.c_void_p, f=abi.c_float_p, i=abi.c_int_p, n=abi.c_int,
                 d=abi.c_float, c=C.POINTER(abi.csc), s=C.POINTER(abi.OSQPSettings))
    L.osqp_set_default_settings.restype = None
    L.osqp_set_default_settings.argtypes = [kinds["s"]]
    for name, args in list(_CALLS.items()) + [(name, "hin" + args) for name, args in MEMBER_CALLS.items()]:
        f = getattr(L, "osqp_amd_batch_" + name)
        f.restype = None if name == "cleanup" else abi.c_int
        f.argtypes = [kinds[k] for k in args]
    L._osqp_amd_batch_bound = True


def _p(a):
    return C.cast(None, abi.c_float_p) if a is None else abi.fptr(a)


def _ip(a):
    return C.cast(None, abi.c_int_p) if a is None else abi.iptr(a)


def _shape(a):
    return tuple(a.__cuda_array_interface__["shape"])


def _outputs(R, D, **cols):
    """The float outputs of a derivative call, zeroed: name -> [R, D, max(k, 1)], or None where k is None (not asked for)."""
    return {name: None if k is None else np.zeros((R, D, max(k, 1))) for name, k in cols.items()}


def _trim(a, k, flat):
    """An output of _outputs as the caller gets it: its k columns, [R, k] for the flat form of the call."""
    return None if a is None else (a[:, 0, :k] if flat else a[:, :, :k])


def _info_columns(out, info):
    for k, name in enumerate(INFO_FIELDS):
        col = info[:, k]
        setattr(out, name, col.astype(np.int64) if name in ("iter", "status_val", "rho_updates") else col)
    return out


def _checked(a):
    """(a, its shape): a host array as contiguous float64, a device array as it is (device_view checks type and strides)."""
    if is_device(a):
        return a, _shape(a)
    a = abi.as_f64(a)
    return a, a.shape


def is_device(a):
    """True for an object that says where it lives in HBM (`__cuda_array_interface__`: a torch CUDA tensor that needs no
    gradient, a cupy array, an object of the caller's own)."""
    return hasattr(a, "__cuda_array_interface__")


def check_matrix_update(B, nnzP, nnzA, Px=None, Px_idx=None, Ax=None, Ax_idx=None):
    """Shape and index checks of BatchOSQP.update_matrices, as interface.py: update makes them for one QP (the C
    entry point reads what the shapes promise).  A 1-D value array is shared by the batch, a 2-D one is [B, k];
    without an index list k is the matrix's nnz, with one it is the list's length.  B is the row count of the call: the
    batch, or the number of listed members of a members= call (compact [count, k]).  Returns the arrays as the C
    side takes them: (Px, Px_idx, P per-member flag, Ax, Ax_idx, A per-member flag)."""
    out = []
    for name, V, I, nnz in (("P", Px, Px_idx, nnzP), ("A", Ax, Ax_idx, nnzA)):
        if V is None:
            if I is not None:
                raise ValueError("%sx_idx given without %sx" % (name, name))
            out += [None, None, 0]
            continue
        V, shape = _checked(V)
        if len(shape) not in (1, 2):
            raise ValueError("%sx must be [k] (shared) or [B, k] (per member)" % name)
        if len(shape) == 2 and shape[0] != B:
            raise ValueError("%sx has %d rows, the batch has %d members" % (name, shape[0], B))
        k = shape[-1]
        if I is None:
            if k != nnz:
                raise ValueError("%sx has %d values per member, %s has %d non-zeros (pass %sx_idx for a partial update)"
                                 % (name, k, name, nnz, name))
        else:
            I = abi.as_i64(I)
            if I.ndim != 1 or I.size != k:
                raise ValueError("%sx_idx must be a vector as long as a member's %sx" % (name, name))
            if I.size and (I.min() < 0 or I.max() >= nnz):
                raise ValueError("%sx_idx out of range [0, %d)" % (name, nnz))
        out += [V, I, int(len(shape) == 2)]
    return tuple(out)


def check_members(B, members):
    """The list checks of BatchOSQP.solve(members=...), as the C entry point makes them: an integer sequence, strictly
    ascending, every index in [0, B), at least one; or a boolean mask of length B with at least one member set.
    Returns the indices as the C side takes them."""
    a = np.asarray(members)
    if a.dtype == np.bool_:
        if a.shape != (B,):
            raise ValueError("a members mask must have length B = %d, not shape %s" % (B, a.shape))
        a = np.flatnonzero(a)
    elif a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("members must be an ascending integer sequence or a boolean mask of length B = %d" % B)
    if a.size < 1:
        raise ValueError("members is empty: a solve needs at least one member")
    if a.size > B:
        raise ValueError("members lists %d indices, the batch has %d members" % (a.size, B))
    if a.min() < 0 or a.max() >= B:
        raise ValueError("members out of range [0, %d)" % B)
    if np.any(np.diff(a) <= 0):
        raise ValueError("members must be strictly ascending (sorted, no duplicates)")
    return abi.as_i64(a)


def device_view(a, shape, typestr, writable=False, name="array"):
    """The device pointer of `a`, an object with `__cuda_array_interface__`, once it is what the C side will read or
    write: `shape` exactly, `typestr` ("<f8", or "<i4" for the integer outputs), C-contiguous (`strides` None or the
    contiguous ones) and, for an output (writable=True), not read-only."""
    cai = getattr(a, "__cuda_array_interface__", None)
    if cai is None:
        raise ValueError("%s is not a device array (no __cuda_array_interface__)" % name)
    shape = tuple(int(d) for d in shape)
    if tuple(cai["shape"]) != shape:
        raise ValueError("%s has shape %s, the handle needs %s" % (name, tuple(cai["shape"]), shape))
    if cai["typestr"] != typestr:
        raise ValueError("%s has type %s, the handle needs %s" % (name, cai["typestr"], typestr))
    strides = cai.get("strides")
    if strides is not None:
        want, step = [], int(typestr[2:])
        for d in reversed(shape):
            want.insert(0, step)
            step *= max(d, 1)
        if any(d > 1 and s != w for d, s, w in zip(shape, strides, want)):
            raise ValueError("%s must be C-contiguous (strides %s, not %s)" % (name, tuple(want), tuple(strides)))
    ptr, readonly = cai["data"]
    if writable and readonly:
        raise ValueError("%s is read-only and the handle writes it" % name)
    return int(ptr or 0)


def io_route(**arrays):
    """"device" when every given (non-None) array is a device object, "host" when none is; a mix raises."""
    given = {k: is_device(a) for k, a in arrays.items() if a is not None}
    if given and all(given.values()):
        return "device"
    if any(given.values()):
        raise ValueError("host and device arrays in one call (%s on the device, %s on the host): pass all of them one way"
                         % (", ".join(k for k, d in given.items() if d), ", ".join(k for k, d in given.items() if not d)))
    return "host"


def check_adjoint(B, n, m, dX, dY=None):
    """Shape checks of BatchOSQP.adjoint, as update makes them: dX [B, n], dY [B, m] or None.  Returns the arrays as
    the C side takes them."""
    dX = abi.as_f64(dX)
    dY = None if dY is None else abi.as_f64(dY)
    if dX.shape != (B, n) or (dY is not None and dY.shape != (B, m)):
        raise ValueError("adjoint arrays must be dX [B, n], dY [B, m]")
    return dX, dY


def check_adjoint_multi(B, n, m, dX, dY=None, **outputs):
    """Shape checks of the [B, D, .] form of BatchOSQP.adjoint / adjoint_into: dX [B, D, n], dY [B, D, m] or None, D >= 1
    cotangents per member that share one KKT inversion; both agree on D, and D <= 65535.  outputs: dq / dl / du / dPx /
    dAx of adjoint_into as (array, k) pairs, checked the same way with their own k.  Host arrays come back as contiguous
    float64, device arrays as they are (device_view checks type and strides).  Returns (dX, dY, D)."""
    given = dict(dX=(dX, n), dY=(dY, m), **outputs)
    out, Ds = {}, {}
    for name, (a, k) in given.items():
        if a is None:
            out[name] = None
            continue
        a, shape = _checked(a)
        if len(shape) != 3 or shape[0] != B or shape[2] != k or shape[1] < 1:
            raise ValueError("%s must be [B, D, %d] with B = %d and D >= 1, not %s" % (name, k, B, shape))
        Ds[name] = shape[1]
        out[name] = a
    if out["dX"] is None:
        raise ValueError("adjoint arrays must be dX [B, D, n], dY [B, D, m]")
    if len(set(Ds.values())) > 1:
        raise ValueError("adjoint arrays must agree on D: %s" % ", ".join("%s D = %d" % kv for kv in Ds.items()))
    D = int(Ds["dX"])
    if D > 65535:
        raise ValueError("at most 65535 cotangents per call, not %d" % D)
    return out["dX"], out["dY"], D


def check_tangent(B, n, m, nnzP, nnzA, dQ=None, dL=None, dU=None, dPx=None, dAx=None, **outputs):
    """Shape checks of BatchOSQP.tangent / tangent_into, as check_adjoint: every given array is [B, k] (one direction
    per member) or [B, D, k] (D directions), k = n for dQ, m for dL and dU, nnzP for dPx, nnzA for dAx; all given
    arrays agree on the form and on D.  outputs: dx / dy of tangent_into, checked the same way with k = n / m.  Host
    arrays come back as contiguous float64, device arrays as they are (device_view checks type and strides).  Returns
    (dQ, dL, dU, dPx, dAx, D, flat): flat is True for the [B, k] form (D = 1), and when nothing is given."""
    cols = dict(dQ=n, dL=m, dU=m, dPx=nnzP, dAx=nnzA, dx=n, dy=m)
    given = dict(dQ=dQ, dL=dL, dU=dU, dPx=dPx, dAx=dAx, **outputs)
    out, forms = {}, {}
    for name, a in given.items():
        if name not in cols:
            raise ValueError("unknown tangent array %r" % name)
        if a is None:
            out[name] = None
            continue
        a, shape = _checked(a)
        if len(shape) not in (2, 3) or shape[0] != B or shape[-1] != cols[name] or (len(shape) == 3 and shape[1] < 1):
            raise ValueError("%s must be [B, %d] or [B, D, %d] with B = %d, not %s" % (name, cols[name], cols[name], B, shape))
        forms[name] = None if len(shape) == 2 else shape[1]
        out[name] = a
    if len(set(forms.values())) > 1:
        raise ValueError("tangent arrays must all be [B, k] or all [B, D, k] with one D: %s"
                         % ", ".join("%s %s" % (k, "[B, k]" if d is None else "D = %d" % d) for k, d in forms.items()))
    D = next(iter(forms.values()), None)
    if D is not None and D > 65535:
        raise ValueError("at most 65535 directions per call, not %d" % D)
    return tuple(out[k] for k in ("dQ", "dL", "dU", "dPx", "dAx")) + (1 if D is None else int(D), D is None)


_BAD_POINTER = (": a pointer is not device memory of the handle's device as the library's HIP runtime knows it (a host "
                "array, another device, or an allocation of a second HIP runtime in this process: import torch before the "
                "library is first loaded)")


class BatchOSQP:
    def __init__(self):
        self._lib = lib()
        _bind(self._lib)
        self._h = None
        self._status_polish = None

    def setup(self, P, A, Q, L, U, Px_all=None, Ax_all=None, device=None, engine="auto", shared_kkt=False, **settings):
        """P (n x n, any triangle content; upper triangle is used), A (m x n): shared
        pattern/values.  Q [B, n], L, U [B, m].  Px_all / Ax_all [B, nnz] optional
        per-QP values in CSC order of triu(P) / A.  engine: "auto" (the register-tiled kernel for
        n <= 128, one single-QP engine per member above) or "streamed" (the streamed-inverse batch
        engine, K^-1 in HBM, any n <= 1024) or "common" (the common-K engine: one model, many right-hand sides --
        the members share P, A, one scaling, one class per row and one rho, so one K^-1 serves the batch and an ADMM
        iteration is one GEMM; no Px_all / Ax_all, n <= 1024; see include/osqp_amd_batch.h).  shared_kkt=True
        (engine="common" only): build the shared KKT pieces after setup (shared_kkt()), so that polish, adjoint and
        tangent are served on the handle."""
        from . import engine_options
        if engine not in ("auto", "streamed", "common"):
            raise ValueError("engine must be 'auto', 'streamed' or 'common', not %r" % (engine,))
        if engine == "common" and (Px_all is not None or Ax_all is not None):
            raise ValueError("engine='common' shares P and A over the batch: it takes no Px_all / Ax_all")
        if shared_kkt and engine != "common":
            raise ValueError("shared_kkt=True is an option of engine='common': the other engines serve polish, adjoint and "
                             "tangent as they are")
        self.engine = engine
        self._shared_kkt = False
        # neither path may hand back an unpolished or unclocked answer to a caller who asked for one: polish is a call
        # on a solved handle and a time limit an argument of solve(), so both paths refuse the settings
        # (OSQP_SETTINGS_VALIDATION_ERROR = 2)
        for k in ("polish", "time_limit"):
            if settings.get(k, 0) and settings[k] > 0:
                raise ValueError("osqp_amd_batch_setup failed with error 2: %s is not implemented by the batched engine" % k)
        self.Pu = abi.CscHolder(sparse.triu(P, format="csc"))
        self.Ah = abi.CscHolder(A)
        Q = abi.as_f64(Q)
        self.B, self.n = Q.shape
        self.m = self.Ah.m
        L = np.maximum(abi.as_f64(L), -abi.OSQP_INFTY)
        U = np.minimum(abi.as_f64(U), abi.OSQP_INFTY)
        if L.shape != (self.B, self.m) or U.shape != (self.B, self.m) or self.Pu.n != self.n or self.Ah.n != self.n:
            raise ValueError("dimension mismatch: Q [B, n], L, U [B, m], P n x n, A m x n")
        if np.any(L > U):
            raise ValueError("lower bound greater than upper bound")          # validate_data, src/auxil.c:868-875
        for nm, V, nnz in (("Px_all", Px_all, self.Pu.nnz), ("Ax_all", Ax_all, self.Ah.nnz)):
            if V is not None and np.shape(V) != (self.B, nnz):
                raise ValueError("%s must be [B, %d]" % (nm, nnz))
        st = abi.OSQPSettings()
        self._lib.osqp_set_default_settings(C.byref(st))
        st.verbose = 0
        for k, v in settings.items():
            if k not in abi.SETTING_NAMES:
                raise ValueError("unknown setting %r" % k)
            setattr(st, k, v)
        if Px_all is not None:
            Px_all = abi.as_f64(Px_all)
        if Ax_all is not None:
            Ax_all = abi.as_f64(Ax_all)
        if device is None:
            device = engine_options()["device"]
        self._many = None
        if engine == "auto" and self.n > BATCH_MAX_N:
            # The one-workgroup-per-QP kernel keeps K^-1 in registers (n <= 128).  Larger members of a batch go
            # one QP per HIP stream through the single-QP engine (osqp_amd/multi.py): same results, the PCG path.
            from .multi import PerMemberBatch
            self._many = PerMemberBatch(P, A, Q, L, U, Px_all, Ax_all, device, settings)
            return self
        h = C.c_void_p()
        call = "osqp_amd_batch_setup" + dict(auto="", streamed="_engine", common="_common")[engine]
        rc = getattr(self._lib, call)(
            C.byref(h), *((ENGINES["streamed"],) if engine == "streamed" else ()), self.B, C.byref(self.Pu.struct),
            C.byref(self.Ah.struct), *(() if engine == "common" else (_p(Px_all), _p(Ax_all))), abi.fptr(Q),
            _p(L if self.m else None), _p(U if self.m else None), C.byref(st), device)
        if rc:
            raise ValueError("%s failed with error %d%s" % (call, rc, ": a row has different classes (loose / inequality / "
                                                            "equality) in two members" if engine == "common" and rc == 1 else ""))
        self._h = h
        if shared_kkt:
            try:
                self.shared_kkt(True)
            except RuntimeError as e:
                self.cleanup()
                raise ValueError(str(e)) from None
        return self

    def _unserved(self, call, never=False):
        """The calls the common-K engine does not serve (the C side refuses them too, with the same words): every one of
        them without the shared KKT pieces (shared_kkt), update_matrices (never=True) with them too."""
        if getattr(self, "engine", None) == "common" and (never or not getattr(self, "_shared_kkt", False)):
            raise RuntimeError("%s is not served by the common-K engine (engine=\"common\")%s; set the batch up with "
                               "engine=\"auto\" or engine=\"streamed\""
                               % (call, " (use update_model for new values of the shared model)" if never else
                                  " without its shared KKT pieces (shared_kkt=True)"))

    def _kernel_batch(self, call, option=None, why=None):
        """Refuses what the one-engine-per-member route (osqp_amd/multi.py, `_many`) does not serve -- it keeps no packed
        batch on the device -- in one of its three sentences: `why` (what the caller meets instead; True: `call` is a
        call of the batch engines), `call(option=...)`, or `call` alone."""
        if self._many is None:
            return
        if why is not None:
            raise RuntimeError("this batch runs one single-QP engine per member (n > %d): %s" % (BATCH_MAX_N, (
                "%s is a call of the batch engines; set the batch up with engine=\"streamed\"" % call) if why is True else why))
        if option is not None:
            raise RuntimeError("%s(%s=...) is not served by the one-engine-per-member route (engine=\"auto\", n > %d); "
                               "set the batch up with engine=\"streamed\" or engine=\"common\"" % (call, option, BATCH_MAX_N))
        raise RuntimeError("%s is not served by the one-engine-per-member route (engine=\"auto\", n > %d)" % (call, BATCH_MAX_N))

    def shared_kkt(self, on=True):
        """The shared KKT pieces of a common-K handle (osqp_amd_batch_common_kkt): on=True builds H = (P~ + delta I)^-1 and
        Wt = A~ H once (a second call does nothing), and polish, adjoint, tangent, kkt_info, adjoint_into, tangent_into
        and results_into(status_polish=) are served from then on; on=False frees them and the calls are refused again.
        Raises RuntimeError with the C return code (4: not a common-K handle, 5: a pivot of P + delta I is not positive,
        6: out of memory)."""
        if getattr(self, "_many", None) is not None or self._h is None:
            raise RuntimeError("shared_kkt is a call of a live common-K handle (engine=\"common\")")
        rc = int(self._lib.osqp_amd_batch_common_kkt(self._h, 1 if on else 0))
        if rc:
            raise RuntimeError("osqp_amd_batch_common_kkt failed (%d)" % rc)
        self._shared_kkt = bool(on)

    def shared_kkt_peek(self, qp=None):
        """Test hook: H [NP, NP] and Wt [m, NP] of a handle with the shared pieces and, with qp given, mred, NS and Sinv
        [NS, NS] of member qp in the inversion currently kept (kkt_info().kept)."""
        NP = self.shape()[1]
        H = np.zeros((NP, NP)); Wt = np.zeros((max(self.m, 1), NP))
        no_i, no_f = C.cast(None, abi.c_int_p), C.cast(None, abi.c_float_p)
        rc = self._lib.osqp_amd_batch_common_kkt_peek(self._h, abi.fptr(H), abi.fptr(Wt), 0, no_i, no_i, no_f)
        if rc:
            raise RuntimeError("osqp_amd_batch_common_kkt_peek failed (%d)" % rc)
        out = dict(H=H, Wt=Wt[:self.m], NP=NP)
        if qp is not None:
            mred = np.zeros(1, np.int64); NS = np.zeros(1, np.int64)
            rc = self._lib.osqp_amd_batch_common_kkt_peek(self._h, no_f, no_f, int(qp), abi.iptr(mred), abi.iptr(NS), no_f)
            if rc:
                raise RuntimeError("osqp_amd_batch_common_kkt_peek failed (%d)" % rc)
            S = np.zeros((int(NS[0]), int(NS[0])))
            rc = self._lib.osqp_amd_batch_common_kkt_peek(self._h, no_f, no_f, int(qp), no_i, no_i, abi.fptr(S))
            if rc:
                raise RuntimeError("osqp_amd_batch_common_kkt_peek failed (%d)" % rc)
            out.update(mred=int(mred[0]), NS=int(NS[0]), Sinv=S)
        return out

    def shape(self):
        """(engine, NP) of a kernel batch: engine 0 = tiled, 1 = streamed, 2 = common-K; K^-1 is NP x NP (padded)."""
        e = np.zeros(1, np.int64); npo = np.zeros(1, np.int64)
        if self._lib.osqp_amd_batch_shape(self._h, abi.iptr(e), abi.iptr(npo)):
            raise RuntimeError("osqp_amd_batch_shape failed")
        return int(e[0]), int(npo[0])

    def rounds(self):
        """Of the last solve: (launches of the ADMM loop, members whose K^-1 solve is refined)."""
        r = np.zeros(1, np.int64); f = np.zeros(1, np.int64)
        if self._lib.osqp_amd_batch_rounds(self._h, abi.iptr(r), abi.iptr(f)):
            raise RuntimeError("osqp_amd_batch_rounds failed")
        return int(r[0]), int(f[0])

    @property
    def last_update_failed(self):
        """One-engine-per-member route: the member whose non-zero code the last update, update_matrices, update_rho or
        warm_start returned (None: every member took the call)."""
        return self._many.last_update_failed

    def _route(self, **arrays):
        route = io_route(**arrays)
        if route == "device":
            self._kernel_batch(None, why="it takes and returns host arrays; there is no packed device image to read or write")
        return route

    def _dev(self, a, cols, name, typestr="<f8", writable=False, rows=None):
        """Device pointer of a [B, cols] array -- [rows, cols] in a members= call -- (None, or nothing to read: NULL)."""
        if a is None:
            return None
        return device_view(a, (self.B if rows is None else rows, cols), typestr, writable, name) or None

    def _members(self, members, call):
        """The list of a members= call as the C side takes it (check_members), once the handle can serve one: the
        one-engine-per-member route keeps no packed batch to address by member."""
        self._kernel_batch(call, option="members")
        return check_members(self.B, members)

    def solved_members(self):
        """Boolean [B]: True where the member's results are those of a solve of the problem the handle holds now -- what
        polish, adjoint and tangent with members= require of the members they list.  Touches no GPU memory."""
        self._kernel_batch("solved_members")
        out = np.zeros(self.B, np.int64)
        rc = self._lib.osqp_amd_batch_solved_members(self._h, abi.iptr(out))
        if rc:
            raise RuntimeError("osqp_amd_batch_solved_members failed (%d)" % rc)
        return out != 0

    def _entry(self, name, mem=None, dev=False):
        """The C entry of a call in the form asked for -- osqp_amd_batch_<name>[_members][_dev] -- as (its name, the
        function, the arguments that follow the handle: the list and its length for a members= call)."""
        call = "osqp_amd_batch_%s%s%s" % (name, "" if mem is None else "_members", "_dev" if dev else "")
        return call, getattr(self._lib, call), () if mem is None else (abi.iptr(mem), int(mem.size))

    def _given(self, dev, mem, want, *arrays):
        """The given arrays of update / warm_start, each (a, k, name, view), are [R, k] -- R = B, or the number of listed
        members --, or ValueError(want).  Returns them as the C side takes them: contiguous float64 on the host route,
        device pointers on the device route (None where view is False: an array the call does not read)."""
        R = self.B if mem is None else int(mem.size)
        if dev:
            if mem is not None and any(a is not None and _shape(a) != (R, k) for a, k, _, _ in arrays):
                raise ValueError(want)               # (the whole-batch form leaves the shape to device_view's own words)
            return [self._dev(a, k, name, rows=R) if view else None for a, k, name, view in arrays]
        out = [None if a is None else abi.as_f64(a) for a, _, _, _ in arrays]
        if any(a is not None and a.shape != (R, k) for a, (_, k, _, _) in zip(out, arrays)):
            raise ValueError(want)
        return out

    def update(self, Q=None, L=None, U=None, members=None):
        """osqp_update_lin_cost / _bounds for every QP (None = keep).  Host arrays, or device arrays (objects with
        `__cuda_array_interface__`, complete when the call is made): those are clamped, checked and scaled on the device.
        members= (an ascending index list or a boolean mask of length B): for the listed members only, with compact
        arrays Q [count, n], L, U [count, m], row k for the k-th listed member; the others keep their data, their results
        and their solved flag (solved_members).  engine="common": returns 1, with nothing changed, when a listed member's
        new bounds would give a row another class than the batch holds for it."""
        mem = None if members is None else self._members(members, "update")
        n, m = self.n, self.m
        want = "update arrays must be Q [B, n], L [B, m], U [B, m]" if mem is None else \
               "update arrays with members= must be compact: Q [%d, %d], L [%d, %d], U [%d, %d] for the %d listed members" \
               % (mem.size, n, mem.size, m, mem.size, m, mem.size)
        dev = self._route(Q=Q, L=L, U=U) == "device"
        Q, L, U = self._given(dev, mem, want, (Q, n, "Q", True), (L, m, "L", True), (U, m, "U", True))
        if not dev:
            L = None if L is None else np.maximum(L, -abi.OSQP_INFTY)
            U = None if U is None else np.minimum(U, abi.OSQP_INFTY)
            if L is not None and U is not None and np.any(L > U):
                raise ValueError("lower bound greater than upper bound")
            if self._many is not None:
                return self._many.update(Q, L, U)
        _, f, lead = self._entry("update", mem, dev)
        return int(f(self._h, *lead, *((Q, L, U) if dev else (_p(Q), _p(L), _p(U)))))

    def update_matrices(self, Px=None, Px_idx=None, Ax=None, Ax_idx=None, members=None):
        """osqp_update_P / _A / _P_A for every QP: new values on the pattern of setup.  Px / Ax: [k] (shared by the
        batch) or [B, k] (per member); k = nnz of triu(P) / A in CSC order, or the length of Px_idx / Ax_idx (slots, one
        list for the batch).  Scaling is recomputed; rho, row classes and iterates stay.  Returns the C return code
        (5: some member's new K is not positive definite; solve then refuses until an update succeeds).  Px / Ax may be
        device arrays; the index lists stay host data.
        members= (an ascending index list or a boolean mask of length B): for the listed members only.  Px / Ax are [k]
        (written to every listed member) or compact [count, k], row r for the r-th listed member.  Only the listed
        members are re-equilibrated and get a new K^-1; the others keep their data, scaling, rho, K^-1, results and solved
        flag.  A handle with shared values keeps one row per member from then on.  5 is returned as long as any member
        of the batch, listed or not, has a K that is not positive definite."""
        self._unserved("update_matrices", never=True)
        mem = None if members is None else self._members(members, "update_matrices")
        dev = self._route(Px=Px, Ax=Ax) == "device"
        try:
            Px, Px_idx, pper, Ax, Ax_idx, aper = check_matrix_update(self._rows(mem), self.Pu.nnz, self.Ah.nnz, Px, Px_idx, Ax, Ax_idx)
        except ValueError as e:
            if mem is None:
                raise
            raise ValueError("with members= the values are [k] or compact [count, k] (%d listed members): %s"
                             % (mem.size, e)) from None
        if Px is None and Ax is None:
            return 0
        if self._many is not None:
            return self._many.update_matrices(Px, Px_idx, pper, Ax, Ax_idx, aper)
        (pP, iP, kP), (pA, iA, kA) = self._matrix_values(dev, Px, Px_idx, Ax, Ax_idx)
        if dev and pP is None and pA is None:
            return 0
        _, f, lead = self._entry("update_matrices", mem, dev)
        return int(f(self._h, *lead, pP, iP, kP, pper, pA, iA, kA, aper))

    @staticmethod
    def _matrix_values(dev, Px, Px_idx, Ax, Ax_idx):
        """New matrix values that check_matrix_update has passed, as update_matrices and update_model hand them to the C
        side: (values, index list, values per member) of P and of A -- host pointers or, on the device route, device
        addresses (a pointer of 0: nothing to write; NULL = keep says the same); the index lists are host data."""
        out = []
        for name, V, I in (("Px", Px, Px_idx), ("Ax", Ax, Ax_idx)):
            if dev:
                out.append((None if V is None else device_view(V, _shape(V), "<f8", name=name) or None, _ip(I),
                            0 if V is None else _shape(V)[-1]))
            else:
                out.append((_p(V), _ip(I), 0 if V is None else V.shape[-1]))
        return out

    def update_model(self, Px=None, Px_idx=None, Ax=None, Ax_idx=None):
        """New values for the shared model of a common-K handle (osqp_amd_batch_common_update_model): osqp_update_P / _A /
        _P_A applied to the one model.  Px / Ax: [k] -- k = nnz of triu(P) / A in CSC order, or the length of Px_idx /
        Ax_idx (slots) -- host arrays or device arrays; the index lists stay host data.  The common scaling is recomputed
        (q^ over the Q the handle holds now), every member's q, l, u are rescaled, the one K^-1 and, where the handle has
        them, the shared KKT pieces are rebuilt inside the call; rho, the row classes and the iterates stay, rho_updates
        restarts.  Returns the C return code (5: the new K is not positive definite and solve refuses until a call
        succeeds -- or, on a handle with the shared pieces whose K is fine, P + delta I is not: the pieces are freed and
        polish, adjoint and tangent are refused again)."""
        if getattr(self, "engine", None) != "common" or self._h is None:
            raise RuntimeError("update_model is a call of the common-K engine (engine=\"common\"); the other engines take new "
                               "matrix values through update_matrices")
        for name, V in (("Px", Px), ("Ax", Ax)):
            if V is not None and len(V.__cuda_array_interface__["shape"] if is_device(V) else np.shape(V)) != 1:
                raise ValueError("engine='common' shares P and A over the batch: update_model takes %s as one [k] array, not "
                                 "[B, k]" % name)
        dev = self._route(Px=Px, Ax=Ax) == "device"
        Px, Px_idx, _, Ax, Ax_idx, _ = check_matrix_update(self.B, self.Pu.nnz, self.Ah.nnz, Px, Px_idx, Ax, Ax_idx)
        f = self._lib.osqp_amd_batch_common_update_model_dev if dev else self._lib.osqp_amd_batch_common_update_model
        rc = int(f(self._h, *(v for of in self._matrix_values(dev, Px, Px_idx, Ax, Ax_idx) for v in of)))
        if rc == 5 and self._shared_kkt:                 # did the shared pieces go?  (NULL outputs: nothing is copied)
            no_i, no_f = C.cast(None, abi.c_int_p), C.cast(None, abi.c_float_p)
            self._shared_kkt = self._lib.osqp_amd_batch_common_kkt_peek(self._h, no_f, no_f, 0, no_i, no_i, no_f) == 0
        return rc

    def update_rho(self, rho, members=None):
        """osqp_update_rho for every QP: a scalar, or [B] values.  Returns 1 (nothing changed) when a value is <= 0.
        members=: for the listed members only, a scalar or [count] values; the others keep rho, K^-1, results and solved
        flag.  engine="common" has one rho for the batch: it returns 1, with nothing changed, for a list short of all B."""
        mem = None if members is None else self._members(members, "update_rho")
        R = self._rows(mem)
        rho = np.asarray(rho, dtype=np.float64)
        if rho.shape not in ((), (R,)):
            raise ValueError("rho must be a scalar or [B]" if mem is None else
                             "rho with members= must be a scalar or [%d], one value per listed member" % R)
        per = int(rho.ndim == 1)
        if per and getattr(self, "engine", None) == "common":
            raise ValueError("engine='common' has one rho for the batch: update_rho takes a scalar")
        rho = np.ascontiguousarray(rho.reshape(-1))
        if self._many is not None:
            return self._many.update_rho(rho, per)
        _, f, lead = self._entry("update_rho", mem)
        return int(f(self._h, *lead, abi.fptr(rho), per))

    def warm_start(self, X=None, Y=None, members=None):
        """osqp_warm_start (_x, _y) for every QP: X [B, n], Y [B, m], unscaled; turns the warm_start setting on.  Host
        arrays or device arrays.  members=: for the listed members only, X [count, n], Y [count, m]; the others keep their
        iterates and their solved flag."""
        mem = None if members is None else self._members(members, "warm_start")
        n, m = self.n, self.m
        want = "warm start arrays must be X [B, n], Y [B, m]" if mem is None else \
               "warm start arrays with members= must be compact: X [%d, %d], Y [%d, %d] for the %d listed members" \
               % (mem.size, n, mem.size, m, mem.size)
        dev = self._route(X=X, Y=Y) == "device"
        X, Y = self._given(dev, mem, want, (X, n, "X", True), (Y, m, "Y", bool(m)))
        if not dev and self._many is not None:
            return self._many.warm_start(X, Y)
        _, f, lead = self._entry("warm_start", mem, dev)
        return int(f(self._h, *lead, *((X, Y) if dev else (_p(X), _p(Y if m else None)))))

    def solve(self, fetch=True, members=None, max_iter=None, time_limit=None):
        """osqp_solve for every member, or (engine="common" only) for the listed ones: members is a strictly ascending
        integer sequence or a boolean mask of length B.  Only the listed members are loaded, iterated and stored; of the
        others nothing changes, and results() returns them as they were.  polish, adjoint and tangent are served once every
        member has been solved on the current problem, by one call or by several.
        max_iter (an integer >= 1) and time_limit (seconds, > 0) hold for this call only (osqp_amd_batch_solve_limited):
        the call ends as a handle set up with that max_iter would, to the bit; a member the clock stops ends with status
        -6 (OSQP_TIME_LIMIT_REACHED), or 2 where the approximate test passes, and keeps its last iterate.  The clock is
        looked at only where termination is checked (every 25th iteration with check_termination=0); solve_report()
        tells what the call ran with."""
        limited = max_iter is not None or time_limit is not None
        if max_iter is not None:
            if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
                raise ValueError("max_iter must be an integer >= 1, not %r" % (max_iter,))
        if time_limit is not None:
            if isinstance(time_limit, bool) or not isinstance(time_limit, (int, float, np.integer, np.floating)) \
                    or not np.isfinite(time_limit) or time_limit <= 0:
                raise ValueError("time_limit must be a finite number of seconds > 0, not %r" % (time_limit,))
        if limited:
            self._kernel_batch("solve", option="max_iter" if max_iter is not None else "time_limit")
        mem = None
        if members is not None:
            if getattr(self, "engine", None) != "common" or self._many is not None or self._h is None:
                raise RuntimeError("solve(members=...) is not served by the %s; it is a call of the common-K engine "
                                   "(engine=\"common\")" % ("one-engine-per-member path (n > %d)" % BATCH_MAX_N
                                                            if self._many is not None else "tiled or the streamed engine"))
            mem = check_members(self.B, members)
        elif self._many is not None:
            self._many.solve()
            return self.results() if fetch else None
        self._status_polish = None
        if limited:
            call = "osqp_amd_batch_solve_limited"
            rc = self._lib.osqp_amd_batch_solve_limited(self._h, _ip(mem), 0 if mem is None else mem.size, int(max_iter or 0),
                                                        float(time_limit or 0.0))
        elif mem is not None:
            call = "osqp_amd_batch_solve_members"
            rc = self._lib.osqp_amd_batch_solve_members(self._h, abi.iptr(mem), mem.size)
        else:
            call = "osqp_amd_batch_solve"
            rc = self._lib.osqp_amd_batch_solve(self._h)
        if rc:
            raise RuntimeError("%s failed (%d)" % (call, rc))
        return self.results() if fetch else None

    def solve_report(self):
        """Of the last solve by any call: (max_iter, time_limit, elapsed, cut) -- the iteration cap and the time limit in
        force (0: none), the seconds between the two device stamps of a solve with a time limit (0 without one) and the
        members the clock stopped.  Touches no GPU memory."""
        self._kernel_batch("solve_report")
        out = np.zeros(4)
        rc = self._lib.osqp_amd_batch_solve_report(self._h, abi.fptr(out))
        if rc:
            raise RuntimeError("osqp_amd_batch_solve_report failed (%d)" % rc)
        return SolveReport(int(out[0]), float(out[1]), float(out[2]), int(out[3]))

    def columns(self):
        """Of the last solve of a common-K handle: (started, packs, ended) -- the columns it started with (B, or the
        number of listed members), how often it packed the running columns to the front, and the columns in use when it
        ended.  Touches no GPU memory."""
        if getattr(self, "engine", None) != "common" or self._h is None:
            raise RuntimeError("columns is a call of the common-K engine (engine=\"common\")")
        out = np.zeros(3, np.int64)
        rc = self._lib.osqp_amd_batch_common_columns(self._h, abi.iptr(out))
        if rc:
            raise RuntimeError("osqp_amd_batch_common_columns failed (%d)" % rc)
        return Columns(*(int(v) for v in out))

    def polish(self, fetch=True, members=None):
        """Polish (src/polish.c) on the device for every member whose last solve ended `solved`, with the handle's
        `delta` and `polish_refine_iter`.  Returns results() -- x, y, obj_val, pri_res, dua_res of the accepted
        members are the polished ones -- with `status_polish` [B]: 1 accepted, -1 tried and rejected (nothing of
        that member changed), 0 not tried.  Needs a solve since setup or the last update.  fetch=False: nothing is
        copied to the host and None is returned (results_into reads the outcome on the device; a later results() fetches
        the status then).
        members=: polish for the listed members only, each of which must be solved on the current problem
        (solved_members); the work is done once per member and solve.  Returns results(members=) -- compact rows -- with
        `status_polish` [count]."""
        self._unserved("polish")
        mem = None if members is None else self._members(members, "polish")
        self._kernel_batch("polish", why=True)
        sp = np.zeros(self._rows(mem), np.int64) if fetch else None
        call, f, lead = self._entry("polish", mem)
        rc = f(self._h, *lead, _ip(sp))
        if rc:
            raise RuntimeError("%s failed (%d)%s" % (call, rc, self._unsolved(mem) if rc == 7 else ""))
        if mem is None:
            self._status_polish = sp if fetch else "device"       # results() reads it when it is first asked for
        if not fetch:
            return None
        out = self.results(members=mem)
        if mem is not None:
            out.status_polish = sp
        return out

    def adjoint(self, dX, dY=None, matrices=False, members=None):
        """Adjoint derivatives of the solution on the device, for every member whose last solve ended `solved`: from
        dX = dl/dx [B, n] and dY = dl/dy [B, m] (None = 0) of a scalar l, a namespace with dq [B, n], dl, du [B, m],
        dPx [B, nnzP] and dAx [B, nnzA] (CSC order of triu(P) / A; None unless matrices=True; an off-diagonal dPx slot
        stands for both halves of P), active [B, m] (-1 active at the lower bound, +1 at the upper, 0 inactive) and
        status_adjoint [B]: 1 computed, -1 a KKT pivot of the wrong sign, 0 not tried (the member did not end
        `solved`); the gradients of members that are not 1 are 0.  The point differentiated is the one the handle
        holds: the polished one where polish() was accepted, the ADMM iterate otherwise.  Changes nothing in the
        handle.  Needs a solve since setup or the last update.
        dX [B, D, n] with dY [B, D, m] (or None): D cotangents per member in one call, on one KKT inversion; the five
        gradients come back [B, D, .], active and status_adjoint per member -- D rows of the Jacobian; slice d carries
        the bits adjoint(dX[:, d], dY[:, d]) returns.
        On one solve, adjoint() and tangent() share the KKT inversion the first of them builds (kkt_info).
        members=: for the listed members only, each solved on the current problem; every array is compact, [count, .] or
        [count, D, .], and the KKT inversion is built for the listed members alone (and shared by later members= calls
        with the same list)."""
        self._unserved("adjoint")
        return self._adjoint("adjoint", False, members, dX, dY, matrices=matrices)

    def _adjoint(self, call, dev, members, dX, dY, into=None, active=None, status=None, matrices=False):
        """The one body of adjoint (dev=False: host arrays in, a namespace of new host arrays out) and adjoint_into
        (dev=True: between the caller's device arrays, `into` = dict(dq, dl, du, dPx, dAx), active, status): the list of a
        members= call, the shape checks with the rows of the call, [R, n] or [R, D, n], and the entry that serves the form."""
        mem = None if members is None else self._members(members, call)
        self._kernel_batch(call, why=True)
        R, n, m = self._rows(mem), self.n, self.m
        cols = dict(dq=n, dl=m, du=m, dPx=self.Pu.nnz, dAx=self.Ah.nnz)
        # whole batch: [B, n] takes the single-cotangent entry point, [B, D, n] the _multi one
        flat, D = len(_shape(dX) if dev else np.shape(dX)) != 3, 1
        try:
            if not flat:
                dX, dY, D = check_adjoint_multi(R, n, m, dX, dY, **({k: (into[k], c) for k, c in cols.items()} if dev else {}))
            elif not dev:                            # (flat device arrays: device_view says what is wrong with which)
                dX, dY = check_adjoint(R, n, m, dX, dY)
        except ValueError as e:
            raise self._compact(e, mem) from None
        if not dev:
            into = _outputs(R, D, **{k: c if matrices or k not in ("dPx", "dAx") else None for k, c in cols.items()})
            active, status = np.zeros((R, max(m, 1)), np.int64), np.zeros(R, np.int64)
        self._sens("adjoint", "adjoint" if flat or mem is not None else "adjoint_multi", dev, mem, flat, D,
                   () if flat and mem is None else (D,),
                   [(dX, n, "dX", False), (dY if dev or m else None, m, "dY", False)] + [(into[k], c, k, True) for k, c in cols.items()],
                   active, status)
        if not dev:
            return SimpleNamespace(**{k: _trim(into[k], c, flat) for k, c in cols.items()}, active=active[:, :m],
                                   status_adjoint=status)

    def _sens(self, kind, entry, dev, mem, flat, D, scalars, floats, active, status):
        """The library call of the derivative bodies (kind: "adjoint" or "tangent"), marshalled and worded in one place.
        floats: the float arrays in the entry's order, each (a, cols, name, writable): host arrays go as pointers, device
        arrays as the address device_view gives once the array is [R, cols] (flat) or [R, D, cols], float64, contiguous
        and, for an output, writable; active [R, m] and status [R]: int64 on the host, int32 on the device."""
        R = self._rows(mem)
        call, f, lead = self._entry(entry, mem, dev)
        if dev:
            args = [None if a is None else device_view(a, (R, k) if flat else (R, D, k), "<f8", w, name) or None
                    for a, k, name, w in floats]
            args += [self._dev(active, self.m, "active", "<i4", True, rows=R),
                     None if status is None else device_view(status, (R,), "<i4", True, "status_" + kind)]
        else:
            args = [_p(a) for a, _, _, _ in floats] + [abi.iptr(active), abi.iptr(status)]
        rc = f(self._h, *lead, *scalars, *args)
        if rc:
            raise RuntimeError("%s failed (%d)%s" % (call, rc, self._unsolved(mem) if rc == 7 else
                                                     _BAD_POINTER if dev and rc == 1 else ""))

    def _rows(self, mem):
        """The rows of a call's per-member arrays: B, or the number of listed members."""
        return self.B if mem is None else int(mem.size)

    @staticmethod
    def _unsolved(mem):
        """What return code 7 of polish, adjoint and tangent says."""
        return ": no solve has run on the current problem" if mem is None else \
               ": a listed member has not been solved on the current problem"

    def _compact(self, e, mem):
        """The error of a shape check made with the rows of the call, worded for a members= call where it is one."""
        if mem is None:
            return e
        R = int(mem.size)
        return ValueError("with members= the arrays are compact (%d listed members): %s"
                          % (R, str(e).replace("B = %d" % R, "count = %d" % R).replace("[B,", "[count,")))

    def kkt_info(self):
        """For the tests and tools: (builds, kept, npol, members) -- passes of KKT formation and inversion over the solved
        members since setup (polish's included), whether an inversion is kept for the next adjoint() / tangent() on this
        solve, its padded order and the members in it.  Touches no GPU memory."""
        self._unserved("kkt_info")
        self._kernel_batch("kkt_info", why="there is no batch KKT buffer")
        out = np.zeros(4, np.int64)
        rc = self._lib.osqp_amd_batch_kkt_info(self._h, abi.iptr(out))
        if rc:
            raise RuntimeError("osqp_amd_batch_kkt_info failed (%d)" % rc)
        return KktInfo(*(int(v) for v in out))

    def tangent(self, dQ=None, dL=None, dU=None, dPx=None, dAx=None, members=None):
        """Forward sensitivities of the solution on the device, for every member whose last solve ended `solved`: from
        tangents of the data -- dQ [B, n], dL, dU [B, m], dPx [B, nnzP], dAx [B, nnzA] (CSC order of triu(P) / A; an
        off-diagonal dPx slot stands for both halves of P), or each of them [B, D, k] for D directions per member
        that share one KKT inversion; None = 0 -- a namespace with dx [B, n] and dy [B, m] (or [B, D, .]), active
        [B, m] and status_tangent [B]: 1 computed, -1 a KKT pivot of the wrong sign, 0 not tried; the tangents of
        members that are not 1 are 0.  Only the tangent of the bound a row is active at counts (dL = dU on an
        equality row).  The point differentiated is the one the handle holds, as for adjoint().  To first order the
        solution of the moved problem is r.x + t.dx, r.y + t.dy.  Changes nothing in the handle.  Needs a solve since
        setup or the last update.
        members=: for the listed members only, as adjoint(members=): compact arrays, [count, k] or [count, D, k]."""
        self._unserved("tangent")
        return self._tangent("tangent", False, members, (dQ, dL, dU, dPx, dAx))

    def _tangent(self, call, dev, members, given, into=None, active=None, status=None):
        """The one body of tangent and tangent_into, as _adjoint: given = (dQ, dL, dU, dPx, dAx), into = dict(dx, dy)."""
        mem = None if members is None else self._members(members, call)
        self._kernel_batch(call, why=True)
        R, n, m, nP, nA = self._rows(mem), self.n, self.m, self.Pu.nnz, self.Ah.nnz
        try:
            dQ, dL, dU, dPx, dAx, D, flat = check_tangent(R, n, m, nP, nA, *given, **(into if dev else {}))
        except ValueError as e:
            raise self._compact(e, mem) from None
        if not dev:
            into = _outputs(R, D, dx=n, dy=m)
            active, status = np.zeros((R, max(m, 1)), np.int64), np.zeros(R, np.int64)
        rows = (lambda a: a) if dev or m else (lambda a: None)      # host arrays of m = 0 columns go as NULL
        self._sens("tangent", "tangent", dev, mem, flat, D, (D,),
                   [(dQ, n, "dQ", False), (rows(dL), m, "dL", False), (rows(dU), m, "dU", False), (dPx, nP, "dPx", False),
                    (dAx, nA, "dAx", False), (into["dx"], n, "dx", True), (rows(into["dy"]), m, "dy", True)], active, status)
        if not dev:
            return SimpleNamespace(dx=_trim(into["dx"], n, flat), dy=_trim(into["dy"], m, flat), active=active[:, :m],
                                   status_tangent=status)

    def results(self, members=None):
        """The results of every member, or with members= the compact rows of the listed ones (status_polish: of the last
        whole-batch polish)."""
        mem = None if members is None else self._members(members, "results")
        if self._many is not None:
            out = self._many.results()
            return _info_columns(out, out.info_raw)
        R, n, m = self._rows(mem), self.n, self.m
        X = np.zeros((R, n)); Y = np.zeros((R, max(m, 1)))
        info = np.zeros((R, 8)); DX = np.zeros((R, n)); DY = np.zeros((R, max(m, 1)))
        self._get(False, mem, X, Y if m else None, info, DX, DY if m else None)
        out = SimpleNamespace(x=X, y=Y[:, :m], dual_inf_cert=DX, prim_inf_cert=DY[:, :m], info_raw=info)
        if mem is None and isinstance(self._status_polish, str):   # polish(fetch=False) ran: the work is done, the call reports it
            sp = np.zeros(self.B, np.int64)
            rc = self._lib.osqp_amd_batch_polish(self._h, abi.iptr(sp))
            if rc and rc != 7:
                raise RuntimeError("osqp_amd_batch_polish failed (%d)" % rc)
            self._status_polish = None if rc else sp       # (7: the problem has changed since; nothing was tried on it)
        sp = self._status_polish
        out.status_polish = np.zeros(R, np.int64) if not isinstance(sp, np.ndarray) else sp[slice(None) if mem is None else mem].copy()
        return _info_columns(out, info)

    def _get(self, dev, mem, X, Y, info, DX, DY):
        """The one body of results and results_into: X, DX [R, n], Y, DY [R, m], info [R, 8] from the handle (None = skip)."""
        arrays = ((X, self.n, "X"), (Y, self.m, "Y"), (info, 8, "info"), (DX, self.n, "DX"), (DY, self.m, "DY"))
        call, f, lead = self._entry("get", mem, dev)
        rc = f(self._h, *lead, *((self._dev(a, k, name, writable=True, rows=self._rows(mem)) if dev else _p(a)) for a, k, name in arrays))
        if rc:
            raise RuntimeError("%s failed (%d)%s" % (call, rc, _BAD_POINTER if dev and rc == 1 else ""))

    def results_into(self, X=None, Y=None, info=None, DX=None, DY=None, status_polish=None, members=None):
        """The results into device arrays of the caller's (None = skip): X, DX [B, n], Y, DY [B, m], info [B, 8]
        (INFO_FIELDS) float64, status_polish [B] int32 (1 accepted, -1 rejected, 0 not tried or no polish since the
        last solve; needs a solve on the current problem).  Device-to-device copies, ready on return; a later solve
        does not touch them.  For m = 0 the m-sized arguments may be None.
        members=: the listed members' rows into compact arrays [count, .]; exactly count rows are written.  status_polish
        is a whole-batch array and is not taken together with members=."""
        if self._route(X=X, Y=Y, info=info, DX=DX, DY=DY, status_polish=status_polish) != "device":
            raise ValueError("results_into writes device arrays (objects with __cuda_array_interface__); results() returns "
                             "host arrays")
        mem = None if members is None else self._members(members, "results_into")
        if mem is not None and status_polish is not None:
            raise ValueError("results_into(members=...) takes no status_polish: it is a [B] array of the whole-batch polish")
        self._get(True, mem, X, Y, info, DX, DY)
        if status_polish is not None:
            self._unserved("results_into(status_polish=...)")
            rc = self._lib.osqp_amd_batch_polish_status_dev(
                self._h, device_view(status_polish, (self.B,), "<i4", True, "status_polish"))
            if rc:
                raise RuntimeError("osqp_amd_batch_polish_status_dev failed (%d)%s"
                                   % (rc, self._unsolved(None) if rc == 7 else _BAD_POINTER if rc == 1 else ""))

    def adjoint_into(self, dX, dY, dq, dl, du, dPx=None, dAx=None, active=None, status_adjoint=None, members=None):
        """adjoint() between device arrays of the caller's: from dX [B, n] and dY [B, m] (None = 0) into dq [B, n], dl, du
        [B, m] and, where given, dPx [B, nnzP], dAx [B, nnzA] (float64), active [B, m], status_adjoint [B] (int32).
        For m = 0 the m-sized arguments may be None.  Ready on return.  With dX [B, D, n] every float array is [B, D, .]
        (D cotangents per member, as adjoint() takes them); active and status_adjoint stay per member."""
        self._unserved("adjoint_into")
        if self._route(dX=dX, dY=dY, dq=dq, dl=dl, du=du, dPx=dPx, dAx=dAx, active=active,
                       status_adjoint=status_adjoint) != "device":
            raise ValueError("adjoint_into reads and writes device arrays (objects with __cuda_array_interface__); adjoint() "
                             "takes and returns host arrays")
        if dX is None or dq is None or (self.m and (dl is None or du is None)):
            raise ValueError("adjoint_into needs dX, dq and, for m > 0, dl and du")
        self._adjoint("adjoint_into", True, members, dX, dY, dict(dq=dq, dl=dl, du=du, dPx=dPx, dAx=dAx), active, status_adjoint)

    def tangent_into(self, dx, dy, dQ=None, dL=None, dU=None, dPx=None, dAx=None, active=None, status_tangent=None,
                     members=None):
        """tangent() between device arrays of the caller's: from dQ, dL, dU, dPx, dAx (None = 0; [B, k], or [B, D, k] for
        D directions) into dx [B, n] and dy [B, m] (or [B, D, .], as the tangents; float64) and, where given, active
        [B, m], status_tangent [B] (int32).  For m = 0 dy may be None.  Ready on return."""
        self._unserved("tangent_into")
        if self._route(dx=dx, dy=dy, dQ=dQ, dL=dL, dU=dU, dPx=dPx, dAx=dAx, active=active,
                       status_tangent=status_tangent) != "device":
            raise ValueError("tangent_into reads and writes device arrays (objects with __cuda_array_interface__); tangent() "
                             "takes and returns host arrays")
        if dx is None or (self.m and dy is None):
            raise ValueError("tangent_into needs dx and, for m > 0, dy")
        self._tangent("tangent_into", True, members, (dQ, dL, dU, dPx, dAx), dict(dx=dx, dy=dy), active, status_tangent)

    def verify(self, X=None, Y=None, DX=None, DY=None, eps_abs=None, eps_rel=None, members=None):
        """The verdict on a point against the raw problem the handle holds now, computed on the device from P, q, A, l, u
        alone -- nothing of the scaling, rho, K^-1 or the stored iterates (include/osqp_amd_batch.h: osqp_amd_batch_verify).
        X [B, n], Y [B, m]: the point, unscaled; DX [B, n], DY [B, m]: certificates; None = the handle's own (what
        results() returns).  Needs no solve and changes nothing in the handle.  Returns a namespace with one [B] array per
        slot (VERIFY_FIELDS): obj, pri_res, dua_res, norm_ax, norm_z, norm_px, norm_aty, norm_q, eps_pri, eps_dua, comp,
        dual_obj, gap (float) and optimal, prim_inf, dual_inf (bool), and V [B, 16], the records as the device wrote them.
        eps_abs, eps_rel: the tolerances of eps_pri and eps_dua (None: the handle's settings).
        members=: for the listed members only, with compact arrays [count, .]."""
        V = self._verify("verify", False, members, None, X, Y, DX, DY, eps_abs, eps_rel)
        out = SimpleNamespace(V=V)
        for k, name in enumerate(VERIFY_FIELDS):
            setattr(out, name, V[:, k] != 0.0 if k >= 13 else V[:, k].copy())
        return out

    def verify_into(self, V, X=None, Y=None, DX=None, DY=None, eps_abs=None, eps_rel=None, members=None):
        """verify() between device arrays of the caller's: X, Y, DX, DY (None = the handle's own) are read in place, V
        [B, 16] float64 ([count, 16] with members=) receives the records (VERIFY_FIELDS).  Ready on return."""
        self._kernel_batch("verify_into", why=True)
        if V is None or self._route(V=V, X=X, Y=Y, DX=DX, DY=DY) != "device":
            raise ValueError("verify_into reads and writes device arrays (objects with __cuda_array_interface__); verify() "
                             "takes and returns host arrays")
        self._verify("verify_into", True, members, V, X, Y, DX, DY, eps_abs, eps_rel)

    def _verify(self, call, dev, members, V, X, Y, DX, DY, eps_abs, eps_rel):
        """The one body of verify (dev=False: host arrays in, the records [R, 16] out) and verify_into (dev=True)."""
        self._kernel_batch(call, why=True)
        mem = None if members is None else self._members(members, call)
        if not dev and self._route(X=X, Y=Y, DX=DX, DY=DY) != "host":
            raise ValueError("verify takes host arrays; verify_into reads and writes device arrays")
        eps = []
        for name, e in (("eps_abs", eps_abs), ("eps_rel", eps_rel)):
            if e is not None and (isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating))
                                  or not np.isfinite(e) or e < 0):
                raise ValueError("%s must be a finite number >= 0 or None (the handle's setting), not %r" % (name, e))
            eps.append(-1.0 if e is None else float(e))
        R, n, m = self._rows(mem), self.n, self.m
        want = "verify arrays must be X, DX [%s, %d], Y, DY [%s, %d]%s" % (
            ("B", n, "B", m, "") if mem is None else (R, n, R, m, ": compact, for the %d listed members" % R))
        arrays = self._given(dev, mem, want, (X, n, "X", True), (Y, m, "Y", bool(m)), (DX, n, "DX", True), (DY, m, "DY", bool(m)))
        name, f, lead = self._entry("verify", mem, dev)
        if dev:
            out = device_view(V, (R, 16), "<f8", True, "V")
        else:
            V = np.zeros((R, 16))
            arrays, out = [_p(a if a is None or a.shape[1] else None) for a in arrays], abi.fptr(V)
        rc = f(self._h, *lead, *arrays, *eps, out)
        if rc:
            raise RuntimeError("%s failed (%d)%s" % (name, rc, _BAD_POINTER if dev and rc == 1 else ""))
        return V

    def member_workspace(self, qp):
        """Test hook: member qp's workspace as the last setup / update / solve left it -- D, E, c, rho (scalar),
        ctype (-1 free, 0 inequality, 1 equality), scaled Pv / Av (CSC order of triu(P) / A) and the kernel's
        K^-1 as an NP x NP matrix (padded with identity to NP = 64 or 128; the streamed engine: n rounded up to 32)."""
        self._kernel_batch("member_workspace", why="there is no packed batch workspace to read")
        NP = self.shape()[1]
        D = np.zeros(self.n); E = np.zeros(max(self.m, 1)); c = np.zeros(1); rho = np.zeros(1)
        ct = np.zeros(max(self.m, 1), np.int64); Pv = np.zeros(max(self.Pu.nnz, 1)); Av = np.zeros(max(self.Ah.nnz, 1))
        K = np.zeros((NP, NP)); npo = np.zeros(1, np.int64)
        rc = self._lib.osqp_amd_batch_member(self._h, int(qp), abi.fptr(D), abi.fptr(E), abi.fptr(c), abi.fptr(rho), abi.iptr(ct),
                                             abi.fptr(Pv), abi.fptr(Av), abi.fptr(K), abi.iptr(npo))
        if rc:
            raise RuntimeError("osqp_amd_batch_member failed (%d)" % rc)
        assert int(npo[0]) == NP
        return dict(D=D, E=E[:self.m], c=float(c[0]), rho=float(rho[0]), ctype=ct[:self.m], Pv=Pv[:self.Pu.nnz],
                    Av=Av[:self.Ah.nnz], Kinv=K, NP=NP)

    def device_arrays(self):
        """The result arrays as they sit in HBM -- X [B, n], Y [B, m], info8 [B, 8] -- as objects carrying
        `__cuda_array_interface__` (no copy; `torch.as_tensor(a, device="cuda")` wraps them for a device-side
        gather).  Valid until the next solve / cleanup."""
        self._kernel_batch("device_arrays", why="its results are host arrays (results()); there is no packed device image to wrap")
        px, py, pi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if self._lib.osqp_amd_batch_device_ptrs(self._h, C.byref(px), C.byref(py), C.byref(pi)):
            raise RuntimeError("osqp_amd_batch_device_ptrs failed")

        class _Dev:
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = dict(shape=shape, typestr="<f8", data=(int(ptr), False), version=2, strides=None)
        return _Dev(px.value, (self.B, self.n)), _Dev(py.value, (self.B, max(self.m, 1))), _Dev(pi.value, (self.B, 8))

    def cleanup(self):
        if getattr(self, "_many", None):
            self._many.cleanup()
            self._many = None
        if self._h is not None:
            self._lib.osqp_amd_batch_cleanup(self._h)
            self._h = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass
