"""BatchOSQP.verify / verify_into (osqp_amd_batch_verify and its _dev, _members, _members_dev forms) as far as they go
without a GPU: the four entries are exported with the signatures of include/osqp_amd_batch.h, each refuses a NULL handle
before it looks at anything else, and the Python layer refuses mixed host and device arrays, bad lists, bad shapes, bad
tolerances and the one-engine-per-member route before any C call (the handle is faked as test_batch_members_host.py
fakes it: no call below may reach the library)."""
import ctypes as C
import inspect

import numpy as np
import pytest

from _members_cases import DevArray
from osqp_amd import abi
from osqp_amd.batch import _CALLS, MEMBER_CALLS, VERIFY_FIELDS, BatchOSQP, _bind
from osqp_amd._lib import lib
from test_batch_members_host import BAD_LISTS, B, M, N, NOT_INIT, _fake

ENTRIES = ("verify", "verify_dev", "verify_members", "verify_members_dev")


def _dev(*shape):
    return DevArray(None, 0x1000, tuple(shape), np.dtype(np.float64))


def test_signatures():
    L = lib()
    _bind(L)
    assert not set(ENTRIES) & set(MEMBER_CALLS) and set(ENTRIES) <= set(_CALLS)
    f8, i8, v = abi.c_float_p, abi.c_int_p, C.c_void_p
    want = dict(verify=[f8] * 4 + [abi.c_float] * 2 + [f8], verify_dev=[v] * 4 + [abi.c_float] * 2 + [v])
    for name in ENTRIES:
        f = getattr(L, "osqp_amd_batch_" + name)
        lead = [C.c_void_p] + ([i8, abi.c_int] if "members" in name else [])
        assert f.restype is abi.c_int and f.argtypes == lead + want[name.replace("_members", "")], name
    assert len(VERIFY_FIELDS) == 16 and VERIFY_FIELDS[:3] == ["obj", "pri_res", "dua_res"]
    assert VERIFY_FIELDS[8:] == ["eps_pri", "eps_dua", "comp", "dual_obj", "gap", "optimal", "prim_inf", "dual_inf"]
    assert list(inspect.signature(BatchOSQP.verify).parameters) == ["self", "X", "Y", "DX", "DY", "eps_abs", "eps_rel", "members"]
    assert list(inspect.signature(BatchOSQP.verify_into).parameters) == ["self", "V", "X", "Y", "DX", "DY", "eps_abs", "eps_rel",
                                                                         "members"]


def test_null_handle_is_refused_first():
    """NULL handle: OSQP_WORKSPACE_NOT_INIT_ERROR whatever else is wrong with the call (a NULL V, a NaN tolerance, a NULL
    list with a count)."""
    L = lib()
    _bind(L)
    null_i = C.cast(None, abi.c_int_p)
    one, V = np.zeros(1, np.int64), np.zeros(16)
    for name in ENTRIES:
        f = getattr(L, "osqp_amd_batch_" + name)
        out = (lambda a: None if a is None else a.ctypes.data) if name.endswith("_dev") else (lambda a: None if a is None else abi.fptr(a))
        for lead in ([(null_i, 0), (abi.iptr(one), 1), (null_i, 3)] if "members" in name else [()]):
            for eps, v in (((-1.0, -1.0), V), ((float("nan"), 1e-3), V), ((1e-3, float("inf")), None), ((-1.0, -1.0), None)):
                assert f(None, *lead, None, None, None, None, *eps, out(v)) == NOT_INIT, (name, lead[1:], eps)


def test_mixed_and_misplaced_arrays_are_refused():
    h = _fake()
    z = np.zeros
    with pytest.raises(ValueError, match="host and device arrays in one call"):
        h.verify(X=z((B, N)), Y=_dev(B, M))
    with pytest.raises(ValueError, match="verify takes host arrays"):
        h.verify(X=_dev(B, N))
    with pytest.raises(ValueError, match="host and device arrays in one call"):
        h.verify_into(_dev(B, 16), X=z((B, N)))
    for V in (None, z((B, 16))):
        with pytest.raises(ValueError, match="verify_into reads and writes device arrays"):
            h.verify_into(V)
    with pytest.raises(ValueError, match="V has shape"):
        h.verify_into(_dev(B, 15))
    with pytest.raises(ValueError, match="V has shape"):
        h.verify_into(_dev(B, 16), members=[0, 1])
    h._h = None


def test_shapes_and_tolerances_are_refused():
    h = _fake()
    z = np.zeros
    for kw in (dict(X=z((B, N + 1))), dict(Y=z((B + 1, M))), dict(DX=z(N)), dict(DY=z((B, M, 1)))):
        with pytest.raises(ValueError, match=r"verify arrays must be X, DX \[B, %d\], Y, DY \[B, %d\]" % (N, M)):
            h.verify(**kw)
    with pytest.raises(ValueError, match="compact, for the 2 listed members"):
        h.verify(X=z((B, N)), members=[1, 4])
    with pytest.raises(ValueError, match="compact, for the 2 listed members"):
        h.verify_into(_dev(2, 16), DY=_dev(B, M), members=[1, 4])
    with pytest.raises(ValueError, match="X has shape"):
        h.verify_into(_dev(B, 16), X=_dev(B, N + 1))
    for name in ("eps_abs", "eps_rel"):
        for bad in (-1.0, float("nan"), float("inf"), "1e-3", True, [1e-3]):
            with pytest.raises(ValueError, match="%s must be a finite number >= 0 or None" % name):
                h.verify(**{name: bad})
            with pytest.raises(ValueError, match="%s must be a finite number >= 0 or None" % name):
                h.verify_into(_dev(B, 16), **{name: bad})
    h._h = None


@pytest.mark.parametrize("bad", BAD_LISTS, ids=[str(k) for k in range(len(BAD_LISTS))])
def test_bad_lists_are_refused(bad):
    h = _fake(engine="common")
    with pytest.raises(ValueError, match="members"):
        h.verify(members=bad)
    with pytest.raises(ValueError, match="members"):
        h.verify_into(_dev(2, 16), members=bad)
    h._h = None


def test_one_engine_per_member_route_refuses():
    h = _fake(engine="auto", many=[])
    for call, fn in (("verify", lambda **kw: h.verify(**kw)), ("verify_into", lambda **kw: h.verify_into(_dev(B, 16), **kw))):
        for kw in ({}, dict(members=[0, 1])):
            with pytest.raises(RuntimeError, match="%s is a call of the batch engines" % call):
                fn(**kw)
    h._h = None
