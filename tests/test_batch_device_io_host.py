"""Host-side contract of the device-array route of the batch engines (no GPU needed): `device_view`'s checks on
hand-made `__cuda_array_interface__` objects, the host / device dispatch of `BatchOSQP.update`, `update_matrices` and
`warm_start`, and the seven osqp_amd_batch_*_dev symbols in the header and in the library."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["osqp_amd_batch_update_dev", "osqp_amd_batch_update_matrices_dev", "osqp_amd_batch_warm_start_dev",
           "osqp_amd_batch_adjoint_dev", "osqp_amd_batch_get_dev", "osqp_amd_batch_polish_status_dev",
           "osqp_amd_batch_check_dev_ptr"]
B, N, M = 3, 5, 7
PTR = 0x7F0000001000


class Fake:
    """What a device array shows of itself; the address is never followed."""

    def __init__(self, shape, typestr="<f8", strides=None, readonly=False, ptr=PTR):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, readonly), version=2, strides=strides)


def test_device_view_accepts_a_good_array():
    from osqp_amd.batch import device_view
    assert device_view(Fake((B, N)), (B, N), "<f8") == PTR
    assert device_view(Fake((B, N), strides=(8 * N, 8)), (B, N), "<f8", writable=True) == PTR     # the contiguous strides, spelt out
    assert device_view(Fake((B,), "<i4", strides=(4,)), (B,), "<i4", writable=True) == PTR
    assert device_view(Fake((B, N), readonly=True), (B, N), "<f8") == PTR                          # an input may be read-only
    assert device_view(Fake((1, N), strides=(800, 8)), (1, N), "<f8") == PTR                       # the stride of an axis of length 1 says nothing


REJECTED = {
    "shape": (Fake((B, N + 1)), False), "rows": (Fake((B + 1, N)), False), "rank": (Fake((B * N,)), False),
    "f4": (Fake((B, N), "<f4"), False), "i8": (Fake((B, N), "<i8"), False), "big_endian": (Fake((B, N), ">f8"), False),
    "row_stride": (Fake((B, N), strides=(8 * (N + 1), 8)), False), "column_major": (Fake((B, N), strides=(8, 8 * B)), False),
    "every_second": (Fake((B, N), strides=(16 * N, 16)), False),
    "readonly_output": (Fake((B, N), readonly=True), True),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_device_view_rejects(case):
    from osqp_amd.batch import device_view
    a, writable = REJECTED[case]
    with pytest.raises(ValueError):
        device_view(a, (B, N), "<f8", writable=writable)


def test_device_view_needs_the_interface():
    from osqp_amd.batch import device_view
    with pytest.raises(ValueError):
        device_view(np.zeros((B, N)), (B, N), "<f8")


def test_route_of_a_call():
    from osqp_amd.batch import io_route
    assert io_route(Q=np.zeros((B, N)), L=None, U=[[0.0] * M] * B) == "host"
    assert io_route(Q=Fake((B, N)), L=None, U=Fake((B, M))) == "device"
    assert io_route(Q=None, L=None) == "host"
    with pytest.raises(ValueError, match="host and device"):
        io_route(Q=Fake((B, N)), L=np.zeros((B, M)))


def _unset_handle():
    """A BatchOSQP with sizes and no handle: the dispatch refuses before the handle would be touched."""
    import osqp_amd
    h = osqp_amd.BatchOSQP()
    h.B, h.n, h.m, h._many = B, N, M, None
    h.Pu, h.Ah = SimpleNamespace(nnz=4), SimpleNamespace(nnz=9)
    return h


def test_mixed_host_and_device_arrays_raise():
    h = _unset_handle()
    with pytest.raises(ValueError, match="host and device"):
        h.update(Q=Fake((B, N)), L=np.zeros((B, M)), U=np.ones((B, M)))
    with pytest.raises(ValueError, match="host and device"):
        h.warm_start(X=np.zeros((B, N)), Y=Fake((B, M)))
    with pytest.raises(ValueError, match="host and device"):
        h.update_matrices(Px=np.ones(4), Ax=Fake((B, 9)))
    with pytest.raises(ValueError):
        h.results_into(X=np.zeros((B, N)))                 # host arrays are results()'s


def test_device_arrays_on_a_per_member_handle_raise():
    h = _unset_handle()
    h._many = []                                           # what setup leaves for n > 128 with engine="auto"
    with pytest.raises(RuntimeError, match="single-QP engine per member"):
        h.update(Q=Fake((B, N)))
    with pytest.raises(RuntimeError, match="single-QP engine per member"):
        h.results_into(X=Fake((B, N)))
    h._many = None


def test_device_shapes_are_checked_before_the_handle():
    h = _unset_handle()
    with pytest.raises(ValueError):
        h.update(Q=Fake((B, N + 1)))
    with pytest.raises(ValueError):
        h.update(L=Fake((B, M), "<f4"), U=Fake((B, M)))
    with pytest.raises(ValueError):
        h.warm_start(X=Fake((B, N), strides=(8, 8 * B)))
    with pytest.raises(ValueError):
        h.results_into(X=Fake((B, N), readonly=True))
    with pytest.raises(ValueError):
        h.adjoint_into(Fake((B, N)), None, Fake((B, N)), Fake((B, M)), Fake((B, M)), status_adjoint=Fake((B,), "<i8"))


def test_header_declares_the_device_entry_points():
    with open(os.path.join(ROOT, "include", "osqp_amd_batch.h")) as f:
        text = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bc_int\s+%s\s*\(" % name, text), name
    assert "Ordering" in text and "hipPointerGetAttributes" in text


def test_library_exports_the_device_entry_points():
    import osqp_amd
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert len(lib.osqp_amd_batch_adjoint_dev.argtypes) == 10 and len(lib.osqp_amd_batch_update_matrices_dev.argtypes) == 9


def test_null_handle_is_refused():
    import osqp_amd
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    assert lib.osqp_amd_batch_update_dev(None, None, None, None) == 7          # OSQP_WORKSPACE_NOT_INIT_ERROR
    assert lib.osqp_amd_batch_get_dev(None, None, None, None, None, None) == 7
    assert lib.osqp_amd_batch_polish_status_dev(None, None) == 7
    assert lib.osqp_amd_batch_check_dev_ptr(None, None) == 7
