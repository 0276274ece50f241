"""Host-side contract of the shared KKT pieces of the common-K engine (no GPU needed): the two new entry points, the
shared_kkt option and the refusals that happen before any device call.  (The refusal of a handle of another engine needs
a live handle: tests/test_gpu_batch_common_kkt.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import sparse


def _problem(n, m, B=2):
    P = sparse.identity(n, format="csc")
    A = sparse.csc_matrix((np.ones(m), (np.arange(m), np.arange(m) % n)), shape=(m, n))
    return P, A, np.ones((B, n)), -np.ones((B, m)), np.ones((B, m))


def _lib():
    import osqp_amd
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    return lib


def test_symbols_exported_and_bound():
    lib = _lib()
    assert len(lib.osqp_amd_batch_common_kkt.argtypes) == 2
    assert len(lib.osqp_amd_batch_common_kkt_peek.argtypes) == 7


def test_null_handle():
    from osqp_amd import abi
    lib = _lib()
    for on in (0, 1):
        assert lib.osqp_amd_batch_common_kkt(None, on) == 7        # OSQP_WORKSPACE_NOT_INIT_ERROR
    no_f, no_i = C.cast(None, abi.c_float_p), C.cast(None, abi.c_int_p)
    H = np.zeros(4)
    assert lib.osqp_amd_batch_common_kkt_peek(None, no_f, no_f, 0, no_i, no_i, no_f) == 7
    assert lib.osqp_amd_batch_common_kkt_peek(None, abi.fptr(H), no_f, 0, no_i, no_i, no_f) == 7
    assert not H.any()


def test_option_belongs_to_the_common_engine():
    import osqp_amd
    P, A, Q, L, U = _problem(4, 3)
    for engine in ("auto", "streamed"):
        with pytest.raises(ValueError, match="shared_kkt"):
            osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, shared_kkt=True)


def test_unserved_depends_on_the_pieces():
    import osqp_amd
    bs = osqp_amd.BatchOSQP()
    bs.engine, bs._shared_kkt = "common", False
    with pytest.raises(RuntimeError, match="common-K"):
        bs._unserved("polish")
    bs._shared_kkt = True
    bs._unserved("polish")
    with pytest.raises(RuntimeError, match="common-K"):
        bs._unserved("update_matrices", never=True)
    bs.engine = "streamed"
    bs._unserved("update_matrices", never=True)
    fresh = osqp_amd.BatchOSQP()
    with pytest.raises(RuntimeError, match="live common-K handle"):
        fresh.shared_kkt()


def test_layer_accepts_the_engine_with_the_pieces():
    from osqp_amd.layer import BatchQPLayer
    P, A, Q, L, U = _problem(4, 3)
    with pytest.raises(ValueError, match="common"):
        BatchQPLayer(P, A, engine="common", shared_kkt=False)
    layer = BatchQPLayer(P, A, engine="common", shared_kkt=True)
    assert layer.h is None and layer.settings["shared_kkt"] is True
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    for kw in (dict(Px=t(np.ones((2, 4)))), dict(Ax=t(np.ones((2, 3))))):
        with pytest.raises(ValueError, match="takes no Px / Ax"):
            layer(t(Q), t(L), t(U), **kw)
    assert layer.h is None                                          # refused before any set-up
