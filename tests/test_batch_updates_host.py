"""Host side of the batch update family (osqp_amd_batch_update_matrices / _update_rho / _warm_start) without a
device: the symbols are exported and bind with the documented signatures, a NULL handle is refused before any
device call, and the Python-side shape and index checks of BatchOSQP.update_matrices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

OSQP_WORKSPACE_NOT_INIT_ERROR = 7      # include/osqp_amd_types.h


@pytest.fixture(scope="module")
def lib():
    import osqp_amd
    from osqp_amd.batch import _bind
    osqp_amd.build()
    L = osqp_amd.lib()
    _bind(L)
    return L


def test_symbols_bind_with_the_documented_signatures(lib):
    from osqp_amd import abi
    H, F, I, i = C.c_void_p, abi.c_float_p, abi.c_int_p, abi.c_int
    want = dict(osqp_amd_batch_update_matrices=[H, F, I, i, i, F, I, i, i], osqp_amd_batch_update_rho=[H, F, i],
                osqp_amd_batch_warm_start=[H, F, F])
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "osqp_amd_batch.h")).read(), flags=re.S)
    for name, argtypes in want.items():
        f = getattr(lib, name)
        assert f.restype is abi.c_int and list(f.argtypes) == argtypes, name
        decl = re.search(r"c_int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl is not None, name
        params = [p.strip() for p in decl.group(1).split(",")]
        kinds = [H if "osqp_amd_batch" in p else F if "c_float" in p else I if "c_int *" in p or "c_int  *" in p else i for p in params]
        assert kinds == argtypes, (name, params)


def test_null_handle_is_refused(lib):
    from osqp_amd import abi
    v = np.ones(4); k = np.zeros(4, np.int64)
    nf, ni = C.cast(None, abi.c_float_p), C.cast(None, abi.c_int_p)
    assert lib.osqp_amd_batch_update_matrices(None, abi.fptr(v), abi.iptr(k), 4, 0, nf, ni, 0, 0) == OSQP_WORKSPACE_NOT_INIT_ERROR
    assert lib.osqp_amd_batch_update_rho(None, abi.fptr(v), 0) == OSQP_WORKSPACE_NOT_INIT_ERROR
    assert lib.osqp_amd_batch_warm_start(None, abi.fptr(v), nf) == OSQP_WORKSPACE_NOT_INIT_ERROR


def test_methods_exist():
    from osqp_amd.batch import BatchOSQP
    for name in ("update_matrices", "update_rho", "warm_start"):
        assert callable(getattr(BatchOSQP, name))


B, NP_, NA = 4, 7, 9
MALFORMED = [dict(Px=np.ones(NP_ + 1)), dict(Ax=np.ones((B + 1, NA))), dict(Ax=np.ones((B, NA - 1))),
             dict(Px=np.ones(3), Px_idx=[0, 1]), dict(Ax=np.ones(2), Ax_idx=[0, NA]), dict(Px=np.ones(2), Px_idx=[-1, 0]),
             dict(Px=np.ones((2, 2, 2))), dict(Ax_idx=[0]), dict(Ax=np.ones((B, 2)), Ax_idx=[[0, 1]] * B),
             dict(Px=np.float64(1.0))]


@pytest.mark.parametrize("kwargs", MALFORMED, ids=[",".join(sorted(k)) + str(n) for n, k in enumerate(MALFORMED)])
def test_malformed_matrix_updates_raise(kwargs):
    from osqp_amd.batch import check_matrix_update
    with pytest.raises(ValueError):
        check_matrix_update(B, NP_, NA, **kwargs)


def test_well_formed_matrix_updates_pass():
    from osqp_amd.batch import check_matrix_update
    assert check_matrix_update(B, NP_, NA) == (None, None, 0, None, None, 0)
    Px, Pi, pper, Ax, Ai, aper = check_matrix_update(B, NP_, NA, Px=np.ones(NP_), Ax=np.ones((B, NA)))
    assert (Px.shape, Pi, pper, Ax.shape, Ai, aper) == ((NP_,), None, 0, (B, NA), None, 1)
    Px, Pi, pper, Ax, Ai, aper = check_matrix_update(B, NP_, NA, Px=[[1.0, 2.0]] * B, Px_idx=[0, NP_ - 1], Ax=[3.0], Ax_idx=[NA - 1])
    assert (Px.shape, pper, Ax.shape, aper) == ((B, 2), 1, (1,), 0)
    assert Pi.dtype == np.int64 and list(Pi) == [0, NP_ - 1] and list(Ai) == [NA - 1]
    assert Px.dtype == np.float64 and Px.flags.c_contiguous
    # more listed slots than the matrix has (all in range): the C side answers with the reference's codes 1 / 2
    check_matrix_update(B, NP_, NA, Px=np.ones(NP_ + 1), Px_idx=np.zeros(NP_ + 1, int))
