"""Host-side contract of the common-K batch engine (no GPU needed): the new entry point, the engine= option and the
refusals that happen before any device call.  (Disagreeing row classes are found on the scaled bounds, which the
device computes: that refusal is in tests/test_gpu_batch_common.py.)"""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse


def _problem(n, m, B=2):
    P = sparse.identity(n, format="csc")
    A = sparse.csc_matrix((np.ones(m), (np.arange(m), np.arange(m) % n)), shape=(m, n))
    return P, A, np.ones((B, n)), -np.ones((B, m)), np.ones((B, m))


def _c_setup_common(P, A, Q, L, U, out=True, **settings):
    import osqp_amd
    from osqp_amd import abi
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    Ph, Ah = abi.CscHolder(sparse.triu(P, format="csc")), abi.CscHolder(A)
    st = abi.OSQPSettings()
    lib.osqp_set_default_settings.restype = None
    lib.osqp_set_default_settings.argtypes = [C.POINTER(abi.OSQPSettings)]
    lib.osqp_set_default_settings(C.byref(st)); st.verbose = 0
    for k, v in settings.items():
        setattr(st, k, v)
    Q, L, U = abi.as_f64(Q), abi.as_f64(L), abi.as_f64(U)
    h = C.c_void_p()
    rc = lib.osqp_amd_batch_setup_common(C.byref(h) if out else None, Q.shape[0], C.byref(Ph.struct), C.byref(Ah.struct),
                                         abi.fptr(Q), abi.fptr(L), abi.fptr(U), C.byref(st), 0)
    assert not h.value, "a refused setup must leave no handle"
    return int(rc)


def test_symbol_exported_and_bound():
    import osqp_amd
    from osqp_amd.batch import ENGINES, _bind
    lib = osqp_amd.lib(); _bind(lib)
    assert lib.osqp_amd_batch_setup_common.argtypes is not None and len(lib.osqp_amd_batch_setup_common.argtypes) == 9
    assert ENGINES["common"] == 2 and ENGINES["tiled"] == 0 and ENGINES["streamed"] == 1


def test_null_arguments_refused():
    import osqp_amd
    from osqp_amd.batch import _bind
    lib = osqp_amd.lib(); _bind(lib)
    P, A, Q, L, U = _problem(4, 3)
    assert _c_setup_common(P, A, Q, L, U, out=False) == 1           # OSQP_DATA_VALIDATION_ERROR: no out pointer
    assert lib.osqp_amd_batch_solve(None) == 7                      # OSQP_WORKSPACE_NOT_INIT_ERROR
    one = np.ones(1)
    from osqp_amd import abi
    assert lib.osqp_amd_batch_update_rho(None, abi.fptr(one), 0) == 7


@pytest.mark.parametrize("setting", ["polish", "time_limit"])
def test_unimplemented_settings(setting):
    import osqp_amd
    P, A, Q, L, U = _problem(300, 10)
    with pytest.raises(ValueError, match="error 2"):
        osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **{setting: 1})
    assert _c_setup_common(P, A, Q, L, U, **{setting: 1}) == 2


def test_n_above_1024(capfd):
    P, A, Q, L, U = _problem(1025, 4)
    assert _c_setup_common(P, A, Q, L, U) == 4
    err = capfd.readouterr().err
    assert "1025" in err and "1024" in err and "common-K" in err, err


def test_lds_limit(capfd):
    # 7 n-vectors of NP = 1024 and 11 m-vectors: m = 1200 needs 163,408 B > 160 KiB (the check kernel's LDS)
    P, A, Q, L, U = _problem(1024, 1200)
    assert _c_setup_common(P, A, Q, L, U) == 4
    err = capfd.readouterr().err
    assert "160 KiB" in err and "common-K" in err, err


def test_per_member_values_refused():
    import osqp_amd
    P, A, Q, L, U = _problem(4, 3)
    with pytest.raises(ValueError, match="Px_all"):
        osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", Px_all=np.ones((2, 4)))
    with pytest.raises(ValueError, match="Ax_all"):
        osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", Ax_all=np.ones((2, 3)))


def test_layer_refuses_the_engine():
    from osqp_amd.layer import BatchQPLayer
    P, A, _, _, _ = _problem(4, 3)
    with pytest.raises(ValueError, match="common"):
        BatchQPLayer(P, A, engine="common")
