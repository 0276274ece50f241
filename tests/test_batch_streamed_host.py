"""Host-side contract of the streamed batch engine (no GPU needed): the engine= option and the refusals of
osqp_amd_batch_setup_engine that happen before any device call."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse


def _problem(n, m, B=2, per_row=1):
    P = sparse.identity(n, format="csc")
    rows = np.repeat(np.arange(m), per_row)
    cols = np.concatenate([(np.arange(per_row) + i) % n for i in range(m)])
    A = sparse.csc_matrix((np.ones(m * per_row), (rows, cols)), shape=(m, n))
    return P, A, np.ones((B, n)), -np.ones((B, m)), np.ones((B, m))


def _c_setup_engine(engine, P, A, Q, L, U, **settings):
    import osqp_amd
    from osqp_amd import abi
    from osqp_amd.batch import _bind, _p
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
    rc = lib.osqp_amd_batch_setup_engine(C.byref(h), engine, Q.shape[0], C.byref(Ph.struct), C.byref(Ah.struct),
                                         _p(None), _p(None), abi.fptr(Q), abi.fptr(L), abi.fptr(U), C.byref(st), 0)
    assert not h.value, "a refused setup must leave no handle"
    return int(rc)


@pytest.mark.parametrize("engine", ["tiled", "Streamed", "", None, 1])
def test_unknown_engine_rejected(engine):
    import osqp_amd
    P, A, Q, L, U = _problem(4, 3)
    with pytest.raises(ValueError, match="engine"):
        osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine)


@pytest.mark.parametrize("setting", ["polish", "time_limit"])
def test_streamed_unimplemented_settings(setting):
    import osqp_amd
    P, A, Q, L, U = _problem(300, 10)
    with pytest.raises(ValueError, match="error 2"):
        osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="streamed", **{setting: 1})
    assert _c_setup_engine(1, P, A, Q, L, U, **{setting: 1}) == 2


def test_streamed_n_above_1024(capfd):
    P, A, Q, L, U = _problem(1025, 4)
    assert _c_setup_engine(1, P, A, Q, L, U) == 4
    err = capfd.readouterr().err
    assert "1025" in err and "1024" in err, err


def test_streamed_lds_limit(capfd):
    # 7 n-vectors of NP = 1024 and 11 m-vectors: m = 1200 needs 163,408 B > 160 KiB
    P, A, Q, L, U = _problem(1024, 1200)
    assert _c_setup_engine(1, P, A, Q, L, U) == 4
    err = capfd.readouterr().err
    assert "160 KiB" in err and "streamed" in err, err


def test_streamed_dense_rows_limit(capfd):
    # every row of A full: 600 rows x 1000 x 1001 / 2 products > 2^26
    P, A, Q, L, U = _problem(1000, 150, per_row=1000)
    assert _c_setup_engine(1, P, A, Q, L, U) == 4
    assert "too dense" in capfd.readouterr().err


def test_unknown_engine_code():
    P, A, Q, L, U = _problem(4, 3)
    assert _c_setup_engine(2, P, A, Q, L, U) == 2
