"""Host-side contract of polish on the batch engines (no GPU needed): polish is a call on a solved handle
(osqp_amd_batch_polish, BatchOSQP.polish); the `polish` setting at setup stays refused on both engines."""
import pytest

from test_batch_streamed_host import _c_setup_engine, _problem


def test_library_exports_polish():
    import osqp_amd
    assert hasattr(osqp_amd.lib(), "osqp_amd_batch_polish")


def test_python_polish_exists():
    import osqp_amd
    from osqp_amd.batch import _bind
    assert callable(getattr(osqp_amd.BatchOSQP, "polish", None))
    lib = osqp_amd.lib(); _bind(lib)
    assert lib.osqp_amd_batch_polish.argtypes is not None and len(lib.osqp_amd_batch_polish.argtypes) == 2


@pytest.mark.parametrize("engine, n", [("auto", 40), ("streamed", 40), ("streamed", 300)])
def test_polish_setting_still_refused(engine, n):
    import osqp_amd
    P, A, Q, L, U = _problem(n, 10)
    with pytest.raises(ValueError, match="error 2"):
        osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, polish=1)
    assert _c_setup_engine(0 if engine == "auto" else 1, P, A, Q, L, U, polish=1) == 2
