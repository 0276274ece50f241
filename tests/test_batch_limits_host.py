"""The per-call limits of a batch solve (osqp_amd_batch_solve_limited, osqp_amd_batch_solve_report; `max_iter=`,
`time_limit=` and `solve_report()` in osqp_amd/batch.py) as far as they go without a GPU: both entries are exported
with the signature batch.py binds and refuse a NULL handle first, and the Python layer refuses bad values and the
one-engine-per-member route before any C call (the handle is faked as test_batch_members_host.py fakes it)."""
import ctypes as C
import inspect

import numpy as np
import pytest

from osqp_amd import abi
from osqp_amd.batch import BatchOSQP, SolveReport, _bind
from osqp_amd._lib import lib
from test_batch_members_host import _fake

NOT_INIT = 7       # OSQP_WORKSPACE_NOT_INIT_ERROR


def test_signatures():
    L = lib()
    _bind(L)
    f = L.osqp_amd_batch_solve_limited
    assert f.restype is abi.c_int and f.argtypes == [C.c_void_p, abi.c_int_p, abi.c_int, abi.c_int, abi.c_float]
    g = L.osqp_amd_batch_solve_report
    assert g.restype is abi.c_int and g.argtypes == [C.c_void_p, abi.c_float_p]
    assert SolveReport._fields == ("max_iter", "time_limit", "elapsed", "cut")
    assert list(inspect.signature(BatchOSQP.solve).parameters) == ["self", "fetch", "members", "max_iter", "time_limit"]


def test_null_handle_is_refused_first():
    """NULL handle: OSQP_WORKSPACE_NOT_INIT_ERROR whatever else is wrong with the call (a negative cap, a NaN limit, a
    NULL list with a count, NULL out)."""
    L = lib()
    _bind(L)
    null_i, null_f = C.cast(None, abi.c_int_p), C.cast(None, abi.c_float_p)
    one = np.zeros(1, np.int64)
    for args in ((null_i, 0, 0, 0.0), (null_i, 3, -1, 0.0), (null_i, 0, 0, float("nan")), (null_i, 0, 0, -1.0),
                 (abi.iptr(one), 1, 5, 1.0), (null_i, 0, 0, float("inf"))):
        assert L.osqp_amd_batch_solve_limited(None, *args) == NOT_INIT, args[1:]
    assert L.osqp_amd_batch_solve_report(None, abi.fptr(np.zeros(4))) == NOT_INIT
    assert L.osqp_amd_batch_solve_report(None, null_f) == NOT_INIT


@pytest.mark.parametrize("engine", ["auto", "streamed", "common"])
def test_bad_values_are_refused_in_python(engine):
    h = _fake(engine=engine)
    for bad in (0, -1, 2.0, 2.5, "3", True, [4], float("nan")):
        with pytest.raises(ValueError, match="max_iter must be an integer >= 1"):
            h.solve(max_iter=bad)
        with pytest.raises(ValueError, match="max_iter must be an integer >= 1"):
            h.solve(max_iter=bad, time_limit=1.0)
    for bad in (0, 0.0, -1e-3, float("nan"), float("inf"), -float("inf"), "1", True, [1.0]):
        with pytest.raises(ValueError, match="time_limit must be a finite number of seconds > 0"):
            h.solve(time_limit=bad)
        with pytest.raises(ValueError, match="time_limit must be a finite number of seconds > 0"):
            h.solve(max_iter=np.int64(3), time_limit=bad)
    h._h = None


def test_members_with_limits_keep_the_members_checks():
    h = _fake(engine="streamed")
    with pytest.raises(RuntimeError, match=r"solve\(members=\.\.\.\) is not served by the tiled or the streamed engine"):
        h.solve(members=[0, 1], max_iter=3)
    h = _fake(engine="common")
    with pytest.raises(ValueError, match="members"):
        h.solve(members=[3, 2], time_limit=1.0)
    h._h = None


def test_one_engine_per_member_route_refuses():
    h = _fake(engine="auto", many=[])
    with pytest.raises(RuntimeError, match=r"solve\(max_iter=\.\.\.\) is not served by the one-engine-per-member route"):
        h.solve(max_iter=5)
    with pytest.raises(RuntimeError, match=r"solve\(time_limit=\.\.\.\) is not served by the one-engine-per-member route"):
        h.solve(time_limit=0.5)
    with pytest.raises(RuntimeError, match=r"solve\(max_iter=\.\.\.\) is not served by the one-engine-per-member route"):
        h.solve(max_iter=5, time_limit=0.5)
    with pytest.raises(RuntimeError, match="solve_report is not served by the one-engine-per-member route"):
        h.solve_report()
    h._h = None
