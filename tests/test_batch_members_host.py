"""The member-list forms of the batch calls (osqp_amd_batch_*_members, `members=` in osqp_amd/batch.py) as far as they go
without a GPU: every new entry is exported with the signature batch.py binds, refuses a NULL handle with
OSQP_WORKSPACE_NOT_INIT_ERROR before it looks at anything else, and the Python layer refuses bad lists, bad masks,
wrong compact shapes and the one-engine-per-member route before any C call (the handle is faked as
test_common_members_cases_host.py fakes it: no call below may reach it)."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

from osqp_amd import abi
from osqp_amd.batch import MEMBER_CALLS, BatchOSQP, _bind
from osqp_amd._lib import lib

B, N, M, NNZP, NNZA = 8, 5, 3, 7, 9
NOT_INIT = 7       # OSQP_WORKSPACE_NOT_INIT_ERROR


class _NoLib:
    """Stands for the library: naming an entry is fine (Python does that before it evaluates the arguments, where the
    shape checks sit), calling one fails the test."""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError("%s was called" % name)
        return call


def _fake(engine="streamed", many=None, shared=True):
    h = BatchOSQP.__new__(BatchOSQP)
    h._lib = _NoLib()
    h.engine, h._many, h._h, h.B, h.n, h.m, h._shared_kkt, h._status_polish = engine, many, object(), B, N, M, shared, None
    h.Pu = sparse.random(N, N, density=1.0, format="csc"); h.Ah = sparse.random(M, N, density=1.0, format="csc")
    return h


def test_signatures():
    L = lib()
    _bind(L)
    kinds = dict(f=abi.c_float_p, i=abi.c_int_p, v=C.c_void_p, n=abi.c_int)
    assert set(MEMBER_CALLS) == {"update_members", "update_members_dev", "warm_start_members", "warm_start_members_dev",
                                 "polish_members", "adjoint_members", "adjoint_members_dev", "tangent_members",
                                 "tangent_members_dev", "get_members", "get_members_dev"}
    for name, args in MEMBER_CALLS.items():
        f = getattr(L, "osqp_amd_batch_" + name)
        assert f.restype is abi.c_int
        assert f.argtypes == [C.c_void_p, abi.c_int_p, abi.c_int] + [kinds[k] for k in args], name
    # the arities of the header: the twin's arguments behind (handle, members, count)
    arity = {k: len(v) for k, v in MEMBER_CALLS.items()}
    assert arity == dict(update_members=3, update_members_dev=3, warm_start_members=2, warm_start_members_dev=2,
                         polish_members=1, adjoint_members=10, adjoint_members_dev=10, tangent_members=10,
                         tangent_members_dev=10, get_members=5, get_members_dev=5)
    assert L.osqp_amd_batch_solved_members.argtypes == [C.c_void_p, abi.c_int_p]


def test_null_handle_is_refused_first():
    """NULL handle: OSQP_WORKSPACE_NOT_INIT_ERROR from every entry, whatever else is wrong with the call (NULL list,
    count = 0, NULL arrays)."""
    L = lib()
    _bind(L)
    null_i = C.cast(None, abi.c_int_p)
    one = np.zeros(1, np.int64)
    for name, args in MEMBER_CALLS.items():
        f = getattr(L, "osqp_amd_batch_" + name)
        rest = [1 if k == "n" else None for k in args]
        assert f(None, null_i, 0, *rest) == NOT_INIT, name
        assert f(None, abi.iptr(one), 1, *rest) == NOT_INIT, name
    assert L.osqp_amd_batch_solved_members(None, abi.iptr(one)) == NOT_INIT
    assert L.osqp_amd_batch_solved_members(None, null_i) == NOT_INIT


BAD_LISTS = ([3, 2], [1, 1], [0, B], [-1, 0], [], np.ones(B - 1, bool), np.zeros(B, bool), [0.5, 1.5], [[0, 1]],
             list(range(B + 1)))


def _calls(h, members):
    z = np.zeros
    R = 2
    return dict(update=lambda: h.update(Q=z((R, N)), members=members),
                warm_start=lambda: h.warm_start(X=z((R, N)), members=members),
                polish=lambda: h.polish(members=members),
                adjoint=lambda: h.adjoint(z((R, N)), z((R, M)), members=members),
                tangent=lambda: h.tangent(dQ=z((R, N)), members=members),
                results=lambda: h.results(members=members))


@pytest.mark.parametrize("bad", BAD_LISTS, ids=[str(k) for k in range(len(BAD_LISTS))])
def test_bad_lists(bad):
    h = _fake()
    for name, call in _calls(h, bad).items():
        with pytest.raises(ValueError, match="members"):
            call()
    h._h = None


def test_wrong_compact_shapes():
    h = _fake()
    S = [1, 4, 6]
    z = np.zeros
    for call in (lambda: h.update(Q=z((B, N)), members=S), lambda: h.update(L=z((3, M + 1)), members=S),
                 lambda: h.update(U=z((2, M)), members=S), lambda: h.update(Q=z(N), members=S)):
        with pytest.raises(ValueError, match=r"Q \[3, %d\], L \[3, %d\], U \[3, %d\]" % (N, M, M)):
            call()
    for call in (lambda: h.warm_start(X=z((B, N)), members=S), lambda: h.warm_start(Y=z((3, M + 2)), members=S)):
        with pytest.raises(ValueError, match=r"X \[3, %d\], Y \[3, %d\]" % (N, M)):
            call()
    for call in (lambda: h.adjoint(z((B, N)), members=S), lambda: h.adjoint(z((3, N)), z((B, M)), members=S)):
        with pytest.raises(ValueError, match=r"compact \(3 listed members\).*dX \[count, n\]"):
            call()
    with pytest.raises(ValueError, match=r"compact \(3 listed members\).*dX must be \[count, D, %d\] with count = 3" % N):
        h.adjoint(z((B, 2, N)), members=S)
    with pytest.raises(ValueError, match=r"compact \(3 listed members\).*agree on D"):
        h.adjoint(z((3, 2, N)), z((3, 1, M)), members=S)
    for call in (lambda: h.tangent(dQ=z((B, N)), members=S), lambda: h.tangent(dL=z((3, 2, M + 1)), members=S),
                 lambda: h.tangent(dPx=z((B, 2, h.Pu.nnz)), members=S)):
        with pytest.raises(ValueError, match=r"compact \(3 listed members\).*\[count, D, \d+\] with count = 3"):
            call()
    # a mask of the wrong length names B
    with pytest.raises(ValueError, match="mask must have length B = %d" % B):
        h.update(Q=z((3, N)), members=np.ones(B + 1, bool))
    h._h = None


def test_device_shapes_are_compact_too():
    class Dev:
        def __init__(self, shape, typestr="<f8"):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(4096, False), version=2, strides=None)
    h = _fake()
    S = [0, 7]
    with pytest.raises(ValueError, match=r"Q \[2, %d\]" % N):
        h.update(Q=Dev((B, N)), members=S)
    with pytest.raises(ValueError, match=r"X \[2, %d\]" % N):
        h.warm_start(X=Dev((B, N)), members=S)
    with pytest.raises(ValueError, match=r"X has shape \(%d, %d\), the handle needs \(2, %d\)" % (B, N, N)):
        h.results_into(X=Dev((B, N)), members=S)
    with pytest.raises(ValueError, match="status_polish"):
        h.results_into(X=Dev((2, N)), status_polish=Dev((B,), "<i4"), members=S)
    with pytest.raises(ValueError, match=r"dq has shape \(%d, %d\), the handle needs \(2, %d\)" % (B, N, N)):
        h.adjoint_into(Dev((2, N)), None, Dev((B, N)), Dev((2, M)), Dev((2, M)), members=S)
    with pytest.raises(ValueError, match=r"compact \(2 listed members\)"):
        h.adjoint_into(Dev((B, 3, N)), None, Dev((B, 3, N)), Dev((B, 3, M)), Dev((B, 3, M)), members=S)
    with pytest.raises(ValueError, match=r"compact \(2 listed members\)"):
        h.tangent_into(Dev((B, N)), Dev((B, M)), dQ=Dev((B, N)), members=S)
    h._h = None


def test_one_engine_per_member_route_refuses():
    h = _fake(engine="auto", many=[])
    calls = _calls(h, [0, 1])
    calls.pop("polish"); calls.pop("adjoint"); calls.pop("tangent")        # (these name the route themselves, below)
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=r"%s\(members=\.\.\.\) is not served by the one-engine-per-member route" % name):
            call()
    for call in (lambda: h.polish(members=[0, 1]), lambda: h.adjoint(np.zeros((2, N)), members=[0, 1]),
                 lambda: h.tangent(dQ=np.zeros((2, N)), members=[0, 1])):
        with pytest.raises(RuntimeError, match="one-engine-per-member route"):
            call()
    with pytest.raises(RuntimeError, match="one-engine-per-member route"):
        h.solved_members()
    h._h = None


def test_common_without_shared_pieces_refuses_in_python():
    h = _fake(engine="common", shared=False)
    for call in (lambda: h.polish(members=[0]), lambda: h.adjoint(np.zeros((1, N)), members=[0]),
                 lambda: h.tangent(dQ=np.zeros((1, N)), members=[0])):
        with pytest.raises(RuntimeError, match="shared KKT pieces"):
            call()
    h._h = None
