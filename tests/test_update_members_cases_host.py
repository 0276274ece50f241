"""The cases of tests/test_gpu_batch_update_members.py, checked on the CPU with the oracle alone, and the member-list
forms of the matrix and rho updates as far as they go without a GPU.

The cases (tests/_update_members_cases.py): for every case and every member -- every list is made of them -- the oracle's
sequence setup, solve, update(Px, Ax), solve
  * ends both solves on the same iteration count, rho_updates and status when the new values move by 1e-15 relative,
    over three draws (the rule at the top of tests/test_gpu_batch_updates.py: no member is let off), and ends them solved;
  * moves D by more than 1e-3 relative through the update;
  * gives a second solution more than 100 x the parity bar (1e-6 relative) away from the one with the old values, from
    the one with the member's new P and the old A, and from the one with any other member's new values: an update that
    is not applied, or a compact row that lands on the wrong member, cannot pass the GPU tests;
and in every list some listed member's rho moves in the first solve.  The two other sequences of the GPU tests -- a member
that is not listed (setup, solve, solve) and one that gets a new rho (setup, solve, update_rho, solve) -- end where they
end when q moves by 1e-15 relative.

The ABI: the three entries are exported and bind with the signatures of include/osqp_amd_batch.h, each returns
OSQP_WORKSPACE_NOT_INIT_ERROR for a NULL handle before anything else, and `update_matrices(members=)` /
`update_rho(members=)` refuse wrong shapes, masks, lists, engine="common" and the one-engine-per-member route before any C
call."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import _update_members_cases as uc
from osqp_amd import abi
from osqp_amd._lib import lib
from osqp_amd.batch import _CALLS, MEMBER_CALLS, BatchOSQP, _bind

NOT_INIT = 7       # OSQP_WORKSPACE_NOT_INIT_ERROR
ENTRIES = ("update_matrices_members", "update_matrices_members_dev", "update_rho_members")


@pytest.fixture(scope="module")
def reports(oracle_mod):
    return {case: uc.seed_report(oracle_mod, case) for case in uc.CASES}


@pytest.mark.parametrize("case", uc.CASES, ids=uc.IDS)
def test_every_member_is_robust_and_its_update_matters(reports, case):
    for b, r in enumerate(reports[case]):
        print("%s member %d: %s" % (case, b, r))
        assert r["status"] == (1, 1), (case, b, r)
        assert r["robust"], (case, b, "a 1e-15 move of the new values changes where the oracle ends")
        assert r["D_moved"] > 1e-3, (case, b, r["D_moved"])
        assert r["matters"] > 100 * uc.PARITY, (case, b, r["matters"])
        assert r["idle_robust"] and r["rho_robust"] and r["rho_status"] == 1, (case, b, r)


@pytest.mark.parametrize("case", uc.CASES, ids=uc.IDS)
def test_in_every_list_some_rho_moves(reports, case):
    for name, S in uc.LISTS.items():
        assert any(reports[case][b]["rho_moved"] > 0 for b in uc.members_of(S)), (case, name)


def test_the_lists():
    for name, S in uc.LISTS.items():
        mem = uc.members_of(S)
        assert mem.size >= 1 and np.all(np.diff(mem) > 0) and mem[0] >= 0 and mem[-1] < uc.B, name
    assert list(uc.members_of(uc.LISTS["all"])) == list(range(uc.B))
    assert uc.members_of(uc.LISTS["but_one"]).size == uc.B - 1
    assert np.asarray(uc.LISTS["mask"]).dtype == np.bool_


def test_twin_arrays():
    cur = np.arange(4.0)
    t = uc.twin_arrays(cur, [1, 3], np.array([[10.0, 11.0], [20.0, 21.0]]), idx=np.array([0, 2]))
    assert t.shape == (uc.B, 2) and list(t[1]) == [10.0, 11.0] and list(t[3]) == [20.0, 21.0] and list(t[0]) == [0.0, 2.0]
    t = uc.twin_arrays(np.tile(cur, (uc.B, 1)) + np.arange(uc.B)[:, None], uc.LISTS["mask"], np.full(4, -1.0))
    assert np.all(t[[0, 2, 3]] == -1.0) and list(t[1]) == [1.0, 2.0, 3.0, 4.0]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_signatures():
    L = lib()
    _bind(L)
    assert not set(ENTRIES) & set(MEMBER_CALLS)
    kinds = dict(f=abi.c_float_p, i=abi.c_int_p, v=C.c_void_p, n=abi.c_int)
    head = [C.c_void_p, abi.c_int_p, abi.c_int]
    for dev in ("", "_dev"):
        f = getattr(L, "osqp_amd_batch_update_matrices_members" + dev)
        twin = getattr(L, "osqp_amd_batch_update_matrices" + dev)
        assert f.restype is abi.c_int and f.argtypes == head + twin.argtypes[1:]
        assert f.argtypes[3:] == [kinds["v" if dev else "f"], abi.c_int_p, abi.c_int, abi.c_int] * 2
    f = L.osqp_amd_batch_update_rho_members
    assert f.restype is abi.c_int and f.argtypes == head + [abi.c_float_p, abi.c_int]
    assert f.argtypes[3:] == L.osqp_amd_batch_update_rho.argtypes[1:]
    for name in ENTRIES:
        assert _CALLS[name].startswith("hin")


def test_null_handle_is_refused_first():
    L = lib()
    _bind(L)
    null_i = C.cast(None, abi.c_int_p)
    one = np.zeros(1, np.int64)
    for name in ENTRIES:
        f = getattr(L, "osqp_amd_batch_" + name)
        rest = [1 if k == "n" else None for k in _CALLS[name][3:]]
        assert f(None, null_i, 0, *rest) == NOT_INIT, name
        assert f(None, abi.iptr(one), 1, *rest) == NOT_INIT, name


# ---- the Python argument checks --------------------------------------------------------------------------------------------
B, N, M, NNZP, NNZA = 8, 5, 3, 7, 9


class _NoLib:
    """Stands for the library: naming an entry is fine, calling one fails the test."""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError("%s was called" % name)
        return call


def _fake(engine="streamed", many=None):
    h = BatchOSQP.__new__(BatchOSQP)
    h._lib = _NoLib()
    h.engine, h._many, h._h, h.B, h.n, h.m, h._shared_kkt, h._status_polish = engine, many, object(), B, N, M, True, None
    h.Pu = sparse.random(N, N, density=1.0, format="csc", random_state=0)
    h.Ah = sparse.random(M, N, density=1.0, format="csc", random_state=0)
    return h


def test_wrong_shapes():
    h, z = _fake(), np.zeros
    nP, nA = h.Pu.nnz, h.Ah.nnz
    for kw, words in ((dict(Px=z((3, nP))), "Px has 3 rows, the batch has 2 members"),
                      (dict(Ax=z((B, nA))), "Ax has %d rows, the batch has 2 members" % B),
                      (dict(Px=z(nP - 1)), "Px has %d values per member" % (nP - 1)),
                      (dict(Ax=z((2, 3)), Ax_idx=[0, 1]), "Ax_idx must be a vector as long as a member's Ax"),
                      (dict(Px=z((2, 1, nP))), "Px must be [k] (shared) or [B, k] (per member)")):
        with pytest.raises(ValueError) as e:
            h.update_matrices(members=[1, 3], **kw)
        assert words in str(e.value) and "with members= the values are [k] or compact [count, k] (2 listed members)" in str(e.value)
    for rho in (z(3), z(B), z((2, 1))):
        with pytest.raises(ValueError, match=r"rho with members= must be a scalar or \[2\]"):
            h.update_rho(rho, members=[1, 3])
    with pytest.raises(ValueError, match=r"rho must be a scalar or \[B\]"):
        h.update_rho(z(2))


@pytest.mark.parametrize("bad, words", [([3, 1], "strictly ascending"), ([1, 1], "strictly ascending"), ([0, B], "out of range"),
                                        ([], "members is empty"), (np.ones(B - 1, bool), "mask must have length B = %d" % B),
                                        (np.zeros(B, bool), "members is empty"), ([0.5], "ascending integer sequence")],
                         ids=lambda v: None if isinstance(v, str) else str(list(v)))
def test_bad_lists_and_masks(bad, words):
    h = _fake()
    with pytest.raises(ValueError, match=words):
        h.update_matrices(Px=np.zeros(h.Pu.nnz), members=bad)
    with pytest.raises(ValueError, match=words):
        h.update_rho(0.5, members=bad)


def test_common_engine_and_the_per_member_route_refuse():
    h = _fake("common")
    with pytest.raises(RuntimeError, match="update_matrices is not served by the common-K engine"):
        h.update_matrices(Px=np.zeros(h.Pu.nnz), members=[1, 3])
    with pytest.raises(ValueError, match="engine='common' has one rho for the batch: update_rho takes a scalar"):
        h.update_rho(np.ones(2), members=[1, 3])
    h = _fake("auto", many=[])
    for call, fn in (("update_matrices", lambda: h.update_matrices(Px=np.zeros(h.Pu.nnz), members=[1, 3])),
                     ("update_rho", lambda: h.update_rho(0.5, members=[1, 3]))):
        with pytest.raises(RuntimeError) as e:
            fn()
        assert "%s(members=...) is not served by the one-engine-per-member route" % call in str(e.value)
