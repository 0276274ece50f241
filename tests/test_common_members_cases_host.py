"""The cases of tests/_common_members_cases.py on the CPU: what tests/test_gpu_batch_common_members.py takes for granted
about its inputs -- the waves in which the members of case W end, hence the packs the engine's rule must make of them, and
the common scaling of a chosen set and its batch -- and the argument checks of BatchOSQP.solve(members=...) and of the two
C entry points that need no device."""
import ctypes as C

import numpy as np
import pytest

from _batch_parity import oracle_ws
from _common_cases import ADAPTIVE, FIXED, common_oracle, qhat, row_classes
from _common_members_cases import (ADAPTIVE_SUBSET_B, GROUP, MIN_ITER, PACK_CHUNK, WAVE_PROVED, WAVES, adaptive_subset_case,
                                   packs_of, subsets, wave_case, wave_reference)
from _common_reference import MARGIN_CHECK, margins

OSQP_WORKSPACE_NOT_INIT_ERROR = 7      # include/osqp_amd_types.h


@pytest.mark.parametrize("name", list(WAVES))
def test_wave_case(oracle_mod, name):
    """Classes common, q^ of the batch that of the hard members, every member solved; the easy members end at the first
    check point and the hard ones at three or more different ones; no verdict within MARGIN_CHECK of its threshold; the
    columns the first pack leaves and the number of packs are the recorded ones."""
    B, h, drop = WAVES[name]
    P, A, Q, L, U, hard = wave_case(B, h, drop)
    easy = np.setdiff1d(np.arange(B), hard)
    assert np.array_equal(qhat(Q), qhat(Q[hard]))
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **FIXED))
    for b in range(B):
        assert np.array_equal(row_classes(L[b], U[b], ws["E"]), ws["ctype"]), (name, b)
    assert np.all(L[easy] <= 0) and np.all(U[easy] >= 0) and not Q[easy].any()
    ref, r = wave_reference(oracle_mod, B, h, drop)
    assert np.all(r.status_val == 1)
    assert np.all(r.iter[easy] == MIN_ITER) and len(set(r.iter[hard].tolist())) >= 3, np.unique(r.iter, return_counts=True)
    assert margins(ref)[1] >= MARGIN_CHECK, margins(ref)
    after, packs = WAVE_PROVED[name]
    assert int((r.iter > MIN_ITER).sum()) == after
    assert packs_of(r.iter)[0] == packs >= 1
    print(name, "iterations", dict(zip(*np.unique(r.iter, return_counts=True))), "packs, columns at the end", packs_of(r.iter))


def test_wave_cases_cover_the_edges():
    proved = {k: v[0] for k, v in WAVE_PROVED.items()}
    assert proved["to-64"] == GROUP and proved["to-65"] == GROUP + 1 and proved["to-17"] == 17
    assert proved["chunk"] > PACK_CHUNK and WAVE_PROVED["two"][1] >= 2
    assert proved["one"] <= GROUP


def test_packs_of_follows_the_rule():
    assert packs_of([25] * 2 + [50] * 128) == (1, 128)              # 128 running of 130: three groups down to two
    assert packs_of([25] * 1 + [50] * 129) == (0, 130)              # 129 running: still three groups
    assert packs_of([25] * 65 + [50] * 65) == (1, 65)               # three groups down to two
    assert packs_of([25] * 66 + [50] * 64) == (1, 64)
    assert packs_of([25] * 10 + [50] * 54) == (0, 64)               # one group: nothing to save
    assert packs_of([25] * 70 + [50] * 100 + [75] * 30) == (2, 30)
    assert packs_of([25] * 200) == (0, 200)                         # nobody left running: no pack


@pytest.mark.parametrize("label,S", subsets(ADAPTIVE_SUBSET_B))
def test_adaptive_subset_case(oracle_mod, label, S):
    """q^ of the batch is q^ of the chosen members, and the classes stay common."""
    P, A, Q, L, U = adaptive_subset_case(S)
    assert np.array_equal(qhat(Q), qhat(Q[S])), label
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **ADAPTIVE))
    for b in range(Q.shape[0]):
        assert np.array_equal(row_classes(L[b], U[b], ws["E"]), ws["ctype"]), (label, b)


# ---- argument checks ---------------------------------------------------------------------------------------------------
BAD_LISTS = [[], [3, 2], [1, 1], [0, 8], [-1, 0], list(range(9)), np.ones(7, bool), np.zeros(8, bool), [0.0, 1.0], [[0, 1]]]


@pytest.mark.parametrize("members", BAD_LISTS, ids=[str(k) for k in range(len(BAD_LISTS))])
def test_malformed_member_lists_raise(members):
    from osqp_amd.batch import check_members
    with pytest.raises(ValueError):
        check_members(8, members)


def test_well_formed_member_lists_pass():
    from osqp_amd.batch import check_members
    assert check_members(8, [0, 3, 7]).tolist() == [0, 3, 7]
    assert check_members(8, range(8)).tolist() == list(range(8))
    mask = np.zeros(8, bool); mask[[1, 6]] = True
    out = check_members(8, mask)
    assert out.tolist() == [1, 6] and out.dtype == np.int64 and out.flags.c_contiguous
    assert check_members(8, np.array([5], np.int32)).tolist() == [5]


def test_other_paths_refuse_members():
    """The tiled and streamed engines and the one-engine-per-member path raise before any device call."""
    from osqp_amd.batch import BatchOSQP
    for engine, many in (("auto", None), ("streamed", None), ("auto", [])):
        h = BatchOSQP.__new__(BatchOSQP)
        h.engine, h._many, h._h, h.B = engine, many, object(), 8
        with pytest.raises(RuntimeError, match="not served"):
            h.solve(members=[0, 1])
        with pytest.raises(RuntimeError, match="common-K"):
            h.columns()
        h._h = None                       # (nothing to clean up)


def test_symbols_bind_and_refuse_null():
    import osqp_amd
    from osqp_amd import abi
    from osqp_amd.batch import _bind
    osqp_amd.build()
    L = osqp_amd.lib()
    _bind(L)
    assert list(L.osqp_amd_batch_solve_members.argtypes) == [C.c_void_p, abi.c_int_p, abi.c_int]
    assert list(L.osqp_amd_batch_common_columns.argtypes) == [C.c_void_p, abi.c_int_p]
    k = np.zeros(3, np.int64)
    assert L.osqp_amd_batch_solve_members(None, abi.iptr(k), 1) == OSQP_WORKSPACE_NOT_INIT_ERROR
    assert L.osqp_amd_batch_common_columns(None, abi.iptr(k)) == OSQP_WORKSPACE_NOT_INIT_ERROR
