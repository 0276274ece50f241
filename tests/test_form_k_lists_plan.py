"""Contribution lists of k_form_K_lists as build_resident makes them (engine.hip; through hipeng_resident_plan_lists, no device),
against scipy.  Entry (i, j) of K = P + sigma I + A' rho A sums one term rho_k a_ki a_kj per row k of A that holds both i and j; the
lists say, per entry and in ascending k, where a_ki sits in M = [P | A'] and where a_kj sits in the CSR copy of A."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import osqp_amd
from osqp_amd import _abi as abi
from tests import _form_k_cases as FC
from tests._form_k_reference import _slots
from tests.test_resident_plan import _plan, _qp


def _lists(P, A, nwg=256):
    """(terms or negative code, Kcp, Kcm, Kca)"""
    f = osqp_amd.lib().hipeng_resident_plan_lists
    f.restype = C.c_longlong
    f.argtypes = [C.POINTER(abi.csc), C.POINTER(abi.csc), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    Pu = abi.CscHolder(sparse.triu(P, format="csc")); Ah = abi.CscHolder(A)
    terms = f(C.byref(Pu.struct), C.byref(Ah.struct), nwg, None, None, None, 0)
    if terms < 0:
        return terms, None, None, None
    st, pl = _plan(P, A, nwg)
    Kcp = np.zeros(st[3] + 1, dtype=np.int32); Kcm = np.zeros(max(terms, 1), dtype=np.int32); Kca = np.zeros(max(terms, 1), dtype=np.int32)
    assert f(C.byref(Pu.struct), C.byref(Ah.struct), nwg, Kcp.ctypes.data, Kcm.ctypes.data, Kca.ctypes.data, terms) == terms
    return terms, Kcp, Kcm[:terms], Kca[:terms]


def _check(P, A, nwg=256):
    terms, Kcp, Kcm, Kca = _lists(P, A, nwg)
    assert terms >= 0, terms
    st, pl = _plan(P, A, nwg)
    n, nnzK = P.shape[0], st[3]
    row_of, col_of, m_of, Ac = _slots(P, A)
    # one term per ordered pair of entries of a row of A
    assert terms == int((np.diff(sparse.csr_matrix(A).indptr).astype(np.int64) ** 2).sum())
    assert Kcp[0] == 0 and Kcp[-1] == terms and (np.diff(Kcp) >= 0).all() and len(Kcp) == nnzK + 1
    slot_to_csr = {int(s): q for q, s in enumerate(m_of)}
    rows_in = [Ac.indices[Ac.indptr[j]:Ac.indptr[j + 1]] for j in range(n)]
    empty = 0
    for i in range(n):
        for e in range(pl["Kptr"][i], pl["Kptr"][i + 1]):
            j = int(pl["Kcol"][e])
            cm, ca = Kcm[Kcp[e]:Kcp[e + 1]], Kca[Kcp[e]:Kcp[e + 1]]
            both = np.intersect1d(rows_in[i], rows_in[j])                       # ascending, each row once
            assert np.array_equal(row_of[ca], both), (i, j)
            assert (col_of[ca] == j).all(), (i, j)                              # a_kj in the CSR copy of A
            at = np.array([slot_to_csr[int(s)] for s in cm], dtype=np.int64)    # (a KeyError: not a slot of the A' part of M)
            assert np.array_equal(row_of[at], both) and (col_of[at] == i).all(), (i, j)     # a_ki in M
            empty += len(both) == 0
    return terms, Kcp, Kcm, Kca, empty


@pytest.mark.parametrize("name", FC.PLAN_CASES)
def test_lists_against_scipy_at_the_edges(name, monkeypatch):
    monkeypatch.setenv("OSQP_AMD_RESIDENT_MIN_N", "1")
    P, A = FC.case(name)
    if name == "m0" and _plan(P, A)[0][0] == 0:
        assert _lists(P, A)[0] == -1                   # the plan does not take m = 0: no lists either
        return
    outs = []
    for threads in ("1", "4"):
        monkeypatch.setenv("OSQP_AMD_SETUP_THREADS", threads)
        outs.append(_check(P, A))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    terms, Kcp, _, _, empty = outs[0]
    lens = np.diff(Kcp)
    if name == "n1":
        assert terms == 2 and list(Kcp) == [0, 2]
    if name == "empty_col":
        assert empty > 0                                # (7, 7) at least: it exists through P and sigma alone
    if name == "no_diag":
        assert sparse.csc_matrix(P).diagonal().max() == 0.0
    if name == "col65":
        assert lens.max() == 65                         # the diagonal of that column
    if name == "row65":
        assert terms >= 65 * 65
    if name == "m0":
        assert terms == 0 and not Kcp.any()
    # the new cases say themselves what they are there for (the turns of k_form_K_lists's own loops)
    pl = _plan(P, A)[1]
    FC.check_premise(name, pl["Kptr"], pl["Kcol"], lens)


def test_lists_of_a_mid_size_problem_do_not_depend_on_the_setup_threads(monkeypatch):
    """One chunk of rows per thread (the edge cases above are one chunk in all: build_resident gives a thread 256 rows at least):
    1 and 4 threads, the grid sized by the engine."""
    P, A = _qp(1100, 500, 5, 0.003)
    outs = []
    for threads in ("1", "4"):
        monkeypatch.setenv("OSQP_AMD_SETUP_THREADS", threads)
        outs.append(_check(P, A, -256))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert outs[0][4] > 0                               # entries that P alone brings


def test_switch_and_budget(monkeypatch):
    """OSQP_AMD_FORM_K_LISTS=0 and a budget the lists do not fit (8 bytes per term, 4 per entry of K and one more) leave the
    plan itself as it was and report no lists."""
    P, A = _qp(700, 1100, 9, 0.01)
    st, pl = _plan(P, A)
    terms, Kcp, _, _ = _lists(P, A)
    assert st[0] == 1 and terms > 0
    need = 8 * terms + 4 * (st[3] + 1)
    assert need < (1 << 20)
    monkeypatch.setenv("OSQP_AMD_FORM_K_LISTS", "0")
    assert _lists(P, A)[0] == -2
    monkeypatch.delenv("OSQP_AMD_FORM_K_LISTS")
    monkeypatch.setenv("OSQP_AMD_FORM_K_LIST_MB", "0")
    assert _lists(P, A)[0] == -2
    st0, pl0 = _plan(P, A)
    assert st0 == st and all(np.array_equal(pl0[k], pl[k]) for k in pl)
    monkeypatch.setenv("OSQP_AMD_FORM_K_LIST_MB", "1")
    assert _lists(P, A)[0] == terms
