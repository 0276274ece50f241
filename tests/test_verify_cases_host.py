"""What tests/test_gpu_verify.py leans on, proved on the CPU: the sparse long-double restatement of the 16 slots
(tests/_verify_sparse_reference.py) is the dense one (tests/_verify_reference.py) wherever the dense one can be formed; it
agrees with the CPU oracle where the two compute the same thing; every case is what tests/_verify_single_cases.py says it is;
no verdict of a device case sits near its threshold; the bars are tight enough to see each one-place defect on the case
meant to catch it; and the two entry points are exported with the header's signatures.

The two references add the same long-double terms in different orders and return float64.  Their sums (`sums`, long
double) agree to 1e-18 of the sum of the absolute terms.  A cast value can therefore differ by the one unit in the last
place a rounding boundary between them costs: `val` is held to 1e-18 relative plus that unit (2^-52), `bar` likewise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _verify_single_cases as sc
from _verify_reference import FIELDS, SCALED, reference as dense_reference
from _verify_sparse_reference import reference as sparse_reference

MARGIN = 1000.0          # bars between every verdict comparison of a device case and its threshold
SEEN = 10.0              # bars a planted defect has to move some slot by
DENSE_OK = [n for n in sc.NAMES if n not in ("trip", "random")]      # n <= 1500: the dense matrices fit
ULP = 2.0 ** -52


def _args(c):
    P, A, e = c["P"], c["A"], sc.eps_of(c)
    return (A.shape[1], A.shape[0], P.indptr, P.indices, P.data, A.indptr, A.indices, A.data, c["q"], c["l"], c["u"], c["x"], c["y"],
            c["dx"], c["dy"], e[0], e[1], *sc.EPS_INF)


def _moved(r, true):
    return np.abs(r.val[:13] - true.val[:13]) / np.where(true.bar[:13] > 0, true.bar[:13], np.inf)


def test_constants_and_sizes():
    k = sc.constants()
    assert k["NT"] % 64 == 0 and k["ROWS"] == k["NT"] // 64 and k["CAP"] >= 1 and k["LONG"] >= 130, k
    c = sc.case("trip")
    n, m = c["A"].shape[1], c["A"].shape[0]
    sweep = k["CAP"] * k["ROWS"]
    assert n == m == sweep + 1 and sc.grid(n, m) == k["CAP"]       # one row and one column past a single sweep of the capped grid
    for name in sc.NAMES:
        c = sc.case(name)
        assert c["P"].has_sorted_indices and c["A"].has_sorted_indices and (c["P"].indices <= np.repeat(np.arange(c["P"].shape[0]), np.diff(c["P"].indptr))).all()
        assert np.all(c["l"] <= c["u"]), name


def test_structure_and_length_cases_are_what_they_claim():
    c = sc.case("structure")
    P, A = c["P"], c["A"]
    assert A.shape == (30, 40) and np.diff(A.indptr)[39] == 0 and not np.any(A.indices == 7)
    assert P[38, 38] == 0 and np.diff(P.indptr)[38] == 1
    assert np.count_nonzero(P.data == 0) == 2 and np.count_nonzero(A.data == 0) == 2
    assert sc.case("structure_noP")["P"].nnz == 0
    D = sc.case("structure_diagP")["P"]
    assert D.nnz == 40 and np.array_equal(D.indices, np.arange(40))
    c, Ls = sc.case("lengths"), sc.lengths()
    L = sc.constants()["LONG"]
    assert Ls[-3:] == (L - 1, L, L + 1)
    P, A = c["P"], c["A"]
    assert A.shape == (700, 1500)
    full = (P + P.T).tocsr()          # (the diagonal is stored: the pattern of the sum is the symmetric pattern)
    assert tuple(np.diff(A.tocsr().indptr)[:9]) == Ls and tuple(np.diff(A.indptr)[:9]) == Ls and tuple(np.diff(full.indptr)[:9]) == Ls
    r = sc.reference("inf_zero")
    assert np.all(np.abs(r.val[10:13]) < 1e29)
    r = sc.reference("inf_nonzero")
    assert r.val[10] == 1e30 and r.val[11] == -1e30 and r.val[12] == 1e30
    for v in ("x", "y"):
        for kind in ("nan", "osqpnan"):
            r = sc.reference("%s_%s" % (kind, v))
            assert np.all(r.val[:13] == sc.OSQP_NAN) and r.val[13] == 0.0
    want = dict(pinf_true=(1.0, 0.0), pinf_spoiled=(0.0, 0.0), pinf_zero=(0.0, 0.0), dinf_true=(0.0, 1.0), dinf_spoiled=(0.0, 0.0),
                dinf_zero=(0.0, 0.0), nan_dy=(0.0, 0.0), osqpnan_dx=(0.0, 0.0))
    for name, (pi, di) in want.items():
        r = sc.reference(name)
        assert (r.val[14], r.val[15]) == (pi, di), (name, r.val[13:])
    assert sc.reference("loose").val[13] == 1.0


@pytest.mark.parametrize("name", DENSE_OK)
def test_sparse_reference_is_the_dense_one(name):
    c = sc.case(name)
    a, b = sparse_reference(*_args(c)), dense_reference(*_args(c))
    assert np.array_equal(a.val[13:], b.val[13:]), name
    tol = lambda v: (1e-18 + ULP) * np.abs(v)
    assert np.all(np.abs(a.val[:13] - b.val[:13]) <= tol(b.val[:13])), (name, a.val, b.val)
    kmax = max(int(np.diff(c["A"].indptr).max(initial=0)), int(np.diff(c["A"].tocsr().indptr).max(initial=0)), c["P"].nnz * 2 + 2 * c["A"].shape[0] + c["A"].shape[1])
    if kmax < 2048:
        assert np.all(np.abs(a.bar - b.bar) <= tol(b.bar)), (name, a.bar, b.bar)
    else:                             # (a sum of 2048 terms or more: its bar is the dense one's or wider, by less than 1 part in 2048)
        assert np.all(a.bar >= b.bar * (1 - ULP)) and np.all(a.bar <= b.bar * (1 + 1.0 / 2048)), (name, a.bar, b.bar)
    for key in b.sums:
        assert abs(a.sums[key][0] - b.sums[key][0]) <= 1e-18 * float(b.sums[key][1]), (name, key)
        assert a.sums[key][2] == b.sums[key][2], (name, key)
    for key in b.margin:
        assert np.isclose(a.margin[key], b.margin[key], rtol=1e-9) or a.margin[key] == b.margin[key], (name, key, a.margin[key], b.margin[key])


@pytest.mark.parametrize("name", ["e65", "e257"])
def test_reference_agrees_with_the_oracle_on_a_solved_run(oracle_mod, name):
    """obj and dua_res are the oracle's info.obj_val and info.dua_res -- the same sums, formed there in the scaled space:
    within SCALED bars; pri_res is the distance of A x to the box, the oracle's is the distance to its own z in the box."""
    c = sc.case(name)
    ro = oracle_mod.OracleOSQP().setup(P=c["P"], q=c["q"], A=c["A"], l=c["l"], u=c["u"]).solve()
    assert ro.info.status_val == 1
    r = sc.reference_of(dict(c, x=ro.x, y=ro.y, dx=ro.dual_inf_cert, dy=ro.prim_inf_cert))
    assert abs(r.val[0] - ro.info.obj_val) <= SCALED * r.bar[0], (r.val[0], ro.info.obj_val)
    assert abs(r.val[2] - ro.info.dua_res) <= SCALED * r.bar[2], (r.val[2], ro.info.dua_res)
    assert r.val[1] <= ro.info.pri_res + SCALED * r.bar[1]
    assert r.val[13] == 1.0 and r.val[14] == 0.0 and r.val[15] == 0.0
    assert min(r.margin.values()) >= MARGIN, r.margin


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_verdict_is_far_from_its_threshold(name):
    r = sc.reference(name)
    for k, g in r.margin.items():
        assert g >= MARGIN, (name, k, g)


def test_after_each_update_the_verdicts_stay_far_and_stale_data_shows():
    """The update tests of the device file run on e65: every verdict on the new data is MARGIN bars from its threshold, and
    a record computed from the old part (a stale q after update_lin_cost, stale Ax after update_A, ...) is more than SEEN
    bars from the true one."""
    c = sc.case("e65")
    for what in sc.UPDATES:
        for partial in ((False, True) if what in ("P", "A", "P_A") else (False,)):
            _, new = sc.update_data(c, what, partial)
            true = sc.reference_of(new)
            assert min(true.margin.values()) >= MARGIN, (what, true.margin)
            for part in {"lin_cost": "q", "bounds": "lu", "lower_bound": "l", "upper_bound": "u", "P": "P", "A": "A", "P_A": "PA"}[what]:
                stale = sc.reference_of(dict(new, **{part: c[part]}))
                assert _moved(stale, true).max() > SEEN, (what, partial, part, _moved(stale, true).max())


def test_a_one_place_defect_moves_a_slot_by_more_than_ten_bars():
    """One value of P, one of A, one q_j, one bound, one half of a symmetric pair of P dropped (on e65); the last entry of a
    row with LONG + 1 entries dropped -- a row of A, a column of A, a row of the symmetric P (on lengths); the last row and
    the last column of the second grid trip never reached (on trip)."""
    c = sc.case("e65")
    P, A, x, y = c["P"], c["A"], c["x"], c["y"]
    n = P.shape[0]
    true = sc.reference("e65")
    assert np.all(np.abs(true.val[10:13]) < 1e29), "finite slots 10-12, so a bound shows in them"
    cols = np.repeat(np.arange(n), np.diff(P.indptr))
    offd = np.flatnonzero((P.indices != cols) & (x[P.indices] != 0) & (x[cols] != 0))
    kP = offd[np.argmax(np.abs(P.data[offd]))]
    acols = np.repeat(np.arange(n), np.diff(A.indptr))
    imax = int(np.argmax(np.abs(A @ x)))             # a value of A shows in maxima alone: take one in the row that attains |A x|oo
    kA = int(np.argmax(np.abs(A.data * x[acols]) * (A.indices == imax)))
    row = np.flatnonzero((y > 0) & (c["u"] < 1e26))[0]
    bump = lambda a, k: np.concatenate([a[:k], [a[k] * (1 + 1e-6)], a[k + 1:]])

    def mat(M, k):
        M = M.copy(); M.data = bump(M.data, k)
        return M
    defects = {
        "a value of P": sc.reference_of(dict(c, P=mat(P, kP))),
        "a value of A": sc.reference_of(dict(c, A=mat(A, kA))),
        "q_j": sc.reference_of(dict(c, q=bump(c["q"], int(np.argmax(np.abs(c["q"] * x)))))),
        "a bound": sc.reference_of(dict(c, u=bump(c["u"], row))),
        "half of a symmetric pair of P": sc.reference_of(c, drop=(int(P.indices[kP]), int(cols[kP]))),
    }
    for what, r in defects.items():
        assert _moved(r, true).max() > SEEN, (what, _moved(r, true).max())

    c, true = sc.case("lengths"), sc.reference("lengths")
    A, P = c["A"], c["P"]
    Acsr = A.tocsr()
    acols = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    last_in_row = int(np.flatnonzero((A.indices == 8) & (acols == Acsr.indices[Acsr.indptr[9] - 1]))[0])
    last_in_col = int(A.indptr[9] - 1)
    pcols = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    jlast = int(pcols[P.indices == 8].max())

    def zero(M, k):
        M = M.copy(); M.data = M.data.copy(); M.data[k] = 0.0
        return M
    long_defects = {
        "the last entry of a long row of A": sc.reference_of(dict(c, A=zero(A, last_in_row))),
        "the last entry of a long column of A": sc.reference_of(dict(c, A=zero(A, last_in_col))),
        "the last entry of a long row of P": sc.reference_of(c, drop_at=(8, jlast)),
    }
    for what, r in long_defects.items():
        assert _moved(r, true).max() > SEEN, (what, _moved(r, true).max())

    c, true = sc.case("trip"), sc.reference("trip")
    n, m = c["A"].shape[1], c["A"].shape[0]
    for what, r in {"the last row of the second trip": sc.reference_of(c, skip_row=m - 1),
                    "the last column of the second trip": sc.reference_of(c, skip_col=n - 1)}.items():
        assert _moved(r, true).max() > SEEN, (what, _moved(r, true).max())


def _header_args(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "osqp_amd.h")).read()
    m = re.search(r"c_int\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_are_exported_with_the_header_signatures():
    import osqp_amd
    from osqp_amd import _abi as abi
    api = abi.bind_api(osqp_amd.lib())
    W = C.POINTER(abi.OSQPWorkspace)

    def ctype(decl):
        if decl.startswith("OSQPWorkspace *"):
            return W
        if "c_float" in decl:
            return abi.c_float_p if ("*" in decl or "[" in decl) else abi.c_float
        assert "c_int" in decl and "[" in decl, decl
        return abi.c_int_p
    for key, name in (("verify", "osqp_amd_verify"), ("verify_info", "osqp_amd_verify_info")):
        assert hasattr(osqp_amd.lib(), name)
        assert api[key].restype is abi.c_int and list(api[key].argtypes) == [ctype(a) for a in _header_args(name)], (name, _header_args(name))
    assert _header_args("osqp_amd_verify")[-1] == "c_float V[16]" and FIELDS == osqp_amd.batch.VERIFY_FIELDS and len(FIELDS) == 16


def test_a_null_workspace_is_refused():
    import osqp_amd
    from osqp_amd import _abi as abi
    api = abi.bind_api(osqp_amd.lib())
    V, out = np.full(16, 7.5), np.full(4, 9, np.int64)
    null = C.POINTER(abi.OSQPWorkspace)()
    nf = C.cast(None, abi.c_float_p)
    assert api["verify"](null, nf, nf, nf, nf, -1.0, -1.0, abi.fptr(V)) == 7          # OSQP_WORKSPACE_NOT_INIT_ERROR
    assert api["verify_info"](null, abi.iptr(out)) == 7
    assert np.all(V == 7.5) and np.all(out == 9)
