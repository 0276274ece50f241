"""GPU tests of BatchOSQP.verify / verify_into (osqp_amd_batch_verify in its four forms, k_batch_verify of
osqp_amd/csrc/batch_verify.h): the 16-slot record of a point against the raw problem a handle holds.

Every float slot is held to the rounding bar of tests/_verify_reference.py (a formula of the term counts and the sums of
absolute terms, written there), every verdict to equality: tests/test_verify_reference_host.py proves on the CPU that no
verdict of the cases below sits within 1000 bars of its threshold, that the reference agrees with the CPU oracle, and
that a one-place defect moves some slot by more than ten bars.  The rest are identities, bit for bit: the device form
against the host form, a list against the rows of the whole call, a member alone against the member in its batch, the
handle with and without a verify in between."""
import ctypes as C

import numpy as np
import pytest

import _verify_cases as vc
from _limits_cases import SHAPES
from _members_cases import Device, bits
from _verify_reference import SCALED, assert_matches, batch_reference

pytestmark = pytest.mark.gpu

ENGINE_CASES = ["tile4", "streamed", "common"]
ARRAYS = ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert", "status_polish")


def _same(a, b, what=""):
    assert np.array_equal(bits(np.asarray(a, dtype=np.float64)), bits(np.asarray(b, dtype=np.float64))), what


def _results_same(r1, r2, what=""):
    for k in ARRAYS:
        _same(getattr(r1, k), getattr(r2, k), (what, k))


# ---- 1. given points, no solve ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.GIVEN)
def test_given_points_straight_after_setup(gpu_lib, name):
    h = vc.handle(name)
    pts = vc.points(name)
    try:
        for eps, kw in ((vc.DEFAULT_EPS, {}), (vc.EPS_GIVEN, dict(eps_abs=vc.EPS_GIVEN[0], eps_rel=vc.EPS_GIVEN[1])),
                        ((vc.EPS_GIVEN[0], vc.DEFAULT_EPS[1]), dict(eps_abs=vc.EPS_GIVEN[0]))):
            v = h.verify(*pts, **kw)
            assert_matches(v.V, vc.reference(name, *pts, eps=eps), (name, eps))
        assert v.optimal.dtype == np.bool_ and v.prim_inf.dtype == np.bool_ and v.dual_inf.dtype == np.bool_
        _same(v.obj, v.V[:, 0]); _same(v.gap, v.V[:, 12])
    finally:
        h.cleanup()


def test_per_member_values_equal_to_the_shared_ones_give_the_same_bits(gpu_lib):
    import osqp_amd
    c, pts = vc.case("tile4"), vc.points("tile4")
    B = c["Q"].shape[0]
    h1 = vc.handle("tile4")
    h2 = osqp_amd.BatchOSQP().setup(c["P"], c["A"], c["Q"], c["L"], c["U"], Px_all=np.tile(c["P"].data, (B, 1)),
                                    Ax_all=np.tile(c["A"].data, (B, 1)))
    try:
        _same(h1.verify(*pts).V, h2.verify(*pts).V)
    finally:
        h1.cleanup(); h2.cleanup()


# ---- 2. the handle's own point ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_point_a_solve_ends_at(gpu_lib, name):
    h = vc.handle(name)
    try:
        r = h.solve()
        eps = tuple(e * (1 + 1e-6) for e in vc.DEFAULT_EPS)
        v = h.verify(eps_abs=eps[0], eps_rel=eps[1])
        ref = vc.reference(name, r.x, r.y, r.dual_inf_cert, r.prim_inf_cert, eps=eps)
        assert_matches(v.V, ref, name)
        for k in ref.margin:
            assert ref.margin[k].min() >= 1000.0, (name, k, ref.margin[k].min())
        solved = r.status_val == 1
        assert solved.any() and np.all(v.optimal[solved]), (name, r.status_val.tolist())
        # clamp(A x) is the nearest point of the box, row by row: no z of the box is closer than it
        assert np.all(v.pri_res <= r.pri_res + SCALED * ref.bar[:, 1]), name
        assert np.all(np.abs(v.dua_res - r.dua_res) <= SCALED * ref.bar[:, 2]), (name, np.abs(v.dua_res - r.dua_res).max())
        assert np.all(np.abs(v.obj - r.obj_val) <= SCALED * ref.bar[:, 0]), (name, np.abs(v.obj - r.obj_val).max())
        # the same point given as arrays: the same bits
        _same(h.verify(X=r.x, Y=r.y, DX=r.dual_inf_cert, DY=r.prim_inf_cert, eps_abs=eps[0], eps_rel=eps[1]).V, v.V, name)
    finally:
        h.cleanup()


# ---- 3. the status mix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", vc.MIX_CAPS)
@pytest.mark.parametrize("engine", ["auto", "streamed"])
def test_status_mix(gpu_lib, engine, cap):
    import osqp_amd
    c = vc.status_mix()
    B = c["Q"].shape[0]
    h = osqp_amd.BatchOSQP().setup(c["P"], c["A"], c["Q"], c["L"], c["U"], engine=engine, max_iter=cap)
    try:
        r = h.solve()
        want = {**vc.MIX_WANT, **(vc.MIX_CUT if cap == 50 else {})}
        assert r.status_val.tolist() == [want.get(b, 1) for b in range(B)]
        v = h.verify()
        assert np.array_equal(v.prim_inf, r.status_val == -3) and np.array_equal(v.dual_inf, r.status_val == -4)
        assert not v.optimal[r.status_val < -2].any() and v.optimal[r.status_val == 1].all()
        _same(h.verify(DX=r.dual_inf_cert, DY=r.prim_inf_cert).V, v.V)
        ref = batch_reference(c["P"], c["A"], c["Q"], c["L"], c["U"], r.x, r.y, r.dual_inf_cert, r.prim_inf_cert,
                              *vc.DEFAULT_EPS, *vc.EPS_INF)
        assert_matches(v.V, ref, (engine, cap))
        for k in ref.margin:
            assert ref.margin[k].min() >= 1000.0, (engine, cap, k, ref.margin[k])
        assert np.all(v.V[r.status_val < -2, :13] == vc.OSQP_NAN)
    finally:
        h.cleanup()


# ---- 4. identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENGINE_CASES)
def test_forms_and_lists_give_the_same_bits(gpu_lib, name):
    h = vc.handle(name)
    dev = Device()
    X, Y, DX, DY = vc.points(name)
    B = X.shape[0]
    try:
        whole = h.verify(X, Y, DX, DY).V
        own = h.verify().V                                    # (no solve yet: the zeros of setup)
        out = dev.put(np.full((B + 1, 16), -7.0), rows=B)
        h.verify_into(out, dev.put(X), dev.put(Y), dev.put(DX), dev.put(DY))
        got = out.get()
        _same(got[:B], whole, name)
        assert np.all(got[B] == -7.0), "a row past the batch was written"
        out = dev.put(np.full((B, 16), -7.0))
        h.verify_into(out)
        _same(out.get(), own, name)
        for S in ([0], [B - 1], list(range(1, min(B - 1, 4))), list(range(B))):
            S = np.array(S)
            _same(h.verify(X[S], Y[S], DX[S], DY[S], members=S).V, whole[S], (name, S.tolist()))
            _same(h.verify(members=S).V, own[S], (name, S.tolist()))
            _same(h.verify(X=X[S], DY=DY[S], members=S).V, h.verify(X=X, DY=DY).V[S], (name, S.tolist()))
            out = dev.put(np.full((len(S) + 1, 16), -7.0), rows=len(S))
            h.verify_into(out, dev.put(X[S]), dev.put(Y[S]), dev.put(DX[S]), dev.put(DY[S]), members=S)
            got = out.get()
            _same(got[:len(S)], whole[S], (name, S.tolist()))
            assert np.all(got[len(S)] == -7.0)
    finally:
        dev.close(); h.cleanup()


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_a_member_alone_and_inside_its_batch(gpu_lib, name):
    """The same problem at B = 1 and inside the batch (B = 70 on the common-K engine): the same record."""
    import osqp_amd
    c = vc.case(name)
    X, Y, DX, DY = vc.points(name)
    B = X.shape[0]
    h = vc.handle(name)
    try:
        whole = h.verify(X, Y, DX, DY).V
        for b in (0, B // 2, B - 2):
            one = slice(b, b + 1)
            h1 = osqp_amd.BatchOSQP().setup(c["P"], c["A"], c["Q"][one], c["L"][one], c["U"][one], engine=c["engine"])
            try:
                _same(h1.verify(X[one], Y[one], DX[one], DY[one]).V, whole[one], (name, b))
            finally:
                h1.cleanup()
    finally:
        h.cleanup()


# ---- 5. nothing moves ----------------------------------------------------------------------------------------------------
def _session(name, with_verify):
    """solve, then results, solved_members, kkt_info, polish, adjoint -- with verify in every form in between, or without."""
    extra = dict(shared_kkt=True) if vc.case(name)["engine"] == "common" else {}
    h = vc.handle(name, **extra)
    X, Y, DX, DY = vc.points(name)
    B, n = X.shape
    dev = Device()
    out = []

    def look():
        if with_verify:
            h.verify(); h.verify(X, Y, DX, DY, eps_abs=1e-5); h.verify(X[1:3], Y[1:3], members=[1, 2])
            h.verify_into(dev.put(np.zeros((B, 16))), dev.put(X))
    try:
        h.solve(fetch=False)
        look()
        out.append(h.results())
        out.append(h.solved_members())
        look()
        h.adjoint(np.ones((B, n)))                       # builds the KKT inversion that is kept
        k1 = h.kkt_info()
        look()
        k2 = h.kkt_info()
        assert k1 == k2 and k2.kept
        out.append(h.adjoint(np.ones((B, n))))
        assert h.kkt_info().builds == k1.builds, "the kept inversion was rebuilt"
        look()
        out.append(h.polish())
        look()
        out.append(h.results())
        out.append((tuple(k2), tuple(h.kkt_info())))
        return out
    finally:
        dev.close(); h.cleanup()


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_verify_changes_nothing_in_the_handle(gpu_lib, name):
    a, b = _session(name, False), _session(name, True)
    _results_same(a[0], b[0], "results"); assert np.array_equal(a[1], b[1])
    for k in ("dq", "dl", "du", "active", "status_adjoint"):
        _same(getattr(a[2], k), getattr(b[2], k), ("adjoint", k))
    _results_same(a[3], b[3], "polish"); _results_same(a[4], b[4], "results after polish")
    assert a[5] == b[5], "kkt_info"


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_a_refused_call_changes_nothing(gpu_lib, name):
    from osqp_amd import abi
    from osqp_amd.batch import _p
    h = vc.handle(name)
    X, Y, DX, DY = vc.points(name)
    B = X.shape[0]
    dev = Device()
    try:
        r0 = h.solve()
        before = h.verify(X, Y, DX, DY).V
        L, hh = h._lib, h._h
        V = np.full((B, 16), -7.0)
        null_f, nan, inf = C.cast(None, abi.c_float_p), float("nan"), float("inf")
        xs = [_p(a) for a in (X, Y, DX, DY)]
        assert L.osqp_amd_batch_verify(hh, *xs, -1.0, -1.0, null_f) == 1
        for eps in ((nan, 1e-3), (1e-3, nan), (inf, 1e-3), (1e-3, -inf)):
            assert L.osqp_amd_batch_verify(hh, *xs, *eps, abi.fptr(V)) == 1, eps
        for lst, cnt in (([1, 1], 2), ([2, 1], 2), ([0, B], 2), ([-1], 1), ([0], 0), (list(range(B)) + [B], B + 1)):
            a = np.array(lst, np.int64)
            assert L.osqp_amd_batch_verify_members(hh, abi.iptr(a), cnt, *xs, -1.0, -1.0, abi.fptr(V)) == 1, lst
            assert L.osqp_amd_batch_verify_members_dev(hh, abi.iptr(a), cnt, None, None, None, None, -1.0, -1.0, None) == 1, lst
        assert L.osqp_amd_batch_verify_members(hh, C.cast(None, abi.c_int_p), 2, *xs, -1.0, -1.0, abi.fptr(V)) == 1
        dV = dev.put(V)
        assert L.osqp_amd_batch_verify_dev(hh, X.ctypes.data, None, None, None, -1.0, -1.0, dV.ptr) == 1      # a host pointer
        assert L.osqp_amd_batch_verify_dev(hh, None, None, None, None, -1.0, -1.0, V.ctypes.data) == 1
        assert L.osqp_amd_batch_verify_dev(hh, None, None, None, None, nan, -1.0, dV.ptr) == 1
        assert L.osqp_amd_batch_verify_dev(hh, None, None, None, None, -1.0, -1.0, None) == 1
        assert np.all(V == -7.0) and np.all(dV.get() == -7.0), "a refused call wrote its output"
        _results_same(h.results(), r0)
        _same(h.verify(X, Y, DX, DY).V, before)
    finally:
        dev.close(); h.cleanup()


# ---- 6. the data follows the updates ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENGINE_CASES)
def test_update_of_chosen_members(gpu_lib, name):
    c = vc.case(name)
    pts = vc.points(name)
    B = pts[0].shape[0]
    S = np.array([1, B - 2])
    h = vc.handle(name)
    try:
        before = h.verify(*pts).V
        Q = c["Q"].copy()
        Q[S] = Q[S] * 1.5 + 0.25
        assert h.update(Q=Q[S], members=S) == 0
        after = h.verify(*pts).V
        assert_matches(after, vc.reference(name, *pts, Q=Q), name)
        rest = np.setdiff1d(np.arange(B), S)
        _same(after[rest], before[rest], name)
        assert not np.array_equal(after[S, 0], before[S, 0])
    finally:
        h.cleanup()


def test_update_matrices_of_chosen_members_streamed(gpu_lib):
    name = "streamed"
    c = vc.case(name)
    pts = vc.points(name)
    B = pts[0].shape[0]
    S = np.array([0, 3])
    h = vc.handle(name)
    try:
        before = h.verify(*pts).V
        Ax_all = np.tile(c["A"].data, (B, 1))
        Ax_all[S] *= np.random.default_rng(5).uniform(0.8, 1.2, (len(S), c["A"].nnz))
        assert h.update_matrices(Ax=Ax_all[S], members=S) == 0
        after = h.verify(*pts).V
        assert_matches(after, vc.reference(name, *pts, Px_all=np.tile(c["P"].data, (B, 1)), Ax_all=Ax_all), name)
        rest = np.setdiff1d(np.arange(B), S)
        _same(after[rest], before[rest], name)
        assert not np.array_equal(after[S, 1], before[S, 1])
    finally:
        h.cleanup()


def test_update_model_common(gpu_lib):
    name = "common"
    c = vc.case(name)
    pts = vc.points(name)
    B = pts[0].shape[0]
    h = vc.handle(name)
    try:
        before = h.verify(*pts).V
        Px = c["P"].data * np.random.default_rng(6).uniform(1.0, 1.2, c["P"].nnz)
        assert h.update_model(Px=Px) == 0
        after = h.verify(*pts).V
        assert_matches(after, vc.reference(name, *pts, Px_all=np.tile(Px, (B, 1)), Ax_all=np.tile(c["A"].data, (B, 1))), name)
        _same(after[:, [1, 3, 4, 6, 7, 10]], before[:, [1, 3, 4, 6, 7, 10]])       # what P does not enter keeps its bits
        assert not np.array_equal(after[:, 0], before[:, 0])
    finally:
        h.cleanup()
