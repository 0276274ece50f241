"""What tests/test_gpu_batch_verify.py leans on, proved on the CPU: the long-double restatement of the 16 slots
(tests/_verify_reference.py) agrees with the CPU oracle where the two compute the same thing; no verdict of a case the
device tests use sits near its threshold; and the bars are tight enough to see a one-place defect."""
import numpy as np
import pytest

import _verify_cases as vc
from _limits_cases import SHAPES
from _verify_reference import SCALED, batch_reference, reference

MARGIN = 1000.0          # bars between every verdict comparison of a device case and its threshold
SEEN = 10.0              # bars a planted defect has to move some slot by
MIX_CAPS = vc.MIX_CAPS


def _oracle_points(orc, c, **kw):
    """The CPU oracle's x, y, certificates and info per member of the batch c."""
    B = c["Q"].shape[0]
    Px, Ax = c.get("Px_all"), c.get("Ax_all")
    out = []
    for b in range(B):
        P, A = c["P"].copy(), c["A"].copy()
        if Px is not None:
            P.data[:], A.data[:] = Px[b], Ax[b]
        out.append(orc.OracleOSQP().setup(P=P, q=c["Q"][b], A=A, l=c["L"][b], u=c["U"][b], **kw).solve())
    arr = lambda f: np.array([f(ro) for ro in out])
    return out, (arr(lambda ro: ro.x), arr(lambda ro: ro.y), arr(lambda ro: ro.dual_inf_cert), arr(lambda ro: ro.prim_inf_cert))


def _ref(c, pts, eps=vc.DEFAULT_EPS):
    return batch_reference(c["P"], c["A"], c["Q"], c["L"], c["U"], *pts, eps[0], eps[1], *vc.EPS_INF,
                           Px_all=c.get("Px_all"), Ax_all=c.get("Ax_all"))


@pytest.mark.parametrize("name", ["tile4", "streamed", "63x65"])
def test_reference_agrees_with_the_oracle_on_a_solved_run(oracle_mod, name):
    """obj and dua_res are the oracle's info.obj_val and info.dua_res -- the same sums, formed there in the scaled space:
    within SCALED bars; pri_res is the distance of A x to the box, the oracle's is the distance to its own z in the box."""
    c = vc.case(name)
    ros, pts = _oracle_points(oracle_mod, c)
    r = _ref(c, pts)
    for b, ro in enumerate(ros):
        assert ro.info.status_val == 1, (name, b)
        assert abs(r.val[b, 0] - ro.info.obj_val) <= SCALED * r.bar[b, 0], (name, b, r.val[b, 0], ro.info.obj_val)
        assert abs(r.val[b, 2] - ro.info.dua_res) <= SCALED * r.bar[b, 2], (name, b, r.val[b, 2], ro.info.dua_res)
        assert r.val[b, 1] <= ro.info.pri_res + SCALED * r.bar[b, 1], (name, b)
        assert r.val[b, 13] == 1.0 and r.val[b, 14] == 0.0 and r.val[b, 15] == 0.0, (name, b)


@pytest.mark.parametrize("cap", MIX_CAPS)
def test_certificate_verdicts_agree_with_the_oracle_status(oracle_mod, cap):
    c = vc.status_mix()
    ros, pts = _oracle_points(oracle_mod, c, max_iter=cap)
    r = _ref(c, pts)
    status = np.array([ro.info.status_val for ro in ros])
    want = {**vc.MIX_WANT, **(vc.MIX_CUT if cap == 50 else {})}
    assert status.tolist() == [want.get(b, 1) for b in range(len(ros))]
    assert np.array_equal(r.val[:, 14] == 1.0, status == -3)
    assert np.array_equal(r.val[:, 15] == 1.0, status == -4)
    assert not np.any(r.val[status < -2, 13])
    assert np.all(r.val[status == 1, 13] == 1.0)
    for k in r.margin:
        assert r.margin[k].min() >= MARGIN, (k, r.margin[k])


@pytest.mark.parametrize("name", vc.GIVEN)
def test_given_points_keep_every_verdict_away_from_its_threshold(name):
    c = vc.case(name)
    pts = vc.points(name)
    for eps in (vc.DEFAULT_EPS, vc.EPS_GIVEN):
        r = vc.reference(name, *pts, eps=eps)
        for k in r.margin:
            assert r.margin[k].min() >= MARGIN, (name, eps, k, r.margin[k])
    # the cases cover what they are there for: finite and infinite slots 10-12, both kinds of NaN
    B = c["Q"].shape[0]
    if c["A"].shape[0] and B >= 3 and np.any(c["U"] > 1e26):
        assert np.any(r.val[:, 10] == 1e30) and np.any(np.abs(r.val[:, 10]) < 1e29), name
    if B >= 3:
        assert np.all(r.val[B - 1, :13] == vc.OSQP_NAN) and r.val[B - 1, 13] == 0.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_solved_points_keep_every_verdict_away_from_its_threshold(oracle_mod, name):
    """The device tests verify the point each engine's own solve ends at.  The oracle's point stands for it here: the
    engines' parity tests hold x and y to 1e-6 of it, and the margins below are ten orders above the bar."""
    c = vc.case(name)
    kw = dict(adaptive_rho=0) if c["engine"] == "common" else {}
    B = min(c["Q"].shape[0], 8)
    sub = {k: (v[:B] if k in "QLU" else v) for k, v in c.items()}
    ros, pts = _oracle_points(oracle_mod, sub, **kw)
    r = _ref(sub, pts, eps=tuple(e * (1 + 1e-6) for e in vc.DEFAULT_EPS))
    assert all(ro.info.status_val == 1 for ro in ros)
    assert np.all(r.val[:, 13] == 1.0)
    for k in r.margin:
        assert r.margin[k].min() >= MARGIN, (name, k, r.margin[k])


@pytest.mark.parametrize("name", ["tile4", "streamed", "common"])
def test_a_one_place_defect_moves_a_slot_by_more_than_ten_bars(name):
    """One value of P, one of A, one q_j, one bound, one half of a symmetric pair of P dropped: each, applied to the
    reference's inputs for member 0 at the case's given point, moves some slot past SEEN bars of the true record.  A
    kernel that made the same mistake would fail the device test."""
    c = vc.case(name)
    X, Y, DX, DY = vc.points(name)
    P, A = c["P"], c["A"]
    n, m = P.shape[0], A.shape[0]
    x, y = X[0], Y[0]

    def run(Px=P.data, Ax=A.data, q=c["Q"][0], l=c["L"][0], u=c["U"][0], drop=None):
        return reference(n, m, P.indptr, P.indices, Px, A.indptr, A.indices, Ax, q, l, u, x, y, DX[0], DY[0],
                         *vc.DEFAULT_EPS, *vc.EPS_INF, drop=drop)
    true = run()
    assert np.all(np.abs(true.val[10:13]) < 1e29), "member 0 has finite slots 10-12, so a bound shows in them"
    cols = np.repeat(np.arange(n), np.diff(P.indptr))
    offd = np.flatnonzero((P.indices != cols) & (x[P.indices] != 0) & (x[cols] != 0))
    kP = offd[np.argmax(np.abs(P.data[offd]))]
    acols = np.repeat(np.arange(n), np.diff(A.indptr))
    kA = np.argmax(np.abs(A.data * x[acols]))
    row = np.flatnonzero((y > 0) & (c["U"][0] < 1e26))[0]
    bump = lambda a, k: np.concatenate([a[:k], [a[k] * (1 + 1e-6)], a[k + 1:]])
    defects = {
        "a value of P": run(Px=bump(P.data, kP)),
        "a value of A": run(Ax=bump(A.data, kA)),
        "q_j": run(q=bump(c["Q"][0], int(np.argmax(np.abs(c["Q"][0] * x))))),
        "a bound": run(u=bump(c["U"][0], row)),
        "half of a symmetric pair of P": run(drop=(int(P.indices[kP]), int(cols[kP]))),
    }
    for what, r in defects.items():
        moved = np.abs(r.val[:13] - true.val[:13]) / np.where(true.bar[:13] > 0, true.bar[:13], np.inf)
        assert moved.max() > SEEN, (name, what, moved.max())
