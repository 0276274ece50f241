"""GPU tests of `BatchOSQP.update_model` (osqp_amd_batch_common_update_model(_dev), `bc_update_model` in batch.hip, k_bc_qhat
and k_bc_rescale in batch_common.h): new values for the shared model of a live common-K handle.

Yardsticks, none of them the call itself: a FRESH handle set up on the new values, to the bit, wherever the call is made
before any solve and no row changes its class under the new E (tests/test_common_model_cases_host.py shows that for every
shape used here) -- the call then has to leave exactly what setup leaves; tests/_common_model_cases.ModelReference, the
batch loop in long double with the call as the header states it, where iterates, rho and counts are carried over the
call, under the bars of test_gpu_batch_common_loop.py (status, iter, rho_updates identical; x, y 1e-6; objective 1e-8;
rho RHO_BAR); the streamed engine's layer on per-member copies of the values for the gradients (relative 1e-6, the bar
of the layer tests)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _common_kkt_reference as kr
from _batch_parity import rel
from _common_cases import ADAPTIVE
from _common_model_cases import BITS, LAYER_SHAPE, MODEL_CASES, bits_case, model_reference, qhat_test_q, sorted_model
from _common_reference import RHO_BAR
from test_gpu_batch_common_loop import _assert_loop_parity

pytestmark = pytest.mark.gpu

RESULT = ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert")
GRADS = ("dq", "dl", "du", "dPx", "dAx")
WORKSPACE = ("D", "E", "c", "ctype", "Pv", "Av", "Kinv", "rho")
HERE = os.path.dirname(os.path.abspath(__file__))


def _handle(P, A, Q, L, U, shared=True, engine="common", **kw):
    import osqp_amd
    extra = dict(shared_kkt=shared) if engine == "common" else {}
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine, **extra, **kw)


def _same(a, b, fields=RESULT):
    return all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) for k in fields)


def _assert_same_handles(h, f, what, shared=True, calls=True):
    """Everything a test can read of handle h equals handle f, to the bit: the workspace of every member, the shared
    pieces, and (calls) a solve, polish, adjoint and tangent on both."""
    for b in range(h.B):
        w, wf = h.member_workspace(b), f.member_workspace(b)
        for k in WORKSPACE:
            assert np.array_equal(w[k], wf[k]), (what, "member", b, k)
    if shared:
        pk, pf = h.shared_kkt_peek(), f.shared_kkt_peek()
        assert np.array_equal(pk["H"], pf["H"]) and np.array_equal(pk["Wt"], pf["Wt"]), (what, "H / Wt")
    if not calls:
        return
    r, rf = h.solve(), f.solve()
    assert _same(r, rf), (what, "solve")
    if shared:
        rng = np.random.default_rng(3)
        gx, gy = rng.standard_normal((h.B, h.n)), rng.standard_normal((h.B, h.m))
        assert _same(h.polish(), f.polish(), RESULT + ("status_polish",)), (what, "polish")
        assert _same(h.adjoint(gx, gy, matrices=True), f.adjoint(gx, gy, matrices=True), GRADS + ("active", "status_adjoint")), (what, "adjoint")
        assert _same(h.tangent(dQ=gx, dL=gy, dU=gy), f.tangent(dQ=gx, dL=gy, dU=gy), ("dx", "dy", "active", "status_tangent")), (what, "tangent")
    return r


def _case(n, m, B):
    c = bits_case((n, m, B), "full")
    return c["P0"], c["A0"], c["P2"], c["A2"], c["Px"], c["Ax"], c["Q"], c["L"], c["U"]


# ---- 1. the call before any solve equals a fresh setup, to the bit -------------------------------------------------------
@pytest.mark.parametrize("shape,mode,shared", BITS, ids=lambda v: str(v).replace(" ", ""))
def test_equals_a_fresh_setup(gpu_lib, shape, mode, shared):
    c = bits_case(shape, mode)
    h = _handle(c["P0"], c["A0"], c["Q"], c["L"], c["U"], shared=shared, **ADAPTIVE)
    before = h.member_workspace(0)
    assert h.update_model(**c["kw"]) == 0
    assert shape[0] == 1 or not np.array_equal(before["D"], h.member_workspace(0)["D"])      # the scaling really moves
    f = _handle(c["P2"], c["A2"], c["Q"], c["L"], c["U"], shared=shared, **ADAPTIVE)
    r = _assert_same_handles(h, f, (shape, mode), shared)
    assert np.all(r.status_val == 1), r.status_val       # polish, adjoint and tangent had every member to work on


def test_two_pivot_sequences_give_the_same_bits(gpu_lib, monkeypatch):
    """With the shared pieces the call inverts K and P~ + delta I side by side (k_bc_pivot2); OSQP_AMD_BATCH_MODEL_PIVOT2=0,
    read at setup, runs bc_rebuild's and osqp_amd_batch_common_kkt's own sequences instead.  (300, 600): two column blocks."""
    c = bits_case((300, 600, 5), "full")
    monkeypatch.setenv("OSQP_AMD_BATCH_MODEL_PIVOT2", "0")
    h = _handle(c["P0"], c["A0"], c["Q"], c["L"], c["U"], **ADAPTIVE)
    monkeypatch.delenv("OSQP_AMD_BATCH_MODEL_PIVOT2")
    h2 = _handle(c["P0"], c["A0"], c["Q"], c["L"], c["U"], **ADAPTIVE)
    assert h.update_model(**c["kw"]) == 0 and h2.update_model(**c["kw"]) == 0
    _assert_same_handles(h, h2, "two pivot sequences against k_bc_pivot2", calls=False)
    _assert_same_handles(h, _handle(c["P2"], c["A2"], c["Q"], c["L"], c["U"], **ADAPTIVE), "two pivot sequences against a fresh handle")


# ---- the device route (torch: a process of its own) --------------------------------------------------------------------
_worker_out = {}


def _worker(tmp_path_factory, mode, inputs=None):
    if mode not in _worker_out:
        tmp = tmp_path_factory.mktemp("common_model_" + mode)
        args = [str(tmp / "out.npz")]
        if inputs is not None:
            np.savez(tmp / "in.npz", **inputs)
            args = [str(tmp / "in.npz")] + args
        p = subprocess.run([sys.executable, os.path.join(HERE, "_common_model_worker.py"), mode] + args, capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        _worker_out[mode] = dict(np.load(tmp / "out.npz"))
    return _worker_out[mode]


def test_device_route_equals_host_route(gpu_lib, tmp_path_factory):
    o = _worker(tmp_path_factory, "dev")
    assert o["rc"].tolist() == [0, 0] and o["rc_idx"].tolist() == [0, 0]
    keys = [k[2:] for k in o if k.startswith("h_")]
    assert len(keys) > 30
    for k in keys:
        assert np.array_equal(o["h_" + k], o["d_" + k]), k
    assert not np.array_equal(o["h_full_H"], o["h_idx_H"])               # (the second call moved the model again)
    assert np.all(o["h_info_raw"][:, 0] > 0)
    # a host pointer is refused and a [B, k] tensor raises; neither writes anything
    assert o["bad_pointer"][0] == 1 and "common" in str(o["two_d"][0])
    for k in o:
        if k.startswith("d_after_ws") and not k.endswith(("Kinv", "rho")):      # (the solve in between has moved rho)
            assert np.array_equal(o[k], o[k.replace("d_after", "d_idx")]), k


# ---- 2. q^ follows update ------------------------------------------------------------------------------------------------
def test_qhat_follows_update(gpu_lib):
    Pu, A, P2, A2, Px, Ax, Q, L, U = _case(33, 66, 5)
    Q2 = qhat_test_q(Q)
    h = _handle(Pu, A, Q, L, U, **ADAPTIVE)
    before = h.member_workspace(0)
    assert h.update(Q=Q2) == 0
    kept = h.member_workspace(0)
    assert all(np.array_equal(before[k], kept[k]) for k in ("D", "E", "c"))      # update keeps the scaling ...
    assert h.update_model(Px=Px, Ax=Ax) == 0
    f = _handle(P2, A2, Q2, L, U, **ADAPTIVE)
    stale = _handle(P2, A2, Q, L, U, **ADAPTIVE).member_workspace(0)
    assert stale["c"] != f.member_workspace(0)["c"]                          # ... and q^ matters to the new one
    _assert_same_handles(h, f, "q^ of the Q given by update")


# ---- 3. iterates, rho and counts are kept; 4. classes stay -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODEL_CASES))
def test_iterates_rho_and_counts_are_kept(gpu_lib, oracle_mod, name):
    c, _, (r1, r2), _ = model_reference(oracle_mod, name)
    h = _handle(c["Pu"], c["A"], c["Q"], c["L"], c["U"], **c["kw"])
    if c["Q2"] is not c["Q"]:
        assert h.update(Q=c["Q2"]) == 0
    g1 = h.solve()
    _assert_loop_parity(g1, r1, name + ", first solve")
    assert np.all(g1.rho_updates >= 1) and set(g1.status_val.tolist()) <= {-2, 2}
    before = h.member_workspace(0)
    assert h.update_model(Px=c["Px"], Ax=c["Ax"]) == 0
    after = h.member_workspace(0)
    assert after["rho"] == before["rho"] != c["ws_old"]["rho"]                 # the adapted rho, not the setting
    assert np.array_equal(after["ctype"], before["ctype"])
    assert not np.array_equal(after["E"], before["E"])
    g2 = h.solve()
    _assert_loop_parity(g2, r2, name + ", second solve")
    assert np.array_equal(g2.rho_updates, np.full(c["B"], len(r2.moves)))       # the count restarted from 0
    if c["row"] is None:
        return
    # the crossing row: an equality row before and after the call, an inequality row once an update with bounds classifies
    # under the new E; K follows at the next solve
    row = c["row"]
    assert before["ctype"][row] == 1 and after["ctype"][row] == 1
    assert h.update(L=c["L"], U=c["U"]) == 0
    h.solve(fetch=False)
    w = h.member_workspace(c["B"] - 1)
    assert w["ctype"][row] == 0 and np.array_equal(np.delete(w["ctype"], row), np.delete(before["ctype"], row))
    Ps, As = kr.scaled_dense(c["Pu"], c["A"], w)
    n = h.n
    rho_vec = np.where(w["ctype"] == -1, 1e-6, np.where(w["ctype"] == 1, 1e3 * w["rho"], w["rho"]))
    K = Ps + 1e-6 * np.eye(n) + As.T @ (rho_vec[:, None] * As)
    res = np.abs(w["Kinv"][:n, :n] @ K - np.eye(n)).max()
    assert res <= 1e-9, res


# ---- 5. refusals and failures --------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu_lib, capfd):
    Pu, A, P2, A2, Px, Ax, Q, L, U = _case(17, 37, 5)
    h, twin = _handle(Pu, A, Q, L, U, **ADAPTIVE), _handle(Pu, A, Q, L, U, **ADAPTIVE)
    h.solve(fetch=False); twin.solve(fetch=False)
    gx = np.ones((h.B, h.n))
    h.adjoint(gx); twin.adjoint(gx)
    assert h.kkt_info().kept == 1
    lib, H = h._lib, h._h
    from osqp_amd import abi
    fp, ip = abi.fptr, abi.iptr
    idxP, idxA = np.arange(Pu.nnz, dtype=np.int64), np.arange(A.nnz, dtype=np.int64)
    longP, longA = np.ones(Pu.nnz + 1), np.ones(A.nnz + 1)
    badP, negA = idxP.copy(), idxA.copy()
    badP[3] = Pu.nnz; negA[0] = -1
    N = None
    calls = [(lambda: lib.osqp_amd_batch_common_update_model(H, fp(longP), ip(np.arange(Pu.nnz + 1)), Pu.nnz + 1, N, N, 0), 1),
             (lambda: lib.osqp_amd_batch_common_update_model(H, N, N, 0, fp(longA), ip(np.arange(A.nnz + 1)), A.nnz + 1), 2),
             # P's count comes first
             (lambda: lib.osqp_amd_batch_common_update_model(H, fp(longP), ip(np.arange(Pu.nnz + 1)), Pu.nnz + 1, fp(longA),
                                                             ip(np.arange(A.nnz + 1)), A.nnz + 1), 1),
             (lambda: lib.osqp_amd_batch_common_update_model(H, fp(Px), ip(idxP), -1, N, N, 0), 1),        # OSQP_DATA_VALIDATION_ERROR
             (lambda: lib.osqp_amd_batch_common_update_model(H, fp(Px), ip(badP), Pu.nnz, N, N, 0), 1),
             (lambda: lib.osqp_amd_batch_common_update_model(H, fp(Px), ip(idxP), Pu.nnz, fp(Ax), ip(negA), A.nnz), 1),
             (lambda: lib.osqp_amd_batch_common_update_model_dev(H, N, ip(np.arange(Pu.nnz + 1)), 0, longA.ctypes.data,
                                                                 ip(np.arange(A.nnz + 1)), A.nnz + 1), 2),
             (lambda: lib.osqp_amd_batch_common_update_model_dev(H, Px.ctypes.data, N, 0, N, N, 0), 1),      # a host pointer
             (lambda: lib.osqp_amd_batch_common_update_model(H, N, N, 0, N, N, 0), 0),
             (lambda: lib.osqp_amd_batch_common_update_model_dev(H, N, N, 0, N, N, 0), 0),
             (lambda: h.update_model(), 0),
             (lambda: lib.osqp_amd_batch_update_matrices(H, fp(Px), N, 0, 0, N, N, 0, 0), 4),
             (lambda: lib.osqp_amd_batch_update_matrices_dev(H, N, N, 0, 0, N, N, 0, 0), 4)]
    for k, (call, want) in enumerate(calls):
        assert call() == want, (k, want)
        assert h.kkt_info().kept == 1, k                  # still solved, the inversion still kept
    with pytest.raises(ValueError, match="common"):
        h.update_model(Px=np.tile(Px, (h.B, 1)))
    with pytest.raises(ValueError):
        h.update_model(Px=Px[:-1])
    with pytest.raises(RuntimeError, match="update_model"):
        h.update_matrices(Px=Px)
    assert _same(h.results(), twin.results())
    _assert_same_handles(h, twin, "after the refused calls")
    # a handle of another engine
    hs = _handle(Pu, A, Q, L, U, engine="streamed", **ADAPTIVE)
    capfd.readouterr()
    assert hs._lib.osqp_amd_batch_common_update_model(hs._h, fp(Px), N, 0, N, N, 0) == 4
    err = capfd.readouterr().err
    assert "osqp_amd_batch_update_matrices" in err and "common-K" in err, err
    assert hs._lib.osqp_amd_batch_common_update_model_dev(hs._h, N, N, 0, N, N, 0) == 4
    with pytest.raises(RuntimeError, match="update_matrices"):
        hs.update_model(Px=Px)


def test_k_not_positive_definite_then_repaired(gpu_lib, capfd):
    Pu, A, P2, A2, Px, Ax, Q, L, U = _case(17, 37, 5)
    h = _handle(Pu, A, Q, L, U, sigma=1e-6, **ADAPTIVE)
    diag = np.flatnonzero(Pu.indices == np.repeat(np.arange(Pu.shape[0]), np.diff(Pu.indptr)))
    slot = diag[5:6]
    capfd.readouterr()
    assert h.update_model(Px=np.array([-1e6]), Px_idx=slot) == 5           # OSQP_NONCVX_ERROR
    err = capfd.readouterr().err
    assert "not positive definite" in err and "QP " not in err, err          # the other engines' words, without a member
    assert h._lib.osqp_amd_batch_solve(h._h) == 5
    with pytest.raises(RuntimeError, match=r"\(5\)"):
        h.solve()
    assert h._shared_kkt                                  # K failed first: the pieces wait for the repair
    assert h.update_model(Px=Px, Ax=Ax) == 0
    f = _handle(P2, A2, Q, L, U, sigma=1e-6, **ADAPTIVE)
    _assert_same_handles(h, f, "after the repair")


def test_hessian_not_positive_definite(gpu_lib, capfd):
    """P~ + delta I fails while K passes: a negative diagonal entry of P under a heavy row of A.  The shared pieces go, the
    solves stay."""
    from scipy import sparse
    P = sparse.identity(3, format="csc")
    A = sparse.csc_matrix(np.diag([1.0, 1.0, 10.0]))
    rng = np.random.default_rng(8)
    Q = rng.standard_normal((3, 3)); L = -np.ones((3, 3)); U = np.ones((3, 3))
    L[:, 2] = U[:, 2] = 0.3                               # an equality row: it weighs 1e3 rho A~^2 in K, far above |P~_22|
    h = _handle(P, A, Q, L, U, adaptive_rho=0)
    assert np.all(h.solve().status_val == 1) and np.all(h.polish().status_polish != 0)
    capfd.readouterr()
    assert h.update_model(Px=np.array([1.0, 1.0, -0.5])) == 5
    err = capfd.readouterr().err
    assert "osqp_amd_batch_common_kkt: a pivot of P + delta I is not positive" in err, err
    assert not h._shared_kkt
    r = h.solve()                                         # served: K is positive definite
    assert r.iter.min() > 0
    with pytest.raises(RuntimeError, match="shared KKT pieces"):
        h.polish()
    assert h._lib.osqp_amd_batch_polish(h._h, None) == 4
    assert "osqp_amd_batch_common_kkt" in capfd.readouterr().err
    assert h.update_model(Px=np.ones(3)) == 0             # a handle without the pieces takes the call as ever
    f = _handle(P, A, Q, L, U, shared=False, adaptive_rho=0)
    for k in ("D", "E", "c", "Pv", "Av", "ctype"):
        assert np.array_equal(h.member_workspace(0)[k], f.member_workspace(0)[k]), k


# ---- 6. the layer --------------------------------------------------------------------------------------------------------
def _layer_inputs(orc):
    """W with zero rows for the members _adjoint_reference excuses at the oracle's point (their cotangent is zero, so they
    add nothing to the summed gradient), the tangents, and the members compared."""
    from _adjoint_reference import adjoint_reference
    from _batch_parity import oracle
    if "inputs" not in _worker_out:
        P, A, Q, L, U = kr.family(LAYER_SHAPE)
        Pu, A = sorted_model(P, A)
        B, n = Q.shape
        rng = np.random.default_rng(4243)
        W = rng.standard_normal((B, n))
        keep, refs = [], []
        for b in range(B):
            ro = oracle(orc, Pu, Q[b], A, L[b], U[b], eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, polish=1).solve()
            ref = adjoint_reference(Pu, A, L[b], U[b], ro.x, ro.y, W[b])
            why = kr.excuse(ref)
            print("member", b, "excused: " + why if why else "compared")
            if why:
                W[b] = 0.0
            else:
                keep.append(b); refs.append(ref)
        _worker_out["inputs"] = (dict(W=W, tP=rng.standard_normal(Pu.nnz), tA=rng.standard_normal(A.nnz)), keep, refs)
    return _worker_out["inputs"]


@pytest.mark.parametrize("route", ["host", "cuda"])
def test_layer(gpu_lib, oracle_mod, tmp_path_factory, route):
    inputs, keep, refs = _layer_inputs(oracle_mod)
    assert len(keep) >= 2
    o = SimpleNamespace(**_worker(tmp_path_factory, route, inputs))
    assert o.c_route[0] == ("host" if route == "host" else "device")
    assert np.all(o.c_status_adjoint[keep] == 1)
    # the second call went through update_model: the same handle, and its count of KKT builds went on
    assert bool(o.same_handle[0]) and bool(o.same_handle_end[0]) and o.builds[1] > o.builds[0] >= 1, o.builds
    for k in ("X", "X_moved", "X_A"):
        e = rel(getattr(o, "c_" + k), getattr(o, "s_" + k))
        assert e < 1e-6, (route, k, e)
    assert rel(o.c_X_own, o.c_X) < 1e-6 and rel(o.c_X_A, o.c_X) > 1e-3          # back to the layer's own values
    # the gradient of a shared value is the sum over the members
    for g, truth in (("gP", "dPx"), ("gA", "dAx")):
        got, want = getattr(o, "c_" + g), getattr(o, "s_" + g).sum(0)
        assert got.shape == want.shape and got.ndim == 1
        e = rel(got, want)
        et = rel(got, sum(getattr(r, truth) for r in refs))
        print(route, g, "against the streamed layer %.1e, against _adjoint_reference %.1e" % (e, et))
        assert e < 1e-6 and et < 1e-6, (route, g, e, et)
    for b in keep:
        e = rel(o.c_tX[b], o.s_tX[b])
        assert e < 1e-6 and np.abs(o.s_tX[b]).max() > 0, (route, "tangent", b, e)
    assert "takes no Px / Ax" in str(o.err_per_member[0]) and "shared model" in str(o.err_short[0])
    assert "must be [B," in str(o.err_streamed[0])
