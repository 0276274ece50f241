"""GPU tests of the common-K batch engine (osqp_amd/csrc/batch_common.h, BatchOSQP(engine="common")): one K^-1 and one
GEMM per ADMM iteration for a batch that shares P, A, the scaling, the row classes and rho.

Bars: `_batch_parity.assert_parity` (status, iterations and rho updates equal; x, y within 1e-6; objective within
1e-8) against the yardsticks of tests/_common_cases.py, and `check_member_kinv`'s 1e-14 and 10x numpy."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import sparse

from _batch_parity import assert_parity, check_member_kinv, oracle, oracle_ws, rel
from _common_cases import (ADAPTIVE, ADAPTIVE_CASES, CASES_UNSCALED, FIXED, MIXED, UNSCALED_MAX_ITER, adaptive_family,
                           common_family, common_oracle, mixed_family, prescaled_oracle, unscale)

pytestmark = pytest.mark.gpu

# n: the edges of the 32-padding of K^-1 and of the GEMM's 4-deep k step and 64-row tile; B: the edges of the 16-column
# MFMA tile.  No B here reaches the 64-member workgroups of the element-wise kernels, the 256-member ones of k_bc_probe
# / k_bc_adopt or a second 64-column tile of the GEMM: B = 63, 64, 65 and 257 are in tests/test_gpu_batch_common_loop.py
SHAPES = [(1, 33), (17, 15), (32, 16), (33, 17), (128, 33), (129, 1), (1024, 17)]


def _max_m(n):
    NP = (n + 31) // 32 * 32
    return (160 * 1024 - 8 * (7 * NP + 320)) // 92


def _common(P, A, Q, L, U, **kw):
    import osqp_amd
    return osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **kw)


def _as_member(ws, ro):
    """The pre-scaled oracle run as the member's expected results (x = D x~, y = E y~ / c, obj = obj~ / c)."""
    x, y, obj = unscale(ws, ro)
    return SimpleNamespace(x=x, y=y, info=SimpleNamespace(status_val=ro.info.status_val, iter=ro.info.iter,
                                                          rho_updates=ro.info.rho_updates, obj_val=obj))


def _check_prescaled(r, orc, ws, Q, L, U, what, kw=FIXED, members=None):
    out = {}
    for b in (range(Q.shape[0]) if members is None else members):
        so = prescaled_oracle(orc, ws, Q, L, U, b, **kw)
        ro = so.solve()
        assert_parity(r, b, _as_member(ws, ro), what)
        out[b] = (so, ro)
    return out


def _check_workspace_f64(bs, qp, so, want_np):
    """check_member_kinv without its long-double reference inverse, which takes 15 s at n = 1024: the scaled data and
    classes against the oracle's workspace to the same 1e-14, and K^-1 through its residual in double: |K^-1 K - I|_max
    within 10x that of numpy's inverse (+ 1e-14), the same factor on the quantity that is cheap to form."""
    g, o = bs.member_workspace(qp), oracle_ws(so)
    n = bs.n
    assert g["NP"] == want_np
    for k in ("D", "E", "Pv", "Av"):
        assert g[k].shape == o[k].shape and np.abs(g[k] - o[k]).max(initial=0.0) <= 1e-14 * np.abs(o[k]).max(initial=0.0), k
    assert abs(g["c"] - o["c"]) <= 1e-14 * abs(o["c"]) and np.array_equal(g["ctype"], o["ctype"])
    rho_vec = np.where(o["ctype"] == -1, 1e-6, np.where(o["ctype"] == 1, 1e3 * g["rho"], g["rho"]))
    Pf = (o["Pu"] + sparse.triu(o["Pu"], 1).T).toarray(); Ad = o["A"].toarray()
    K = Pf + o["sigma"] * np.eye(n) + Ad.T @ (rho_vec[:, None] * Ad)
    pad = np.eye(want_np); pad[:n, :n] = g["Kinv"][:n, :n]
    assert np.array_equal(g["Kinv"], pad)
    res_np = np.abs(np.linalg.inv(K) @ K - np.eye(n)).max()
    res_g = np.abs(g["Kinv"][:n, :n] @ K - np.eye(n)).max()
    assert res_g <= 10.0 * res_np + 1e-14, (res_g, res_np)


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(getattr(a, k)[rows], getattr(b, k)[rows], equal_nan=True)
               for k in ("x", "y", "info_raw", "dual_inf_cert", "prim_inf_cert"))


# ---- 1. shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", SHAPES)
def test_shapes(gpu_lib, oracle_mod, n, B):
    for m in sorted({0, 1, min(2 * n + 3, _max_m(n))}):
        P, A, Q, L, U, _ = common_family(n, m, B, 1000 + n + m)
        bs = _common(P, A, Q, L, U, **FIXED)
        NP = (n + 31) // 32 * 32
        assert bs.shape() == (2, NP)
        so0 = common_oracle(oracle_mod, P, A, Q, L, U, **FIXED)
        for qp in {0, B - 1}:                            # the common workspace, whichever member is asked for
            if n <= 129:
                check_member_kinv(bs, qp, so0, "setup n=%d m=%d" % (n, m), NP)
            elif qp == 0:
                _check_workspace_f64(bs, qp, so0, NP)
        r = bs.solve()
        _check_prescaled(r, oracle_mod, oracle_ws(so0), Q, L, U, "n=%d m=%d B=%d" % (n, m, B))
        assert bs.rounds()[0] == 1 and bs.rounds()[1] in (0, B)
        bs.cleanup()


# ---- 2. scaling = 0 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", CASES_UNSCALED)
def test_unscaled_direct_parity(gpu_lib, oracle_mod, n, m):
    P, A, Q, L, U, _ = common_family(n, m, 5, 1000 + n + m)
    for kw in (dict(FIXED, scaling=0), dict(FIXED, scaling=0, max_iter=UNSCALED_MAX_ITER)):
        r = _common(P, A, Q, L, U, **kw).solve()
        sts = []
        for b in range(5):
            ro = oracle(oracle_mod, P, Q[b], A, L[b], U[b], **kw).solve()
            assert_parity(r, b, ro, "unscaled %s" % (kw,))
            sts.append(ro.info.status_val)
        if "max_iter" in kw and (n, m) == CASES_UNSCALED[-1]:
            assert -2 in sts and 1 in sts, sts           # a member that ends at max_iter next to solved ones


# ---- 3. identical members: the reference's plain run, adaptive rho included ------------------------------------------
@pytest.mark.parametrize("n,m,qscale", ADAPTIVE_CASES)
@pytest.mark.parametrize("B", [1, 17])
def test_identical_members(gpu_lib, oracle_mod, n, m, qscale, B):
    P, A, Q, L, U, _ = adaptive_family(n, m, 5, qscale)
    Qc, Lc, Uc = (np.tile(V[0], (B, 1)) for V in (Q, L, U))
    bs = _common(P, A, Qc, Lc, Uc, **ADAPTIVE)
    r = bs.solve()
    ro = oracle(oracle_mod, P, Q[0], A, L[0], U[0], **ADAPTIVE).solve()
    for b in range(B):
        assert_parity(r, b, ro, "identical B=%d" % B)
    for k in ("x", "y", "info_raw"):                     # all copies are bit-equal
        assert np.array_equal(getattr(r, k), np.tile(getattr(r, k)[0], (B, 1))), k
    assert np.all(r.rho_updates > 0) and bs.rounds()[0] >= 2
    assert np.all(r.rho == bs.member_workspace(0)["rho"]) and r.rho[0] != 0.1


# ---- 4. adaptive rho, differing members, default (unscaled) termination ---------------------------------------------
def _gamma(k):
    u = 2.0 ** -53
    return k * u / (1 - k * u)


@pytest.mark.parametrize("n,m,qscale", ADAPTIVE_CASES)
def test_adaptive_differing_members(gpu_lib, n, m, qscale):
    """No reference run has this batch's rho (a geometric mean), so the results are checked against their definitions,
    recomputed in long double from the returned x, y: obj_val = 1/2 x'Px + q'x and dua_res = |Px + q + A'y|_inf.
    Bar: the rounding bound of a dot product, gamma_k * sum |terms|, gamma_k = k u / (1 - k u), u = 2^-53.  The kernel
    forms both on the scaled data and unscales: k = the longest row of [P A'] (the terms of one sum) + 64 for the
    chain of scaling products -- 10 Ruiz passes x 3 products on every matrix entry, 10 + 10 on D and c, which makes
    c D P D the scaled P to 50 roundings, and up to 6 products unscaling x, y and the residual; for obj_val the n
    column sums are added up too: k + n.  pri_res: z lies in [l, u] and |Ax - z|_inf = pri_res, so
    l - pri_res <= Ax <= u + pri_res up to the same bound on the row sums of A."""
    B = 5
    P, A, Q, L, U, _ = adaptive_family(n, m, B, qscale)
    bs = _common(P, A, Q, L, U, **ADAPTIVE)
    r = bs.solve()
    assert np.all(r.status_val == 1), r.status_val
    assert np.all(r.rho == r.rho[0]) and r.rho[0] != 0.1 and np.all(r.rho_updates > 0), (r.rho, r.rho_updates)
    assert bs.rounds()[0] >= 2 and bs.member_workspace(0)["rho"] == r.rho[0]
    ld = np.longdouble
    Pf = (P + sparse.triu(P, 1).T).toarray().astype(ld); Ad = A.toarray().astype(ld)
    k = int(max((Pf[j] != 0).sum() + (Ad[:, j] != 0).sum() for j in range(n))) + 1 + 64
    krow = int(max((Ad[i] != 0).sum() for i in range(m))) + 64
    for b in range(B):
        x, y, q = r.x[b].astype(ld), r.y[b].astype(ld), Q[b].astype(ld)
        terms = np.abs(Pf * x[None, :]).sum(axis=1) + np.abs(q) + (np.abs(Ad) * np.abs(y)[:, None]).sum(axis=0)
        dua = np.abs(Pf @ x + q + Ad.T @ y)
        print("member", b, "dua_res", r.dua_res[b], float(dua.max()), "bound", float(_gamma(k) * terms.max()))
        assert abs(ld(r.dua_res[b]) - dua.max()) <= _gamma(k) * terms.max(), b
        obj = 0.5 * x @ (Pf @ x) + q @ x
        oterms = 0.5 * (np.abs(x)[:, None] * np.abs(Pf) * np.abs(x)[None, :]).sum() + (np.abs(q) * np.abs(x)).sum()
        print("member", b, "obj_val", r.obj_val[b], float(obj), "bound", float(_gamma(k + n) * oterms))
        assert abs(ld(r.obj_val[b]) - obj) <= _gamma(k + n) * oterms, b
        ax = Ad @ x
        slack = ld(r.pri_res[b]) + _gamma(krow) * (np.abs(Ad) @ np.abs(x))
        lo, hi = np.maximum(L[b], -1e30).astype(ld), np.minimum(U[b], 1e30).astype(ld)
        assert np.all(ax >= lo - slack) and np.all(ax <= hi + slack), b


# ---- 5. independence of position and batch size ---------------------------------------------------------------------
def test_member_bits_do_not_depend_on_the_batch(gpu_lib):
    n, m = 17, 37
    P, A, Q, L, U, _ = common_family(n, m, 33, 1000 + n + m)
    kw = dict(FIXED, scaling=0)
    r33 = _common(P, A, Q, L, U, **kw).solve()
    r1 = _common(P, A, Q[3:4], L[3:4], U[3:4], **kw).solve()
    idx = [3] + [b for b in range(17) if b != 3]
    r17 = _common(P, A, Q[idx], L[idx], U[idx], **kw).solve()
    assert r33.status_val[3] == 1
    for k in ("x", "y", "info_raw"):
        assert np.array_equal(getattr(r33, k)[3], getattr(r1, k)[0]), k
        assert np.array_equal(getattr(r33, k)[3], getattr(r17, k)[0]), k


# ---- 6. mixed statuses ------------------------------------------------------------------------------------------------
def test_mixed_statuses(gpu_lib, oracle_mod):
    from osqp_amd import abi
    P, A, Q, L, U = mixed_family()
    pinf, dinf, B = MIXED["pinf"], MIXED["dinf"], MIXED["B"]
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **FIXED))
    r = _common(P, A, Q, L, U, **FIXED).solve()
    res = _check_prescaled(r, oracle_mod, ws, Q, L, U, "mixed")
    assert r.status_val[pinf] == abi.OSQP_PRIMAL_INFEASIBLE and r.status_val[dinf] == abi.OSQP_DUAL_INFEASIBLE
    assert all(r.status_val[b] == abi.OSQP_SOLVED for b in range(B) if b not in (pinf, dinf))
    for b in (pinf, dinf):
        assert np.all(np.isnan(r.x[b]) | (r.x[b] == abi.OSQP_NAN)) and np.all(np.isnan(r.y[b]) | (r.y[b] == abi.OSQP_NAN))
    assert rel(r.prim_inf_cert[pinf], res[pinf][1].prim_inf_cert) < 1e-5
    assert rel(r.dual_inf_cert[dinf], res[dinf][1].dual_inf_cert) < 1e-5
    assert r.obj_val[pinf] == abi.OSQP_INFTY and r.obj_val[dinf] == -abi.OSQP_INFTY
    keep = [b for b in range(B) if b not in (pinf, dinf)]
    rk = _common(P, A, Q[keep], L[keep], U[keep], **FIXED).solve()
    for k in ("x", "y", "info_raw"):
        assert np.array_equal(getattr(r, k)[keep], getattr(rk, k)), k


# ---- 7. live handle ---------------------------------------------------------------------------------------------------
def _live_problem():
    n, m, B = 33, 66, 5
    P, A, Q, L, U, X0 = common_family(n, m, B, 1000 + n + m)
    rng = np.random.default_rng(5)
    Q2 = Q * 1.3 + 0.1 * rng.standard_normal(Q.shape)
    fin = np.isfinite(L) & np.isfinite(U) & (U > L)
    L2 = np.where(fin, L - 0.2, L); U2 = np.where(fin, U + 0.1, U)     # the same classes
    return P, A, Q, L, U, X0, Q2, L2, U2


def test_live_handle_sequence(gpu_lib, oracle_mod):
    P, A, Q, L, U, X0, Q2, L2, U2 = _live_problem()
    B, m = Q.shape[0], A.shape[0]
    ws = oracle_ws(common_oracle(oracle_mod, P, A, Q, L, U, **FIXED))
    D, E, c = ws["D"], ws["E"], ws["c"]
    bs = _common(P, A, Q, L, U, **FIXED)
    r = bs.solve()
    sos = _check_prescaled(r, oracle_mod, ws, Q, L, U, "solve 0")
    assert bs.update(Q=Q2, L=L2, U=U2) == 0
    Xw = X0 + 0.01; Yw = 0.1 * np.ones((B, m))
    assert bs.warm_start(X=Xw, Y=Yw) == 0
    assert bs.update_rho(0.3) == 0
    r = bs.solve()
    for b in range(B):
        so = sos[b][0]
        so.update(q=c * D * Q2[b], l=E * np.maximum(L2[b], -1e30), u=E * np.minimum(U2[b], 1e30))
        so.warm_start(x=Xw[b] / D, y=c * Yw[b] / E)
        assert so.update_rho(0.3) == 0
        assert_parity(r, b, _as_member(ws, so.solve()), "update, warm start, rho")
    assert np.all(r.rho == 0.3) and bs.member_workspace(0)["rho"] == 0.3
    # a class change common to all members: some inequality rows become equality rows everywhere
    ineq = np.flatnonzero(ws["ctype"] == 0)[:5]
    L3, U3 = L2.copy(), U2.copy()
    mid = (A @ X0.T).T
    L3[:, ineq] = U3[:, ineq] = mid[:, ineq]
    assert bs.update(L=L3, U=U3) == 0
    r = bs.solve()
    for b in range(B):
        so = sos[b][0]
        so.update(l=E * np.maximum(L3[b], -1e30), u=E * np.minimum(U3[b], 1e30))
        assert_parity(r, b, _as_member(ws, so.solve()), "common class change")
    g = bs.member_workspace(B - 1)
    assert np.all(g["ctype"][ineq] == 1)
    so3 = oracle(oracle_mod, ws["Pu"], c * D * Q2[0], ws["A"], E * np.maximum(L3[0], -1e30), E * np.minimum(U3[0], 1e30),
                 scaling=0, adaptive_rho=0, rho=0.3)
    o3 = oracle_ws(so3)
    rho_vec = np.where(o3["ctype"] == -1, 1e-6, np.where(o3["ctype"] == 1, 1e3 * 0.3, 0.3))
    Pf = (ws["Pu"] + sparse.triu(ws["Pu"], 1).T).toarray(); Ad = ws["A"].toarray()
    K = Pf + ws["sigma"] * np.eye(P.shape[0]) + Ad.T @ (rho_vec[:, None] * Ad)
    n = P.shape[0]
    assert rel(g["Kinv"][:n, :n] @ K, np.eye(n)) < 1e-9         # K was rebuilt with the new classes


def test_class_change_in_one_member_is_refused(gpu_lib, capfd):
    P, A, Q, L, U, X0, Q2, L2, U2 = _live_problem()
    a, b = _common(P, A, Q, L, U, **FIXED), _common(P, A, Q, L, U, **FIXED)
    ra, rb = a.solve(), b.solve()
    assert _same(ra, rb)
    ws_ct = a.member_workspace(0)["ctype"]
    row = int(np.flatnonzero((ws_ct == 0) & np.isfinite(L[3]) & np.isfinite(U[3]))[2])
    Lb, Ub = L.copy(), U.copy()
    Lb[3, row] = Ub[3, row] = 0.5 * (L[3, row] + U[3, row])           # an equality row in member 3 only
    capfd.readouterr()
    assert a.update(L=Lb, U=Ub) == 1
    err = capfd.readouterr().err
    assert "member 3" in err and "row %d" % row in err, err
    ga, gb = a.member_workspace(3), b.member_workspace(3)
    assert all(np.array_equal(ga[k], gb[k]) for k in ("ctype", "Kinv", "E", "D"))
    assert a.update(Q=Q2) == 0 and b.update(Q=Q2) == 0
    assert _same(a.solve(), b.solve())                   # nothing of the refused update was written
    with pytest.raises(ValueError, match="scalar"):
        a.update_rho(np.full(Q.shape[0], 0.2))
    one = np.full(Q.shape[0], 0.2)
    from osqp_amd import abi
    assert a._lib.osqp_amd_batch_update_rho(a._h, abi.fptr(one), 1) == 1
    assert _same(a.solve(), b.solve())


def test_device_route_equals_host_route(gpu_lib, tmp_path):
    """update, warm_start and results_into on torch CUDA tensors against the host route, bit for bit, and a refused
    device update that writes nothing.  In a child process: torch brings a HIP runtime of its own
    (tests/_common_device_worker.py says why)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_common_device_worker.py")
    out = tmp_path / "out.npz"
    p = subprocess.run([sys.executable, worker, str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    g = np.load(out)
    assert int(g["refused"]) == 1
    for k in ("x", "y", "info", "x2", "info2"):
        assert np.array_equal(g["h_" + k], g["d_" + k]), k
    assert np.all(g["h_info"][:, 1] == 1) and not np.array_equal(g["h_x"], g["h_x2"])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def test_unserved_calls(gpu_lib, capfd):
    P, A, Q, L, U, _ = common_family(17, 37, 3, 1054)
    bs, ref = _common(P, A, Q, L, U, **FIXED), _common(P, A, Q, L, U, **FIXED)
    assert _same(bs.solve(), ref.solve())
    lib, h, N = bs._lib, bs._h, None
    calls = {
        "update_matrices": lambda: lib.osqp_amd_batch_update_matrices(h, N, N, 0, 0, N, N, 0, 0),
        "update_matrices_dev": lambda: lib.osqp_amd_batch_update_matrices_dev(h, N, N, 0, 0, N, N, 0, 0),
        "polish": lambda: lib.osqp_amd_batch_polish(h, N),
        "polish_status_dev": lambda: lib.osqp_amd_batch_polish_status_dev(h, N),
        "adjoint": lambda: lib.osqp_amd_batch_adjoint(h, *[N] * 9),
        "adjoint_dev": lambda: lib.osqp_amd_batch_adjoint_dev(h, *[N] * 9),
        "adjoint_multi": lambda: lib.osqp_amd_batch_adjoint_multi(h, 1, *[N] * 9),
        "adjoint_multi_dev": lambda: lib.osqp_amd_batch_adjoint_multi_dev(h, 1, *[N] * 9),
        "tangent": lambda: lib.osqp_amd_batch_tangent(h, 1, *[N] * 9),
        "tangent_dev": lambda: lib.osqp_amd_batch_tangent_dev(h, 1, *[N] * 9),
        "kkt_info": lambda: lib.osqp_amd_batch_kkt_info(h, N),
    }
    for name, call in calls.items():
        capfd.readouterr()
        assert call() == 4, name
        err = capfd.readouterr().err
        assert "osqp_amd_batch_" + name + " " in err and "common-K" in err, (name, err)
    for call in (bs.polish, lambda: bs.adjoint(np.zeros_like(Q)), bs.tangent, bs.kkt_info,
                 lambda: bs.update_matrices(Px=np.ones(P.nnz))):
        with pytest.raises(RuntimeError, match="common-K"):
            call()
    assert _same(bs.solve(), ref.solve())                # the handle is untouched and usable


def test_setup_refusals(gpu_lib, capfd):
    P, A, Q, L, U, _ = common_family(17, 37, 4, 1054)
    ct = _common(P, A, Q, L, U, **FIXED).member_workspace(0)["ctype"]
    row = int(np.flatnonzero(ct == 0)[1])
    Lb, Ub = L.copy(), U.copy()
    Lb[2, row] = Ub[2, row] = 0.0                        # an equality row in member 2 only
    capfd.readouterr()
    with pytest.raises(ValueError, match="error 1"):
        _common(P, A, Q, Lb, Ub, **FIXED)
    err = capfd.readouterr().err
    assert "member 2" in err and "row %d" % row in err, err
    # indefinite P with a tiny sigma: K is not positive definite
    n = 20
    Pn = sparse.diags(np.r_[-1.0, np.ones(n - 1)], format="csc")
    An = sparse.eye(3, n, format="csc")
    with pytest.raises(ValueError, match="error 5"):
        _common(Pn, An, np.ones((2, n)), -np.ones((2, 3)), np.ones((2, 3)), sigma=1e-6, **FIXED)
    assert "non-convex" in capfd.readouterr().err


def test_device_arrays_match_results(gpu_lib):
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    P, A, Q, L, U, _ = common_family(33, 66, 17, 1099)
    bs = _common(P, A, Q, L, U, **FIXED)
    r = bs.solve()
    got = []
    for a in bs.device_arrays():
        ai = a.__cuda_array_interface__
        h = np.empty(ai["shape"])
        assert hip.hipMemcpy(h.ctypes.data, ai["data"][0], h.nbytes, 2) == 0       # hipMemcpyDeviceToHost
        got.append(h)
    X, Y, I = got
    assert np.array_equal(X, r.x) and np.array_equal(Y[:, :66], r.y) and np.array_equal(I, r.info_raw)
