"""GPU tests of the single-QP engine's scaling, residual, certificate and update kernels on their own, against the plain
long-double reference of tests/_engine_reference.py (itself checked on the CPU by tests/test_engine_reference.py), through the C
shim only: hipeng_create with the raw q, l, u, hipeng_ruiz_scale, hipeng_matrices_changed, hipeng_upload_rho (the set-up's order), hipeng_set_iterates, hipeng_set_z,
hipeng_run_admm(1), hipeng_residuals, hipeng_certificates, hipeng_download, hipeng_spmv, hipeng_get_stats.

Cases (one seeded generator, _engine_reference.make_case):
  tiny1, tiny3  1 x 1 and 3 x 2: one thread, one block
  m0            20 x 0: the m == 0 branches
  offtile       257 x 300: last workgroup partly filled
  empty         300 x 2100, rows 10..2070 of A empty, 5 variables without an entry: > 2048 rows in one block run, norm 0 -> 1
  long          600 x 40: rows of A with 511, 512, 513 entries, one dense row of P (IS_LONG on A and on M)
  huge          8200 x 12: rows of A with 8192 and 8191 entries (k_huge_dot partials in k_residuals, long_row_dot in k_certificates)
  scales        40 x 60: norms 1e-6, 1e-4, 1e4, 1e7 exactly, |q|_inf 1e7; scales_p0: P = 0, |q|_inf 1e-6  (one sweep, Ruiz only)
  bounds        40 x 60: +-1e30, equalities, +-1e25, +-1e26 (finite: the comparison is strict), 1e27 on a row whose E is 1e-2
`long`, `huge` and `empty` run on the launch-per-step kernels (OSQP_AMD_RESIDENT=0 OSQP_AMD_DENSE_DIRECT=0); the small cases run
that way and with the defaults.  Every test prints the form that served (hipeng_resident_info [9], [1]) and error / bar.

Bars, U = 2**-52, none tuned on the device's output:
  Ruiz outputs      R U relative; R counted from the kernels per sweep (_engine_reference.ruiz_roundings): D, E 3 (sqrt, reciprocal,
                    accumulating product); A entry 6; c s + 3; q s + 6; P entry s + 9; l, u: E + 1, with s the additions on one
                    term's path through the reduction of the mean column norm (device_sum_adds: 18 to 23).  No sweep: exact.
                    In `long` and `huge` the largest entry of the long rows, of the dense row of M and of its P part sits in
                    lane 63, in lane 0 of a later turn and at the end of a row whose length is no multiple of 64.
                    The read-outs of both device copies of the matrices equal the returned values exactly (for a non-zero
                    double, equality is bit equality).
  max-norm fields   (L + 4) U S, L the longest contributing row, S the largest sum |a_ij| |v_j| + |other terms|
  summed fields     (N + L + 4) U sum |terms|
  ADMM step         ||x~_dev - x~||_2 <= pcg_eps_rel ||b||_2 / lam_min(K) + 50 U ||x~||_2 on the PCG forms (pcg_eps_rel = 1e-12,
                    pcg_max_iter 20 000), 10 x the error of numpy's unrefined float64 solve + 50 U ||x~||_2 on the direct forms;
                    times alpha for x, alpha ||A_i||_1 for z, rho_i times that for y, plus the rounding of the update formulas.
                    Not on `tiny1` (its only variable is eliminated from the linear system: the bar is that of the whole K) nor
                    on `empty` (lam_min(K) = sigma on the variables without an entry: the bar would be 7e-4) nor the `scales`
                    pair (Ruiz only).
The residual, certificate and step references are evaluated on the vectors and the scaled data the device returned, so no
comparison depends on the stage before it."""
import functools
import time

import numpy as np
import pytest
from scipy import sparse

from tests import _engine_reference as R
from tests._hipeng import Engine

pytestmark = pytest.mark.gpu

U = R.U
STEP_ENV = dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=0)
PCG_EPS = 1e-12
CONFIGS = [(n, "steps") for n in R.CASES] + [(n, "default") for n in R.SMALL]
STATE_CONFIGS = [(n, e) for n, e in CONFIGS if not n.startswith("scales")]
STEP_CONFIGS = [(n, e) for n, e in CONFIGS if n in ("tiny3", "m0", "offtile", "long", "huge", "bounds")]


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.make_case(name)


def _open(name, env, alpha=1.6):
    c = _case(name)
    t = time.time()
    e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=STEP_ENV if env == "steps" else {}, q=c["q"], l=c["l"], u=c["u"],
               alpha=alpha, pcg_eps_rel=PCG_EPS, pcg_max_iter=20000)
    inf = e.info()
    print(f"[engine-kernels] {name}/{env}: hipeng_create {time.time() - t:.2f} s, form {inf[9]} in use {inf[1]}, eliminated {e.elim()}")
    return c, e


def _scaled(c, e, passes):
    """Ruiz on the device and the rho vector, in the order of the solver's set-up; then the Problem of what Ruiz returned."""
    o = e.ruiz_scale(passes)
    e.matrices_changed()
    e.set_rho(c["rho"])
    Pu, A = c["Pu"].copy(), c["A"].copy()
    Pu.data, A.data = o["Px"].copy(), o["Ax"].copy()
    return o, R.Problem(Pu, A, o["q"], o["l"], o["u"], o["D"] if passes else None, o["E"] if passes else None)


def _relerr(got, ref):
    ref = np.atleast_1d(np.asarray(ref, dtype=R.LD))
    got = np.atleast_1d(np.asarray(got, dtype=R.LD))
    den = np.where(ref == 0, 1, np.abs(ref))
    return float((np.abs(got - ref) / den).max()) if ref.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
# (a) Ruiz
# ---------------------------------------------------------------------------------------------------------------
# (the threshold cases: one sweep, so that the compared norms are exact inputs)
RUIZ_CONFIGS = [(n, e, p) for n, e in CONFIGS for p in ((1,) if n.startswith("scales") else (0, 1, 10))]


@pytest.mark.parametrize("name,env,passes", RUIZ_CONFIGS)
def test_ruiz_scale(name, env, passes):
    c, e = _open(name, env)
    try:
        o = e.ruiz_scale(passes)
        r = R.ruiz(c["Pu"], c["A"], c["q"], c["l"], c["u"], passes)
        for k in ("D", "E", "c", "q", "l", "u", "Px", "Ax"):
            err, bar = _relerr(o[k], r[k]), r["R_device"][k] * U
            print(f"[engine-kernels] {name}/{env} passes {passes} {k}: {err / U:.2f} U, R {r['R_device'][k]}")
            assert err <= bar, (name, env, passes, k, err / U, r["R_device"][k])
        # both device copies of the matrices, read out with unit vectors, hold the returned values
        e.matrices_changed()
        n, m = c["n"], c["m"]
        A = sparse.csc_matrix((o["Ax"], c["A"].indices, c["A"].indptr), shape=(m, n))
        Pu = sparse.csc_matrix((o["Px"], c["Pu"].indices, c["Pu"].indptr), shape=(n, n))
        P = (Pu + sparse.triu(Pu, 1).T).toarray() if n <= 1024 else (Pu + sparse.triu(Pu, 1).T).tocsc()
        Ac, Ar = A.tocsc(), A.tocsr()
        cols, rows = R.sample(c)
        for j in cols:
            unit = np.zeros(n); unit[j] = 1.0
            want = np.asarray(P[:, j].todense()).ravel() if sparse.issparse(P) else P[:, j]
            assert np.array_equal(e.spmv(2, unit), want), (name, env, "P column", j)
            if m:
                assert np.array_equal(e.spmv(0, unit), np.asarray(Ac[:, j].todense()).ravel()), (name, env, "A column (CSR copy)", j)
        for i in rows:
            unit = np.zeros(m); unit[i] = 1.0
            assert np.array_equal(e.spmv(1, unit), np.asarray(Ar[i, :].todense()).ravel()), (name, env, "A row (A' part of M)", i)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# (b) residual scalars, (c) certificates
# ---------------------------------------------------------------------------------------------------------------
def _state(c, e, passes):
    o, pb = _scaled(c, e, passes)
    x, y, z = R.iterates(c)
    e.set_iterates(x, y, z)
    e.run_admm(1)
    return pb, e.download(False)


@pytest.mark.parametrize("passes", [0, 10])
@pytest.mark.parametrize("name,env", STATE_CONFIGS)
def test_residuals_and_certificates(name, env, passes):
    c, e = _open(name, env)
    try:
        pb, (x, y, z, dx, dy) = _state(c, e, passes)
        got = e.residuals()
        val, bar, dyp = R.residual_scalars(pb, x, y, z, dx, dy)
        for k in val:
            err = abs(got[k] - val[k])
            print(f"[engine-kernels] {name}/{env} passes {passes} {k}: dev {got[k]:.17g} ref {val[k]:.17g} err/bar {err / bar[k] if bar[k] else err:.3f}")
            assert err <= bar[k], (name, env, passes, k, got[k], val[k], err, bar[k])
        dev_dyp = e.download(True)[4]
        assert np.array_equal(dev_dyp, dyp), (name, env, "projected delta_y", np.flatnonzero(dev_dyp != dyp)[:8])
        assert e.residuals() == got, "a second evaluation of the same iterates differs"
        # (c)
        n_calls = 0
        for un in (0, 1):
            epss = R.eps_pair(pb, dx, un) if c["m"] else (1.0,)
            for eps in epss:
                cv, cb, count, gap = R.certificate_scalars(pb, dx, dyp, eps, un)
                assert gap > 0.0, (name, passes, un, eps, gap)        # (every row decided beyond its rounding bound)
                dev = e.certificates(eps, un)
                n_calls += 1
                print(f"[engine-kernels] {name}/{env} passes {passes} unscaled {un} eps_dx {eps:.3e}: rows {count}, device flag {dev['Adx_viol']}")
                assert (dev["Adx_viol"] > 0) == (count > 0), (name, env, un, eps, dev["Adx_viol"], count)
                for k in cv:
                    err = abs(dev[k] - cv[k])
                    assert err <= cb[k], (name, env, passes, un, k, dev[k], cv[k], err, cb[k])
        # a later call does not see an earlier call's count
        if c["m"]:
            small = 0.5 * R.eps_pair(pb, dx, 0)[1]
            assert R.certificate_scalars(pb, dx, dyp, small, 0)[2] > 0
            assert e.certificates(small, 0)["Adx_viol"] > 0
            big = 4.0 * float(np.abs(pb.A @ dx.astype(R.LD)).max()) + 1.0
            assert e.certificates(big, 0)["Adx_viol"] == 0.0
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["finite_u", "finite_l", "free"])
def test_certificate_ties(kind):
    """(A dx)_i == +-eps_dx exactly on both rows of A (single power-of-two entries a and -a on one variable): the inequalities
    are strict, so nothing is violated -- with a finite u, with a finite l, and with neither."""
    a = {"finite_u": 2.0, "finite_l": 4.0, "free": 0.5}[kind]
    Pu = sparse.csc_matrix(np.array([[2.0, -0.5], [0.0, 3.0]]))
    A = sparse.csc_matrix(np.array([[a, 0.0], [-a, 0.0]]))
    l = np.full(2, -1.0 if kind == "finite_l" else -R.INF)
    u = np.full(2, 1.0 if kind == "finite_u" else R.INF)
    e = Engine(Pu, A, None, sigma=R.SIGMA, env=STEP_ENV, q=np.array([1.0, -0.5]), l=l, u=u, pcg_eps_rel=PCG_EPS, pcg_max_iter=20000)
    try:
        e.ruiz_scale(0)
        e.matrices_changed()
        e.set_rho(np.full(2, R.RHO))
        e.set_iterates(np.array([0.3, -0.2]), np.array([0.1, -0.1]), np.array([0.5, 0.25]))
        e.run_admm(1)
        dx = e.download(False)[3]
        assert dx[0] != 0.0
        e.residuals()
        eps = abs(a * dx[0])                                          # exact: a is a power of two
        assert e.certificates(eps, 0)["Adx_viol"] == 0.0, (kind, dx[0], eps)
        below = np.nextafter(eps, 0.0)
        assert (e.certificates(below, 0)["Adx_viol"] > 0) == (kind != "free"), (kind, "one ulp below the tie")
        assert e.certificates(eps, 0)["Adx_viol"] == 0.0
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# (d) one ADMM step
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("name,env", STEP_CONFIGS)
def test_admm_step(name, env, alpha):
    c, e = _open(name, env, alpha=alpha)
    try:
        assert e.elim() == 0                      # the bar below is that of the whole reduced system
        o, pb = _scaled(c, e, 10)
        x0, y0, z0 = R.iterates(c)
        e.set_iterates(x0, y0, z0)
        e.run_admm(1)
        x1, y1, z1, dx, dy = e.download(False)
        st8 = e.stats()
        assert (st8["admm_done"], st8["pcg_forced"], st8["neg_curvature"]) == (1, 0, 0), st8
        inf = e.info()
        direct = inf[9] in (3, 4) and inf[1] == 1
        st = R.admm_step(pb, R.SIGMA, alpha, c["rho"], x0, z0, y0)
        bars = R.step_bars(st, alpha, c["rho"], direct, PCG_EPS)
        l, u = o["l"], o["u"]
        # exact identities
        assert np.all(l <= z1) and np.all(z1 <= u)
        assert np.array_equal(y0 + dy, y1) and np.array_equal(x1 - x0, dx)
        v, bz = st["v"].astype(float), bars["z"]
        lo, hi = v < l - bz, v > u + bz
        assert np.array_equal(z1[lo], l[lo]) and np.array_equal(z1[hi], u[hi]), (name, env, alpha)
        for k, got in (("x", x1), ("z", z1), ("y", y1)):
            err = np.abs(got.astype(R.LD) - st[k]).astype(float)
            ratio = float((err / np.maximum(bars[k], 1e-300)).max()) if err.size else 0.0
            print(f"[engine-kernels] {name}/{env} alpha {alpha} form {inf[9]} direct {direct} {k}+: max err {err.max() if err.size else 0.0:.2e}, err/bar {ratio:.3e}"
                  f" (bar on x~ {bars['x_tilde']:.2e}, lam_min {st['lam_min']:.2e})")
            assert np.all(err <= bars[k]), (name, env, alpha, k, ratio)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# the same path through the solver: the ADMM iterates put back after a polish that is not adopted
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,m", [(0, 40, 60), (6, 20, 30), (19, 40, 60)])
def test_resolve_after_polish_not_adopted(oracle_mod, seed, n, m):
    """At eps = 1e-2 the polish of these QPs is not adopted (status_polish -1): the solver puts (x, z, y) back with
    hipeng_set_iterates + hipeng_set_z, with a z that is about 1e-2 off A x.  The warm-started solve that follows takes one
    iteration; its x, y match the oracle's to the parity bar of the suite (1e-6 relative) only if that iteration's linear
    solve started from z~ = A x."""
    import osqp_amd
    from osqp_amd.problems import random_sparse_qp
    pb = random_sparse_qp(n, m, seed=seed)
    kw = dict(polish=1, eps_abs=1e-2, eps_rel=1e-2, check_termination=1)
    so, sg = oracle_mod.OracleOSQP().setup(**pb, **kw), osqp_amd.OSQP().setup(**pb, **kw)
    ro, rg = so.solve(), sg.solve()
    assert ro.info.status_polish == rg.info.status_polish == -1 and ro.info.iter == rg.info.iter, (ro.info, rg.info)
    so.update_settings(polish=0); sg.update_settings(polish=0)
    ro, rg = so.solve(), sg.solve()
    assert (rg.info.status, rg.info.iter) == (ro.info.status, ro.info.iter) == ("solved", 1), (rg.info, ro.info)
    for got, ref in ((rg.x, ro.x), (rg.y, ro.y)):
        assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), (seed, np.abs(got - ref).max())
