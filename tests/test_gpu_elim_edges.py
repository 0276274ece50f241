"""GPU tests of the slack-elimination path of the single-QP engine (engine.hip: build_elim; engine_aux_kernels.h: k_elim_refresh, k_elim_split; the
`gone` / rhoe / elim_vb / row_apply special cases of k_precond, k_refresh_m, k_pcg_init, k_cg_A, k_cg_B, k_form_K and
k_admm_finalize, the xte read-back of hipeng_kkt_solve, elim_rhs_dirty on the host) one ADMM step at a time through the C shim,
against _engine_reference.admm_step -- a long-double-refined solve of the FULL K = P + sigma I + A' rho A that knows nothing of
elimination -- on the scaled data the device returned.  Every test opens the engine as tests/test_gpu_pcg_edges.py does (raw q,
l, u, pcg_eps_rel = 1e-12, Ruiz with 10 passes, hipeng_matrices_changed, hipeng_upload_rho), asserts the form,
hipeng_elim_count == len(claims) and hipeng_row_eliminated row by row.

Cases (tests/_elim_cases.py; tests/test_elim_cases_host.py proves on the CPU that each is what it claims, that its bars are sharp
and that six one-place mutations of the eliminated step miss them by more than 10 x): all_gone (+ 1 x 1), one_gone_1 / _2, pyy,
rivals, lone_rows, rounds (also with the finalize grid forced to one workgroup), long_rows and huge_gone (OSQP_AMD_SPLIT 0 and 1),
blocks_gone on form 0; res_gone_e8 / _e20 on form 1.

Bars (_elim_cases.step_bars_elim, none tuned on the device's output): ||x~_X,dev - x~_X||_2 <= pcg_eps_rel ||b~_X||_2 / lam_min(S) +
50 U ||x~||_2 on the variables that stay, |rho a| / D_y ||A_iX||_1 times that plus (L_i + 13) U T / D_y on an eliminated one, carried
through x+, z+, y+ as _engine_reference.step_bars does.  Every assertion is on all elements of x+, z+, y+.

Tests: one step (alpha 1.0 and 1.6, z != A x); three steps, each against a reference step from the state downloaded before it, and
run_admm(3) on a twin engine bit-equal to them; a step straight after each host call that touches the right-hand side or the
operator, in two orders (pyy, long_rows); the plugin solve; the resident K against the reduced matrix; rhoe / ecoef / edinv / xte
through hipeng_elim_peek; the same step with OSQP_AMD_ELIM=0.  Worst err / bar per test and the planted-defect table: DESIGN 4.
Wall time of the module on an MI355X: 88 tests in 8 s (the slowest, the host-state sequence on long_rows, 0.8 s; huge_gone, the
largest case, 0.1 s per test)."""
import time

import numpy as np
import pytest
from scipy import sparse

from tests import _elim_cases as EC
from tests import _engine_reference as R
from tests._hipeng import Engine, PCG_STOP

pytestmark = pytest.mark.gpu

LD, U = R.LD, R.U
STEPS = dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=0)
FORM0 = (0, 0, 0, 0)
VARIANTS = ([(n, {}) for n in EC.NAMES if n not in ("long_rows", "huge_gone")]
            + [(n, dict(OSQP_AMD_SPLIT=s)) for n in ("long_rows", "huge_gone") for s in (0, 1)] + [("rounds", dict(OSQP_AMD_FIN_GRID=1))])
IDS = ["-".join([n] + [f"{k[9:]}={v}" for k, v in x.items()]) for n, x in VARIANTS]
_ST = {}                                   # reference steps, shared among the tests: (case, what was changed, alpha, salt) -> (digest of the data, st)


def _env(name, extra=None, elim=True):
    c = EC.make(name)
    if name.startswith("res_gone"):
        env = dict(OSQP_AMD_DENSE_DIRECT=0, OSQP_AMD_RESIDENT_MIN_N=1, OSQP_AMD_RESIDENT_NWG=c["claims"]["nwg"])
        form = (1, 1, c["claims"]["E"], c["claims"]["nwg"])
    else:
        env, form = dict(STEPS), FORM0
    env.update(extra or {})
    if not elim:
        env["OSQP_AMD_ELIM"] = 0
    return env, form


class Rig:
    """One engine on a case, opened and scaled as the solver's set-up does, and the data it currently holds (scaled space)."""

    def __init__(self, name, alpha=1.6, extra=None, elim=True, monkeypatch=None):
        self.name, self.alpha, self.elim = name, alpha, elim
        self.tag = name + "".join(f" {k[9:]}={v}" for k, v in (extra or {}).items()) + ("" if elim else " ELIM=0")
        c = self.c = EC.make(name)
        env, form = _env(name, extra, elim)
        if monkeypatch is not None:                 # (OSQP_AMD_FIN_GRID is read when the iteration is launched, not at create)
            for k, v in (extra or {}).items():
                monkeypatch.setenv(k, str(v))
        t = time.time()
        self.e = e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=env, q=c["q"], l=c["l"], u=c["u"], alpha=alpha, pcg_eps_rel=EC.PCG_EPS,
                            pcg_max_iter=20000)
        try:
            o = e.ruiz_scale(10)
            e.matrices_changed()
            e.set_rho(c["rho"])
            self.t_open = time.time() - t
            self.D, self.E = o["D"], o["E"]
            self.cur = dict(Px=o["Px"].copy(), Ax=o["Ax"].copy(), q=o["q"].copy(), l=o["l"].copy(), u=o["u"].copy(), rho=c["rho"].copy(), sigma=R.SIGMA)
            self.changed, self._pb = "", None
            inf = e.info()
            assert (inf[9], inf[1], inf[2], inf[3]) == form, (self.tag, "form, in use, E, workgroups", inf[:10], form)
            self.erow, self.ecol = EC.claimed(c) if elim else (np.full(c["n"], -1), np.full(c["m"], -1))
            assert e.elim() == (len(c["claims"]["gone"]) if elim else 0), (self.tag, e.elim())
            got = np.array([e.row_eliminated(i) for i in range(c["m"])])
            assert np.array_equal(got, (self.ecol >= 0).astype(int)), (self.tag, np.flatnonzero(got != (self.ecol >= 0))[:8])
            assert e.row_eliminated(-1) == 0 and e.row_eliminated(c["m"]) == 0
        except BaseException:
            e.close()
            raise

    def close(self):
        self.e.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set(self, what, **kw):
        """Record a change of the data the engine holds (the caller made the upload)."""
        self.cur.update(kw)
        self.changed += "/" + what
        self._pb = None

    def matrices(self, Px=None, Ax=None):
        Pu, A = self.c["Pu"].copy(), self.c["A"].copy()
        Pu.data, A.data = (self.cur["Px"] if Px is None else Px).copy(), (self.cur["Ax"] if Ax is None else Ax).copy()
        return Pu, A

    def problem(self):
        if self._pb is None:
            Pu, A = self.matrices()
            self._pb = R.Problem(Pu, A, self.cur["q"], self.cur["l"], self.cur["u"], self.D, self.E)
        return self._pb

    def expect(self, x0, z0, y0, key):
        """(st, bars) of the reference step from (x0, z0, y0) on the current data; st is shared among the tests (a twin engine asks
        for the same step), the digest makes sure it is the same one."""
        cur, pb = self.cur, self.problem()
        digest = hash(b"".join(np.ascontiguousarray(v, dtype=float).tobytes() for v in
                               (cur["Px"], cur["Ax"], cur["q"], cur["l"], cur["u"], cur["rho"], [cur["sigma"], self.alpha], x0, z0, y0)))
        k = (self.name, self.changed, self.alpha, key)
        if k not in _ST or _ST[k][0] != digest:
            _ST[k] = (digest, R.admm_step(pb, cur["sigma"], self.alpha, cur["rho"], x0, z0, y0))
        st = _ST[k][1]
        if self.elim:
            red = EC.reduced(pb, cur["sigma"], cur["rho"], self.erow, EC.rhs(pb, cur["sigma"], cur["rho"], x0, z0, y0))
            bars = EC.step_bars_elim(pb, st, red, self.erow, cur["sigma"], self.alpha, cur["rho"], EC.PCG_EPS, x0, z0, y0)
        else:
            bars = R.step_bars(st, self.alpha, cur["rho"], False, EC.PCG_EPS)
        return st, bars

    def step(self, what, key, start=None):
        """One run_admm(1) -- from `start` = (x, y, z) through hipeng_set_iterates / hipeng_set_z, or from the state the device holds
        (downloaded first, nothing uploaded) -- against the reference: the exact identities, then every element of x+, z+, y+.
        Returns (worst err / bar, (x+, y+, z+), st, bars)."""
        e, tag = self.e, f"{self.tag} {what}"
        if start is not None:
            x0, y0, z0 = start
            e.set_iterates(x0, y0, z0)
        else:
            x0, y0, z0 = e.download(False)[:3]
        t = time.time()
        e.run_admm(1)
        x1, y1, z1, dx, dy = e.download(False)
        t = time.time() - t
        s8 = e.stats()
        assert (s8["admm_done"], s8["pcg_forced"], s8["neg_curvature"]) == (1, 0, 0), (tag, s8)
        st, bars = self.expect(x0, z0, y0, key)
        l, u = self.cur["l"], self.cur["u"]
        assert np.all(l <= z1) and np.all(z1 <= u), tag
        for what_id, a, b in (("y + dy == y+", y0 + dy, y1), ("x+ - x == dx", x1 - x0, dx)):
            assert np.array_equal(a, b), (tag, what_id, np.flatnonzero(a != b)[:8], a[a != b][:8], b[a != b][:8])
        v, bz = st["v"].astype(float), bars["z"]
        lo, hi = v < l - bz, v > u + bz
        assert np.array_equal(z1[lo], l[lo]) and np.array_equal(z1[hi], u[hi]), tag
        worst, text, bad = 0.0, [], []
        for k, got in (("x", x1), ("z", z1), ("y", y1)):
            err = np.abs(got.astype(LD) - st[k]).astype(float)
            ratio = float((err / np.maximum(bars[k], 1e-300)).max()) if err.size else 0.0
            worst = max(worst, ratio)
            text.append(f"{k}+ {err.max() if err.size else 0.0:.2e} err/bar {ratio:.3e}")
            if not np.all(err <= bars[k]):
                w = int((err / np.maximum(bars[k], 1e-300)).argmax())
                bad.append((k, w, float(err[w]), float(bars[k][w])))
        inf = e.info()
        print(f"[elim-edges] {tag}: form {inf[9]} E {inf[2]} nwg {inf[3]} gave up {inf[10]} eliminated {e.elim()} pcg iterations {s8['pcg_iters_last']}"
              f" step {t:.3f} s; {'; '.join(text)} (bar on x~_X {bars['x_tilde']:.2e} = {bars['x_tilde'] / max(st['norm_xt'], 1e-300):.1e} ||x~||)"
              f" worst err/bar {worst:.3e}")
        assert not bad, (tag, bad)
        assert inf[10] == 0, (tag, "a resident launch gave up", inf)
        return worst, (x1, y1, z1), st, bars


# ---------------------------------------------------------------------------------------------------------------
# one step
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("name,extra", VARIANTS, ids=IDS)
def test_one_step(name, extra, alpha, monkeypatch):
    """From non-zero x, y and a z that is not A x (hipeng_set_z): the first right-hand side is k_refresh_m's."""
    with Rig(name, alpha, extra, monkeypatch=monkeypatch) as r:
        r.step("one step", 0, start=R.iterates(r.c))


# ---------------------------------------------------------------------------------------------------------------
# second and third step: the right-hand side is k_admm_finalize's elim_vb
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,extra", VARIANTS, ids=IDS)
def test_three_steps(name, extra, monkeypatch):
    with Rig(name, 1.6, extra, monkeypatch=monkeypatch) as r, Rig(name, 1.6, extra, monkeypatch=monkeypatch) as twin:
        start = R.iterates(r.c)
        r.step("step 1 of 3", 0, start=start)
        r.step("step 2 of 3", "second")
        _, (x3, y3, z3), _, _ = r.step("step 3 of 3", "third")
        twin.e.set_iterates(*start)
        twin.e.run_admm(3)
        xt, yt, zt = twin.e.download(False)[:3]
        assert twin.e.stats()["admm_done"] == 3
        assert np.array_equal(xt, x3) and np.array_equal(yt, y3) and np.array_equal(zt, z3), (r.tag, "run_admm(3) is not three run_admm(1)")


# ---------------------------------------------------------------------------------------------------------------
# host state: what raises elim_rhs_dirty, and the use_cvec toggle
# ---------------------------------------------------------------------------------------------------------------
def _op_q(r, rng):
    q = r.cur["q"] * rng.uniform(0.5, 1.5, r.c["n"]) + 0.1 * rng.standard_normal(r.c["n"])
    r.e.upload_q(q)
    r.set("q", q=q)


def _op_bounds(r, rng):
    """An equality row with an eliminated variable becomes a range, and gets the rho of one."""
    l, u, rho = r.cur["l"].copy(), r.cur["u"].copy(), r.cur["rho"].copy()
    rows = np.flatnonzero((r.ecol >= 0) & (l == u))
    i = rows[0] if rows.size else np.flatnonzero(r.ecol >= 0)[0]
    l[i], u[i], rho[i] = l[i] - 0.3, u[i] + 0.2, EC.RHO
    r.e.upload_bounds(l, u)
    r.e.set_rho(rho)
    r.set("bounds", l=l, u=u, rho=rho)


def _op_rho(r, rng):
    rho = r.cur["rho"].copy()
    rows = np.flatnonzero(r.ecol >= 0)
    rho[rows] = 10.0 ** rng.uniform(-3.0, 3.0, rows.size)
    rho[rows[0]], rho[rows[-1]] = 1e-3, 1e3
    r.e.set_rho(rho)
    r.set("rho", rho=rho)


def _op_matrices(r, rng):
    """Same pattern: every eliminated coefficient a changes sign and magnitude (x -2 or x -0.5), a stored P_yy of 0 becomes 0.5, and
    every other stored P_yy > 0 of an eliminated variable becomes 0 (not where a = 0: D_y would be sigma alone)."""
    Pu, A = sparse.csc_matrix(r.c["Pu"]), sparse.csc_matrix(r.c["A"])
    Px, Ax = r.cur["Px"].copy(), r.cur["Ax"].copy()
    flip = 0
    for j in np.flatnonzero(r.erow >= 0):
        ka = A.indptr[j]
        Ax[ka] *= rng.choice([-2.0, -0.5])
        for k in range(Pu.indptr[j], Pu.indptr[j + 1]):
            if Px[k] == 0.0:
                Px[k] = 0.5
            elif Ax[ka] != 0.0:
                flip += 1
                if flip % 2:
                    Px[k] = 0.0
    Pm, Am = r.matrices(Px, Ax)
    r.e.set_matrices(Pm, Am)
    r.set("matrices", Px=Px, Ax=Ax)


def _op_sigma(r, rng):
    sigma = 1e-3 if r.cur["sigma"] != 1e-3 else 1e-5
    r.e.set_sigma(sigma)
    r.set("sigma", sigma=sigma)


def _op_cold(r, rng):
    r.e.cold_start()


def _op_kkt(r, rng):
    """A plugin solve between two steps (use_cvec on and off again, xte overwritten), then the iterates are set again."""
    b = rng.standard_normal(r.c["n"] + r.c["m"])
    r.e.L.hipeng_kkt_solve(r.e.h, r.e.abi.fptr(r.e.abi.as_f64(b).copy()))


def _op_changed(r, rng):
    """hipeng_matrices_changed on unchanged values: z~ is formed again from the PCG vector (zero at the eliminated variables) and
    completed by k_refresh_m(zt_partial = 1), which also forms the start vector's m-part."""
    r.e.matrices_changed()


OPS = dict(q=_op_q, bounds=_op_bounds, rho=_op_rho, matrices=_op_matrices, cold=_op_cold, kkt=_op_kkt, sigma=_op_sigma, changed=_op_changed)
ORDERS = (("q", "changed", "bounds", "rho", "matrices", "cold", "kkt", "sigma"), ("sigma", "kkt", "matrices", "cold", "q", "rho", "changed", "bounds"))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", ["pyy", "long_rows"])
def test_a_step_after_each_host_call(name, order):
    """After each call the next step starts from what the device holds -- nothing is uploaded in between that would form the
    right-hand side again -- except after hipeng_cold_start (from zero: b_y = -q_y) and after the plugin solve (hipeng_set_iterates,
    as the solver does)."""
    rng = np.random.default_rng(40 + order)
    with Rig(name, 1.6) as r:
        r.step("first step", 0, start=R.iterates(r.c))
        for k, op in enumerate(ORDERS[order]):
            OPS[op](r, rng)
            start = None
            if op == "kkt":
                x, y, z = R.iterates(r.c, salt=5 + k)
                start = (x, y, z)
            r.step(f"after {op} ({'/'.join(ORDERS[order][:k + 1])})", ("host", order, k), start=start)
            if op == "cold":
                x0, y0, z0 = np.zeros(r.c["n"]), np.zeros(r.c["m"]), np.zeros(r.c["m"])
                st, _ = r.expect(x0, z0, y0, ("host", order, k))
                Y = np.flatnonzero(r.erow >= 0)
                assert np.all(st["x_tilde"][Y] != 0.0)                     # b_y = -q_y reached every eliminated variable of the reference


# ---------------------------------------------------------------------------------------------------------------
# plugin solve
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.NAMES)
def test_plugin_solve(name):
    """hipeng_kkt_solve on the unscaled case with its rho: Engine.check's bar (for huge_gone the same residual bar through the
    sparse long-double operators: Engine.check's reference forms and factors K as a dense array), then on two right-hand sides
    z~ = A x~ on every row to its rounding bound and x~ of the eliminated variables against the refined solve of the full K."""
    c = EC.make(name)
    env, form = _env(name)
    e = Engine(c["Pu"], c["A"], c["rho"], sigma=R.SIGMA, env=env, pcg_eps_rel=EC.PCG_EPS, pcg_max_iter=20000)
    try:
        assert e.elim() == len(c["claims"]["gone"])
        if name != "huge_gone":
            e.check("elim-edges " + name, form[0])
        pb = R.Problem(c["Pu"], c["A"], c["q"], c["l"], c["u"])
        erow, _ = EC.claimed(c)
        rl = c["rho"].astype(LD)
        L = np.diff(pb.A.indptr)
        rng = np.random.default_rng(3)
        n, m = c["n"], c["m"]
        for k in range(2):
            b = rng.standard_normal(n + m) * (1.0 if k == 0 else rng.uniform(0.1, 10.0, n + m))
            out = e.solve(b)
            xt, zt = out[:n], out[n:]
            rhs = b[:n].astype(LD) + pb.AT @ (rl * b[n:].astype(LD))
            Kx = pb.P @ xt.astype(LD) + LD(R.SIGMA) * xt + pb.AT @ (rl * (pb.A @ xt.astype(LD)))
            res = float(np.abs(rhs - Kx).max() / np.abs(rhs).max())
            assert res <= 10.0 * PCG_STOP, (name, res)
            # z~ = A x~: every row, (L_i + 4) roundings of the row sum and one more where a x~_y is added to it
            azt, bz = (pb.A @ xt.astype(LD)), (L + 5) * U * np.asarray(pb.Aa @ np.abs(xt).astype(LD)).astype(float)
            ez = np.abs(zt.astype(LD) - azt).astype(float)
            assert np.all(ez <= bz), (name, "z~ != A x~", int((ez / np.maximum(bz, 1e-300)).argmax()), float((ez / np.maximum(bz, 1e-300)).max()))
            # x~ of the eliminated variables
            ref, _ = EC.refine(pb, R.SIGMA, c["rho"], rhs, np.zeros(n))
            red = EC.reduced(pb, R.SIGMA, c["rho"], erow, rhs)
            nx = float(np.sqrt((ref * ref).sum()))
            bxt, bar_xt, _ = EC.xtilde_bars(pb, red, erow, c["rho"], EC.PCG_EPS, ref, nx, np.abs(b[:n]), c["rho"] * np.abs(b[n:]))
            ex = np.abs(xt.astype(LD) - ref).astype(float)
            Y, X = red["Y"], red["X"]
            print(f"[elim-edges] {name} plugin solve {k}: residual {res:.2e}, z~ - A x~ worst err/bar {float((ez / np.maximum(bz, 1e-300)).max()) if m else 0:.3f}, "
                  f"eliminated x~ worst err/bar {float((ex[Y] / bar_xt[Y]).max()):.3e}, ||err_X|| / bar {float(np.linalg.norm(ex[X])) / bxt:.3e}")
            assert np.all(ex[Y] <= bar_xt[Y]), (name, float((ex[Y] / bar_xt[Y]).max()))
            assert np.linalg.norm(ex[X]) <= bxt, (name, float(np.linalg.norm(ex[X])), bxt)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# resident K
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", sorted(EC.RES_GONE))
def test_resident_K_is_the_reduced_matrix(E):
    with Rig("res_gone_e%d" % E) as r:
        K = r.e.resident_dump()
        pb = r.problem()
        red = EC.reduced(pb, R.SIGMA, r.cur["rho"], r.erow)
        X, Y = red["X"], red["Y"]
        S = red["S"].toarray()
        Kpat = ((abs(pb.P) + sparse.eye(pb.n) + abs(pb.A).T @ abs(pb.A)) != 0).toarray()
        scale = max(float(np.abs(S).max()), 1.0)
        err = float(np.abs(K[np.ix_(X, X)].astype(LD) - S).max())
        print(f"[elim-edges] res_gone_e{E}: max |K_XX - S| {err:.2e}, bar {1e-13 * scale:.2e}; stored entries in eliminated rows {int(Kpat[Y].sum())}")
        assert err <= 1e-13 * scale
        assert np.array_equal(K, K.T)
        assert np.all(K[Y, Y] == 1.0)
        off = K.copy()
        off[Y, Y] = 0.0
        assert not off[Y].any() and not off[:, Y].any() and int(Kpat[Y].sum()) > 2 * Y.size


# ---------------------------------------------------------------------------------------------------------------
# derived arrays
# ---------------------------------------------------------------------------------------------------------------
def _derived(r, what):
    """k_elim_refresh against long double: a = A(i, y) exactly; D = (P_yy + sigma) + (rho a) a and 1 / D: 5 roundings; rho~ =
    (rho (P_yy + sigma)) / D: 1 + 1 + 4 + 1 = 7 (all terms positive: relative errors add, with 1 % for their products)."""
    pb = r.problem()
    red = EC.reduced(pb, r.cur["sigma"], r.cur["rho"], r.erow)
    rows = r.ecol >= 0
    a, edinv, rhoe = r.e.elim_peek("ecoef"), r.e.elim_peek("edinv"), r.e.elim_peek("rhoe")
    assert np.array_equal(a, red["a"].astype(float)), (r.tag, what)
    assert np.array_equal(rhoe[~rows], r.cur["rho"][~rows]) and not edinv[~rows].any(), (r.tag, what)
    e1 = np.abs(edinv.astype(LD) * red["Dy"] - 1).astype(float)[rows]
    e2 = np.abs(rhoe.astype(LD) / red["rhoe"] - 1).astype(float)[rows]
    print(f"[elim-edges] {r.tag} {what}: 1 / D_y off by {e1.max() / U:.2f} U (bar 5), rho~ by {e2.max() / U:.2f} U (bar 7)")
    assert np.all(e1 <= 5.05 * U) and np.all(e2 <= 7.07 * U), (r.tag, what, e1.max() / U, e2.max() / U)


@pytest.mark.parametrize("name", ["pyy", "rivals", "long_rows", "rounds", "res_gone_e8"])
def test_derived_arrays(name):
    rng = np.random.default_rng(9)
    with Rig(name) as r:
        _derived(r, "after set_rho")
        _op_matrices(r, rng)
        _derived(r, "after upload_matrices")
        _op_sigma(r, rng)
        _derived(r, "after a new sigma")
        _op_rho(r, rng)
        _derived(r, "after a rho of 1e-3 .. 1e3")
        x, y, z = R.iterates(r.c)
        r.e.set_iterates(x, y, z)
        xte = r.e.elim_peek("xte")
        Y = np.flatnonzero(r.erow >= 0)
        assert np.array_equal(xte[r.erow[Y]], x[Y]), (r.tag, "k_elim_split")


# ---------------------------------------------------------------------------------------------------------------
# twin: the same step with OSQP_AMD_ELIM=0
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,extra", VARIANTS, ids=IDS)
def test_twin_without_elimination(name, extra, monkeypatch):
    start = R.iterates(EC.make(name))
    with Rig(name, 1.6, extra, monkeypatch=monkeypatch) as r:
        _, got, st, bars = r.step("one step", 0, start=start)
    with Rig(name, 1.6, extra, elim=False, monkeypatch=monkeypatch) as t:
        e = t.e
        e.set_iterates(*start)
        e.run_admm(1)
        x1, y1, z1 = e.download(False)[:3]
        s8 = e.stats()
        assert (s8["admm_done"], s8["neg_curvature"]) == (1, 0), (t.tag, s8)
        st2, bars2 = t.expect(start[0], start[2], start[1], 0)
        tight = bars2["x_tilde"] <= 1e-8 * st["norm_xt"]
        worst, both = 0.0, 0.0
        for k, a, b in (("x", x1, got[0]), ("y", y1, got[1]), ("z", z1, got[2])):
            err = np.abs(a.astype(LD) - st[k]).astype(float)
            worst = max(worst, float((err / np.maximum(bars2[k], 1e-300)).max()))
            d = np.abs(a - b) / np.maximum(bars[k] + bars2[k], 1e-300)
            both = max(both, float(d.max()))
            assert np.all(np.abs(a - b) <= bars[k] + bars2[k]), (t.tag, k, float(d.max()))
            if tight:
                assert np.all(err <= bars2[k]), (t.tag, k, float((err / np.maximum(bars2[k], 1e-300)).max()))
        print(f"[elim-edges] {t.tag}: pcg iterations {s8['pcg_iters_last']} forced {s8['pcg_forced']}; bar on x~ from lam_min(K) {bars2['x_tilde']:.2e} = "
              f"{bars2['x_tilde'] / st['norm_xt']:.1e} ||x~|| ({'asserted' if tight else 'above 1e-8 ||x~||: not asserted'}), worst err/bar {worst:.3e}; "
              f"the two engines differ by {both:.3e} of the sum of their bars")
