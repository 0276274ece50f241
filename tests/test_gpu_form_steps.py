"""GPU tests of whole ADMM steps on every linear-solve form of the single-QP engine (hipeng_resident_info [9]: 0 launch-per-step
PCG, 1 resident PCG, 2 block-resident PCG, 3 block-direct, 4 dense-direct) from extrapolated start vectors and straight after
each host call, one hipeng_run_admm(1) at a time against _engine_reference.admm_step from the state downloaded before it.

Every engine is opened as tests/test_gpu_pcg_edges.py opens its own: raw q, l, u, pcg_eps_rel = 1e-12 (extrapolation on),
hipeng_ruiz_scale(10), hipeng_matrices_changed, hipeng_upload_rho; the scaled data the device returned feeds the reference.  So
blk_refresh and dd_refresh also run behind a device-side rescale.  Form, route and layout are asserted after opening;
hipeng_resident_info [9], [1] and [10] == 0 after every step: an engine that left its form (direct_disable, a resident give-up)
fails the test.

Cases (tests/_form_cases.py; tests/test_form_cases_host.py proves on the CPU that each is what it claims, that cond(K) <= 1e4
after Ruiz and that every one-place defect of the step misses the bars by more than 10 x):
  form 0  f0_blocks (dense blocks of P and remainder), f0_long_split (long rows, OSQP_AMD_SPLIT=1)
  form 1  f1_e8 / f1_e20, OSQP_AMD_RESIDENT_PIPE 1 and 0
  form 2  f2_nh0 (two blocks of 32), f2_nh1 (64 blocks of 128 and one huge row)
  form 3  blocks 32, 33, 64, 127, 128: f3_plain, f3_kc1, f3_kc17, f3_kc17_plainrhs (OSQP_AMD_BLOCK_PLAIN=1); 64 blocks of 128:
          f3_huge1, f3_huge4, f3_huge4_nofin (OSQP_AMD_BLOCK_FIN_DOTS=0), f3_huge5 (the huge rows as coupling rows)
  form 4  f4_b2 (B2 unknowns with 0, 3 and 8 neighbours), f4_b2_nd0 (no dense row), f4_slack_pyy0 / _pyy03 (ten engine-eliminated
          slacks), f4_symv384 / f4_symv1152 (OSQP_AMD_DENSE_SYMV=1), f4_vd (nnz(A) >= 2e5: k_vd)

Tests:
  chains      one hipeng_set_iterates, then 5 x run_admm(1) (4 on the n = 8192 cases) under OSQP_AMD_EXTRAP_SCHED=1,2 -- the steps
              start from theta = 0, 0.5, 1, 1, 1 -- each checked on every element of x+, z+, y+, the identities y + dy == y+ and
              x+ - x == dx to the bit, the clamped rows; stats (admm_done, pcg_forced 0, neg_curvature 0; pcg_iters_last 1 on the
              direct forms); a twin engine's run_admm(k) bit-equal to them.  The default 5 / 12 schedule over 14 steps on one case
              per form.
  host calls  three steps in (full extrapolation), then a step straight after each of q, bounds, bounds+rho, rho, matrices,
              changed, sigma, cold, kkt, warm x only, warm y only, set_z, in two orders (_form_cases.ORDERS), from what the device
              holds -- nothing uploaded in between, except after cold (from zero) and after kkt (hipeng_set_iterates, as the solver
              does).  One case per form, f3_kc17, f4_slack_pyy0 and f4_symv384.

Bars, none tuned on device output: forms 0-2 _engine_reference.step_bars(direct=False, 1e-12); forms 3-4 step_bars(direct=True);
the slack cases _elim_cases.step_bars_elim with the direct term in place of the PCG term.
One case, f4_b2_nd0 (cond(K) 5e2), misses step_bars(direct=True) at the third step of its chain with no defect found: x+ is off
by 2.9e-12 against a bar of 2.6e-12.  The x~ term there is 10 x the error of a float64 LU solve of K x~ = b; the direct forms
compute x~ = v_n + K^-1 r with r = b - K v_n, and at that step the start vector, extrapolated with theta = 1 while the iterates
still jump, leaves ||r|| = 6 ||b||: the float64 inverse of K (LAPACK) applied to that residual is off by 1.8e-12 in x~ on the CPU,
where the LU solve of K x~ = b is off by 1.1e-13.  For this case alone the x~ term is therefore 10 x
_form_cases.inverse_residual_error + 50 U ||x~||: the start vector's n-part follows from the reference's own x~ history and the
schedule, nothing from the device enters it.  The CPU test proves the one-place defects against the same bar; on the MI355X the
five steps of the chain then sit at 0.11 - 0.12 of it (the device is 1.1 - 1.2 x the float64 inverse's own error).

Found by the host-call test: reset_start left vold, the previous [x~ | rho z~], as it was, so a schedule that extrapolates at the
first k_admm_finalize after a reset mixed the rho / A from before the call into the m-part of the next start vector.
Worst err / bar per form and the module's wall time: DESIGN 4."""
import functools
import time

import numpy as np
import pytest

from tests import _elim_cases as EC
from tests import _engine_reference as R
from tests import _form_cases as FC
from tests import _pcg_cases as PC
from tests._hipeng import Engine

pytestmark = pytest.mark.gpu

LD = R.LD
_ST = {}                                   # reference steps shared among the tests (a twin case asks for the same step): key -> (digest, st)
_KEEP = {}                                 # factorisation and lam_min of the reference while P, A, rho, sigma stay: digest -> dict
WORST = {}                                 # form -> worst err / bar seen, printed by each test


@functools.lru_cache(maxsize=None)
def _br_nwg():
    """The grid k_pcg_blockres takes on this device (the smallest problem form 2 accepts reports it)."""
    c = PC.br_probe()
    e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=FC.BLOCKRES, q=c["q"], l=c["l"], u=c["u"], alpha=FC.ALPHA, pcg_eps_rel=FC.PCG_EPS, pcg_max_iter=20000)
    try:
        inf = e.info()
        assert inf[9] == 2 and inf[1] == 1, inf
        return int(inf[3])
    finally:
        e.close()


def _digest(*arrays):
    return hash(b"".join(np.ascontiguousarray(v, dtype=float).tobytes() for v in arrays))


class Rig:
    """One engine on a case of tests/_form_cases.py, opened and scaled as the solver's set-up does, and the data it holds."""

    def __init__(self, name, sched="1,2"):
        c = self.c = FC.make(name)
        cl = self.cl = c["claims"]
        self.name, self.form, self.direct = name, cl["form"], cl["form"] >= 3
        self.tag = f"{name} sched {sched or '5,12'}"
        env = dict(c["env"])
        if sched:
            env["OSQP_AMD_EXTRAP_SCHED"] = sched
        self.e = e = Engine(c["Pu"], c["A"], None, sigma=R.SIGMA, env=env, q=c["q"], l=c["l"], u=c["u"], alpha=FC.ALPHA, pcg_eps_rel=FC.PCG_EPS,
                            pcg_max_iter=20000)
        try:
            o = e.ruiz_scale(10)
            e.matrices_changed()
            e.set_rho(c["rho"])
            self.cur = dict(Px=o["Px"].copy(), Ax=o["Ax"].copy(), q=o["q"].copy(), l=o["l"].copy(), u=o["u"].copy(), rho=c["rho"].copy(), sigma=R.SIGMA,
                            D=o["D"], E=o["E"])
            self._pb = None
            inf = e.info()
            want = dict(cl["info"])
            if self.form == 2:
                want[3] = _br_nwg()
            self.in_use = inf[1]
            assert inf[9] == self.form and all(inf[k] == v for k, v in want.items()), (self.tag, "form and slots", inf, self.form, want)
            assert inf[1] == 1 or self.form == 0, (self.tag, inf)
            if "layout" in cl:
                lay = e.layout()
                got = dict(dense=lay[0], dense_rows=lay[1], long=lay[3], huge=lay[4], folded=lay[5], split=lay[6])
                assert {k: got[k] for k in cl["layout"]} == cl["layout"], (self.tag, got, cl["layout"])
            gone = cl.get("gone", {})
            self.erow, self.ecol = EC.claimed(c) if gone else (np.full(c["n"], -1), np.full(c["m"], -1))
            assert e.elim() == len(gone), (self.tag, e.elim())
            assert all(e.row_eliminated(i) == 1 for i in gone.values()), self.tag
        except BaseException:
            e.close()
            raise

    def close(self):
        self.e.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def problem(self):
        if self._pb is None:
            self._pb = FC.problem(self.c, self.cur)
        return self._pb

    def expect(self, x0, z0, y0, key, vn=None):
        cur, pb = self.cur, self.problem()
        dk = _digest(cur["Px"], cur["Ax"], cur["rho"], [cur["sigma"]])
        digest = _digest(cur["q"], cur["l"], cur["u"], [dk], x0, z0, y0)
        k = (self.c["name"], key)
        if k not in _ST or _ST[k][0] != digest:
            if dk not in _KEEP:
                _KEEP.clear()                        # (one set of factors at a time: the n = 8192 ones are large)
                _KEEP[dk] = {}
            _ST[k] = (digest, R.admm_step(pb, cur["sigma"], FC.ALPHA, cur["rho"], x0, z0, y0, reuse=_KEEP[dk]))
        st = _ST[k][1]
        if self.cl["bars"] == "direct_inv":
            assert vn is not None, "the re-derived x~ term needs the start vector: chains only"
            bars = R.step_bars(dict(st, plain_err=FC.inverse_residual_error(self.c, cur, st, x0, z0, y0, vn)), FC.ALPHA, cur["rho"], True, FC.PCG_EPS)
        elif self.cl["bars"] == "direct_elim":
            red = EC.reduced(pb, cur["sigma"], cur["rho"], self.erow, EC.rhs(pb, cur["sigma"], cur["rho"], x0, z0, y0))
            bars = EC.step_bars_elim(pb, st, red, self.erow, cur["sigma"], FC.ALPHA, cur["rho"], FC.PCG_EPS, x0, z0, y0, direct=True)
        else:
            bars = R.step_bars(st, FC.ALPHA, cur["rho"], self.direct, FC.PCG_EPS)
        return st, bars

    def check_form(self, tag):
        inf = self.e.info()
        assert (inf[9], inf[1], inf[10]) == (self.form, self.in_use, 0), (tag, "the engine left its form: [9], [1], [10]", inf)
        return inf

    def step(self, what, key, start=None, vn=None):
        """One run_admm(1) -- from `start` = (x, y, z) through hipeng_set_iterates / hipeng_set_z, or from the state the device holds
        (downloaded first, nothing uploaded) -- against the reference; vn: the n-part of the start vector by the reference's own
        x~ history (the "direct_inv" bar).  Returns (worst err / bar, (x+, y+, z+), st)."""
        e, tag = self.e, f"{self.tag} {what}"
        if start is not None:
            e.set_iterates(*start)
        x0, y0, z0 = start if start is not None else e.download(False)[:3]
        t = time.time()
        e.run_admm(1)
        x1, y1, z1, dx, dy = e.download(False)
        t = time.time() - t
        s8 = e.stats()
        assert (s8["admm_done"], s8["pcg_forced"], s8["neg_curvature"]) == (1, 0, 0), (tag, s8)
        if self.direct:
            assert s8["pcg_iters_last"] == 1, (tag, s8)
        inf = self.check_form(tag)
        st, bars = self.expect(x0, z0, y0, key, vn)
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
        WORST[self.form] = max(WORST.get(self.form, 0.0), worst)
        route = f" route {'chol' if inf[5] else 'sweep'}" if self.form == 4 else ""
        print(f"[form-steps] {tag}: form {inf[9]} in use {inf[1]}{route} [2] {inf[2]} [3] {inf[3]} [15] {inf[15]} gave up {inf[10]} eliminated {e.elim()}"
              f" pcg iterations {s8['pcg_iters_last']} step {t:.3f} s; {'; '.join(text)} (bar on x~ {bars['x_tilde']:.2e} = "
              f"{bars['x_tilde'] / max(st['norm_xt'], 1e-300):.1e} ||x~||) worst err/bar {worst:.3e}; worst of form {self.form} so far {WORST[self.form]:.3e}")
        assert not bad, (tag, bad)
        return worst, (x1, y1, z1), st

    # ---- the host calls of _form_cases.op_changes, made on the device ----
    def call(self, op, rng):
        e, c = self.e, self.c
        data, it = FC.op_changes(op, c, self.cur, [v for v in (e.download(False)[k] for k in (0, 1, 2))], rng)
        self.cur.update(data)
        self._pb = None
        if "q" in data:
            e.upload_q(data["q"])
        if "l" in data:
            e.upload_bounds(data["l"], data["u"])
        if "rho" in data:
            e.set_rho(data["rho"])
        if "Px" in data:
            e.set_matrices(*FC.matrices(c, self.cur))
        if "sigma" in data:
            e.set_sigma(data["sigma"])
        if op == "changed":
            e.matrices_changed()
        if it is None:
            return None
        if it[0] == "cold":
            e.cold_start()
        elif it[0] == "kkt":
            assert e.L.hipeng_kkt_solve(e.h, e.abi.fptr(e.abi.as_f64(it[1]).copy())) == 0
            return it[2][0], it[2][1], it[2][2]          # (x, y, z): set again by the step, as the solver does
        elif it[0] == "x":
            assert e.L.hipeng_set_iterates(e.h, e._p(e.abi.as_f64(it[1])), None) == 0
        elif it[0] == "y":
            assert e.L.hipeng_set_iterates(e.h, None, e._p(e.abi.as_f64(it[1]))) == 0
        else:
            assert e.L.hipeng_set_z(e.h, e._p(e.abi.as_f64(it[1]))) == 0
        return None


def _chain(name, sched, steps):
    t = time.time()
    with Rig(name, sched) as r, Rig(name, sched) as twin:
        start = R.iterates(r.c)
        worst, last = 0.0, None
        # the start vector's n-part by the reference's own x~: x at the reset, then x~ + theta (x~ - the previous x~), theta by the
        # schedule at the count of solves since the reset (k_admm_finalize)
        sch = tuple(int(v) for v in sched.split(",")) if sched else (5, 12)
        vn = prev = start[0]
        for k in range(steps):
            w, last, st = r.step(f"step {k + 1} of {steps}", ("chain", sched, k), start=start if k == 0 else None, vn=vn)
            worst = max(worst, w)
            xt = st["x_tilde"].astype(float)
            vn, prev = xt + FC.theta(k + 1, sch) * (xt - prev), xt
        twin.e.set_iterates(*start)
        twin.e.run_admm(steps)
        xt, yt, zt = twin.e.download(False)[:3]
        s8 = twin.e.stats()
        assert (s8["admm_done"], s8["pcg_forced"], s8["neg_curvature"]) == (steps, 0, 0), (twin.tag, s8)
        twin.check_form(twin.tag + " twin")
        same = [np.array_equal(a, b) for a, b in zip((xt, yt, zt), last)]
        assert all(same), (r.tag, f"run_admm({steps}) is not {steps} x run_admm(1): x, y, z equal", same,
                           [float(np.abs(a - b).max()) for a, b in zip((xt, yt, zt), last)])
        print(f"[form-steps] {r.tag}: form {r.form} chain of {steps}: worst err/bar {worst:.3e}, twin run_admm({steps}) bit-equal; {time.time() - t:.1f} s")


@pytest.mark.parametrize("name", FC.NAMES)
def test_chain_through_the_extrapolation_schedule(name):
    """OSQP_AMD_EXTRAP_SCHED=1,2: the steps start from theta = 0 (the reset), 0.5 and 1."""
    _chain(name, "1,2", 4 if FC.make(name)["claims"]["large"] else 5)


@pytest.mark.parametrize("name", FC.PER_FORM)
def test_chain_default_schedule(name):
    """The default schedule (theta = 0 until the 5th solve after a reset, 0.5 until the 12th, then 1) over 14 steps."""
    _chain(name, "", 14)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", FC.HOST_CALL_CASES + tuple(n for n in FC.NAMES if FC.make(n)["claims"]["large"]))
def test_a_step_after_each_host_call(name, order):
    """_form_cases.orders: every host call on the small cases; q, rho and matrices on the n = 8192 ones."""
    t = time.time()
    rng = np.random.default_rng(40 + order)
    with Rig(name, "1,2") as r:
        worst = 0.0
        for k in range(3):
            w, _, _ = r.step(f"step {k + 1} of 3", ("chain", "1,2", k), start=R.iterates(r.c) if k == 0 else None)
            worst = max(worst, w)
        seq = FC.orders(r.c)[order]
        for k, op in enumerate(seq):
            start = r.call(op, rng)
            w, _, _ = r.step(f"after {op} ({'/'.join(seq[:k + 1])})", ("host", order, k), start=start)
            worst = max(worst, w)
        print(f"[form-steps] {r.tag}: form {r.form} order {order}: {len(seq)} host calls, worst err/bar {worst:.3e}; {time.time() - t:.1f} s")
