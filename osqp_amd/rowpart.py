"""Row-partitioned single-QP solve over G GPUs (BASELINE config 5 "1 -> 8 MI355X").

One process per GPU (torch.distributed; backend "nccl" = RCCL over xGMI, "gloo" for rehearsals).  The reference has
no counterpart -- its linear solve is one thread (lin_sys/direct/qdldl/qdldl_interface.c:216) -- so the contract is
the survey's: the rows of A and the (block-diagonal) entries of P are sharded, the n-vectors are replicated, and the
only data-path traffic is

  * ONE all-reduce of an n-vector per PCG iteration:  K u = sigma u + sum_g [ P_g u + A_g' (rho_g . (A_g u)) ],
  * ONE all-reduce of an n-vector per ADMM iteration for the right-hand side  A'(rho z - y) = sum_g A_g'(.)_g,
  * two n-vectors and a handful of scalars at each termination check.

Because every rank holds the same x, r, p, ... after the all-reduce (a ring all-reduce leaves identical bits on every
rank), the PCG dot products are computed redundantly and need NO scalar collective, and all ranks take the same
decisions.  The m-vectors z, y, l, u, rho live only on the rank that owns their rows.

Algorithm = the reference's ADMM (src/osqp.c:354-532, src/auxil.c:161-225) in the scaled space of scale_data
(src/scaling.c:44-156) with the indirect KKT solve of engine.hip (Jacobi-PCG on P + sigma I + A' rho A), termination
and rho adaptation as src/auxil.c:13-74, 240-359, 681-740.  Scope: statuses solved / solved inaccurate / maximum
iterations reached, and with eps_prim_inf / eps_dual_inf > 0 primal / dual infeasible and their inaccurate forms with
certificates (src/auxil.c:361-512; two more all-reduces per check); q, the bounds, the iterates and rho of a set-up
solver can be replaced (update, warm_start, update_rho).  No polish and no matrix updates in this variant.

The SpMVs -- the part that touches the matrices -- run in the HIP kernels of the rank's shard engine
(hipeng_spmv_dev); vectors are torch tensors in HBM and the O(n) vector arithmetic between collectives is
torch element-wise code: with a collective after every operator apply this variant is bound by all-reduce latency,
not by those passes.  Expected break-even: an all-reduce of 400 KB over xGMI costs ~20-30 us
against ~26 us for a whole single-GPU PCG iteration at config 5 -- the partition pays only when the local operator
apply is well above that, i.e. for P blocks / A shards of several hundred MB per GPU.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
from scipy import sparse

from . import _abi

RHO_MIN, RHO_MAX, RHO_TOL, RHO_EQ = 1e-6, 1e6, 1e-4, 1e3
OSQP_INFTY = 1e30
INF_BOUND = OSQP_INFTY * 1e-4
DIV_TOL = 1e-30
_DEFAULTS = dict(rho=0.1, sigma=1e-6, alpha=1.6, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000, check_termination=25,
                 adaptive_rho=1, adaptive_rho_interval=0, adaptive_rho_tolerance=5.0, scaled_termination=0,
                 pcg_eps_rel=1e-9, pcg_max_iter=0, eps_prim_inf=0.0, eps_dual_inf=0.0)
INFEASIBLE = ("primal infeasible", "primal infeasible inaccurate", "dual infeasible", "dual infeasible inaccurate")


def _settings(settings):
    st = dict(_DEFAULTS)
    for k, v in settings.items():
        if k not in st:
            raise ValueError("unsupported setting %r in the row-partitioned variant" % k)
        st[k] = v
    if st["eps_prim_inf"] < 0 or st["eps_dual_inf"] < 0:
        raise ValueError("eps_prim_inf and eps_dual_inf must not be negative (0 switches the test off)")
    return st


def _row_class(l, u):
    """-1 free, 1 equality, 0 inequality from the scaled bounds (set_rho_vec, src/auxil.c:28-52)."""
    return np.where((l < -INF_BOUND) & (u > INF_BOUND), -1, np.where(u - l < RHO_TOL, 1, 0))


def _full(v, count, name):
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.shape != (count,):
        raise ValueError("%s must have %d entries" % (name, count))
    return v


def _rows_of(v, m, r0, r1, name):
    return np.ascontiguousarray(_full(v, m, name)[r0:r1])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _engine_on(device, **setup_kw):
    """A single-GPU solver set up on `device`; the device option is as before afterwards."""
    import osqp_amd
    old = osqp_amd.engine_options()["device"]
    osqp_amd.set_engine_options(device=device)
    try:
        return osqp_amd.OSQP().setup(**setup_kw)
    finally:
        osqp_amd.set_engine_options(device=old)


def _shard_engine(Pu_g, A_g, device):
    """The rank's shard (P_g, A_g) resident in an ordinary engine: scaling = 0 on already scaled data (a shard with no rows still
    needs one for its part of P).  Returns the solver, its library with the signatures bound, and the engine."""
    n, m = Pu_g.shape[0], A_g.shape[0]
    solver = _engine_on(device, P=Pu_g, q=np.zeros(n), A=A_g, l=-np.ones(m), u=np.ones(m), scaling=0, sigma=1.0)
    return solver, bind_live(solver._lib), solver.engine()


def _ranges(indptr, world):
    """Contiguous ranges of the rows (columns) behind a CSR (CSC) indptr with about equal numbers of non-zeros."""
    cuts = [0] + [int(np.searchsorted(indptr, indptr[-1] * g / world)) for g in range(1, world)] + [len(indptr) - 1]
    return [(cuts[g], max(cuts[g], cuts[g + 1])) for g in range(world)]


def shard_rows(A, world):
    """Contiguous row ranges of A with about equal numbers of non-zeros."""
    return _ranges(sparse.csr_matrix(A).indptr, world)


def shard_triu(Pu, world):
    """Split the stored upper triangle of P by contiguous column ranges: P = sum_g sym(P_g)."""
    Pc = sparse.csc_matrix(Pu)
    n = Pc.shape[0]
    out = []
    for j0, j1 in _ranges(Pc.indptr, world):
        part = sparse.csc_matrix(Pc[:, j0:j1])
        M = sparse.hstack([sparse.csc_matrix((n, j0)), part, sparse.csc_matrix((n, n - j1))], format="csc")
        out.append(sparse.triu(M, format="csc"))
    return out


class ScipyOps:
    """SpMV back end on the CPU (rehearsals of the collective logic with gloo): same interface as HipOps."""

    def __init__(self, Pu_g, A_g, device=None):
        import torch
        self.torch = torch
        self.P = (Pu_g + sparse.triu(Pu_g, 1).T).tocsr()
        self.A = sparse.csr_matrix(A_g)
        self.At = self.A.T.tocsr()
        self.device = torch.device("cpu")

    def vec(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).clone()

    def A_mul(self, x):
        return self.torch.from_numpy(self.A @ x.numpy())

    def At_mul(self, y):
        return self.torch.from_numpy(self.At @ y.numpy())

    def P_mul(self, x):
        return self.torch.from_numpy(self.P @ x.numpy())

    def diag_terms(self):
        return self.P.diagonal(), self.A.multiply(self.A).tocsc()


class HipOps:
    """SpMV back end on the rank's GPU: the shard (P_g, A_g) is resident in a HIP engine (set up with scaling = 0 on
    already scaled data) and the products run in its k_spmv kernels on device pointers."""

    def __init__(self, Pu_g, A_g, device=0):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.n, self.m = Pu_g.shape[0], A_g.shape[0]
        self._A = sparse.csr_matrix(A_g)
        self._P = Pu_g
        self.solver, self._L, self._e = _shard_engine(Pu_g, A_g, device)

    def vec(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(self.device)

    def _spmv(self, which, x, outlen):
        t = self.torch
        x = x.contiguous()
        y = t.zeros(max(outlen, 1), dtype=t.float64, device=self.device)
        t.cuda.current_stream(self.device).synchronize()          # x written by torch before the engine's stream reads it
        rc = self._L.hipeng_spmv_dev(self._e, which, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()))
        if rc or self._L.hipeng_sync(self._e):
            raise RuntimeError("hipeng_spmv_dev failed (%d)" % rc)
        return y[:outlen]

    def A_mul(self, x):
        return self._spmv(0, x, self.m)

    def At_mul(self, y):
        if self.m == 0:
            return self.torch.zeros(self.n, dtype=self.torch.float64, device=self.device)
        return self._spmv(1, y, self.n)

    def P_mul(self, x):
        return self._spmv(2, x, self.n)

    def diag_terms(self):
        Pf = self._P + sparse.triu(self._P, 1).T
        return Pf.diagonal(), self._A.multiply(self._A).tocsc()


def scaled_problem_from_handle(s):
    """The scaled problem (scale_data, src/scaling.c:44-156) read back from the mirrors of a set-up workspace:
    P (upper triangle), q, A, l, u and D, E, c."""
    w = s.work
    n, m = s.n, s.m

    def mat(cp, rows):
        c = cp.contents
        p = np.ctypeslib.as_array(c.p, shape=(n + 1,)).copy(); nnz = int(p[-1])
        i = np.ctypeslib.as_array(c.i, shape=(max(nnz, 1),))[:nnz].copy(); x = np.ctypeslib.as_array(c.x, shape=(max(nnz, 1),))[:nnz].copy()
        return sparse.csc_matrix((x, i, p), shape=(rows, n))
    d = w.data.contents
    out = dict(P=mat(d.P, n), A=mat(d.A, m), q=s._vec(d.q, n), l=s._vec(d.l, m), u=s._vec(d.u, m))
    if w.settings.contents.scaling:
        sc = w.scaling.contents
        out.update(D=s._vec(sc.D, n), E=s._vec(sc.E, m), c=float(sc.c))
    else:
        out.update(D=np.ones(n), E=np.ones(m), c=1.0)
    return out


def scaled_problem_from_engine(P, q, A, l, u, scaling=10, device=0):
    """scale_data as the single-GPU engine performs it (hipeng_ruiz_scale), so that the row-partitioned variant
    iterates in exactly the scaled space of the single-GPU path."""
    s = _engine_on(device, P=P, q=q, A=A, l=l, u=u, scaling=scaling)
    out = scaled_problem_from_handle(s)
    s.cleanup()
    return out


class _RowPartitioned:
    """What the torch-driven and the C-driven solver share: the rank's place in the group, its shard, the checks of full-length
    arguments, the gather of an m-vector and the shape of a result.  `self.dev`: where the rank's tensors live (set by setup)."""

    def __init__(self, group=None, world=None):
        # world=1: no process group and no torch at all (a plain C caller's situation; tools/rccl_world1_probe.py)
        self.torch = self.dist = None
        self.group, self.world, self.rank = group, 1, 0
        if world != 1:
            import torch
            import torch.distributed as dist
            self.torch, self.dist = torch, dist
            if dist.is_initialized():
                self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)

    def _shard(self, scaled):
        """Sets n, m, rows and the rank's [r0, r1); returns the rank's (P_g, A_g)."""
        self.n, self.m = scaled["P"].shape[0], scaled["A"].shape[0]
        self.rows = shard_rows(scaled["A"], self.world)
        self.r0, self.r1 = self.rows[self.rank]
        return shard_triu(scaled["P"], self.world)[self.rank], sparse.csr_matrix(scaled["A"])[self.r0:self.r1]

    def _rows(self, v, name):
        return _rows_of(v, self.m, self.r0, self.r1, name)

    def _update_args(self, q, l, u):
        """The arguments of update(): q of full length, the rank's rows of l and u (None: not given)."""
        if (l is None) != (u is None):
            raise ValueError("l and u are updated together in the row-partitioned variant")
        q = None if q is None else _full(q, self.n, "q")
        return (q, None, None) if l is None else (q, self._rows(l, "l"), self._rows(u, "u"))

    def _gather_rows(self, yl):
        """An m-vector from the row shards (once per solve, off the data path): the rank's rows as a numpy array or a tensor in,
        the full numpy vector out; gathered device to device with nccl, on the host otherwise."""
        if self.world == 1:
            return yl if isinstance(yl, np.ndarray) else yl.cpu().numpy()
        t, d = self.torch, self.dist
        yl = t.from_numpy(yl) if isinstance(yl, np.ndarray) else yl
        per = max(b - a for a, b in self.rows)
        pad = t.zeros(per, dtype=t.float64, device=self.dev if d.get_backend(self.group) == "nccl" else "cpu")
        pad[:yl.numel()] = yl
        out = t.empty(self.world * per, dtype=t.float64, device=pad.device)
        d.all_gather_into_tensor(out, pad, group=self.group)
        out = out.cpu().numpy()
        return np.concatenate([out[g * per:g * per + (b - a)] for g, (a, b) in enumerate(self.rows)])

    @staticmethod
    def _result(x, y, prim_inf_cert, dual_inf_cert, **info):
        return SimpleNamespace(x=x, y=y, info=SimpleNamespace(**info), prim_inf_cert=prim_inf_cert, dual_inf_cert=dual_inf_cert)


class RowPartitionedOSQP(_RowPartitioned):
    """osqp_setup / osqp_solve for ONE QP whose matrices are sharded over the ranks of a torch.distributed group."""

    def __init__(self, group=None):
        super().__init__(group)
        self.collectives = 0

    @property
    def _unscaled(self):
        """The unscaled forms of residuals, norms and certificates decide (scaled data without scaled_termination)."""
        return self.scaled_data and not self.st["scaled_termination"]

    # ---- collectives (device to device with nccl; staged through the host for a gloo rehearsal) ----
    def _allreduce(self, t, op="sum"):
        if self.world == 1:
            return t
        d = self.dist
        self.collectives += 1
        rop = d.ReduceOp.SUM if op == "sum" else d.ReduceOp.MAX
        if t.is_cuda and d.get_backend(self.group) != "nccl":
            h = t.cpu(); d.all_reduce(h, op=rop, group=self.group); t.copy_(h)
        else:
            d.all_reduce(t, op=rop, group=self.group)
        return t

    def setup(self, scaled, ops_factory, device=0, **settings):
        """`scaled`: dict(P (triu), q, A, l, u, D, E, c) -- the scaled problem, identical on every rank;
        `ops_factory(Pu_g, A_g, device)` builds the rank's SpMV back end (HipOps on a GPU)."""
        st = self.st = _settings(settings)
        Pg, Ag = self._shard(scaled)
        n, r0, r1 = self.n, self.r0, self.r1
        o = self.ops = ops_factory(Pg, Ag, device)
        self.dev = o.device
        self.q = o.vec(scaled["q"]); self.l = o.vec(scaled["l"][r0:r1]); self.u = o.vec(scaled["u"][r0:r1])
        self.D = o.vec(scaled["D"]); self.Dinv = 1.0 / self.D
        self.E = o.vec(scaled["E"][r0:r1]); self.Einv = 1.0 / self.E
        self.c = float(scaled["c"]); self.cinv = 1.0 / self.c
        self.scaled_data = bool(np.any(scaled["D"] != 1.0) or np.any(scaled["E"] != 1.0) or scaled["c"] != 1.0)
        self.cls = _row_class(scaled["l"][r0:r1], scaled["u"][r0:r1])
        self.has_eq = bool(self._allreduce(o.vec([float((self.cls == 1).any())]), "max").item() > 0)
        self._pdiag, self._a2 = o.diag_terms()           # this rank's share of diag(P) and of A.^2 (column sums weighted by rho)
        t = self.torch
        self.x = t.zeros(n, dtype=t.float64, device=o.device); self.xt = self.x.clone()
        self.z = t.zeros(r1 - r0, dtype=t.float64, device=o.device); self.y = self.z.clone()
        self._set_rho(st["rho"])
        self.rho_updates = 0
        self.status = "unsolved"
        return self

    # ---- a live solver: unscaled arrays of full length in, the rank's rows taken here (every rank calls each of these) ----
    def update(self, q=None, l=None, u=None):
        """osqp_update_lin_cost / osqp_update_bounds (src/osqp.c:765-846).  l and u come together.  Returns 1 on every rank, with
        nothing changed on any, when l > u on some row; a row that changes class on some rank rebuilds rho per row and the
        preconditioner on every rank."""
        o = self.ops
        q, lo, hi = self._update_args(q, l, u)
        if l is not None:
            lo, hi = np.maximum(lo, -OSQP_INFTY), np.minimum(hi, OSQP_INFTY)
            E = self.E.cpu().numpy()
            ls, us = E * lo, E * hi
            cls = _row_class(ls, us)
            flags = self._allreduce(o.vec([float((lo > hi).any()), float((cls != self.cls).any()), float((cls == 1).any())]), "max")
            bad, changed, has_eq = (bool(v > 0) for v in flags.cpu().numpy())
            if bad:
                return 1
        if q is not None:
            self.q = (self.D * o.vec(q)) * self.c
            self.rho_updates = 0                         # reset_info
        if l is not None:
            self.l, self.u, self.cls, self.has_eq = o.vec(ls), o.vec(us), cls, has_eq
            self.rho_updates = 0
            if changed:
                self._set_rho(self.rho)
        return 0

    def warm_start(self, x=None, y=None):
        """osqp_warm_start (src/osqp.c:942-1010): x_s = Dinv x, z = A x_s on the rank's rows, y_s = c Einv y; x~ starts from x_s."""
        o = self.ops
        if x is not None:
            self.x = self.Dinv * o.vec(_full(x, self.n, "x"))
            self.xt = self.x.clone()
            if self.r1 > self.r0:
                self.z = o.A_mul(self.x)
        if y is not None:
            self.y = (self.Einv * o.vec(self._rows(y, "y"))) * self.c
        return 0

    def update_rho(self, rho):
        """osqp_update_rho (src/osqp.c:1281-1330): rho <= 0 returns 1 and changes nothing; rho_updates is not reset."""
        if not rho > 0:
            return 1
        self._set_rho(float(rho))
        return 0

    def _set_rho(self, rho):
        rho = min(max(rho, RHO_MIN), RHO_MAX)
        self.rho = rho
        rv = np.where(self.cls == -1, RHO_MIN, np.where(self.cls == 1, RHO_EQ * rho, rho))
        self.rho_vec = self.ops.vec(rv)
        # Jacobi preconditioner: diag(P) + sigma + sum_i rho_i A_ij^2, the shard sums meet in one all-reduce
        local = self._pdiag + (np.asarray(self._a2.T @ rv).ravel() if self.m and rv.size else 0.0)
        diag = self._allreduce(self.ops.vec(local))
        self.minv = 1.0 / (diag + self.st["sigma"])

    # ---- operator and PCG -------------------------------------------------------------------------
    def _K(self, u):
        o = self.ops
        part = o.P_mul(u)
        if self.r1 > self.r0:
            part = part + o.At_mul(self.rho_vec * o.A_mul(u))
        return self._allreduce(part) + self.st["sigma"] * u       # the one n-vector all-reduce of a PCG iteration

    def _pcg(self, b, x0, eps_rel):
        n = self.n
        cap = self.st["pcg_max_iter"] or max(20000, 10 * n)
        x = x0.clone()
        r = b - self._K(x)
        tol2 = max(eps_rel * eps_rel * float(b @ b), DIV_TOL)
        z = self.minv * r
        p = z.clone()
        rz = float(r @ z)
        it = 0
        while float(r @ r) > tol2 and it < cap:
            Kp = self._K(p)
            a = rz / float(p @ Kp)
            x += a * p
            r -= a * Kp
            z = self.minv * r
            rz2 = float(r @ z)
            p = z + (rz2 / rz) * p
            rz = rz2
            it += 1
        self.pcg_iters += it
        return x

    # ---- residuals, termination, rho ---------------------------------------------------------------
    def _info(self):
        t, o = self.torch, self.ops
        Ax = o.A_mul(self.x) if self.r1 > self.r0 else self.z
        pri = Ax - self.z
        mx = lambda v: v.abs().max() if v.numel() else t.zeros((), dtype=t.float64, device=o.device)       # (a rank without rows)
        loc = t.stack([mx(self.Einv * pri), mx(self.Einv * self.z), mx(self.Einv * Ax), mx(pri), mx(self.z), mx(Ax)])
        pri_u, z_u, Ax_u, pri_s, z_s, Ax_s = (float(v) for v in self._allreduce(loc, "max"))
        both = t.cat([o.P_mul(self.x), o.At_mul(self.y) if self.r1 > self.r0 else t.zeros_like(self.x)])
        both = self._allreduce(both)
        Px, Aty = both[:self.n], both[self.n:]
        dua = Px + self.q + Aty
        f = lambda v, S=None: float((v if S is None else S * v).abs().max())
        s = dict(pri_u=pri_u, z_u=z_u, Ax_u=Ax_u, pri_s=pri_s, z_s=z_s, Ax_s=Ax_s,
                 dua_u=f(dua, self.Dinv), dua_s=f(dua), q_u=f(self.q, self.Dinv), q_s=f(self.q), Aty_u=f(Aty, self.Dinv), Aty_s=f(Aty),
                 Px_u=f(Px, self.Dinv), Px_s=f(Px), obj=float(self.x @ (0.5 * Px + self.q)) * self.cinv)
        self.sc = s
        un = self._unscaled
        self.pri_res = 0.0 if self.m == 0 else (s["pri_u"] if un else s["pri_s"])
        self.dua_res = self.cinv * s["dua_u"] if un else s["dua_s"]

    def _cert_scalars(self):
        """The seven scalars of is_primal_infeasible / is_dual_infeasible (src/auxil.c:361-512) from dx, dy: one all-reduce (sum) of
        [P_g dx ; A_g' dy ; u'dy+ + l'dy-] and one (max) of [|E dy| ; row violation], everything computed every time."""
        t, o, n, un = self.torch, self.ops, self.n, self._unscaled
        have = self.r1 > self.r0
        zero = t.zeros((), dtype=t.float64, device=o.device)
        dx = self.x - self.x_prev
        dy = self.y - self.y_prev
        infu, infl = self.u > INF_BOUND, self.l < -INF_BOUND
        dy = t.where(infu & infl, t.zeros_like(dy), t.where(infu, t.minimum(dy, t.zeros_like(dy)), t.where(infl, t.maximum(dy, t.zeros_like(dy)), dy)))
        self.dx, self.dy = dx, dy
        ndy, viol, lhs = zero, zero, zero
        if have:
            ndy = ((self.E * dy) if un else dy).abs().max()
            lhs = (self.u * dy.clamp(min=0.0) + self.l * dy.clamp(max=0.0)).sum()
            adx = o.A_mul(dx)
            if un:
                adx = self.Einv * adx
            # the largest (A dx)_i of a row with a finite u and -(A dx)_i of one with a finite l; never below 0 (the test is `> eps |dx|`)
            viol = t.maximum(t.where(~infu, adx, t.zeros_like(adx)).max(), t.where(~infl, -adx, t.zeros_like(adx)).max()).clamp(min=0.0)
        sums = self._allreduce(t.cat([o.P_mul(dx), o.At_mul(dy) if have else t.zeros_like(dx), lhs.reshape(1)]))
        mx = self._allreduce(t.stack([ndy, viol]), "max")
        Pdx, Atdy = sums[:n], sums[n:2 * n]
        f = lambda v, S: float((S * v if un else v).abs().max())
        self.cs = dict(ndy=float(mx[0]), viol=float(mx[1]), lhs=float(sums[2 * n]), nAtdy=f(Atdy, self.Dinv),
                       ndx=f(dx, self.D), qdx=float(self.q @ dx), nPdx=f(Pdx, self.Dinv))

    def _verdict(self, approximate=False):
        """check_termination with the infeasibility tests (src/auxil.c:716-783): None, "solved", "primal infeasible" or "dual infeasible";
        only all-reduced and replicated values are looked at, so every rank decides alike.  A test whose tolerance is 0 is off before its
        scalars are looked up: with both off there is no self.cs, and this is the residual test alone."""
        un, s, st = self._unscaled, self.sc, self.st
        k = 10.0 if approximate else 1.0
        eps_abs, eps_rel = k * st["eps_abs"], k * st["eps_rel"]
        prim_ok = self.m == 0 or self.pri_res < eps_abs + eps_rel * (max(s["z_u"], s["Ax_u"]) if un else max(s["z_s"], s["Ax_s"]))
        nrm = self.cinv * max(s["q_u"], s["Aty_u"], s["Px_u"]) if un else max(s["q_s"], s["Aty_s"], s["Px_s"])
        dual_ok = self.dua_res < eps_abs + eps_rel * nrm
        if prim_ok and dual_ok:
            return "solved"
        ep, ed, cost = k * st["eps_prim_inf"], k * st["eps_dual_inf"], (self.c if un else 1.0)
        if not prim_ok and ep > 0:
            c = self.cs
            if c["ndy"] > DIV_TOL and c["lhs"] < ep * c["ndy"] and c["nAtdy"] < ep * c["ndy"]:
                return "primal infeasible"
        if not dual_ok and ed > 0:
            c = self.cs
            if c["ndx"] > DIV_TOL and c["qdx"] < cost * ed * c["ndx"] and c["nPdx"] < cost * ed * c["ndx"] and not c["viol"] > ed * c["ndx"]:
                return "dual infeasible"
        return None

    def _rho_estimate(self):
        s = self.sc
        pri = (s["pri_s"] if self.m else 0.0) / (max(s["z_s"], s["Ax_s"]) + DIV_TOL)
        dua = s["dua_s"] / (max(s["q_s"], s["Aty_s"], s["Px_s"]) + DIV_TOL)
        return min(max(self.rho * np.sqrt(pri / dua), RHO_MIN), RHO_MAX)

    # ---- solve ---------------------------------------------------------------------------------------
    def solve(self):
        st, o, t = self.st, self.ops, self.torch
        e = min(st["eps_abs"] or st["eps_rel"], st["eps_rel"] or st["eps_abs"])
        eps_pcg = max(1e-13, min(st["pcg_eps_rel"], 1e-5 * e))      # the rule of osqp_solve (osqp_host.c)
        if self.has_eq:
            eps_pcg = max(1e-13, 1e-3 * eps_pcg)
        interval = st["adaptive_rho_interval"] or (4 * st["check_termination"] if st["check_termination"] else 100)
        self.pcg_iters = 0
        alpha, sigma = st["alpha"], st["sigma"]
        cert = st["eps_prim_inf"] > 0 or st["eps_dual_inf"] > 0

        def check():             # one termination check: the verdict of check_termination, on seven more scalars with a test on
            self._info()
            if cert:
                self._cert_scalars()
            return self._verdict()
        status, it, checked = "unsolved", 0, False
        for it in range(1, st["max_iter"] + 1):
            w = self.rho_vec * self.z - self.y
            b = sigma * self.x - self.q + self._allreduce(o.At_mul(w) if self.r1 > self.r0 else t.zeros_like(self.x))
            self.xt = self._pcg(b, self.xt, eps_pcg)
            zt = o.A_mul(self.xt) if self.r1 > self.r0 else self.z
            checked = bool(st["check_termination"]) and it % st["check_termination"] == 0
            if cert and (checked or it == st["max_iter"]):          # this iteration ends in a check: x and y as they are now
                self.x_prev, self.y_prev = self.x, self.y
            self.x = alpha * self.xt + (1.0 - alpha) * self.x
            v = alpha * zt + (1.0 - alpha) * self.z
            zn = t.minimum(t.maximum(v + self.y / self.rho_vec, self.l), self.u)
            self.y = self.y + self.rho_vec * (v - zn)
            self.z = zn
            if checked:
                v = check()
                if v:
                    status = v
                    break
            if st["adaptive_rho"] and it % interval == 0:
                if not checked:
                    self._info()
                new = self._rho_estimate()
                if new > self.rho * st["adaptive_rho_tolerance"] or new < self.rho / st["adaptive_rho_tolerance"]:
                    self._set_rho(new)
                    self.rho_updates += 1
        if not checked:
            status = check() or "unsolved"
        if status == "unsolved":     # the approximate branch: 10 x every tolerance on the same scalars
            v = self._verdict(approximate=True)
            status = v + " inaccurate" if v else "maximum iterations reached"
        self.status = status
        obj, rho_estimate = self.sc["obj"], self._rho_estimate()
        nan_x, nan_m = np.full(self.n, np.nan), np.full(self.m, np.nan)
        prim_inf_cert, dual_inf_cert = nan_m, nan_x
        if status in INFEASIBLE:
            # store_solution (src/auxil.c:536-560): no solution, the certificate normalised, the iterates back to zero (rho stays)
            un = self._unscaled
            x, y = nan_x, nan_m
            if status.startswith("primal"):
                obj = OSQP_INFTY
                prim_inf_cert = self._gather_rows(((self.E * self.dy) if un else self.dy) * (1.0 / self.cs["ndy"]))
            else:
                obj = -OSQP_INFTY
                dual_inf_cert = (((self.D * self.dx) if un else self.dx) * (1.0 / self.cs["ndx"])).cpu().numpy()
            self.x, self.xt = t.zeros_like(self.x), t.zeros_like(self.x)
            self.z, self.y = t.zeros_like(self.z), t.zeros_like(self.z)
        else:
            # unscale; y is gathered from the row shards
            x = (self.D * self.x).cpu().numpy()
            y = self._gather_rows(self.E * self.y * self.cinv)
        return self._result(x, y, prim_inf_cert, dual_inf_cert, status=status, iter=it, obj_val=obj, pri_res=self.pri_res, dua_res=self.dua_res,
                            rho_updates=self.rho_updates, rho_estimate=rho_estimate, pcg_iters=self.pcg_iters, collectives=self.collectives)


# ------------------------------------------------------------------------------------------------------------------
# The same solve driven from C (include/osqp_amd_rowpart.h, csrc/rowpart_native.h): kernels, collectives and the PCG's
# stopping decisions are issued by osqp_amd_rp_solve on the shard engine's stream.  Python only shards the matrices,
# creates the engine and -- for a gloo rehearsal -- lends its process group as the collective.
# ------------------------------------------------------------------------------------------------------------------
class _RpSettings(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("rho", "sigma", "alpha", "eps_abs", "eps_rel", "adaptive_rho_tolerance", "pcg_eps_rel")] + \
               [(k, C.c_int) for k in ("max_iter", "check_termination", "adaptive_rho", "adaptive_rho_interval", "scaled_termination", "pcg_max_iter")]


class _RpInfo(C.Structure):
    _fields_ = [("status", C.c_int), ("iter", C.c_int), ("rho_updates", C.c_int), ("pcg_iters", C.c_longlong), ("collectives", C.c_longlong),
                ("obj_val", C.c_double), ("pri_res", C.c_double), ("dua_res", C.c_double), ("rho_estimate", C.c_double)]


_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p)
_PRIMAL = (_abi.OSQP_PRIMAL_INFEASIBLE, _abi.OSQP_PRIMAL_INFEASIBLE_INACCURATE)
_DUAL = (_abi.OSQP_DUAL_INFEASIBLE, _abi.OSQP_DUAL_INFEASIBLE_INACCURATE)
_STATUS = {v: _abi.STATUS[v] for v in (_abi.OSQP_SOLVED, _abi.OSQP_SOLVED_INACCURATE, _abi.OSQP_MAX_ITER_REACHED) + _PRIMAL + _DUAL}

# every entry point this module calls (include/osqp_amd_engine.h, include/osqp_amd_rowpart.h): result type, argument types
_H = _P = C.c_void_p
_SIGNATURES = {
    "hipeng_spmv_dev": (C.c_int, [_H, C.c_int, _P, _P]),
    "hipeng_sync": (C.c_int, [_H]),
    "osqp_amd_rp_create": (_H, [_H, _P, _P, _P, _P, _P, C.c_double, C.c_int, C.c_int, C.POINTER(_RpSettings), C.c_int, C.c_int, _ALLREDUCE_FN, _P]),
    "osqp_amd_rp_solve": (C.c_int, [_H, C.POINTER(_RpInfo)]),
    "osqp_amd_rp_get_solution": (C.c_int, [_H, _P, _P]),
    "osqp_amd_rp_free": (None, [_H]),
    "osqp_amd_rp_rccl_unique_id": (C.c_int, [_P, C.c_int]),
    "osqp_amd_rp_use_rccl": (C.c_int, [_H, _P, C.c_int]),
    "osqp_amd_rp_peek": (C.c_int, [_H, C.c_int, _P, C.c_longlong]),
    "osqp_amd_rp_test_verdict": (C.c_int, [_P, C.c_int, C.c_double, C.c_int, _P, C.c_double, C.c_double, C.c_int]),
    "osqp_amd_rp_set_infeasibility": (C.c_int, [_H, C.c_double, C.c_double]),
    "osqp_amd_rp_get_certificates": (C.c_int, [_H, _P, _P]),
    "osqp_amd_rp_update_lin_cost": (C.c_int, [_H, _P]),
    "osqp_amd_rp_update_bounds": (C.c_int, [_H, _P, _P]),
    "osqp_amd_rp_warm_start": (C.c_int, [_H, _P, _P]),
    "osqp_amd_rp_update_rho": (C.c_int, [_H, C.c_double]),
}


def bind_live(L):
    """Declares the signatures of _SIGNATURES on the library L and returns it."""
    for name, (res, args) in _SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


class _DevView:
    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = dict(shape=(int(count),), typestr="<f8", data=(int(ptr), False), version=2, strides=None)


class NativeRowPartitionedOSQP(_RowPartitioned):
    """osqp_setup / osqp_solve of ONE row-partitioned QP through the C entry points osqp_amd_rp_*.
    collective = "rccl": ncclAllReduce of librccl on the engine's stream (the production path, one GPU per rank);
                 "group": the torch.distributed group as a callback (any backend; gloo stages through the host);
                 "auto": rccl when the group's backend is nccl, else group."""

    def __init__(self, group=None, collective="auto", world=None):
        super().__init__(group, world)
        d = self.dist
        if collective == "auto":
            collective = "rccl" if (d is not None and d.is_initialized() and d.get_backend(group) == "nccl") else "group"
        self.collective = collective
        self._rp = None

    def _group_allreduce(self, user, buf, count, op, stream):
        # the callback form of the collective: everything queued on the engine's stream first, then the group's all-reduce on
        # the wrapped device memory, complete before this returns (osqp_amd_rowpart.h: "a synchronous one")
        try:
            t, d = self.torch, self.dist
            if self._L.hipeng_sync(self._e):
                return 1
            v = t.as_tensor(_DevView(buf, count), device=self.dev)
            rop = d.ReduceOp.MAX if op else d.ReduceOp.SUM
            if d.get_backend(self.group) == "nccl":
                d.all_reduce(v, op=rop, group=self.group)
            else:
                h = v.cpu(); d.all_reduce(h, op=rop, group=self.group); v.copy_(h)
            t.cuda.synchronize(self.dev)
            return 0
        except Exception as ex:                          # an exception must not unwind through the C frames
            import sys
            print("osqp_amd.rowpart: collective failed: %r" % (ex,), file=sys.stderr)
            return 1

    def setup(self, scaled, device=0, **settings):
        t, d = self.torch, self.dist
        st = _settings(settings)
        eps_inf = (float(st.pop("eps_prim_inf")), float(st.pop("eps_dual_inf")))
        Pg, Ag = self._shard(scaled)
        r0, r1 = self.r0, self.r1
        self.shard, self._L, self._e = _shard_engine(Pg, Ag, device)
        L = self._L
        self.dev = t.device("cuda", device) if t is not None else None
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        lg, ug = f64(scaled["l"][r0:r1]), f64(scaled["u"][r0:r1])
        has_eq = float(np.any(ug - lg < RHO_TOL))
        if self.world > 1:
            flag = t.tensor([has_eq], dtype=t.float64, device=self.dev if d.get_backend(self.group) == "nccl" else "cpu")
            d.all_reduce(flag, op=d.ReduceOp.MAX, group=self.group)
            has_eq = float(flag.item())
        kinds = dict(_RpSettings._fields_)
        s = _RpSettings(**{k: (float(v) if kinds[k] is C.c_double else int(v)) for k, v in st.items()})
        self._cb = _ALLREDUCE_FN(self._group_allreduce)              # kept alive with the object
        q, D, E = f64(scaled["q"]), f64(scaled["D"]), f64(scaled["E"][r0:r1])
        self._rp = L.osqp_amd_rp_create(self._e, _ptr(q), _ptr(lg), _ptr(ug), _ptr(D), _ptr(E), float(scaled["c"]), int(self.m), int(has_eq > 0),
                                        C.byref(s), self.world, self.rank, self._cb, None)
        if not self._rp:
            raise RuntimeError("osqp_amd_rp_create failed")
        if eps_inf[0] > 0 or eps_inf[1] > 0:              # (a handle that never makes the call solves as before the tests existed)
            self.set_infeasibility(*eps_inf)
        if self.collective == "rccl" and self.world > 1:
            idb = t.zeros(128, dtype=t.uint8)
            if self.rank == 0:
                idb = t.frombuffer(bytearray(self._rccl_id()), dtype=t.uint8).clone()
            on = self.dev if d.get_backend(self.group) == "nccl" else "cpu"
            idb = idb.to(on)
            d.broadcast(idb, src=0, group=self.group)
            raw = bytes(idb.cpu().numpy().tobytes())
            bad = t.tensor([float(L.osqp_amd_rp_use_rccl(self._rp, raw, 128) != 0)], dtype=t.float64, device=on)
            d.all_reduce(bad, op=d.ReduceOp.MAX, group=self.group)
            if bad.item() > 0:                         # every rank takes the same decision: the group serves as the collective
                import sys
                print("osqp_amd.rowpart: RCCL could not be attached on some rank; the process group is the collective", file=sys.stderr)
                L.osqp_amd_rp_use_rccl(self._rp, None, 0)
                self.collective = "group"
        return self

    def _rccl_id(self):
        raw = (C.c_char * 128)()
        if self._L.osqp_amd_rp_rccl_unique_id(raw, 128) != 128:
            raise RuntimeError("osqp_amd_rp_rccl_unique_id failed")
        return raw.raw

    def use_rccl_world1(self):
        """Test hook: the built-in RCCL provider on a one-rank communicator (dlopen, ncclCommInitRank, the stream-ordered call)."""
        return self._L.osqp_amd_rp_use_rccl(self._rp, self._rccl_id(), 128)

    def set_infeasibility(self, eps_prim_inf, eps_dual_inf):
        """Switch the infeasibility tests on (0: that test off); every rank with the same values."""
        if self._L.osqp_amd_rp_set_infeasibility(self._rp, float(eps_prim_inf), float(eps_dual_inf)):
            raise ValueError("eps_prim_inf and eps_dual_inf must not be negative")

    # ---- a live handle: unscaled arrays of full length in, the rank's rows taken here (every rank calls each of these) ----
    def _call(self, name, *args):
        rc = getattr(self._L, name)(self._rp, *args)
        if rc not in (0, 1):
            raise RuntimeError("%s failed (%d)" % (name, rc))
        return int(rc)

    def update(self, q=None, l=None, u=None):
        """New q and / or new bounds (l and u together).  Returns 1 on every rank, with the bounds unchanged on all of them, when l > u
        on some row."""
        q, lo, hi = self._update_args(q, l, u)
        # the bounds first: refused bounds leave q as it was, too
        if l is not None and self._call("osqp_amd_rp_update_bounds", _ptr(lo), _ptr(hi)):
            return 1
        if q is not None:
            self._call("osqp_amd_rp_update_lin_cost", _ptr(q))
        return 0

    def warm_start(self, x=None, y=None):
        x = None if x is None else _full(x, self.n, "x")
        yl = None if y is None else self._rows(y, "y")
        return self._call("osqp_amd_rp_warm_start", _ptr(x), _ptr(yl))

    def update_rho(self, rho):
        return self._call("osqp_amd_rp_update_rho", float(rho))

    def solve(self):
        info, k = _RpInfo(), self.r1 - self.r0
        rc = self._L.osqp_amd_rp_solve(self._rp, C.byref(info))
        if rc:
            raise RuntimeError("osqp_amd_rp_solve failed (%d)" % rc)
        x, yl = np.zeros(self.n), np.zeros(max(k, 1))
        if self._L.osqp_amd_rp_get_solution(self._rp, _ptr(x), _ptr(yl)):
            raise RuntimeError("osqp_amd_rp_get_solution failed")
        y = self._gather_rows(yl[:k])
        dual_inf_cert, prim_inf_cert = np.full(self.n, np.nan), np.full(self.m, np.nan)
        if info.status in _PRIMAL + _DUAL:
            pl = np.full(max(k, 1), np.nan)
            if self._L.osqp_amd_rp_get_certificates(self._rp, _ptr(dual_inf_cert), _ptr(pl)):
                raise RuntimeError("osqp_amd_rp_get_certificates failed")
            if info.status in _PRIMAL:                   # (the status is the same on every rank: all of them gather, or none)
                prim_inf_cert = self._gather_rows(pl[:k])
        return self._result(x, y, prim_inf_cert, dual_inf_cert, status=_STATUS.get(info.status, "unsolved"),
                            **{f: getattr(info, f) for f, _ in _RpInfo._fields_ if f != "status"})

    _PEEK = ("x", "xt", "z", "y", "rv", "minv", "b", "r", "sc15", "S", "dx", "dy", "sc7", "q", "l", "u")
    _S_FIELDS = ("rz0", "rz1", "rr", "tol2", "bb", "done", "iters", "cap", "bad")

    def peek(self, name):
        """For the tests (osqp_amd_rp_peek): one array of the handle's state in the scaled space, copied to the host; nothing
        is written on the device.  "S": the PCG's device-side record as a dict."""
        which = self._PEEK.index(name)
        cap = {"sc15": 15, "S": 9, "sc7": 7}.get(name, max(self.n, self.r1 - self.r0, 1))
        out = np.zeros(cap)
        k = self._L.osqp_amd_rp_peek(self._rp, which, _ptr(out), cap)
        if k < 0:
            raise RuntimeError("osqp_amd_rp_peek failed (%d)" % k)
        return dict(zip(self._S_FIELDS, out[:k])) if name == "S" else out[:k].copy()

    def cleanup(self):
        if self._rp:
            self._L.osqp_amd_rp_free(self._rp)
            self._rp = None
