// rowpart_native.h -- included at the end of engine.hip (it uses the engine's k_spmv of engine_aux_kernels.h, DevMat of
// engine_device.h and the allocation helpers of the host side).
//
// ONE QP over several GPUs by rows, the whole loop driven from C: include/osqp_amd_rowpart.h has the contract.  Per rank:
// the shard (P_g, A_g) in an ordinary engine, n-vectors replicated, m-vectors of the rank's rows.  All kernels and
// collectives go to the shard engine's stream; the PCG scalars live on the device (every rank computes the same ones),
// kernels of iterations issued past convergence return at once, and the host looks at one flag per group of iterations.
//
//   ADMM iteration (src/osqp.c:387-424):  w = rho z - y;  buf = A_g' w;  ALL-REDUCE(buf);  b = sigma x - q + buf
//                                         x~ = PCG(b, x~);  z~ = A_g x~;  update_x / update_z / update_y on the rank's rows
//   PCG iteration:                        t = rho (A_g p);  part = [P_g | A_g'] [p; t];  ALL-REDUCE(part);  Kp = part + sigma p
//                                         alpha = rz / p'Kp;  x~ += alpha p;  r -= alpha Kp;  z = Minv r;  p = z + (rz'/rz) p
//   termination check (src/auxil.c:681-740): six maxima (ALL-REDUCE max), [P x; A' y] (ALL-REDUCE of 2n), norms on the device.
//   with osqp_amd_rp_set_infeasibility (src/auxil.c:361-512):  dx = x - x_prev;  dy = y - y_prev projected on the polar of the
//                                         recession cone;  ALL-REDUCE([P_g dx; A_g' dy; u'dy+ + l'dy-]);  ALL-REDUCE max([|E dy|; row violation])
#include <dlfcn.h>
#include "../../include/osqp_amd_types.h"
#include "../../include/osqp_amd_rowpart.h"

#define RP_G 128                 // workgroups (= partials per dot product) of the n- and m-vector kernels
#define RP_DIV_TOL 1e-30         // the literal, not OSQP_DIVISION_TOL: 1.0 / 1e30 is another double
// The scalars of a termination check, in the order the device holds them (rp->sc15), the read-back carries them and the host keeps
// them (rp->sc); DESIGN.md section 7 has the table.  _U: unscaled with Einv / Dinv, _S: in the space the loop iterates in.
enum RpScalar {
  RSC_PRI_U, RSC_Z_U, RSC_AX_U, RSC_PRI_S, RSC_Z_S, RSC_AX_S,                               // k_rp_pri: |Ax - z|, |z|, |Ax| over the rows (ALL-REDUCE max)
  RSC_DUA_U, RSC_DUA_S, RSC_Q_U, RSC_Q_S, RSC_ATY_U, RSC_ATY_S, RSC_PX_U, RSC_PX_S, RSC_OBJ,   // k_rp_dua: |Px + q + A'y|, |q|, |A'y|, |Px|, x'(Px/2 + q)
  // the seven of the infeasibility tests, written only by a check with a test on: |E dy|, row violation (both ALL-REDUCE max),
  // u'dy+ + l'dy- (summed over the ranks), |Dinv A'dy|, |D dx|, q'dx, |Dinv P dx|
  RSC_NDY, RSC_VIOL, RSC_LHS, RSC_NATDY, RSC_NDX, RSC_QDX, RSC_NPDX,
  RSC_ALL, RSC_CHECK = RSC_NDY, RSC_CERT = RSC_ALL - RSC_CHECK,                           // 22 = 15 + 7
  RSC_CHECK_PAD = 16, RSC_ALL_PAD = 24                                                  // what a check zeroes and the buffers hold: padded to eight doubles
};
static_assert(RSC_CHECK == 15 && RSC_CERT == 7, "osqp_amd_rp_peek and osqp_amd_rp_test_verdict promise these counts");
// what a termination check finds (rp_verdict_of; osqp_amd_rp_test_verdict exports the values)
enum { RP_GO_ON = 0, RP_RESIDUALS_PASS = 1, RP_PRIMAL_INF = 3, RP_DUAL_INF = 4 };
struct RpS { double rz[2]; double rr, tol2, bb; int done, iters, cap, bad; };

// sum of RP_G partials, the same order in every workgroup and on every rank
__device__ __forceinline__ double rp_total(const double *part, double *red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < RP_G; i += TB) s += part[i];
  return block_sum(s, red);
}
__global__ void __launch_bounds__(TB) k_rp_w(int m, const double *rho, const double *z, const double *y, double *out) {
  for (int i = blockIdx.x * TB + threadIdx.x; i < m; i += gridDim.x * TB) out[i] = rho[i] * z[i] - y[i];
}
__global__ void __launch_bounds__(TB) k_rp_scale(int m, const double *rho, double *t) {
  for (int i = blockIdx.x * TB + threadIdx.x; i < m; i += gridDim.x * TB) t[i] *= rho[i];
}
// b = sigma x - q + A'(rho z - y); partials of b'b
__global__ void __launch_bounds__(TB) k_rp_b(int n, double sigma, const double *x, const double *q, const double *buf, double *b, double *pbb) {
  __shared__ double red[16];
  double s = 0.0;
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) { const double v = sigma * x[j] - q[j] + buf[j]; b[j] = v; s += v * v; }
  s = block_sum(s, red);
  if (threadIdx.x == 0) pbb[blockIdx.x] = s;
}
// r = b - (part + sigma x~);  z = Minv r;  p = z;  partials of r'z and r'r
__global__ void __launch_bounds__(TB) k_rp_r0(int n, double sigma, const double *b, const double *part, const double *xt, const double *minv,
                                              double *r, double *zz, double *p, double *prz, double *prr) {
  __shared__ double red[16];
  double s0 = 0.0, s1 = 0.0;
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) {
    const double rj = b[j] - (part[j] + sigma * xt[j]), zj = minv[j] * rj;
    r[j] = rj; zz[j] = zj; p[j] = zj; s0 += rj * zj; s1 += rj * rj;
  }
  s0 = block_sum(s0, red); s1 = block_sum(s1, red);
  if (threadIdx.x == 0) { prz[blockIdx.x] = s0; prr[blockIdx.x] = s1; }
}
__global__ void __launch_bounds__(TB) k_rp_s0(RpS *S, const double *pbb, const double *prz, const double *prr, double eps, int cap) {
  __shared__ double red[16];
  const double bb = rp_total(pbb, red), rz = rp_total(prz, red), rr = rp_total(prr, red);
  if (threadIdx.x == 0) {
    S->bb = bb; S->rz[0] = rz; S->rr = rr; S->tol2 = fmax(eps * eps * bb, RP_DIV_TOL);
    S->iters = 0; S->cap = cap; S->bad = 0; S->done = !(rr > S->tol2);
  }
}
// Kp = part + sigma p; partials of p'Kp
__global__ void __launch_bounds__(TB) k_rp_pkp(int n, double sigma, const RpS *S, const double *part, const double *p, double *Kp, double *ppkp) {
  if (S->done) return;
  __shared__ double red[16];
  double s = 0.0;
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) { const double v = part[j] + sigma * p[j]; Kp[j] = v; s += p[j] * v; }
  s = block_sum(s, red);
  if (threadIdx.x == 0) ppkp[blockIdx.x] = s;
}
__global__ void __launch_bounds__(TB) k_rp_upd(int n, int par, const RpS *S, const double *ppkp, const double *p, const double *Kp, const double *minv,
                                               double *xt, double *r, double *zz, double *prz, double *prr) {
  if (S->done) return;
  __shared__ double red[16];
  const double pkp = rp_total(ppkp, red);
  const double a = pkp > 0.0 ? S->rz[par] / pkp : 0.0;          // (p'Kp <= 0: K is not positive definite; k_rp_dir ends the solve and reports it)
  double s0 = 0.0, s1 = 0.0;
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) {
    xt[j] += a * p[j];
    const double rj = r[j] - a * Kp[j], zj = minv[j] * rj;
    r[j] = rj; zz[j] = zj; s0 += rj * zj; s1 += rj * rj;
  }
  s0 = block_sum(s0, red); s1 = block_sum(s1, red);
  if (threadIdx.x == 0) { prz[blockIdx.x] = s0; prr[blockIdx.x] = s1; }
}
// p = z + (rz'/rz) p; workgroup 0 closes the iteration (new r'z into the other slot: the others still read the old one)
__global__ void __launch_bounds__(TB) k_rp_dir(int n, int par, RpS *S, const double *ppkp, const double *prz, const double *prr, const double *zz, double *p) {
  if (S->done) return;
  __shared__ double red[16];
  const double rz2 = rp_total(prz, red), rr = rp_total(prr, red), pkp = rp_total(ppkp, red);
  const double beta = rz2 / S->rz[par];
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) p[j] = zz[j] + beta * p[j];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    S->rz[par ^ 1] = rz2; S->rr = rr;
    const int it = S->iters + 1;
    S->iters = it;
    if (!(pkp > 0.0)) S->bad = 1;
    if (!(rr > S->tol2) || it >= S->cap || !(pkp > 0.0)) S->done = 1;      // (written after every workgroup of this launch has passed its own test or not: both are fine, p is not used again)
  }
}
__global__ void __launch_bounds__(TB) k_rp_admm_x(int n, double alpha, const double *xt, double *x) {
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) x[j] = alpha * xt[j] + (1.0 - alpha) * x[j];
}
// update_z / update_y (src/auxil.c:190-225) on the rank's rows
__global__ void __launch_bounds__(TB) k_rp_admm_z(int m, double alpha, const double *zt, const double *rho, const double *l, const double *u, double *z, double *y) {
  for (int i = blockIdx.x * TB + threadIdx.x; i < m; i += gridDim.x * TB) {
    const double v = alpha * zt[i] + (1.0 - alpha) * z[i];
    const double zn = fmin(fmax(v + y[i] / rho[i], l[i]), u[i]);
    y[i] += rho[i] * (v - zn);
    z[i] = zn;
  }
}
// rho per row from its bounds (set_rho_vec, src/auxil.c:28-52)
__global__ void __launch_bounds__(TB) k_rp_rho(int m, double rho, const double *l, const double *u, double *rv) {
  for (int i = blockIdx.x * TB + threadIdx.x; i < m; i += gridDim.x * TB) {
    const double lo = l[i], hi = u[i];
    rv[i] = (lo < -INF_BOUND && hi > INF_BOUND) ? RHO_MIN : ((hi - lo < RHO_TOL) ? RHO_EQ_OVER_RHO_INEQ * rho : rho);
  }
}
// this rank's share of diag(P) + sum_i rho_i A_ij^2 (the Jacobi preconditioner before the all-reduce), from the rows of [P_g | A_g']
__global__ void __launch_bounds__(TB) k_rp_diag(DevMat M, int n, const double *rho, double *out) {
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) {
    double d = 0.0;
    for (int k = M.rowptr[j]; k < M.split[j]; ++k) if (M.col[k] == j) d += M.val[k];
    for (int k = M.split[j]; k < M.rowptr[j + 1]; ++k) { const double a = M.val[k]; d += rho[M.col[k] - n] * a * a; }
    out[j] = d;
  }
}
__global__ void __launch_bounds__(TB) k_rp_minv(int n, double sigma, const double *diag, double *minv) {
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) minv[j] = 1.0 / (diag[j] + sigma);
}
__device__ __forceinline__ double block_max(double v, double *red) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
// primal side of a check: maxima over the rank's rows of |Einv (Ax - z)|, |Einv z|, |Einv Ax|, |Ax - z|, |z|, |Ax|  (one workgroup)
__global__ void __launch_bounds__(TB) k_rp_pri(int m, const double *ax, const double *z, const double *Einv, double *out6) {
  __shared__ double red[16];
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < m; i += TB) {
    const double a = ax[i], zi = z[i], e = Einv[i], d = a - zi;
    v[0] = fmax(v[0], fabs(e * d)); v[1] = fmax(v[1], fabs(e * zi)); v[2] = fmax(v[2], fabs(e * a));
    v[3] = fmax(v[3], fabs(d)); v[4] = fmax(v[4], fabs(zi)); v[5] = fmax(v[5], fabs(a));
  }
  for (int k = 0; k < 6; ++k) { const double t = block_max(v[k], red); if (threadIdx.x == 0) out6[k] = t; __syncthreads(); }
}
// dual side: both = [P x ; A' y] summed over the ranks.  out: dua_u, dua_s, q_u, q_s, Aty_u, Aty_s, Px_u, Px_s, x'(0.5 P x + q)  (one workgroup)
__global__ void __launch_bounds__(TB) k_rp_dua(int n, const double *both, const double *q, const double *Dinv, const double *x, double *out9) {
  __shared__ double red[16];
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, obj = 0.0;
  for (int j = threadIdx.x; j < n; j += TB) {
    const double px = both[j], aty = both[n + j], qj = q[j], di = Dinv[j], d = px + qj + aty;
    v[0] = fmax(v[0], fabs(di * d)); v[1] = fmax(v[1], fabs(d)); v[2] = fmax(v[2], fabs(di * qj)); v[3] = fmax(v[3], fabs(qj));
    v[4] = fmax(v[4], fabs(di * aty)); v[5] = fmax(v[5], fabs(aty)); v[6] = fmax(v[6], fabs(di * px)); v[7] = fmax(v[7], fabs(px));
    obj += x[j] * (0.5 * px + qj);
  }
  for (int k = 0; k < 8; ++k) { const double t = block_max(v[k], red); if (threadIdx.x == 0) out9[k] = t; __syncthreads(); }
  obj = block_sum(obj, red);
  if (threadIdx.x == 0) out9[8] = obj;
}
__global__ void __launch_bounds__(TB) k_rp_unscale(int n, const double *s, const double *v, double f, double *out) {
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) out[j] = s[j] * v[j] * f;
}

// ---- infeasibility tests (is_primal_infeasible / is_dual_infeasible, src/auxil.c:361-512), only after osqp_amd_rp_set_infeasibility ----
// out7 = sc15 + RSC_NDY: the seven of enum RpScalar, by their distance from RSC_NDY (E, Einv, D, Dinv: null under scaled_termination
// or unscaled data).  None of the seven depends on a tolerance, so the host applies eps and 10 eps to the same read-back.
__global__ void __launch_bounds__(TB) k_rp_delta_x(int n, const double *x, const double *xp, double *dx) {
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) dx[j] = x[j] - xp[j];
}
// dy = y - y_prev projected on the polar of the recession cone of [l, u] (src/auxil.c:374-387)
__global__ void __launch_bounds__(TB) k_rp_delta_y(int m, const double *y, const double *yp, const double *l, const double *u, double *dy) {
  for (int i = blockIdx.x * TB + threadIdx.x; i < m; i += gridDim.x * TB) {
    double d = y[i] - yp[i];
    if (u[i] > INF_BOUND) d = l[i] < -INF_BOUND ? 0.0 : fmin(d, 0.0);
    else if (l[i] < -INF_BOUND) d = fmax(d, 0.0);
    dy[i] = d;
  }
}
// replicated side: |D dx| and q'dx, in one workgroup's fixed order on every rank
__global__ void __launch_bounds__(TB) k_rp_cert_x(int n, const double *dx, const double *q, const double *D, double *out7) {
  __shared__ double red[16];
  double nx = 0.0, s = 0.0;
  for (int j = threadIdx.x; j < n; j += TB) { const double d = dx[j]; nx = fmax(nx, fabs(D ? D[j] * d : d)); s += q[j] * d; }
  nx = block_max(nx, red);
  s = block_sum(s, red);
  if (threadIdx.x == 0) { out7[4] = nx; out7[5] = s; }
}
// the rank's rows: |E dy|, the largest (Einv A dx)_i of a row with a finite u and -(Einv A dx)_i of one with a finite l (never below
// 0: the test is `> eps |dx|` with eps |dx| >= 0), and this rank's share of u'dy+ + l'dy-
__global__ void __launch_bounds__(TB) k_rp_cert_rows(int m, const double *dy, const double *E, const double *Einv, const double *l, const double *u,
                                                     const double *adx, double *out7, double *lhs) {
  __shared__ double red[16];
  double ny = 0.0, viol = 0.0, s = 0.0;
  for (int i = threadIdx.x; i < m; i += TB) {
    const double d = dy[i], a = Einv ? Einv[i] * adx[i] : adx[i];
    ny = fmax(ny, fabs(E ? E[i] * d : d));
    s += u[i] * fmax(d, 0.0) + l[i] * fmin(d, 0.0);
    if (u[i] < INF_BOUND) viol = fmax(viol, a);
    if (l[i] > -INF_BOUND) viol = fmax(viol, -a);
  }
  ny = block_max(ny, red);
  viol = block_max(viol, red);
  s = block_sum(s, red);
  if (threadIdx.x == 0) { out7[0] = ny; out7[1] = viol; *lhs = s; }
}
// after the all-reduce of cb = [P dx ; A'dy ; lhs]: |Dinv A'dy|, |Dinv P dx|, and lhs beside the other scalars
__global__ void __launch_bounds__(TB) k_rp_cert_fin(int n, const double *cb, const double *Dinv, double *out7) {
  __shared__ double red[16];
  double na = 0.0, np = 0.0;
  for (int j = threadIdx.x; j < n; j += TB) {
    const double di = Dinv ? Dinv[j] : 1.0;
    np = fmax(np, fabs(Dinv ? di * cb[j] : cb[j])); na = fmax(na, fabs(Dinv ? di * cb[n + j] : cb[n + j]));
  }
  na = block_max(na, red);
  np = block_max(np, red);
  if (threadIdx.x == 0) { out7[2] = cb[2 * n]; out7[3] = na; out7[6] = np; }
}
// certificate as store_solution leaves it (src/auxil.c:545-555, 762-780): (s v) / |s v|_inf in place
__global__ void __launch_bounds__(TB) k_rp_cert_out(int n, const double *s, double f, double *v) {
  for (int j = blockIdx.x * TB + threadIdx.x; j < n; j += gridDim.x * TB) v[j] = (s ? s[j] * v[j] : v[j]) * f;
}
// ---- updates of a live handle ----
// new bounds of the rank's rows, nothing of the handle written yet: clamp to +-OSQP_INFTY, scale by E into ln / un; flags3 = [l > u on
// some row, some row changes class (k_rp_rho's three), some row is an equality row]  (one workgroup)
__global__ void __launch_bounds__(TB) k_rp_bounds(int m, const double *lin, const double *uin, const double *E, const double *l, const double *u,
                                                  double *ln, double *un, double *flags3) {
  __shared__ double red[16];
  double bad = 0.0, chg = 0.0, eq = 0.0;
  for (int i = threadIdx.x; i < m; i += TB) {
    const double lo = fmax(lin[i], -OSQP_INFTY), hi = fmin(uin[i], OSQP_INFTY);
    if (lo > hi) bad = 1.0;
    const double a = E[i] * lo, b = E[i] * hi;
    ln[i] = a; un[i] = b;
    const int was = (l[i] < -INF_BOUND && u[i] > INF_BOUND) ? -1 : (u[i] - l[i] < RHO_TOL), now = (a < -INF_BOUND && b > INF_BOUND) ? -1 : (b - a < RHO_TOL);
    if (was != now) chg = 1.0;
    if (now == 1) eq = 1.0;
  }
  bad = block_max(bad, red);
  chg = block_max(chg, red);
  eq = block_max(eq, red);
  if (threadIdx.x == 0) { flags3[0] = bad; flags3[1] = chg; flags3[2] = eq; }
}

// ---- RCCL through dlopen (no link-time dependency; a process that already loaded librccl gets that copy) ----
struct RpNcclId { char b[128]; };
struct RpRccl {
  void *lib = nullptr, *comm = nullptr;
  int (*GetUniqueId)(RpNcclId *) = nullptr;
  int (*CommInitRank)(void **, int, RpNcclId, int) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
};
static int rp_rccl_open(RpRccl &R) {
  if (R.lib) return 0;
  const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
  for (const char *nm : names) if ((R.lib = dlopen(nm, RTLD_NOW | RTLD_NOLOAD))) break;
  if (!R.lib) for (const char *nm : names) if ((R.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) break;
  if (!R.lib) { fprintf(stderr, "osqp_amd: librccl.so could not be loaded (%s)\n", dlerror()); return HIPENG_ERR_HIP; }
  R.GetUniqueId = reinterpret_cast<int (*)(RpNcclId *)>(dlsym(R.lib, "ncclGetUniqueId"));
  R.CommInitRank = reinterpret_cast<int (*)(void **, int, RpNcclId, int)>(dlsym(R.lib, "ncclCommInitRank"));
  R.AllReduce = reinterpret_cast<int (*)(const void *, void *, size_t, int, int, void *, hipStream_t)>(dlsym(R.lib, "ncclAllReduce"));
  R.CommDestroy = reinterpret_cast<int (*)(void *)>(dlsym(R.lib, "ncclCommDestroy"));
  if (!R.GetUniqueId || !R.CommInitRank || !R.AllReduce || !R.CommDestroy) { fprintf(stderr, "osqp_amd: librccl.so lacks the nccl entry points\n"); return HIPENG_ERR_HIP; }
  return 0;
}

struct osqp_amd_rp {
  hipeng *e = nullptr;
  int n = 0, m = 0, m_total = 0, world = 1, rank = 0, has_eq = 0;
  osqp_amd_rp_settings st{};
  osqp_amd_rp_allreduce_fn ar = nullptr; void *user = nullptr;
  RpRccl rccl;
  double c = 1.0, rho = 0.1;
  bool scaled = false;
  double *x, *xt, *q, *D, *Dinv, *minv, *r, *zz, *Kp, *b, *part, *both, *stage;      // n (both: 2n, stage: n + m)
  double *z, *y, *l, *u, *E, *Einv, *rv, *zt, *ax;                                   // m
  double *pa, *pb, *pc, *sc15;                                                      // RP_G partials x 3; the check scalars (enum RpScalar, RSC_ALL_PAD doubles)
  double *xp, *yp, *dxy, *cb, *ln, *un;                                             // x, y before the update (n, m); [dx ; dy] (n + m); [P dx ; A'dy ; lhs] (2n + 1); staged bounds (m)
  double eps_pinf = 0.0, eps_dinf = 0.0;                                            // 0: that test is off (osqp_amd_rp_set_infeasibility)
  int last_status = 0;
  RpS *S = nullptr, *hS = nullptr;                                                  // device / pinned host
  double *h15 = nullptr;
  long long collectives = 0, pcg_iters = 0;
  int last_iters = 4, rho_updates = 0;
  bool rho_set = false;                                                             // rv and minv hold rp->rho (false until the first solve)
  double sc[RSC_ALL];
};

// the unscaled forms of residuals, norms and certificates decide (scaled data without scaled_termination)
static inline bool rp_unscaled(const osqp_amd_rp *rp) { return rp->scaled && !rp->st.scaled_termination; }
static inline bool rp_primal(int status) { return status == OSQP_PRIMAL_INFEASIBLE || status == OSQP_PRIMAL_INFEASIBLE_INACCURATE; }
static inline bool rp_dual(int status) { return status == OSQP_DUAL_INFEASIBLE || status == OSQP_DUAL_INFEASIBLE_INACCURATE; }
static inline bool rp_infeasible(int status) { return rp_primal(status) || rp_dual(status); }

static int rp_allreduce(osqp_amd_rp *rp, double *buf, long long count, int op) {
  if (rp->world <= 1 && !rp->rccl.comm) return 0;
  rp->collectives++;
  if (rp->rccl.comm) return rp->rccl.AllReduce(buf, buf, (size_t)count, 8 /* ncclFloat64 */, op ? 2 /* ncclMax */ : 0 /* ncclSum */, rp->rccl.comm, rp->e->stream) ? HIPENG_ERR_HIP : 0;
  return rp->ar ? rp->ar(rp->user, buf, count, op, (void *)rp->e->stream) : HIPENG_ERR_ARG;
}
static inline dim3 rp_grid() { return dim3(RP_G); }
// part = [P_g | A_g'] [u ; rho (A_g u)] for the u that sits in stage[0, n)
static void rp_apply_local(osqp_amd_rp *rp) {
  hipeng *e = rp->e;
  const int n = rp->n, m = rp->m;
  if (m > 0) {
    launch_spmv(e, e->c.A, rp->stage, rp->stage + n, 0);
    hipLaunchKernelGGL(k_rp_scale, rp_grid(), dim3(TB), 0, e->stream, m, (const double *)rp->rv, rp->stage + n);
  }
  launch_spmv(e, e->c.M, rp->stage, rp->part, 0);
}
static int rp_set_rho(osqp_amd_rp *rp, double rho) {
  hipeng *e = rp->e;
  rho = std::min(std::max(rho, RHO_MIN), RHO_MAX);
  rp->rho = rho;
  if (rp->m > 0) hipLaunchKernelGGL(k_rp_rho, rp_grid(), dim3(TB), 0, e->stream, rp->m, rho, (const double *)rp->l, (const double *)rp->u, rp->rv);
  hipLaunchKernelGGL(k_rp_diag, rp_grid(), dim3(TB), 0, e->stream, e->c.M, rp->n, (const double *)rp->rv, rp->part);
  if (int rc = rp_allreduce(rp, rp->part, rp->n, 0)) return rc;
  hipLaunchKernelGGL(k_rp_minv, rp_grid(), dim3(TB), 0, e->stream, rp->n, rp->st.sigma, (const double *)rp->part, rp->minv);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" osqp_amd_rp *osqp_amd_rp_create(void *shard_engine, const double *q, const double *l_loc, const double *u_loc, const double *D, const double *E_loc,
                                           double c, int m_total, int has_eq_any, const osqp_amd_rp_settings *settings, int world, int rank,
                                           osqp_amd_rp_allreduce_fn allreduce, void *user) {
  hipeng *e = static_cast<hipeng *>(shard_engine);
  if (!e || !q || !D || !settings || world < 1 || rank < 0 || rank >= world || (e->m > 0 && (!l_loc || !u_loc || !E_loc))) return nullptr;
  if (hipSetDevice(e->device) != hipSuccess) return nullptr;
  osqp_amd_rp *rp = new osqp_amd_rp();
  rp->e = e; rp->n = e->n; rp->m = e->m; rp->m_total = m_total; rp->world = world; rp->rank = rank; rp->has_eq = has_eq_any;
  rp->st = *settings; rp->ar = allreduce; rp->user = user; rp->c = c;
  const size_t n = (size_t)e->n, m = (size_t)e->m;
  double **nv[] = {&rp->x, &rp->xt, &rp->q, &rp->D, &rp->Dinv, &rp->minv, &rp->r, &rp->zz, &rp->Kp, &rp->b, &rp->part};
  double **mv[] = {&rp->z, &rp->y, &rp->l, &rp->u, &rp->E, &rp->Einv, &rp->rv, &rp->zt, &rp->ax};
  bool bad = false;
  for (double **p : nv) bad = bad || dev_alloc(e, p, n);
  for (double **p : mv) bad = bad || dev_alloc(e, p, m);
  bad = bad || dev_alloc(e, &rp->both, 2 * n) || dev_alloc(e, &rp->stage, n + m) || dev_alloc(e, &rp->pa, (size_t)RP_G) || dev_alloc(e, &rp->pb, (size_t)RP_G) ||
        dev_alloc(e, &rp->pc, (size_t)RP_G) || dev_alloc(e, &rp->sc15, (size_t)RSC_ALL_PAD) || dev_alloc(e, &rp->S, (size_t)1) ||
        dev_alloc(e, &rp->xp, n) || dev_alloc(e, &rp->yp, m) || dev_alloc(e, &rp->dxy, n + m) || dev_alloc(e, &rp->cb, 2 * n + 1) ||
        dev_alloc(e, &rp->ln, m) || dev_alloc(e, &rp->un, m);
  if (!bad) bad = hipHostMalloc((void **)&rp->hS, sizeof(RpS)) != hipSuccess || hipHostMalloc((void **)&rp->h15, RSC_ALL_PAD * sizeof(double)) != hipSuccess;
  if (bad) { delete rp; return nullptr; }
  std::vector<double> Dinv(n), Einv(m);
  bool scaled = c != 1.0;
  for (size_t j = 0; j < n; j++) { Dinv[j] = 1.0 / D[j]; scaled = scaled || D[j] != 1.0; }
  for (size_t i = 0; i < m; i++) { Einv[i] = 1.0 / E_loc[i]; scaled = scaled || E_loc[i] != 1.0; }
  rp->scaled = scaled;
  auto up = [&](double *dst, const double *src, size_t k) { return k == 0 || hipMemcpyAsync(dst, src, k * sizeof(double), hipMemcpyHostToDevice, e->stream) == hipSuccess; };
  bool ok = up(rp->q, q, n) && up(rp->D, D, n) && up(rp->Dinv, Dinv.data(), n) && up(rp->l, l_loc, m) && up(rp->u, u_loc, m) && up(rp->E, E_loc, m) && up(rp->Einv, Einv.data(), m);
  ok = ok && hipStreamSynchronize(e->stream) == hipSuccess;          // (the inverses are locals)
  if (!ok) { osqp_amd_rp_free(rp); return nullptr; }
  return rp;
}

extern "C" int osqp_amd_rp_rccl_unique_id(void *out, int cap_bytes) {
  if (!out || cap_bytes < 128) return -1;
  RpRccl R;
  if (rp_rccl_open(R)) return -1;
  RpNcclId id;
  if (R.GetUniqueId(&id)) return -1;
  memcpy(out, id.b, 128);
  return 128;
}
extern "C" int osqp_amd_rp_use_rccl(osqp_amd_rp *rp, const void *unique_id, int id_bytes) {
  if (rp && !unique_id && id_bytes == 0) {           // detach: back to the callback
    if (rp->rccl.comm) rp->rccl.CommDestroy(rp->rccl.comm);
    rp->rccl.comm = nullptr;
    return 0;
  }
  if (!rp || !unique_id || id_bytes != 128) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(rp->e->device));
  if (int rc = rp_rccl_open(rp->rccl)) return rc;
  RpNcclId id;
  memcpy(id.b, unique_id, 128);
  if (rp->rccl.CommInitRank(&rp->rccl.comm, rp->world, id, rp->rank)) { rp->rccl.comm = nullptr; return HIPENG_ERR_HIP; }
  return 0;
}

// one termination check: fills rp->sc (the fifteen scalars; with cert the seven of the infeasibility tests behind them, two more
// all-reduces, the same one read-back) and pri_res / dua_res
static int rp_check(osqp_amd_rp *rp, double *pri_res, double *dua_res, bool cert) {
  hipeng *e = rp->e;
  const int n = rp->n, m = rp->m;
  HIPCHK(hipMemsetAsync(rp->sc15, 0, (cert ? RSC_ALL_PAD : RSC_CHECK_PAD) * sizeof(double), e->stream));
  if (m > 0) {
    launch_spmv(e, e->c.A, rp->x, rp->ax, 0);
    hipLaunchKernelGGL(k_rp_pri, dim3(1), dim3(TB), 0, e->stream, m, (const double *)rp->ax, (const double *)rp->z, (const double *)rp->Einv, rp->sc15 + RSC_PRI_U);
  }
  if (int rc = rp_allreduce(rp, rp->sc15 + RSC_PRI_U, RSC_DUA_U - RSC_PRI_U, 1)) return rc;
  HIPCHK(hipMemcpyAsync(rp->stage, rp->x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  if (m > 0) HIPCHK(hipMemcpyAsync(rp->stage + n, rp->y, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  launch_spmv(e, e->c.M, rp->stage, rp->both, 1);            // P_g x
  launch_spmv(e, e->c.M, rp->stage, rp->both + n, 2);        // A_g' y
  if (int rc = rp_allreduce(rp, rp->both, 2ll * n, 0)) return rc;
  hipLaunchKernelGGL(k_rp_dua, dim3(1), dim3(TB), 0, e->stream, n, (const double *)rp->both, (const double *)rp->q, (const double *)rp->Dinv, (const double *)rp->x, rp->sc15 + RSC_DUA_U);
  const bool un = rp_unscaled(rp);
  if (cert) {
    double *dx = rp->dxy, *dy = rp->dxy + n, *out7 = rp->sc15 + RSC_NDY;
    hipLaunchKernelGGL(k_rp_delta_x, rp_grid(), dim3(TB), 0, e->stream, n, (const double *)rp->x, (const double *)rp->xp, dx);
    if (m > 0) hipLaunchKernelGGL(k_rp_delta_y, rp_grid(), dim3(TB), 0, e->stream, m, (const double *)rp->y, (const double *)rp->yp, (const double *)rp->l, (const double *)rp->u, dy);
    hipLaunchKernelGGL(k_rp_cert_x, dim3(1), dim3(TB), 0, e->stream, n, (const double *)dx, (const double *)rp->q, un ? (const double *)rp->D : nullptr, out7);
    launch_spmv(e, e->c.M, rp->dxy, rp->cb, 1);                // P_g dx
    launch_spmv(e, e->c.M, rp->dxy, rp->cb + n, 2);            // A_g' dy
    if (m > 0) launch_spmv(e, e->c.A, dx, rp->ax, 0);
    hipLaunchKernelGGL(k_rp_cert_rows, dim3(1), dim3(TB), 0, e->stream, m, (const double *)dy, un ? (const double *)rp->E : nullptr, un ? (const double *)rp->Einv : nullptr,
                       (const double *)rp->l, (const double *)rp->u, (const double *)rp->ax, out7, rp->cb + 2 * n);
    if (int rc = rp_allreduce(rp, rp->cb, 2ll * n + 1, 0)) return rc;
    if (int rc = rp_allreduce(rp, out7, RSC_LHS - RSC_NDY, 1)) return rc;          // |E dy| and the row violation
    hipLaunchKernelGGL(k_rp_cert_fin, dim3(1), dim3(TB), 0, e->stream, n, (const double *)rp->cb, un ? (const double *)rp->Dinv : nullptr, out7);
  }
  const size_t got = (cert ? RSC_ALL : RSC_CHECK) * sizeof(double);
  HIPCHK(hipMemcpyAsync(rp->h15, rp->sc15, got, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  memcpy(rp->sc, rp->h15, got);
  const double *s = rp->sc;
  *pri_res = rp->m_total == 0 ? 0.0 : (un ? s[RSC_PRI_U] : s[RSC_PRI_S]);
  *dua_res = un ? s[RSC_DUA_U] / rp->c : s[RSC_DUA_S];
  return 0;
}
// check_termination with the infeasibility tests (src/auxil.c:716-783) on the scalars of a check: RP_GO_ON, RP_RESIDUALS_PASS,
// RP_PRIMAL_INF or RP_DUAL_INF.  Only all-reduced and replicated values are looked at: every rank decides alike.  A test whose
// tolerance is 0 is off before any of its scalars is read, so with both off (a check without cert leaves s[RSC_NDY..] as they were)
// this is the residual test alone.  (un: the unscaled forms decide; c: the cost scaling; eps4: eps_abs, eps_rel, eps_prim_inf, eps_dual_inf)
static int rp_verdict_of(const double *s, bool un, double c, int m_total, const double *eps4, double pri_res, double dua_res, bool approximate) {
  const double k = approximate ? 10.0 : 1.0, ea = k * eps4[0], er = k * eps4[1];
  const bool prim_ok = m_total == 0 || pri_res < ea + er * (un ? std::max(s[RSC_Z_U], s[RSC_AX_U]) : std::max(s[RSC_Z_S], s[RSC_AX_S]));
  const double nrm = un ? std::max(s[RSC_Q_U], std::max(s[RSC_ATY_U], s[RSC_PX_U])) / c : std::max(s[RSC_Q_S], std::max(s[RSC_ATY_S], s[RSC_PX_S]));
  const bool dual_ok = dua_res < ea + er * nrm;
  if (prim_ok && dual_ok) return RP_RESIDUALS_PASS;
  const double ep = k * eps4[2], ed = k * eps4[3], cs = un ? c : 1.0;
  if (!prim_ok && ep > 0.0 && s[RSC_NDY] > RP_DIV_TOL && s[RSC_LHS] < ep * s[RSC_NDY] && s[RSC_NATDY] < ep * s[RSC_NDY]) return RP_PRIMAL_INF;
  if (!dual_ok && ed > 0.0 && s[RSC_NDX] > RP_DIV_TOL && s[RSC_QDX] < cs * ed * s[RSC_NDX] && s[RSC_NPDX] < cs * ed * s[RSC_NDX] && !(s[RSC_VIOL] > ed * s[RSC_NDX])) return RP_DUAL_INF;
  return RP_GO_ON;
}
static int rp_verdict(const osqp_amd_rp *rp, double pri_res, double dua_res, bool approximate) {
  const double eps4[4] = {rp->st.eps_abs, rp->st.eps_rel, rp->eps_pinf, rp->eps_dinf};
  return rp_verdict_of(rp->sc, rp_unscaled(rp), rp->c, rp->m_total, eps4, pri_res, dua_res, approximate);
}
// the status a verdict ends the solve with: at a check within the budget, or in the approximate branch once the budget is spent
static int rp_status_of(int verdict, bool approximate) {
  switch (verdict) {
    case RP_RESIDUALS_PASS: return approximate ? OSQP_SOLVED_INACCURATE : OSQP_SOLVED;
    case RP_PRIMAL_INF:     return approximate ? OSQP_PRIMAL_INFEASIBLE_INACCURATE : OSQP_PRIMAL_INFEASIBLE;
    case RP_DUAL_INF:       return approximate ? OSQP_DUAL_INFEASIBLE_INACCURATE : OSQP_DUAL_INFEASIBLE;
    default:                return OSQP_MAX_ITER_REACHED;
  }
}
// for the tests: the verdict on given scalars, host arithmetic only (no handle, no device)
extern "C" int osqp_amd_rp_test_verdict(const double *sc22, int unscaled, double c, int m_total, const double *eps4, double pri_res, double dua_res, int approximate) {
  if (!sc22 || !eps4) return HIPENG_ERR_ARG;
  return rp_verdict_of(sc22, unscaled != 0, c, m_total, eps4, pri_res, dua_res, approximate != 0);
}
static double rp_rho_estimate(const osqp_amd_rp *rp) {
  const double *s = rp->sc;
  const double pri = (rp->m_total ? s[RSC_PRI_S] : 0.0) / (std::max(s[RSC_Z_S], s[RSC_AX_S]) + RP_DIV_TOL);
  const double dua = s[RSC_DUA_S] / (std::max(s[RSC_Q_S], std::max(s[RSC_ATY_S], s[RSC_PX_S])) + RP_DIV_TOL);
  return std::min(std::max(rp->rho * std::sqrt(pri / dua), RHO_MIN), RHO_MAX);
}
// cold_start (src/auxil.c:536-560 ends in it): the iterates x, x~, z, y back to zero; rho and rho_updates stay
static int rp_cold_start(osqp_amd_rp *rp) {
  for (double *v : {rp->x, rp->xt}) HIPCHK(hipMemsetAsync(v, 0, (size_t)rp->n * sizeof(double), rp->e->stream));
  if (rp->m > 0) for (double *v : {rp->z, rp->y}) HIPCHK(hipMemsetAsync(v, 0, (size_t)rp->m * sizeof(double), rp->e->stream));
  return 0;
}

extern "C" int osqp_amd_rp_solve(osqp_amd_rp *rp, osqp_amd_rp_info *info) {
  if (!rp || !info) return HIPENG_ERR_ARG;
  hipeng *e = rp->e;
  HIPCHK(hipSetDevice(e->device));
  const osqp_amd_rp_settings &st = rp->st;
  const int n = rp->n, m = rp->m;
  const dim3 g = rp_grid(), tb(TB);
  const double ee = std::min(st.eps_abs > 0 ? st.eps_abs : st.eps_rel, st.eps_rel > 0 ? st.eps_rel : st.eps_abs);
  double eps_pcg = std::max(1e-13, std::min(st.pcg_eps_rel, 1e-5 * ee));            // the rule of osqp_solve (osqp_host.c)
  if (rp->has_eq) eps_pcg = std::max(1e-13, 1e-3 * eps_pcg);
  const int interval = st.adaptive_rho_interval ? st.adaptive_rho_interval : (st.check_termination ? 4 * st.check_termination : 100);
  const int cap = st.pcg_max_iter ? st.pcg_max_iter : std::max(20000, 10 * n);
  rp->pcg_iters = 0; rp->collectives = 0;
  // the first solve builds rho per row and the preconditioner from the setting; a later one starts from the kept iterates with the
  // rho the previous solve ended on, and rho_updates counts on (osqp_solve keeps work->settings->rho and info->rho_updates)
  if (!rp->rho_set) {
    if (int rc = rp_set_rho(rp, st.rho)) return rc;
    rp->rho_set = true;
  }
  const bool cert = rp->eps_pinf > 0.0 || rp->eps_dinf > 0.0;
  int verdict = RP_GO_ON, it = 0;
  bool checked = false;
  double pri_res = 0.0, dua_res = 0.0;
  for (it = 1; it <= st.max_iter; it++) {
    // right-hand side
    HIPCHK(hipMemsetAsync(rp->stage, 0, (size_t)n * sizeof(double), e->stream));
    if (m > 0) hipLaunchKernelGGL(k_rp_w, g, tb, 0, e->stream, m, (const double *)rp->rv, (const double *)rp->z, (const double *)rp->y, rp->stage + n);
    launch_spmv(e, e->c.M, rp->stage, rp->part, 2);   // A_g' w
    if (int rc = rp_allreduce(rp, rp->part, n, 0)) return rc;
    hipLaunchKernelGGL(k_rp_b, g, tb, 0, e->stream, n, st.sigma, (const double *)rp->x, (const double *)rp->q, (const double *)rp->part, rp->b, rp->pa);
    // PCG from the previous x~
    HIPCHK(hipMemcpyAsync(rp->stage, rp->xt, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    rp_apply_local(rp);
    if (int rc = rp_allreduce(rp, rp->part, n, 0)) return rc;
    hipLaunchKernelGGL(k_rp_r0, g, tb, 0, e->stream, n, st.sigma, (const double *)rp->b, (const double *)rp->part, (const double *)rp->xt, (const double *)rp->minv,
                       rp->r, rp->zz, rp->stage, rp->pb, rp->pc);
    hipLaunchKernelGGL(k_rp_s0, dim3(1), tb, 0, e->stream, rp->S, (const double *)rp->pa, (const double *)rp->pb, (const double *)rp->pc, eps_pcg, cap);
    int issued = 0;
    for (;;) {
      // a group of iterations, then one look at the flag: the first group is as long as the previous solve was, the next ones two
      const int group = issued == 0 ? std::max(1, rp->last_iters) : 2;
      for (int k = 0; k < group; k++, issued++) {
        const int par = issued & 1;
        rp_apply_local(rp);                                   // p sits in stage[0, n)
        if (int rc = rp_allreduce(rp, rp->part, n, 0)) return rc;
        hipLaunchKernelGGL(k_rp_pkp, g, tb, 0, e->stream, n, st.sigma, (const RpS *)rp->S, (const double *)rp->part, (const double *)rp->stage, rp->Kp, rp->pa);
        hipLaunchKernelGGL(k_rp_upd, g, tb, 0, e->stream, n, par, (const RpS *)rp->S, (const double *)rp->pa, (const double *)rp->stage, (const double *)rp->Kp,
                           (const double *)rp->minv, rp->xt, rp->r, rp->zz, rp->pb, rp->pc);
        hipLaunchKernelGGL(k_rp_dir, g, tb, 0, e->stream, n, par, rp->S, (const double *)rp->pa, (const double *)rp->pb, (const double *)rp->pc, (const double *)rp->zz, rp->stage);
      }
      HIPCHK(hipMemcpyAsync(rp->hS, rp->S, sizeof(RpS), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      if (rp->hS->done || issued >= cap) break;
    }
    if (rp->hS->bad) { fprintf(stderr, "osqp_amd: row-partitioned PCG met p'Kp <= 0 (the problem is not convex)\n"); return HIPENG_ERR_ARG; }
    rp->last_iters = rp->hS->iters;
    rp->pcg_iters += rp->hS->iters;
    // x, z, y
    if (m > 0) launch_spmv(e, e->c.A, rp->xt, rp->zt, 0);
    checked = st.check_termination && it % st.check_termination == 0;
    if (cert && (checked || it == st.max_iter)) {          // this iteration ends in a check: x and y as they are now, for dx and dy
      HIPCHK(hipMemcpyAsync(rp->xp, rp->x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      if (m > 0) HIPCHK(hipMemcpyAsync(rp->yp, rp->y, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    }
    hipLaunchKernelGGL(k_rp_admm_x, g, tb, 0, e->stream, n, st.alpha, (const double *)rp->xt, rp->x);
    if (m > 0) hipLaunchKernelGGL(k_rp_admm_z, g, tb, 0, e->stream, m, st.alpha, (const double *)rp->zt, (const double *)rp->rv, (const double *)rp->l, (const double *)rp->u, rp->z, rp->y);
    HIPCHK(hipGetLastError());
    if (checked) {
      if (int rc = rp_check(rp, &pri_res, &dua_res, cert)) return rc;
      if ((verdict = rp_verdict(rp, pri_res, dua_res, false)) != RP_GO_ON) break;
    }
    if (st.adaptive_rho && it % interval == 0) {
      if (!checked) if (int rc = rp_check(rp, &pri_res, &dua_res, false)) return rc;
      const double nw = rp_rho_estimate(rp);
      if (nw > rp->rho * st.adaptive_rho_tolerance || nw < rp->rho / st.adaptive_rho_tolerance) {
        if (int rc = rp_set_rho(rp, nw)) return rc;
        rp->rho_updates++;
      }
    }
  }
  if (it > st.max_iter) it = st.max_iter;
  if (!checked) {
    if (int rc = rp_check(rp, &pri_res, &dua_res, cert)) return rc;
    verdict = rp_verdict(rp, pri_res, dua_res, false);
  }
  // nothing within the budget: the approximate branch, 10 x every tolerance on the same scalars
  const int status = verdict != RP_GO_ON ? rp_status_of(verdict, false) : rp_status_of(rp_verdict(rp, pri_res, dua_res, true), true);
  info->status = status; info->iter = it; info->rho_updates = rp->rho_updates; info->pcg_iters = rp->pcg_iters;
  info->obj_val = rp->sc[RSC_OBJ] / rp->c; info->pri_res = pri_res; info->dua_res = dua_res; info->rho_estimate = rp_rho_estimate(rp);
  rp->last_status = status;
  if (rp_infeasible(status)) {
    // store_solution (src/auxil.c:536-560): no solution, the certificate normalised in place, the iterates back to zero
    const bool un = rp_unscaled(rp), prim = rp_primal(status);
    info->obj_val = prim ? OSQP_INFTY : -OSQP_INFTY;
    if (prim) { if (m > 0) hipLaunchKernelGGL(k_rp_cert_out, g, tb, 0, e->stream, m, un ? (const double *)rp->E : nullptr, 1.0 / rp->sc[RSC_NDY], rp->dxy + n); }
    else hipLaunchKernelGGL(k_rp_cert_out, g, tb, 0, e->stream, n, un ? (const double *)rp->D : nullptr, 1.0 / rp->sc[RSC_NDX], rp->dxy);
    HIPCHK(hipGetLastError());
    if (int rc = rp_cold_start(rp)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  info->collectives = rp->collectives;
  return 0;
}

extern "C" int osqp_amd_rp_set_infeasibility(osqp_amd_rp *rp, double eps_prim_inf, double eps_dual_inf) {
  if (!rp || !(eps_prim_inf >= 0.0) || !(eps_dual_inf >= 0.0)) return HIPENG_ERR_ARG;
  rp->eps_pinf = eps_prim_inf; rp->eps_dinf = eps_dual_inf;
  return 0;
}
extern "C" int osqp_amd_rp_get_certificates(osqp_amd_rp *rp, double *dual_inf_cert, double *prim_inf_cert_loc) {
  if (!rp || !dual_inf_cert || (rp->m > 0 && !prim_inf_cert_loc)) return HIPENG_ERR_ARG;
  hipeng *e = rp->e;
  const bool prim = rp_primal(rp->last_status), dual = rp_dual(rp->last_status);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (dual) HIPCHK(hipMemcpy(dual_inf_cert, rp->dxy, (size_t)rp->n * sizeof(double), hipMemcpyDeviceToHost));
  else std::fill(dual_inf_cert, dual_inf_cert + rp->n, NAN);
  if (prim && rp->m > 0) HIPCHK(hipMemcpy(prim_inf_cert_loc, rp->dxy + rp->n, (size_t)rp->m * sizeof(double), hipMemcpyDeviceToHost));
  else if (rp->m > 0) std::fill(prim_inf_cert_loc, prim_inf_cert_loc + rp->m, NAN);
  return 0;
}

// ---- a live handle: unscaled host arrays in, scaled on the device with the handle's D, E, c.  Every rank calls each of them. ----
static int rp_upload(osqp_amd_rp *rp, double *dst, const double *src, size_t k) {
  if (k) HIPCHK(hipMemcpyAsync(dst, src, k * sizeof(double), hipMemcpyHostToDevice, rp->e->stream));
  return 0;
}
extern "C" int osqp_amd_rp_update_lin_cost(osqp_amd_rp *rp, const double *q) {
  if (!rp || !q) return HIPENG_ERR_ARG;
  hipeng *e = rp->e;
  HIPCHK(hipSetDevice(e->device));
  if (int rc = rp_upload(rp, rp->part, q, (size_t)rp->n)) return rc;
  hipLaunchKernelGGL(k_rp_unscale, rp_grid(), dim3(TB), 0, e->stream, rp->n, (const double *)rp->D, (const double *)rp->part, rp->c, rp->q);      // (D q) c
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));            // (q is the caller's)
  rp->rho_updates = 0;                                // reset_info (src/osqp.c:788)
  return 0;
}
extern "C" int osqp_amd_rp_update_bounds(osqp_amd_rp *rp, const double *l_loc, const double *u_loc) {
  if (!rp || (rp->m > 0 && (!l_loc || !u_loc))) return HIPENG_ERR_ARG;
  hipeng *e = rp->e;
  const size_t m = (size_t)rp->m;
  HIPCHK(hipSetDevice(e->device));
  if (int rc = rp_upload(rp, rp->zt, l_loc, m)) return rc;
  if (int rc = rp_upload(rp, rp->ax, u_loc, m)) return rc;
  hipLaunchKernelGGL(k_rp_bounds, dim3(1), dim3(TB), 0, e->stream, rp->m, (const double *)rp->zt, (const double *)rp->ax, (const double *)rp->E,
                     (const double *)rp->l, (const double *)rp->u, rp->ln, rp->un, rp->pa);
  HIPCHK(hipGetLastError());
  if (int rc = rp_allreduce(rp, rp->pa, 3, 1)) return rc;
  double f[3];
  HIPCHK(hipMemcpyAsync(f, rp->pa, sizeof(f), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (f[0] > 0.0) return 1;                           // l > u on some rank: nothing written on any (src/osqp.c:814-821)
  if (m) {
    HIPCHK(hipMemcpyAsync(rp->l, rp->ln, m * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(rp->u, rp->un, m * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  }
  rp->has_eq = f[2] > 0.0;
  rp->rho_updates = 0;                                // reset_info (src/osqp.c:834)
  // a row changed class on some rank: rho per row and the preconditioner again, on every rank (update_rho_vec, src/auxil.c:54-74);
  // before the first solve there is nothing to rebuild yet
  if (f[1] > 0.0 && rp->rho_set) return rp_set_rho(rp, rp->rho);
  return 0;
}
extern "C" int osqp_amd_rp_warm_start(osqp_amd_rp *rp, const double *x, const double *y_loc) {
  if (!rp) return HIPENG_ERR_ARG;
  hipeng *e = rp->e;
  const int n = rp->n, m = rp->m;
  HIPCHK(hipSetDevice(e->device));
  if (x) {
    if (int rc = rp_upload(rp, rp->part, x, (size_t)n)) return rc;
    hipLaunchKernelGGL(k_rp_unscale, rp_grid(), dim3(TB), 0, e->stream, n, (const double *)rp->Dinv, (const double *)rp->part, 1.0, rp->x);      // Dinv x
    HIPCHK(hipMemcpyAsync(rp->xt, rp->x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, e->stream));                                    // the PCG starts from x~
    if (m > 0) launch_spmv(e, e->c.A, rp->x, rp->z, 0);
  }
  if (y_loc && m > 0) {
    if (int rc = rp_upload(rp, rp->zt, y_loc, (size_t)m)) return rc;
    hipLaunchKernelGGL(k_rp_unscale, rp_grid(), dim3(TB), 0, e->stream, m, (const double *)rp->Einv, (const double *)rp->zt, rp->c, rp->y);      // (Einv y) c
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}
extern "C" int osqp_amd_rp_update_rho(osqp_amd_rp *rp, double rho) {
  if (!rp) return HIPENG_ERR_ARG;
  if (!(rho > 0.0)) return 1;
  HIPCHK(hipSetDevice(rp->e->device));
  if (int rc = rp_set_rho(rp, rho)) return rc;
  rp->rho_set = true;
  return 0;
}

extern "C" int osqp_amd_rp_get_solution(osqp_amd_rp *rp, double *x, double *y_loc) {
  if (!rp || !x) return HIPENG_ERR_ARG;
  hipeng *e = rp->e;
  if (rp_infeasible(rp->last_status)) {             // no solution (src/auxil.c:537-539)
    std::fill(x, x + rp->n, NAN);
    if (y_loc) std::fill(y_loc, y_loc + rp->m, NAN);
    return 0;
  }
  HIPCHK(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_rp_unscale, rp_grid(), dim3(TB), 0, e->stream, rp->n, (const double *)rp->D, (const double *)rp->x, 1.0, rp->part);
  HIPCHK(hipMemcpyAsync(x, rp->part, (size_t)rp->n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (rp->m > 0 && y_loc) {
    hipLaunchKernelGGL(k_rp_unscale, rp_grid(), dim3(TB), 0, e->stream, rp->m, (const double *)rp->E, (const double *)rp->y, 1.0 / rp->c, rp->zt);
    HIPCHK(hipMemcpyAsync(y_loc, rp->zt, (size_t)rp->m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// ---- for the tests: one array of the handle's state on the host (reads only) ----
extern "C" int osqp_amd_rp_peek(osqp_amd_rp *rp, int which, double *out, long long cap) {
  if (!rp || !out) return HIPENG_ERR_ARG;
  hipeng *e = rp->e;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  const int n = rp->n, m = rp->m;
  const struct { const double *src; long long count; } tab[] = {          // by OSQP_AMD_RP_PEEK_*
      {rp->x, n}, {rp->xt, n}, {rp->z, m}, {rp->y, m}, {rp->rv, m}, {rp->minv, n}, {rp->b, n}, {rp->r, n}, {rp->sc15, RSC_CHECK}, {nullptr, 9},
      {rp->dxy, n}, {rp->dxy + n, m}, {rp->sc15 + RSC_NDY, RSC_CERT}, {rp->q, n}, {rp->l, m}, {rp->u, m}};
  static_assert(sizeof(tab) / sizeof(tab[0]) == OSQP_AMD_RP_PEEK_U + 1, "one entry per selector");
  if (which < 0 || which > OSQP_AMD_RP_PEEK_U || cap < tab[which].count) return HIPENG_ERR_ARG;
  const long long count = tab[which].count;
  if (which == OSQP_AMD_RP_PEEK_S) {                  // a struct, not doubles: converted here
    RpS s;
    HIPCHK(hipMemcpy(&s, rp->S, sizeof(RpS), hipMemcpyDeviceToHost));
    const double v[9] = {s.rz[0], s.rz[1], s.rr, s.tol2, s.bb, (double)s.done, (double)s.iters, (double)s.cap, (double)s.bad};
    memcpy(out, v, sizeof(v));
  } else if (count > 0) HIPCHK(hipMemcpy(out, tab[which].src, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
  return (int)count;
}

extern "C" void osqp_amd_rp_free(osqp_amd_rp *rp) {
  if (!rp) return;
  if (rp->rccl.comm) rp->rccl.CommDestroy(rp->rccl.comm);
  if (rp->hS) (void)hipHostFree(rp->hS);
  if (rp->h15) (void)hipHostFree(rp->h15);
  delete rp;                 // (the device vectors belong to the shard engine's allocation list and go with it)
}
