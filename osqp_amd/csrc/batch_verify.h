// batch_verify.h -- the verdict on a point (x, y) against the RAW problem a batch handle holds, included by batch.hip
// after the engines.  It serves every engine alike: it reads only the shared pattern, the raw values io.Px / io.Ax
// (shared, per member, or the common-K engine's one model: io.strideP / io.strideA), the raw io.Q, io.L, io.U and
// the unscaled point -- nothing of D, E, c, rho, K^-1 or the stored iterates -- and writes one record of 16 doubles:
//    0 obj = x'Px / 2 + q'x      1 pri_res = |Ax - z|oo, z = clamp(Ax, l, u)      2 dua_res = |Px + q + A'y|oo
//    3 |Ax|oo   4 |z|oo   5 |Px|oo   6 |A'y|oo   7 |q|oo
//    8 eps_pri = eps_abs + eps_rel max(3, 4)          9 eps_dua = eps_abs + eps_rel max(5, 6, 7)
//   10 comp = max_i max(y+_i (u_i - z_i), y-_i (z_i - l_i))      11 dual_obj = -x'Px / 2 - sum_i (u_i y+_i - l_i y-_i)
//   12 gap = obj - dual_obj      13 optimal: pri_res < eps_pri and dua_res < eps_dua (strict, auxil.c:725,737)
//   14 prim_inf: is_primal_infeasible (auxil.c:361-424) on dy      15 dual_inf: is_dual_infeasible (auxil.c:426-512) on dx
// y+ = max(y, 0), y- = max(-y, 0).  The compute_pri_res / _tol, compute_dua_res / _tol of auxil.c:240-359 and the two
// certificate tests are the reference's with D = E = I, c = 1, statement by statement, its inequalities as coded.
// Infinite bounds (u > 1e26, l < -1e26: OSQP_INFTY * MIN_SCALING): a term of 10 or 11 whose multiplier part is 0 counts
// 0; a nonzero multiplier part on an infinite bound makes 10 +OSQP_INFTY, 11 -OSQP_INFTY and 12 +OSQP_INFTY.
// "NaN" below is an IEEE NaN or the number OSQP_NAN, which is what the handle stores for a member without a solution
// (store_solution).  One in x or y: 0-12 are OSQP_NAN, 13 is 0, 14 and 15 are computed all the same.  One in dy / dx:
// 14 / 15 is 0.
//   k_batch_verify   one workgroup per listed member.  LDS holds x and y, then dx and the projected dy: the vectors
//                    that are gathered from.  An entry of A x, P x, A'y, A'dy, P dx, A dx is consumed by the thread
//                    that formed it and never stored.  A row of A goes through the CSR view, a column through the CSC
//                    arrays, a row of P through the full symmetric pattern (Fp / Fi / Fk: the stored triangle as both
//                    halves), each in pattern order; a thread adds its entries in index order and the workgroup's sums
//                    and maxima meet in a fixed tree (b_reduce_many, b_max).  No atomics: a member's record does not
//                    depend on the batch around it, on its place in it or on the list.  Thread 0 writes the record.

#define BV_NT 256
#define BV_SLOTS 16
#define BV_SCRATCH 80      // b_reduce_many<4, 10, 3>: (4 + 1) * 13 doubles

struct BVer {
  const double *X, *Y, *DX, *DY;   // the point and the certificates
  int own;                 // bit k: array k (X, Y, DX, DY) is the handle's [B][.], read at the member's row; else the
                           // caller's, read at the workgroup's
  double eps_abs, eps_rel, eps_pinf, eps_dinf;
  double *V;               // [workgroups][BV_SLOTS]
};

__host__ __device__ __forceinline__ size_t bv_lds_bytes(int n, int m) {
  return (sizeof(double) * ((size_t)n + (size_t)m + BV_SCRATCH) + 15) & ~(size_t)15;
}
__device__ __forceinline__ bool bv_nan(double v) { return v != v || v == OSQP_NAN; }

__global__ void __launch_bounds__(BV_NT) k_batch_verify(BPattern p, BIO io, BVer v, const int *list) {
  constexpr int NW = BV_NT / 64;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const long long qp = list ? list[blockIdx.x] : blockIdx.x, row = blockIdx.x;
  const int n = p.n, m = p.m, tid = threadIdx.x;
  double *x = lds, *y = x + n, *buf = y + m;
  const double *Pv = io.Px + qp * io.strideP, *Av = io.Ax + qp * io.strideA;
  const double *q = io.Q + qp * n, *l = io.L + qp * m, *u = io.U + qp * m;
  const double *X = v.X + ((v.own & 1) ? qp : row) * n, *Y = v.Y + ((v.own & 2) ? qp : row) * m;
  const double *DX = v.DX + ((v.own & 4) ? qp : row) * n, *DY = v.DY + ((v.own & 8) ? qp : row) * m;
  double *out = v.V + row * BV_SLOTS;

  // ---- slots 0-13 ------------------------------------------------------------------------------------------------
  enum { M_PRI, M_AX, M_Z, M_DUA, M_PX, M_ATY, M_Q, M_COMP, M_INF, M_NAN, NMAX };
  enum { S_XPX, S_QX, S_SUP, NSUM };
  double mx[NMAX], sm[NSUM];
#pragma unroll
  for (int k = 0; k < NMAX; ++k) mx[k] = 0.0;
#pragma unroll
  for (int k = 0; k < NSUM; ++k) sm[k] = 0.0;
  for (int j = tid; j < n; j += BV_NT) { const double t = X[j]; x[j] = t; if (bv_nan(t)) mx[M_NAN] = 1.0; }
  for (int i = tid; i < m; i += BV_NT) { const double t = Y[i]; y[i] = t; if (bv_nan(t)) mx[M_NAN] = 1.0; }
  __syncthreads();
  for (int i = tid; i < m; i += BV_NT) {
    double a = 0.0;
    for (int k = p.Rp[i]; k < p.Rp[i + 1]; ++k) a += Av[p.Rk[k]] * x[p.Rj[k]];
    const double li = l[i], ui = u[i], z = fmin(fmax(a, li), ui);
    mx[M_PRI] = fmax(mx[M_PRI], fabs(a - z)); mx[M_AX] = fmax(mx[M_AX], fabs(a)); mx[M_Z] = fmax(mx[M_Z], fabs(z));
    const double yp = fmax(y[i], 0.0), ym = fmax(-y[i], 0.0);
    if (yp != 0.0) {
      if (ui > BINF) mx[M_INF] = 1.0;
      else { mx[M_COMP] = fmax(mx[M_COMP], yp * (ui - z)); sm[S_SUP] += ui * yp; }
    }
    if (ym != 0.0) {
      if (li < -BINF) mx[M_INF] = 1.0;
      else { mx[M_COMP] = fmax(mx[M_COMP], ym * (z - li)); sm[S_SUP] -= li * ym; }
    }
  }
  for (int j = tid; j < n; j += BV_NT) {
    double px = 0.0, aty = 0.0;
    for (int k = p.Fp[j]; k < p.Fp[j + 1]; ++k) px += Pv[p.Fk[k]] * x[p.Fi[k]];
    for (int k = p.Ap[j]; k < p.Ap[j + 1]; ++k) aty += Av[k] * y[p.Ai[k]];
    const double qj = q[j];
    mx[M_DUA] = fmax(mx[M_DUA], fabs((px + qj) + aty));
    mx[M_PX] = fmax(mx[M_PX], fabs(px)); mx[M_ATY] = fmax(mx[M_ATY], fabs(aty)); mx[M_Q] = fmax(mx[M_Q], fabs(qj));
    sm[S_XPX] += x[j] * px; sm[S_QX] += qj * x[j];
  }
  b_reduce_many<NW, NMAX, NSUM>(mx, sm, buf);
  if (tid == 0) {
    const double *r = buf + NW * (NMAX + NSUM), *t = r + NMAX;
    const bool inf = r[M_INF] != 0.0;
    const double obj = 0.5 * t[S_XPX] + t[S_QX], dobj = inf ? -OSQP_INFTY : -0.5 * t[S_XPX] - t[S_SUP];
    const double eps_pri = v.eps_abs + v.eps_rel * fmax(r[M_AX], r[M_Z]);
    const double eps_dua = v.eps_abs + v.eps_rel * fmax(fmax(r[M_PX], r[M_ATY]), r[M_Q]);
    const double rec[14] = {obj, r[M_PRI], r[M_DUA], r[M_AX], r[M_Z], r[M_PX], r[M_ATY], r[M_Q], eps_pri, eps_dua,
                            inf ? OSQP_INFTY : r[M_COMP], dobj, inf ? OSQP_INFTY : obj - dobj,
                            (r[M_PRI] < eps_pri && r[M_DUA] < eps_dua) ? 1.0 : 0.0};
    const bool nan = r[M_NAN] != 0.0;
    for (int k = 0; k < 13; ++k) out[k] = nan ? OSQP_NAN : rec[k];
    out[13] = nan ? 0.0 : rec[13];
  }
  __syncthreads();       // buf is read; x and y are free

  // ---- slots 14, 15: dx in x's place, dy projected on the polar of the recession cone of [l, u] in y's ---------------
  enum { C_NDY, C_NDX, C_NANDY, C_NANDX, CMAX };
  enum { C_INEQ, C_QDX, CSUM };
  double cm[CMAX] = {0.0, 0.0, 0.0, 0.0}, cs[CSUM] = {0.0, 0.0};
  for (int i = tid; i < m; i += BV_NT) {
    double d = DY[i];
    if (bv_nan(d)) cm[C_NANDY] = 1.0;
    const double li = l[i], ui = u[i];
    if (ui > BINF) d = li < -BINF ? 0.0 : fmin(d, 0.0);
    else if (li < -BINF) d = fmax(d, 0.0);
    y[i] = d;
    cm[C_NDY] = fmax(cm[C_NDY], fabs(d));
    cs[C_INEQ] += ui * fmax(d, 0.0) + li * fmin(d, 0.0);
  }
  for (int j = tid; j < n; j += BV_NT) {
    const double d = DX[j];
    if (bv_nan(d)) cm[C_NANDX] = 1.0;
    x[j] = d;
    cm[C_NDX] = fmax(cm[C_NDX], fabs(d));
    cs[C_QDX] += q[j] * d;
  }
  b_reduce_many<NW, CMAX, CSUM>(cm, cs, buf);
  const double *c = buf + NW * (CMAX + CSUM);
  const double ndy = c[C_NDY], ndx = c[C_NDX], ineq = c[CMAX + C_INEQ], qdx = c[CMAX + C_QDX];
  const bool nandy = c[C_NANDY] != 0.0, nandx = c[C_NANDX] != 0.0;
  double natdy = 0.0, npdx = 0.0, viol = 0.0;
  for (int j = tid; j < n; j += BV_NT) {
    double atdy = 0.0, pdx = 0.0;
    for (int k = p.Ap[j]; k < p.Ap[j + 1]; ++k) atdy += Av[k] * y[p.Ai[k]];
    for (int k = p.Fp[j]; k < p.Fp[j + 1]; ++k) pdx += Pv[p.Fk[k]] * x[p.Fi[k]];
    natdy = fmax(natdy, fabs(atdy)); npdx = fmax(npdx, fabs(pdx));
  }
  for (int i = tid; i < m; i += BV_NT) {
    double adx = 0.0;
    for (int k = p.Rp[i]; k < p.Rp[i + 1]; ++k) adx += Av[p.Rk[k]] * x[p.Rj[k]];
    if ((u[i] < BINF && adx > v.eps_dinf * ndx) || (l[i] > -BINF && adx < -v.eps_dinf * ndx)) viol = 1.0;
  }
  natdy = b_max<NW>(natdy, buf); npdx = b_max<NW>(npdx, buf); viol = b_max<NW>(viol, buf);
  if (tid == 0) {
    out[14] = (!nandy && ndy > OSQP_DIVISION_TOL && ineq < v.eps_pinf * ndy && natdy < v.eps_pinf * ndy) ? 1.0 : 0.0;
    out[15] = (!nandx && ndx > OSQP_DIVISION_TOL && qdx < v.eps_dinf * ndx && npdx < v.eps_dinf * ndx && viol == 0.0) ? 1.0 : 0.0;
  }
}
