// engine_block_direct.h -- included by engine.hip after engine_pcg_blockres.h and before dense_direct.h (it uses Ctx, DenseP and
// dense_block_mv_x of engine_device.h; dense_direct.h uses its INV_TB for k_dd_pivot and k_dd_chol).
// The block-direct solve (FORM_BLOCK_DIRECT): BdCtx, k_blk_invert, k_blk_apply, k_blk_finish, the coupled form's k_cpl_dot /
// k_cpl_solve / k_blk_apply_back / k_blk_apply_multi, and the capacitance inverse k_cap_diag / k_cap_step.

// ---------------------------------------------------------------------------
// Block-direct solve: the portfolio family (BASELINE config 5) without any iteration at all.
//
// Same structure as k_pcg_blockres accepts: P = dense diagonal blocks only, every row of A single-entry except nh <= 4
// huge rows.  Then  K = B + A_h' R_h A_h  with B = blockdiag(P_b + sigma I + diag(sum_i rho_i a_ij^2)) and the nh huge
// rows as a low-rank term, and by the Woodbury identity
//     K^-1 r = t - W c,     t = B^-1 r,   W = B^-1 A_h' (n x nh),   c = (R_h^-1 + A_h W)^-1 (A_h t).
// The blocks are inverted explicitly (k_blk_invert: in-place Gauss-Jordan in LDS, no pivoting -- B_b is positive
// definite or the problem is not convex: a non-positive pivot is reported as negative curvature) whenever rho, sigma or
// the matrices change, and kept in HBM in the layout of the dense blocks of P.  One linear solve is then
//     k_blk_apply   t = B^-1 r0 : ONE pass over the 50 MB of inverse blocks (the dense_block_mv of k_cg_B, which the PCG
//                   ran 26 times per ADMM iteration) + the partials of A_h t
//     k_blk_finish  c from the partials (nh x nh system, inverted on the host at refresh), x~ = x~0 + t - W c
// applied to the residual r0 = b - K x~0 of the warm start k_pcg_init forms anyway (one step of iterative refinement
// on top of the previous x~: the error of the explicit inverse, ~cond(B) eps, multiplies the CORRECTION, not x~).
// Config 5: 258 -> 4x us per ADMM iteration.  OSQP_AMD_BLOCK_DIRECT=0 keeps the block-resident PCG.
// ---------------------------------------------------------------------------
struct BdCtx {
  double *binv;            // inverse blocks, layout of Ctx::dP.val (DenseBlk::off / pitch)
  double *t;               // [n] B^-1 r
  double *wh;              // [nh][n] W = B^-1 A_h'
  double *cinv;            // [nh][nh] (R_h^-1 + A_h W)^-1
  double *part;            // [MAX_HUGE_FOLD][nblk] partials of A_h t per block
  int    *flag;            // [0] a pivot was not positive
  double *chk;             // [2] checks of a fresh inverse (bit patterns of non-negative doubles, atomicMax): blocks, capacitance matrix
  double *cap0;            // [kc][kc] the capacitance matrix as formed (coupled form): its inverse is checked against it
  int     fin_dots;        // the kernel that writes x~ also leaves the folded huge rows' partials of A x~ for k_admm_finalize (no k_huge_dot launch)
  // coupled form (kc > 0): EVERY row of A with two or more entries -- sector rows, the budget row, whatever their length -- is a
  // term of the low-rank part; nothing of W is stored (see k_cpl_dot)
  int     kc;
  const int *crow;         // [kc] the coupling rows of A
  const int *cidx;         // [m] position of a row in crow, -1 for the single-entry rows
  const int *chuge;        // [kc] which folded huge row (Ctx::hrow) a coupling row is, -1: none
  const int *cbptr;        // [n + 1] / cbent: per column j the entries of the coupling rows, {position in crow, slot of the value in M.val}
  const int2 *cbent;
  double *cs, *cc;         // [kc] S t and Cinv S t
  double *cap;             // [kc][kc] capacitance matrix R^-1 + S B^-1 S', inverted in place (k_cap_invert)
  double *cap2;            // [kc][kc] the other copy of the pivot steps
  double *wm;              // [16][n] scratch of the refresh: B^-1 S' for 16 coupling rows
};

#define INV_TB 1024
__global__ void __launch_bounds__(INV_TB) k_blk_invert(Ctx c, BdCtx bd) {
  extern __shared__ __attribute__((aligned(16))) double bl[];       // b x b, row pitch b
  __shared__ double colp[DENSE_MAX], rowp[DENSE_MAX];
  const double sigma = c.prm->sigma;
  // thread -> column j and the rows i = i0, i0 + 8, ... (no index arithmetic in the sweep: a division per element made this
  // kernel 2.85 ms for the 400 blocks of config 5; with 256 threads -- one wavefront per SIMD, nothing to hide the LDS round trips
  // of the sweep behind -- it was 1.9 ms)
  constexpr int RS = INV_TB / DENSE_MAX, RU = DENSE_MAX / RS;        // row step 8, up to 16 rows per thread
  const int t = threadIdx.x, j = t & (DENSE_MAX - 1), i0 = t / DENSE_MAX;
  for (int db = blockIdx.x; db < c.dP.nblk; db += gridDim.x) {
    const DenseBlk d = c.dP.blk[db];
    const int b = d.b;
    if (j < b) for (int i = i0; i < b; i += RS) bl[i * b + j] = c.dP.val[d.off + (size_t)i * d.pitch + j];
    __syncthreads();
    if (t < b) {                       // diagonal: sigma + the single-entry rows of A at this column (the huge rows are the low-rank part)
      const int jj = d.c0 + t;
      double dadd = sigma;
      for (int k = c.Mk.rowptr[jj]; k < c.Mk.rowptr[jj + 1]; ++k) {
        const int row = c.Mk.col[k] - c.n;
        if (bd.kc && bd.cidx[row] >= 0) continue;           // (coupled form: such a row is part of S)
        const double a = c.Mk.val[k]; dadd += c.rho[row] * a * a;
      }
      bl[t * b + t] += dadd;
    }
    __syncthreads();
    for (int p = 0; p < b; ++p) {
      if (t < b) { colp[t] = bl[t * b + p]; rowp[t] = bl[p * b + t]; }
      __syncthreads();
      const double piv = rowp[p];
      if (!(piv > 0.0) && t == 0) atomicOr(bd.flag, 1);
      const double inv = 1.0 / piv;
      if (j < b) {
        const double rj = rowp[j] * inv;              // row p of the result (j != p)
        double cur[RU], cp[RU];                       // all rows of the thread: their LDS reads are in flight together
#pragma unroll
        for (int u = 0; u < RU; ++u) { const int i = i0 + RS * u; if (i < b) { cur[u] = bl[i * b + j]; cp[u] = colp[i]; } else { cur[u] = 0.0; cp[u] = 0.0; } }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          const int i = i0 + RS * u;
          if (i >= b) continue;
          double v;
          if (i == p) v = (j == p) ? inv : rj;
          else if (j == p) v = -cp[u] * inv;
          else v = cur[u] - cp[u] * rj;
          bl[i * b + j] = v;
        }
      }
      __syncthreads();
    }
    if (j < d.pitch) for (int i = i0; i < b; i += RS) bd.binv[d.off + (size_t)i * d.pitch + j] = j < b ? bl[i * b + j] : 0.0;
    __syncthreads();
  }
}

// out_b = Binv_b in_b for every block (in, out contiguous n-vectors), and the partials of A_h out for the huge rows
__global__ void __launch_bounds__(TB) k_blk_apply(Ctx c, BdCtx bd, const double *in, double *out, int gated) {
  if (gated) { const State *st = c.st; if (st->stalled || !st->run) return; }
  __shared__ double scratch[5 * DENSE_MAX];
  __shared__ double red[16];
  const DenseP inv{c.dP.nblk, c.dP.blk, bd.binv};
  for (int db = blockIdx.x; db < c.dP.nblk; db += gridDim.x) {
    const DenseBlk d = c.dP.blk[db];
    const double y = dense_block_mv(inv, d, in, scratch);
    const int j = d.c0 + threadIdx.x;
    const bool on = (int)threadIdx.x < d.b;
    if (on) out[j] = y;
    for (int h = 0; h < c.nh; ++h) {
      const double s = block_sum(on ? c.hcol[(size_t)h * c.n + j] * y : 0.0, red);
      if (threadIdx.x == 0) bd.part[(size_t)h * c.dP.nblk + db] = s;
    }
    __syncthreads();
  }
}

// (A x~)_h of the folded huge rows for k_admm_finalize, by the kernel that has just written x~: this workgroup's partial into its
// slot of Ctx::part_h, zeros into the slots no workgroup of this launch owns (k_huge_dot, which other paths run, fills all gridA)
__device__ __forceinline__ void fin_huge_partials(const Ctx &c, const double *hd, double *red) {
  for (int h = 0; h < c.nh; ++h) {
    const double s = block_sum(hd[h], red);
    if (threadIdx.x == 0)
      for (int slot = blockIdx.x; slot < c.gridA; slot += gridDim.x) c.part_h[(size_t)h * c.gridA + slot] = slot == (int)blockIdx.x ? s : 0.0;
  }
}

// x~ = x~0 + t - W c with c = Cinv (A_h t); the linear solve is complete (one "PCG iteration" in the statistics)
__global__ void __launch_bounds__(TB) k_blk_finish(Ctx c, BdCtx bd) {
  State *st = c.st;
  if (st->stalled || !st->run) return;
  __shared__ double red[16];
  __shared__ double cs[MAX_HUGE_FOLD];
  double sh[MAX_HUGE_FOLD];
#pragma unroll
  for (int h = 0; h < MAX_HUGE_FOLD; ++h) {
    double s = 0.0;
    if (h < c.nh) for (int i = threadIdx.x; i < c.dP.nblk; i += TB) s += bd.part[(size_t)h * c.dP.nblk + i];
    sh[h] = h < c.nh ? block_sum(s, red) : 0.0;
    // plain form: K^-1 b = t0 - W Cinv (A_h t0 - R^-1 beta), t0 = B^-1 b0, b = b0 + A_h' beta: beta_h = rho_h z_h - y_h is what
    // made `t - W c` cancel to eight digits when it sat inside b (rho_eq = 4 050 on the budget row); here it never meets B^-1
    if (c.plain_rhs && h < c.nh) sh[h] -= c.vb[c.n + c.hrow[h]] / c.rho[c.hrow[h]];
  }
  if (threadIdx.x < MAX_HUGE_FOLD) {
    double v = 0.0;
    for (int h = 0; h < c.nh; ++h) v += bd.cinv[threadIdx.x * MAX_HUGE_FOLD + h] * sh[h];
    cs[threadIdx.x] = (int)threadIdx.x < c.nh ? v : 0.0;
  }
  __syncthreads();
  static_assert(MAX_HUGE_FOLD == 4, "initialisers below");
  double hd[MAX_HUGE_FOLD] = {0.0, 0.0, 0.0, 0.0};
  for (int j = blockIdx.x * TB + threadIdx.x; j < c.n; j += gridDim.x * TB) {
    double v = bd.t[j];
    for (int h = 0; h < c.nh; ++h) v -= bd.wh[(size_t)h * c.n + j] * cs[h];
    const double xt = c.plain_rhs ? v : c.vx[j] + v;
    c.va[j] = xt;
    if (bd.fin_dots) for (int h = 0; h < c.nh; ++h) hd[h] += c.hcol[(size_t)h * c.n + j] * xt;
  }
  if (bd.fin_dots) fin_huge_partials(c, hd, red);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->iters[0] = 1; st->iters[1] = 0; st->done = 1;
    if (*bd.flag) st->neg_curv = 1;
  }
}

// ---- coupled form: P = dense diagonal blocks, A = single-entry rows + kc <= CPL_MAX rows of any shape ---------------------------
// (SURVEY C5 "+ 500 sparse sector rows": rows that tie variables of different blocks together.)  K = B + S' R S with S the kc
// coupling rows, and   K^-1 r = t - B^-1 S' c,   t = B^-1 r,   c = (R^-1 + S B^-1 S')^-1 S t.   W = B^-1 S' would be n x kc dense
// (200 MB at 500 rows), so it is never formed: the second term is a second pass over the inverse blocks (50 MB).  Per solve:
//     k_blk_apply (t)  ->  k_cpl_dot (S t, one workgroup per coupling row)  ->  k_cpl_solve (c: kc x kc dense product, one wavefront
//     per row)  ->  k_blk_apply_back (S' c gathered on the fly as the input of the block product; x~ = x~0 + t - result).
// The capacitance matrix is built at refresh from kc block passes (column r = S B^-1 S' e_r) and inverted by one workgroup
// in place (k_cap_invert: Gauss-Jordan without pivoting, the matrix is positive definite when K is).
#define CPL_MAX 512
// out[blockIdx.y * ostride + r] = (row crow[r] of A) . x[blockIdx.y * xstride ...]; use_part: a folded huge row takes the per-block
// partials the block pass left instead of walking its 50 000 entries (single right-hand side only)
__global__ void __launch_bounds__(TB) k_cpl_dot(Ctx c, BdCtx bd, const double *x, double *out, int gated, int use_part, long long xstride, long long ostride, int nrhs) {
  if (gated) { const State *st = c.st; if (st->stalled || !st->run) return; }
  if ((int)blockIdx.y >= nrhs) return;
  __shared__ double red[16];
  x += (size_t)blockIdx.y * xstride; out += (size_t)blockIdx.y * ostride;
  const int i = bd.crow[blockIdx.x], h = use_part ? bd.chuge[blockIdx.x] : -1;
  double s = 0.0;
  if (h >= 0) {
    for (int q = threadIdx.x; q < c.dP.nblk; q += TB) s += bd.part[(size_t)h * c.dP.nblk + q];
  } else {
    const int k0 = c.A.rowptr[i], k1 = c.A.rowptr[i + 1];
    int k = k0 + (int)threadIdx.x;
    for (; k + 3 * TB < k1; k += 4 * TB) {
      const double v0 = c.A.val[k], v1 = c.A.val[k + TB], v2 = c.A.val[k + 2 * TB], v3 = c.A.val[k + 3 * TB];
      const double x0 = x[c.A.col[k]], x1 = x[c.A.col[k + TB]], x2 = x[c.A.col[k + 2 * TB]], x3 = x[c.A.col[k + 3 * TB]];
      s += v0 * x0; s += v1 * x1; s += v2 * x2; s += v3 * x3;
    }
    for (; k < k1; k += TB) s += c.A.val[k] * x[c.A.col[k]];
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}
__global__ void __launch_bounds__(TB) k_cpl_solve(Ctx c, BdCtx bd) {
  { const State *st = c.st; if (st->stalled || !st->run) return; }
  const int r = blockIdx.x * (TB / 64) + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= bd.kc) return;
  double s = 0.0;
  if (c.plain_rhs) for (int q = lane; q < bd.kc; q += 64) { const int i = bd.crow[q]; s += bd.cap[(size_t)r * bd.kc + q] * (bd.cs[q] - c.vb[c.n + i] / c.rho[i]); }   // (S t0 - R^-1 beta)
  else for (int q = lane; q < bd.kc; q += 64) s += bd.cap[(size_t)r * bd.kc + q] * bd.cs[q];
  s = wave_sum(s);
  if (lane == 0) bd.cc[r] = s;
}
// entry j of S' v for a kc-vector v: the coupling rows' entries of column j as (position in crow, slot of the value in M), a list
// of their own (through M itself: split/rowptr -> col -> cidx -> v, four dependent loads; here three)
__device__ __forceinline__ double cpl_back_entry(const Ctx &c, const BdCtx &bd, const double *v, int j) {
  double s = 0.0;
  for (int k = bd.cbptr[j]; k < bd.cbptr[j + 1]; ++k) { const int2 e = bd.cbent[k]; s += c.M.val[e.y] * v[e.x]; }
  return s;
}
// x~ = x~0 + t - B^-1 S' c, the solve is complete
__global__ void __launch_bounds__(TB) k_blk_apply_back(Ctx c, BdCtx bd) {
  State *st = c.st;
  if (st->stalled || !st->run) return;
  __shared__ double scratch[5 * DENSE_MAX];
  __shared__ double red[16];
  const DenseP inv{c.dP.nblk, c.dP.blk, bd.binv};
  double hd[MAX_HUGE_FOLD] = {0.0, 0.0, 0.0, 0.0};
  for (int db = blockIdx.x; db < c.dP.nblk; db += gridDim.x) {
    const DenseBlk d = c.dP.blk[db];
    const double y = dense_block_mv_x<true>(inv, d, [&](int j) { return cpl_back_entry(c, bd, bd.cc, j); }, scratch);
    const int j = d.c0 + threadIdx.x;
    if ((int)threadIdx.x < d.b) {
      const double xt = c.plain_rhs ? bd.t[j] - y : c.vx[j] + (bd.t[j] - y);
      c.va[j] = xt;
      if (bd.fin_dots) for (int h = 0; h < c.nh; ++h) hd[h] += c.hcol[(size_t)h * c.n + j] * xt;
    }
    __syncthreads();
  }
  if (bd.fin_dots) fin_huge_partials(c, hd, red);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->iters[0] = 1; st->iters[1] = 0; st->done = 1;
    if (*bd.flag) st->neg_curv = 1;
  }
}
// Refresh: W_g = B^-1 S_g' for a group of 16 coupling rows [r0, r0 + 16) at once -- the one place of this path where a block
// meets several vectors, so the product runs on the matrix cores: v_mfma_f64_16x16x4_f64, D (16 rows of the block x 16
// right-hand sides) += A (16 x 4 tile of the inverse block, read transposed: the block is symmetric, so 4 rows x 16
// contiguous doubles per wave load) x B (4 x 16 tile of S_g' from LDS).  Wavefront w owns rows [32 w, 32 w + 32) of the block.
// One pass over the 50 MB of inverse blocks serves 16 columns of the capacitance matrix (the VALU kernel above: one).
// out: [16][n].
typedef double mfma_d4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(TB) k_blk_apply_multi(Ctx c, BdCtx bd, int r0, double *out) {
  __shared__ double xl[DENSE_MAX * 16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  static_assert(TB == 256 && DENSE_MAX == 128, "four wavefronts x two 16-row tiles cover a block");
  for (int db = blockIdx.x; db < c.dP.nblk; db += gridDim.x) {
    const DenseBlk d = c.dP.blk[db];
    const double *dv = bd.binv + d.off;
    double a[2][DENSE_MAX / 4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kt = 0; kt < DENSE_MAX / 4; ++kt) {
        const int k = 4 * kt + lk, i = 32 * w + 16 * t + li;
        a[t][kt] = (k < d.b && i < d.b) ? dv[(size_t)k * d.pitch + i] : 0.0;
      }
    for (int q = threadIdx.x; q < DENSE_MAX * 16; q += TB) xl[q] = 0.0;
    __syncthreads();
    if ((int)threadIdx.x < d.b) {
      const int j = d.c0 + threadIdx.x;
      for (int k = c.M.split[j]; k < c.M.rowptr[j + 1]; ++k) {
        const int q = bd.cidx[c.M.col[k] - c.n] - r0;
        if (q >= 0 && q < 16) xl[threadIdx.x * 16 + q] = c.M.val[k];
      }
    }
    __syncthreads();
    mfma_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kt = 0; kt < DENSE_MAX / 4; ++kt) {
      const double bv = xl[(4 * kt + lk) * 16 + li];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][kt], bv, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1][kt], bv, acc1, 0, 0, 0);
    }
    // D[row = lk + 4 r][col = li]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i0 = 32 * w + lk + 4 * r, i1 = i0 + 16;
      if (i0 < d.b) out[(size_t)li * c.n + d.c0 + i0] = acc0[r];
      if (i1 < d.b) out[(size_t)li * c.n + d.c0 + i1] = acc1[r];
    }
    __syncthreads();
  }
}
// cap <- (cap + R^-1)^-1: Gauss-Jordan without pivoting (the matrix is positive definite when K is), one launch per pivot over
// the whole machine, from one copy of the matrix into the other (no element is read after it was rewritten).  One workgroup
// walking the 2 MB in global memory took 61 us per pivot (31 ms at 501 rows); a launch takes 3.
__global__ void __launch_bounds__(TB) k_cap_diag(Ctx c, BdCtx bd) {
  const int r = blockIdx.x * TB + threadIdx.x;
  if (r >= bd.kc) return;
  const double rho = c.rho[bd.crow[r]];
  if (!(rho > 0.0)) atomicOr(bd.flag, 1);
  bd.cap[(size_t)r * bd.kc + r] += 1.0 / rho;
}
__global__ void __launch_bounds__(TB) k_cap_step(BdCtx bd, const double *src, double *dst, int p) {
  const int kc = bd.kc;
  const long long e = (long long)blockIdx.x * TB + threadIdx.x;
  if (e >= (long long)kc * kc) return;
  const int i = (int)(e / kc), j = (int)(e - (long long)i * kc);
  const double piv = src[(size_t)p * kc + p];
  if (e == 0 && !(piv > 0.0)) atomicOr(bd.flag, 1);
  const double inv = 1.0 / piv, rj = src[(size_t)p * kc + j] * inv, ci = src[(size_t)i * kc + p];
  double v;
  if (i == p) v = (j == p) ? inv : rj;
  else if (j == p) v = -ci * inv;
  else v = src[e] - ci * rj;
  dst[e] = v;
}
