// engine_block_check.h -- included by engine.hip right after dense_direct.h (it uses dd_probe_value from there, BdCtx and CPL_MAX
// from engine_block_direct.h).
// The checks of the block-direct solve's fresh inverses: k_blk_check, k_cap_check.

// Checks of the block-direct solve's fresh inverses (blk_refresh), as the dense-direct solve has them: k_blk_invert and the
// capacitance steps are Gauss-Jordan (error ~ cond^2 eps).  Per block: u = probe values, y = Binv_b u, z = B_b y with B_b = P_b +
// diag as k_blk_invert forms it; chk[0] = max |z - u| over all blocks.
__global__ void __launch_bounds__(TB) k_blk_check(Ctx c, BdCtx bd) {
  __shared__ double scratch[5 * DENSE_MAX];
  __shared__ double red[16];
  const double sigma = c.prm->sigma;
  const DenseP inv{c.dP.nblk, c.dP.blk, bd.binv};
  double worst = 0.0;
  for (int db = blockIdx.x; db < c.dP.nblk; db += gridDim.x) {
    const DenseBlk d = c.dP.blk[db];
    const double y = dense_block_mv_x(inv, d, [](int j) { return dd_probe_value(j); }, scratch);
    const int j = d.c0 + threadIdx.x;
    const bool on = (int)threadIdx.x < d.b;
    if (on) bd.t[j] = y;
    __syncthreads();
    double z = dense_block_mv_x(c.dP, d, [&](int jj) { return bd.t[jj]; }, scratch);
    if (on) {
      double dadd = sigma;
      for (int k = c.Mk.rowptr[j]; k < c.Mk.rowptr[j + 1]; ++k) {
        const int row = c.Mk.col[k] - c.n;
        if (bd.kc && bd.cidx[row] >= 0) continue;
        const double a = c.Mk.val[k]; dadd += c.rho[row] * a * a;
      }
      z += dadd * y;
      const double e = fabs(z - dd_probe_value(j));
      worst = fmax(worst, e == e ? e : 1e300);
    }
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = worst;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long *>(bd.chk), (unsigned long long)__double_as_longlong(fmax(fmax(red[0], red[1]), fmax(red[2], red[3]))));
}
// coupled form: w = cap u, z = cap0 w (cap0: the capacitance matrix as formed, cap: its inverse); chk[1] = max |z - u|.  One workgroup.
__global__ void __launch_bounds__(TB) k_cap_check(BdCtx bd) {
  __shared__ double u[CPL_MAX], w[CPL_MAX], red[16];
  const int kc = bd.kc;
  for (int r = threadIdx.x; r < kc; r += TB) u[r] = dd_probe_value(r);
  __syncthreads();
  for (int r = threadIdx.x; r < kc; r += TB) { double s = 0.0; for (int q = 0; q < kc; ++q) s += bd.cap[(size_t)r * kc + q] * u[q]; w[r] = s; }
  __syncthreads();
  double worst = 0.0;
  for (int r = threadIdx.x; r < kc; r += TB) { double s = 0.0; for (int q = 0; q < kc; ++q) s += bd.cap0[(size_t)r * kc + q] * w[q]; const double e = fabs(s - u[r]); worst = fmax(worst, e == e ? e : 1e300); }
  for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = worst;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long *>(bd.chk + 1), (unsigned long long)__double_as_longlong(fmax(fmax(red[0], red[1]), fmax(red[2], red[3]))));
}
