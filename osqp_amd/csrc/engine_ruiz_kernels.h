// engine_ruiz_kernels.h -- included by engine.hip after engine_check_kernels.h (it uses TB, Ctx, the SC_* slots and the reductions of
// engine_device.h).
// Ruiz equilibration on the device: clip_scaling, k_ruiz_norms, k_ruiz_apply, k_ruiz_cost_norms, k_ruiz_cost_scalar,
// k_ruiz_cost_apply, k_ruiz_finish (hipeng_ruiz_scale drives them).

// ---------------------------------------------------------------------------
// Ruiz equilibration on the device (reference src/scaling.c:44-156).  One wavefront
// per matrix row; the products are formed in the reference's order
// ((val * row factor) * column factor, then * c) so both device copies of A hold the
// same bits.  Scratch: dn (n), en (m) live in kp / dy; scalars in scal[SC_RUIZ..].
// ---------------------------------------------------------------------------
__device__ __forceinline__ double clip_scaling(double v) {
  if (v < 1e-4) v = 1.0;
  if (v > 1e4) v = 1e4;
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// dn[j] = 1/sqrt(clip(max |column j of [P;A]|)), en[i] = 1/sqrt(clip(max |row i of A|))
__global__ void __launch_bounds__(TB) k_ruiz_norms(Ctx c, double *dn, double *en) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (TB / 64) + (threadIdx.x >> 6), nw = gridDim.x * (TB / 64);
  for (int r = w; r < c.n + c.m; r += nw) {
    const bool isM = r < c.n;
    const DevMat &X = isM ? c.M : c.A;
    const int row = isM ? r : r - c.n;
    double mx = 0.0;
    for (int k = X.rowptr[row] + lane; k < X.rowptr[row + 1]; k += 64) mx = fmax(mx, fabs(X.val[k]));
    mx = wave_max(mx);
    if (lane == 0) { if (isM) dn[row] = 1.0 / sqrt(clip_scaling(mx)); else en[row] = 1.0 / sqrt(clip_scaling(mx)); }
  }
}

// apply the pass: matrices, q, accumulated D and E
__global__ void __launch_bounds__(TB) k_ruiz_apply(Ctx c, const double *dn, const double *en,
                                                   double *Mval, double *Aval) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (TB / 64) + (threadIdx.x >> 6), nw = gridDim.x * (TB / 64);
  for (int r = w; r < c.n + c.m; r += nw) {
    if (r < c.n) {
      const int j = r, sp = c.M.split[j];
      const double dj = dn[j];
      for (int k = c.M.rowptr[j] + lane; k < c.M.rowptr[j + 1]; k += 64) {
        const int cc = c.M.col[k];
        // P(j,cc): row factor of the stored entry, then column factor; A'(j, n+i): E_i then D_j
        if (k < sp) {
          // the stored triu entry has row = min(j,cc), column = max(j,cc)
          const double fr = j < cc ? dj : dn[cc], fc = j < cc ? dn[cc] : dj;
          Mval[k] = (Mval[k] * fr) * fc;
        } else Mval[k] = (Mval[k] * en[cc - c.n]) * dj;
      }
      if (lane == 0) { c.q[j] = c.q[j] * dj; c.D[j] = dj * c.D[j]; }
    } else {
      const int i = r - c.n;
      const double ei = en[i];
      for (int k = c.A.rowptr[i] + lane; k < c.A.rowptr[i + 1]; k += 64) Aval[k] = (Aval[k] * ei) * dn[c.A.col[k]];
      if (lane == 0) c.E[i] = ei * c.E[i];
    }
  }
}

// cost normalisation, step 1: per-workgroup partial sums of the P column norms, max |q|
__global__ void __launch_bounds__(TB) k_ruiz_cost_norms(Ctx c) {
  __shared__ double red[16];
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (TB / 64) + (threadIdx.x >> 6), nw = gridDim.x * (TB / 64);
  double acc = 0.0, qm = 0.0;
  for (int j = w; j < c.n; j += nw) {
    double mx = 0.0;
    for (int k = c.M.rowptr[j] + lane; k < c.M.split[j]; k += 64) mx = fmax(mx, fabs(c.M.val[k]));
    mx = wave_max(mx);
    if (lane == 0) { acc += mx; qm = fmax(qm, fabs(c.q[j])); }
  }
  acc = block_sum(acc, red);
  block_max_to(qm, c.scal + SCI(SC_QDX), red);      // reuse a slot: max |q|
  if (threadIdx.x == 0) c.part_s0[blockIdx.x] = acc;
}

// step 2 (one workgroup): c_t = 1 / clip(max(mean colnorm, clip(|q|_inf))), c *= c_t
__global__ void __launch_bounds__(TB) k_ruiz_cost_scalar(Ctx c, int nparts) {
  __shared__ double red[16];
  double s[1];
  reduce_parts<1>(c.part_s0, nullptr, nullptr, nparts, red, s);
  if (threadIdx.x == 0) {
    const double mean = s[0] / (double)c.n;
    double ct = fmax(mean, clip_scaling(c.scal[SCI(SC_QDX)]));
    ct = 1.0 / clip_scaling(ct);
    c.scal[SCI(SC_OBJ)] = ct;                          // this pass's factor
    c.scal[SCI(SC_DYLHS)] = c.scal[SCI(SC_DYLHS)] * ct;  // accumulated c
    c.scal[SCI(SC_QDX)] = 0.0;
  }
}

// step 3: P <- c_t P, q <- c_t q
__global__ void __launch_bounds__(TB) k_ruiz_cost_apply(Ctx c, double *Mval) {
  const double ct = c.scal[SCI(SC_OBJ)];
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (TB / 64) + (threadIdx.x >> 6), nw = gridDim.x * (TB / 64);
  for (int j = w; j < c.n; j += nw) {
    for (int k = c.M.rowptr[j] + lane; k < c.M.split[j]; k += 64) Mval[k] *= ct;
    if (lane == 0) c.q[j] *= ct;
  }
}

// finish: l, u <- E l, E u ; Dinv, Einv
__global__ void __launch_bounds__(TB) k_ruiz_finish(Ctx c) {
  for (int i = blockIdx.x * TB + threadIdx.x; i < c.m; i += gridDim.x * TB) {
    const double e = c.E[i];
    c.l[i] = c.l[i] * e; c.u[i] = c.u[i] * e; c.Einv[i] = 1.0 / e;
  }
  for (int j = blockIdx.x * TB + threadIdx.x; j < c.n; j += gridDim.x * TB) c.Dinv[j] = 1.0 / c.D[j];
}
