// engine_pcg_blockres.h -- included by engine.hip after engine_pcg_resident.h (it uses the RES_* constants, the bounded waits and
// the granule exchange defined there, and cg_step of engine_pcg_steps.h).
// The block-resident PCG (FORM_BLOCKRES): BrCtx and k_pcg_blockres.


// ---------------------------------------------------------------------------
// Block-resident PCG: the resident idea for the portfolio family (BASELINE config 5), whose n = 50 000 is far beyond
// the vector exchange of k_pcg_resident -- and which needs none.  If P consists of dense diagonal blocks only and every
// row of A either has a single entry (bounds) or is one of at most four huge rows (a budget constraint), then
//     K = blockdiag(P_b + sigma I + diag(sum_i rho_i a_ij^2))  +  sum_h rho_h a_h a_h'
// and a workgroup that owns whole blocks needs nobody else's vector elements: K_b u_b is a dense product from registers
// (each row of a block split over two threads, 64 entries each), the low-rank part needs the scalars s_h = a_h'u, and
// delta = (Ku, u) = sum_g (K_b u_b, u_b) + sum_h rho_h s_h^2.  So ONE exchange of 3 + nh scalars per workgroup and
// iteration (tagged 8-byte granules, the exchange (2) of k_pcg_resident) carries gamma, delta', ||r||^2 and the s_h;
// everything else is local.  Chronopoulos-Gear recurrences with a fresh product (cg_step), 3 barriers per iteration.
// The 50 MB of blocks are read once per launch instead of once per PCG iteration.
// ---------------------------------------------------------------------------
struct BrCtx { int nwg; const int *blk0; double *sbuf; int *dbg; };

template <int NH>
__global__ void __launch_bounds__(RES_TB) k_pcg_blockres(Ctx c, BrCtx bc) {
  constexpr int NV = 3 + NH;                 // scalars per workgroup and iteration
  __shared__ double ul[256];                 // u of the own rows
  __shared__ double red[8 * 8];              // per-wavefront partials
  __shared__ double tot[8];                  // totals; [7]: a wait timed out
  __shared__ double sval[256 * NV];          // every workgroup's scalars during the exchange
  State *st = c.st;
  TL_MARK(c, 6);
  if (st->stalled || !st->run || st->res_fail) return;
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6, nwg = bc.nwg;
#ifdef OSQP_AMD_TIMELINE
  __shared__ long long btl[6 * 64];          // phase stamps of the first 64 iterations (workgroup 0)
#define BTL(k) do { if (blockIdx.x == 0 && threadIdx.x == 0 && nx >= 1 && nx <= 64) btl[(nx - 1) * 6 + (k)] = wall_clock64(); } while (0)
#else
#define BTL(k) do { } while (0)
#endif
  const Params prm = *c.prm;
  const unsigned ep0 = st->res_epoch;
  // the row of this thread pair: row rl of the workgroup's (at most two) blocks, columns [64 h, 64 h + 64) of its block
  const int rl = t >> 1, h = t & 1;
  int j = -1, cb = 0, bw = 0, c0 = 0, pitch = 0; size_t off = 0;
  {
    int base = 0;
    for (int q = bc.blk0[g]; q < bc.blk0[g + 1]; ++q) {
      const DenseBlk d = c.dP.blk[q];
      if (rl >= base && rl < base + d.b) { j = d.c0 + (rl - base); cb = base; bw = d.b; c0 = d.c0; off = (size_t)d.off; pitch = d.pitch; }
      base += d.b;
    }
  }
  const bool row = j >= 0, own = row && h == 0;
  double dadd = 0.0, hc[NH > 0 ? NH : 1], hrho[NH > 0 ? NH : 1];
#pragma unroll
  for (int q = 0; q < NH; ++q) { hc[q] = 0.0; hrho[q] = c.rho[c.hrow[q]]; }
  if (row) {
    dadd = prm.sigma;
    for (int k = c.M.split[j]; k < c.M.rowptr[j + 1]; ++k) {          // single-entry rows of A at this column
      const int i = c.M.col[k] - c.n;
      bool huge = false;
#pragma unroll
      for (int q = 0; q < NH; ++q) huge |= i == c.hrow[q];
      if (!huge) { const double a = c.M.val[k]; dadd += c.rho[i] * a * a; }
    }
#pragma unroll
    for (int q = 0; q < NH; ++q) hc[q] = c.hcol[(size_t)q * c.n + j];
  }
  double kv[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int cc = h * 64 + k;
    // K_b is symmetric: entry (row, cc) is read as (cc, row), so that the lanes of a wave instruction -- consecutive rows --
    // read consecutive addresses (row-wise it was one 64-byte segment per lane: 100 us per launch)
    kv[k] = (row && cc < bw) ? c.dP.val[off + (size_t)cc * pitch + (j - c0)] + (cc == j - c0 ? dadd : 0.0) : 0.0;
  }
  double rr0 = 0.0, bb = 0.0;
  for (int i = lane; i < c.gridM; i += 64) { rr0 += c.part_rr[i]; bb += c.part_bb[i]; }
  rr0 = wave_sum(rr0); bb = wave_sum(bb);
  const double tol2 = fmax(prm.eps_rel * prm.eps_rel * bb, prm.eps_abs * prm.eps_abs);
  if (rr0 <= tol2) {
    if (g == 0 && t == 0) { st->done = 1; st->tol2 = tol2; }
    return;
  }
  double r_ = 0, u_ = 0, p_ = 0, s_ = 0, x_ = 0, mi = 0;
  if (own) { r_ = c.init_r[(size_t)j * c.init_stride]; u_ = c.init_z[j]; x_ = c.vx[j]; mi = c.minv[j]; }
  if (t < 256) ul[t] = 0.0;
  if (t == 0) tot[7] = 0.0;
  __syncthreads();
  double gam_old = 0.0, alp_old = 0.0;
  int iters = 0, nx = 0;
  bool conv = false, bad = false, failed = false;
  while (true) {
    ++nx;
    const unsigned tag = ep0 + (unsigned)nx;
    const int par = (int)(tag & 1u);
    BTL(0);
    if (own) ul[rl] = u_;
    __syncthreads();
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 64; ++k) acc += kv[k] * ul[cb + h * 64 + k];
    acc += dpp_move<0xB1>(acc);                      // the two halves of the row
    BTL(1);
    double v[NV];
    v[0] = own ? r_ * u_ : 0.0; v[1] = own ? acc * u_ : 0.0; v[2] = own ? r_ * r_ : 0.0;
#pragma unroll
    for (int q = 0; q < NH; ++q) v[3 + q] = own ? hc[q] * u_ : 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) { const double w_ = wave_sum(v[i]); if (lane == 0) red[wv * 8 + i] = w_; }
    __syncthreads();
    BTL(2);
    unsigned long long *gb = reinterpret_cast<unsigned long long *>(bc.sbuf) + (size_t)par * nwg * RES_GSTRIDE;
    if (wv == 0 && lane < 2 * NV) {
      const int i = lane >> 1;
      double sv = 0.0;
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8) sv += red[w8 * 8 + i];
      const unsigned half = (lane & 1) ? (unsigned)__double2hiint(sv) : (unsigned)__double2loint(sv);
      __hip_atomic_store(gb + (size_t)g * RES_GSTRIDE + lane, ((unsigned long long)tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (wv < ((nwg + 63) >> 6)) {
      // one workgroup's 2 NV granules per lane, all loads in flight together, only what is still missing (see k_pcg_resident)
      const int o = t;
      const __amdgpu_buffer_rsrc_t rg = res_rsrc(gb, (size_t)nwg * RES_GSTRIDE * 8);
      unsigned pend = o < nwg ? (1u << (2 * NV)) - 1u : 0u;
      int miss16 = -1;
      unsigned *svw = reinterpret_cast<unsigned *>(sval) + 2 * NV * o;
      unsigned seen = 0, rounds = 0;
      long long t0 = wall_clock64();
      int late = 0;
      bool gave = false;
      while (true) {
        u32x2 gv[2 * NV];
#pragma unroll
        for (int q = 0; q < 2 * NV; ++q) if (pend & (1u << q)) gv[q] = __builtin_amdgcn_raw_buffer_load_b64(rg, (o * RES_GSTRIDE + q) * 8, 0, AUX_SC1 | AUX_VOL);
#pragma unroll
        for (int q = 0; q < 2 * NV; ++q)
          if (pend & (1u << q)) { if (gv[q].y == tag) { svw[q] = gv[q].x; pend &= ~(1u << q); } else seen = gv[q].y; }
        if (!__any(pend != 0)) break;
        asm volatile("" ::: "memory");
        if (++rounds & 15u) { __builtin_amdgcn_s_sleep(1); continue; }
        const int verdict = res_spin_check(st, t0, late);
        if (verdict) {
          const unsigned long long miss = __ballot(pend != 0);
          const int fl = miss ? (int)__ffsll((long long)miss) - 1 : 0;
          const unsigned sv = (unsigned)__builtin_amdgcn_readlane((int)seen, fl);
          const int gi = __builtin_amdgcn_readlane((int)pend, fl);
          if (lane == 0) { res_note(st, bc.dbg, g, verdict, 2, nx, miss ? 64 * wv + fl : -1, sv, t0, rounds, gi); tot[7] = 1.0; }
          gave = true;
          break;
        }
        if (rounds == 16u) { const unsigned long long ms = __ballot(pend != 0); miss16 = ms ? 64 * wv + (int)__ffsll((long long)ms) - 1 : -1; }
        if ((rounds & 63u) == 0 && wv == 0) {          // a long wait: say it again
          if (lane < 2 * NV) {
            const int i = lane >> 1;
            double sv2 = 0.0;
#pragma unroll
            for (int w8 = 0; w8 < 8; ++w8) sv2 += red[w8 * 8 + i];
            const unsigned half = (lane & 1) ? (unsigned)__double2hiint(sv2) : (unsigned)__double2loint(sv2);
            __hip_atomic_store(gb + (size_t)g * RES_GSTRIDE + lane, ((unsigned long long)tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          if (lane == 0) atomicAdd(&st->res_repub, 1);
        }
        if ((rounds & 255u) == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __builtin_amdgcn_s_sleep(1);
      }
      if (rounds >= 16u && lane == 0 && !gave) res_slow_note(st, t0, nx, g, miss16, 2);
    }
    BTL(3);
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) if (lane + 64 * q < nwg) a += sval[NV * (lane + 64 * q) + i];
        a = wave_sum(a);
        if (lane == 0) tot[i] = a;
      }
    }
    __syncthreads();
    BTL(4);
    if (tot[7] != 0.0) { failed = true; break; }
    const double gam = tot[0], rr = tot[2];
    double del = tot[1];
#pragma unroll
    for (int q = 0; q < NH; ++q) del += hrho[q] * (tot[3 + q] * tot[3 + q]);
    const CgStep cs = cg_step(rr, gam, del, gam_old, alp_old, tol2, iters, 0, prm, false);
    if (cs.stop) { conv = cs.conv; bad = cs.bad && !cs.conv; break; }
    ++iters; gam_old = gam; alp_old = cs.alpha;
    if (own) {
      double w_ = acc;
#pragma unroll
      for (int q = 0; q < NH; ++q) w_ += (hrho[q] * tot[3 + q]) * hc[q];
      p_ = cs.first ? u_ : (u_ + cs.beta * p_);
      s_ = cs.first ? w_ : (w_ + cs.beta * s_);
      x_ += cs.alpha * p_;
      r_ -= cs.alpha * s_;
      u_ = mi * r_;
    }
    BTL(5);
  }
#ifdef OSQP_AMD_TIMELINE
  if (g == 0 && t == 0 && !failed) {
    const int cnt = (nx - 1 < 64 ? nx - 1 : 64) * 6;          // (the last trip broke out before its stamp 5)
    const unsigned long long k0 = atomicAdd(c.tl, (unsigned long long)cnt + 1);
    if (k0 + cnt + 1 < TL_CAP - 2) {
      for (int q = 0; q < cnt; ++q) c.tl[1 + k0 + q] = ((unsigned long long)(40 + q % 6) << 56) | ((unsigned long long)btl[q] & 0x00FFFFFFFFFFFFFFull);
      c.tl[1 + k0 + cnt] = (46ull << 56) | (wall_clock64() & 0x00FFFFFFFFFFFFFFull);
    }
  }
#endif
  if (failed) {
    if (t == 0) {
      __hip_atomic_store(&st->res_fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int *d = bc.dbg + (size_t)RES_DBG * g;
      d[0] = nx; d[1] = 3; d[2] = iters;
    }
    return;
  }
  if (own && iters > 0) c.va[j] = x_;
  if (g == 0 && t == 0) {
    st->iters[0] = iters; st->iters[1] = 0;
    st->done = conv ? 1 : 2;
    if (bad) st->neg_curv = 1;
    st->tol2 = tol2;
    st->res_epoch = ep0 + (unsigned)nx;
  }
}
