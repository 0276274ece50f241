// engine_pcg_steps.h -- included by engine.hip after engine_device.h (it uses TB and the other constants, the TL* macros, Ctx, State,
// the reductions, the SpMV pieces and LDS_DECL from there).
// The launch-per-step PCG (FORM_STEPS, and the fall-back of every other form): k_vd, k_pcg_init, CgStep / cg_step (the resident and
// block-resident launches use it too), k_cg_A, k_huge_reduce, k_cg_B, k_huge_dot, huge_row_sum (k_residuals uses it too), elim_vb
// (k_refresh_m uses it too) and k_admm_finalize, the last kernel of every ADMM iteration whatever the form.

// ---------------------------------------------------------------------------
// PCG kernels
// ---------------------------------------------------------------------------
// Every row kernel walks its row blocks with a workgroup-stride loop, so the
// number of dot-product partials equals the launch grid (<= MAX_PARTS).

// First kernel of an ADMM iteration: right-hand side b = sigma x - q + A'(rho z - y)
// (compute_rhs folded into the reduced system), initial residual r = b - K x~0
// with the warm start x~0 (the previous x~, linearly extrapolated by k_admm_finalize once the
// iterates move smoothly: ADMM iterates follow a linear recurrence, so 2 x~_k - x~_{k-1} is 2-10x
// closer to x~_{k+1} than x~_k is), preconditioned residual and the three start-up dot
// products.  One dual-stream pass over M.
__global__ void __launch_bounds__(TB) k_vd(Ctx c) {
  for (int k = blockIdx.x * TB + threadIdx.x; k < c.n + c.m; k += gridDim.x * TB) c.vd[k] = c.vb[k] - c.vx[k];
}
// RESFORM (the K == 0 graphs of a k_pcg_resident engine, launch_init): the only reader of r0 and u0 = Minv r0 is the resident launch,
// which wants its own rows of both, and they sit side by side in the exchanged vector's layout.  This form stores r0 at
// r0pos[u0map[j]] and u0 at u0pos[u0map[j]] -- whole lines per workgroup of the resident launch -- and leaves out init_r (one
// double in every 32-byte record) and init_z.  Same arithmetic, same partials, same returns.
template <bool DENSE, bool RESFORM>
__global__ void __launch_bounds__(TB) k_pcg_init(Ctx c, int bench, double *r0pos) {
  State *st = c.st;
  TL_MARK(c, 1);
  TLK_DECL;
  TLK_AT(0, 0); TLK_LAST(0);
  LDS_DECL(2);
  // rows inside dense diagonal blocks of P: P x~0 by the block product, A' part from the remainder
  // matrix; all other rows below (Mm = remainder matrix then, M itself otherwise)
  const DevMat &Mm = DENSE ? c.Mk : c.M;
  // Loads in three flights, as in k_admm_finalize (see there): the early returns gate stores only, every prefetch is an
  // unconditional load at a clamped index.  Flight A: the state, the parameters and this workgroup's first stream block (engines without dense
  // blocks of P; with them the dense rows come first and the stream blocks keep the plain form).
  const int s_stalled = st->stalled, s_fail = st->res_fail, s_hist = st->hist_r;
  const long long s_admm = st->admm_done, s_target = st->admm_target;
  const Params prm = *c.prm;
  // (the DENSE instantiation loads nothing here: everything below folds to the empty block)
  RowBlk b = RowBlk{0, 0, 0, 0};
  if constexpr (!DENSE) {
    b = Mm.blk[max(min((int)blockIdx.x, Mm.nstream - 1), 0)];
    if ((int)blockIdx.x >= Mm.nstream) b = RowBlk{0, 0, 0, 0};
  }
  TLK_AT(1, b.k1);
  // what the start-up of one row reads besides its two sums
  struct RowIn { double base0, base1, vx, minv; int u0, er; };
  // (u0 and er are looked at only where c.u0pos / c.nelim say so; where their arrays do not exist the load goes to minv instead of
  // into a branch, whose merge would wait for the whole flight)
  const unsigned short *u0m = c.u0pos ? c.u0map : reinterpret_cast<const unsigned short *>(c.minv);
  const int *erw = c.nelim ? c.erow : reinterpret_cast<const int *>(c.minv);
  auto row_load = [&](int j) {
    RowIn r;
    r.base0 = (prm.use_cvec ? c.cvec : c.xy)[j]; r.base1 = c.q[j];
    r.vx = c.vx[j]; r.minv = c.minv[j];
    r.u0 = (int)u0m[j]; r.er = erw[j];
    return r;
  };
  // Flight B: the chunk's indices and values, the row pointers of the row this thread helps to sum in the first round, and
  // that row's scalars in the lane that will start it.
  constexpr int E = MAX_CHUNK / TB;
  const int cnt = b.k1 - b.k0;
  int cc[E] = {}; double vv[E] = {};
  const int RL = lanes_for(b.r1 - b.r0), rg = threadIdx.x / RL, rlane = threadIdx.x % RL;
  const int jf = b.r0 + rg, jfc = max(min(jf, b.r1 - 1), 0);
  int p0 = 0, p1 = 0;
  RowIn rf = {};
  if constexpr (!DENSE) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int kc = max(min(b.k0 + (int)threadIdx.x + e * TB, b.k1 - 1), 0);
      cc[e] = Mm.col[kc]; vv[e] = Mm.val[kc];
    }
    p0 = Mm.rowptr[jfc]; p1 = Mm.rowptr[jfc + 1];
    rf = row_load(jfc);
  }
  // A solve that ran out of unrolled PCG iterations (`stalled`, raised by k_admm_finalize) is continued by
  // this graph launch: no new right-hand side, the iteration kernels below pick the recurrences up where they
  // stopped (K is even, so the parity of every ping-pong buffer is preserved).
  if (!bench) {
    if (s_stalled || s_fail) return;
    if (s_admm >= s_target) { if (blockIdx.x == 0 && threadIdx.x == 0) st->run = 0; return; }
  }
  double prz = 0, prr = 0, pbb = 0;
  if (DENSE)
  for (int db = blockIdx.x; db < c.dP.nblk; db += gridDim.x) {
    const DenseBlk d = c.dP.blk[db];
    // plain_rhs (block-direct engines): no P x~0 -- the 50 MB pass over the blocks of P that the residual form needs -- and the
    // low-rank rows' terms stay out of the right-hand side (k_blk_finish / k_cpl_solve put them back in closed form)
    double sA = c.plain_rhs ? 0.0 : dense_block_mv(c.dP, d, c.vx, lprod);
    if ((int)threadIdx.x < d.b) {
      const int j = d.c0 + threadIdx.x;
      double sB = 0.0;
      if (c.plain_rhs) {
        for (int k = Mm.rowptr[j]; k < Mm.rowptr[j + 1]; ++k) { const int cc = Mm.col[k]; if (c.plain_skip && c.plain_skip[cc - c.n] >= 0) continue; sB += Mm.val[k] * c.vb[cc]; }
      } else {
        for (int k = Mm.rowptr[j]; k < Mm.rowptr[j + 1]; ++k) { const int cc = Mm.col[k]; const double v = Mm.val[k]; sA += v * c.vx[cc]; sB += v * c.vb[cc]; }
        for (int k = 0; k < c.nh; ++k) { const double hc = c.hcol[(size_t)k * c.n + j]; sA += hc * c.vx[c.n + c.hrow[k]]; sB += hc * c.vb[c.n + c.hrow[k]]; }   // huge rows of A live outside Mk
      }
      const double base = prm.use_cvec ? c.cvec[j] : (prm.sigma * c.xy[j] - c.q[j]);
      const double bj = base + sB;
      const double rj = c.plain_rhs ? bj : bj - prm.sigma * c.vx[j] - sA;
      const double zj = c.minv[j] * rj;
      if constexpr (RESFORM) { const int p = (int)c.u0map[j]; r0pos[p] = rj; c.u0pos[p] = zj; }
      else {
        c.init_r[(size_t)j * c.init_stride] = rj;
        c.init_z[j] = zj;
        if (c.u0pos) c.u0pos[c.u0map[j]] = zj;
      }
      prz += rj * zj; prr += rj * rj; pbb += bj * bj;
    }
    __syncthreads();
  }
  // row j of the start-up given sA = (M [x~0 | rho z~0])_j and sB = (M [0 | rho z - y])_j, by one thread
  auto row_apply = [&](int j, double sA, double sB, const RowIn &r) {
    if (DENSE) for (int k = 0; k < c.nh; ++k) { const double hc = c.hcol[(size_t)k * c.n + j]; sA += hc * c.vx[c.n + c.hrow[k]]; sB += hc * c.vb[c.n + c.hrow[k]]; }
    const double base = prm.use_cvec ? r.base0 : (prm.sigma * r.base0 - r.base1);
    const bool gone = c.nelim && r.er >= 0;                // eliminated from the system: no residual, no direction
    const double bj = gone ? 0.0 : base + sB;
    const double rj = gone ? 0.0 : bj - prm.sigma * r.vx - sA;
    const double zj = r.minv * rj;
    if constexpr (RESFORM) { r0pos[r.u0] = rj; c.u0pos[r.u0] = zj; }
    else {
      c.init_r[(size_t)j * c.init_stride] = rj;
      c.init_z[j] = zj;
      if (c.u0pos) c.u0pos[r.u0] = zj;
    }
    prz += rj * zj; prr += rj * rj; pbb += bj * bj;
  };
  auto row_start = [&](int j, double sA, double sB) { row_apply(j, sA, sB, row_load(j)); };
  // this workgroup's first stream block -- Flight C: the two gathers per entry; then the row sums, and the first round of
  // rows on what flight B brought
  if (!DENSE) {
    double xa[E], xb[E];
    TLK_AT(2, cc[E - 1]);
#pragma unroll
    for (int e = 0; e < E; ++e) { xa[e] = c.vx[cc[e]]; xb[e] = c.vb[cc[e]]; }      // (beyond the chunk: the clamped entry's column again)
    TLK_AT(3, xb[E - 1]);
#pragma unroll
    for (int e = 0; e < E; ++e) { const int k = threadIdx.x + e * TB; if (k < cnt) { lprod[k] = vv[e] * xa[e]; lprod[MAX_CHUNK + k] = vv[e] * xb[e]; } }
    __syncthreads();
    TLK_AT(4, 0);
    // the summation order is free here (PCG-internal): several lanes per row
    if (jf < b.r1) {
      const double sA = row_sum_par(lprod, p0 - b.k0, p1 - b.k0, rlane, RL);
      const double sB = row_sum_par(lprod + MAX_CHUNK, p0 - b.k0, p1 - b.k0, rlane, RL);
      if (rlane == 0) row_apply(jf, sA, sB, rf);
    }
    TLK_AT(5, prz);
    for (int j = jf + TB / RL; j < b.r1; j += TB / RL) {
      const int a0 = Mm.rowptr[j] - b.k0, a1 = Mm.rowptr[j + 1] - b.k0;
      const double sA = row_sum_par(lprod, a0, a1, rlane, RL);
      const double sB = row_sum_par(lprod + MAX_CHUNK, a0, a1, rlane, RL);
      if (rlane == 0) row_start(j, sA, sB);
    }
    __syncthreads();
  }
  // ... the blocks beyond the grid (with dense blocks of P: all stream blocks) in the plain form
  for (int bi = DENSE ? blockIdx.x : blockIdx.x + gridDim.x; bi < Mm.nstream; bi += gridDim.x) {
    const RowBlk bb = Mm.blk[bi];
    stage_products<2>(Mm, bb, c.vx, c.vb, lprod, lprod + MAX_CHUNK);
    __syncthreads();
    const int RLb = lanes_for(bb.r1 - bb.r0), rgb = threadIdx.x / RLb, rlb = threadIdx.x % RLb;
    for (int j = bb.r0 + rgb; j < bb.r1; j += TB / RLb) {
      const int a0 = Mm.rowptr[j] - bb.k0, a1 = Mm.rowptr[j + 1] - bb.k0;
      const double sA = row_sum_par(lprod, a0, a1, rlb, RLb);
      const double sB = row_sum_par(lprod + MAX_CHUNK, a0, a1, rlb, RLb);
      if (rlb == 0) row_start(j, sA, sB);
    }
    __syncthreads();
  }
  // long rows: one wavefront each, both products in one pass over the row (two whole-workgroup reductions per row made this
  // kernel 44 us on the Lasso)
  for (int bi = Mm.nstream + blockIdx.x * (TB / 64) + (threadIdx.x >> 6); bi < Mm.nblk; bi += gridDim.x * (TB / 64)) {
    const RowBlk lb = Mm.blk[bi];
    const int lane = threadIdx.x & 63;
    if (c.vd) {              // r_j = base - sigma x~0_j + (M (vb - vx))_j: one gather per entry
      const double acc = wave_row_dot(Mm, lb.k0, lb.k1, [&](int cc) { return c.vd[cc]; });
      if (lane == 0) row_start(lb.r0, -acc, 0.0);
      continue;
    }
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    const bool narrow = Mm.col16 != nullptr;
    constexpr int UI = 8;
    for (int k0 = lb.k0 + lane; k0 - lane < lb.k1; k0 += 64 * UI) {
      int cc[UI]; double vv[UI], xa[UI], xb[UI];
#pragma unroll
      for (int q = 0; q < UI; ++q) {
        const int kc = min(k0 + 64 * q, lb.k1 - 1);
        cc[q] = narrow ? (int)Mm.col16[kc] : Mm.col[kc];
        vv[q] = Mm.val[kc];
      }
#pragma unroll
      for (int q = 0; q < UI; ++q) { xa[q] = c.vx[cc[q]]; xb[q] = c.vb[cc[q]]; }
#pragma unroll
      for (int q = 0; q < UI; ++q) if (k0 + 64 * q >= lb.k1) vv[q] = 0.0;
#pragma unroll
      for (int q = 0; q < UI; q += 2) { a0 += vv[q] * xa[q]; b0 += vv[q] * xb[q]; a1 += vv[q + 1] * xa[q + 1]; b1 += vv[q + 1] * xb[q + 1]; }
    }
    const double sA = wave_sum(a0 + a1), sB = wave_sum(b0 + b1);
    if (lane == 0) row_start(lb.r0, sA, sB);
  }
  block_sum3(prz, prr, pbb, red);
  TLK_AT(6, prz);
  if (threadIdx.x == 0) {
    c.part_rz[blockIdx.x] = prz; c.part_rr[blockIdx.x] = prr; c.part_bb[blockIdx.x] = pbb;
    if (blockIdx.x == 0) {
      st->run = 1; st->done = 0; st->neg_curv = 0; st->iters[0] = 0; st->iters[1] = 0;
      if (s_hist < (1 << 20)) st->hist_r = s_hist + 1;
    }
  }
  TLK_LAST(1);
  TLK_FLUSH(c, 100, 7);
}

// ---------------------------------------------------------------------------
// Chronopoulos-Gear PCG: two kernels per iteration instead of three.
//   u = Minv r, w = K u, gamma = (r,u), delta = (w,u)
//   beta = gamma/gamma_old, alpha = gamma / (delta - beta*gamma/alpha_old)
//   p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s
// k_cg_A does the vector update for its own slice AND t = rho.(A u_new), with
// u_new recomputed from (r_old, w, s_old, Minv) at every gathered column (same
// expression, hence the same bits, as the value the owner stores); r and s are
// ping-ponged on the parity of `it` so gathers never see half-updated data.
// k_cg_B applies w = [P|A'][u;t] + sigma u and emits the three dot partials.
// flags: bit2 = benchmark, bit3 = "pre" pass (pure operator apply on u0, first convergence test),
//        bit4 / bit5 = vector update only / operator apply only (split mode)
// ---------------------------------------------------------------------------
#define EPT (MAX_CHUNK / TB)

// Scalars of one Chronopoulos-Gear step from the three reduced dot products.
struct CgStep { double alpha, beta; bool first, stop, conv, bad; };
__device__ __forceinline__ CgStep cg_step(double rr, double gam, double del, double gam_old, double alp_old,
                                          double tol2, int iters_prev, int neg, const Params &prm, bool bench) {
  CgStep s;
  s.first = gam_old == 0.0;              // the pre pass zeroes gam[1]: first update of this solve
  s.bad = false;
  if (s.first) { s.beta = 0.0; s.alpha = gam / del; }
  else {
    s.beta = gam / gam_old;
    const double den = del - s.beta * gam / alp_old;     // = p'Kp in exact arithmetic
    if (!(den > 0.0) && del > 0.0) {
      // u'Ku > 0 but the two-term recurrence lost positivity.  Near the stop (||r|| within 1e4 of the
      // tolerance) this is the rounding floor of an ill-conditioned system: restart the directions
      // from u (p = u, s = w).  Anywhere else -- and always during the setup-time convexity probe --
      // it is what an indefinite K produces, and is reported as negative curvature.
      if (!prm.no_restart && rr <= 1e8 * tol2) { s.first = true; s.beta = 0.0; s.alpha = gam / del; }
      else { s.alpha = gam / den; s.bad = true; }
    } else s.alpha = gam / den;
  }
  if (bench) { s.beta = 0.5; s.alpha = 1e-3; s.bad = false; }
  s.conv = rr <= tol2;
  s.bad = s.bad || !(s.alpha > 0.0) || !(del > 0.0);      // breakdown / negative curvature
  s.stop = !bench && (s.conv || iters_prev >= prm.pcg_max_iter || neg || s.bad);
  return s;
}
__global__ void __launch_bounds__(TB) k_cg_A(Ctx c, int it, int flags) {
  State *st = c.st;
  TL_MARK(c, 2);
  const bool bench = flags & 4, upd_only = flags & 16, apply_only = flags & 32;
  const bool pre = (flags & 8) || apply_only;   // gather u directly (no recompute)
  // An unrolled slot whose turn never comes costs a whole kernel if it prefetches its operands before it
  // looks at the flags (the wave cannot retire before its loads land: 4-6 us instead of 1.4, measured with
  // `make TIMELINE=1`).  Slots at or beyond the PREVIOUS solve's iteration count (left in the state by
  // k_admm_finalize, same cache line as the flags) therefore look first; so does a graph that continues a
  // stalled solve.  The count moves by about one between consecutive ADMM iterations.  Looking first costs a
  // dependent load before anything else is issued, so slots below the smallest count of the last window
  // (baked into the graph node: flags >> 8) skip it.
  if (!bench && it >= (flags >> 8) && (it >= st->iters_last || st->stalled) && (!st->run || st->done)) return;
  // ---- issue every independent load before looking at the flags ----
  const int stalled = st->stalled, run = st->run, done = st->done, neg = st->neg_curv;
  const int iters_prev = st->iters[(it + 1) & 1];
  const double tol2_old = st->tol2, gam_old = st->gam[(it + 1) & 1], alp_old = st->alp[(it + 1) & 1];
  const Params prm = *c.prm;
  const bool has_blk = (int)blockIdx.x < c.A.nstream;
  RowBlk b = {0, 0, 0, 0};
  if (has_blk) b = c.A.blk[blockIdx.x];
  const int cnt = b.k1 - b.k0;
  const bool small = has_blk;
  const G4 *gold = c.g4 + (size_t)((it + 1) & 1) * c.n;
  G4 *gnew = c.g4 + (size_t)(it & 1) * c.n;
  int ecol[EPT]; double eval[EPT], g0[EPT], g1[EPT], g2[EPT], g3[EPT];
  int RL = lanes_for(b.r1 - b.r0);
  int rg = threadIdx.x / RL, rlane = threadIdx.x % RL;
  int rp0 = 0, rp1 = 0;
  double prho = 0.0;                   // rho of this lane group's first row
  if (small) {
    if (b.r0 + rg < b.r1) { rp0 = c.A.rowptr[b.r0 + rg]; rp1 = c.A.rowptr[b.r0 + rg + 1]; prho = c.rhoe[b.r0 + rg]; }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int k = threadIdx.x + e * TB;
      if (k < cnt) { ecol[e] = c.A.col[b.k0 + k]; eval[e] = c.A.val[b.k0 + k]; }
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int k = threadIdx.x + e * TB;
      if (k < cnt) {
        const int cc = ecol[e];
        if (pre) g0[e] = c.ut[cc];
        else { const G4 g = gold[cc]; g0[e] = g.r; g1[e] = g.w; g2[e] = g.s; g3[e] = g.m; }
      }
    }
  }
  // dot-product partials of the previous kernel (pre: rr, bb ; else: rr, gamma, delta)
  double q0 = 0, q1 = 0, q2 = 0;
  if (!apply_only) {
    const double *a1 = pre ? c.part_bb : c.part_gam;
    for (int i = threadIdx.x; i < c.gridM; i += TB) { q0 += c.part_rr[i]; q1 += a1[i]; if (!pre) q2 += c.part_del[i]; }
  }
  const int j0 = blockIdx.x * TB + threadIdx.x;
  double o_u = 0, o_w = 0, o_p = 0, o_s = 0, o_r = 0, o_x = 0, o_m = 0;
  if (!pre && j0 < c.n) {
    const G4 g = gold[j0];
    o_u = c.ut[j0]; o_w = g.w; o_p = c.pdir[j0]; o_s = g.s; o_r = g.r; o_x = gam_old == 0.0 ? c.vx[j0] : c.va[j0]; o_m = g.m;
  }
  if (!bench && (!run || done || ((flags & 8) && stalled))) return;   // pre pass: skipped when this graph continues a solve
  LDS_DECL(1);
  double sums[3];
  bool first = false;
  double alpha = 0.0, beta = 0.0, tol2 = tol2_old;
  sums[0] = q0; sums[1] = q1; sums[2] = q2;
  if (!apply_only) block_sum3(sums[0], sums[1], sums[2], red);
  if (apply_only) {
    // second half of a split iteration: the update kernel before this one did the scalars
  } else if (pre) {
    tol2 = fmax(prm.eps_rel * prm.eps_rel * sums[1], prm.eps_abs * prm.eps_abs);
    if (!bench && sums[0] <= tol2) {
      if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->tol2 = tol2; }
      return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->tol2 = tol2; st->gam[1] = 0.0; st->alp[1] = 0.0; }
  } else {
    const double gam = sums[1];
    const bool fresh = gam_old == 0.0;
    const CgStep cs = cg_step(sums[0], gam, sums[2], gam_old, alp_old, tol2, iters_prev, neg, prm, bench);
    first = cs.first; alpha = cs.alpha; beta = cs.beta;
    if (cs.stop) {
      if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = cs.conv ? 1 : 2; if (cs.bad && !cs.conv) st->neg_curv = 1; }
      return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st->gam[it & 1] = gam; st->alp[it & 1] = alpha; st->iters[it & 1] = iters_prev + 1;
    }
    // own slice: p, s, x, r, u (first element per thread was prefetched above)
    for (int j = j0; j < c.n; j += gridDim.x * TB) {
      double uj, wj, po, so, ro, xo, mi;
      if (j == j0) { uj = o_u; wj = o_w; po = o_p; so = o_s; ro = o_r; xo = o_x; mi = o_m; }
      else { const G4 g = gold[j]; uj = c.ut[j]; wj = g.w; po = c.pdir[j]; so = g.s; ro = g.r; xo = fresh ? c.vx[j] : c.va[j]; mi = g.m; }
      const double pj = first ? uj : (uj + beta * po);
      const double sj = first ? wj : (wj + beta * so);
      const double rj = ro - alpha * sj;
      c.pdir[j] = pj; gnew[j].s = sj; gnew[j].r = rj;
      c.va[j] = xo + alpha * pj;
      c.ut[j] = mi * rj;
    }
  }
  if (upd_only) return;
  // ---- t = rho . (A u_new) ----
  double *t = c.ut + c.n;
  for (int bi = blockIdx.x; bi < c.A.nstream; bi += gridDim.x) {
    if (bi != (int)blockIdx.x) { b = c.A.blk[bi]; RL = lanes_for(b.r1 - b.r0); rg = threadIdx.x / RL; rlane = threadIdx.x % RL; }
    const int cn = b.k1 - b.k0;
    if (bi != (int)blockIdx.x) {
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const int k = threadIdx.x + e * TB;
        if (k < cn) { ecol[e] = c.A.col[b.k0 + k]; eval[e] = c.A.val[b.k0 + k]; }
      }
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const int k = threadIdx.x + e * TB;
        if (k < cn) {
          const int cc = ecol[e];
          if (pre) g0[e] = c.ut[cc];
          else { const G4 g = gold[cc]; g0[e] = g.r; g1[e] = g.w; g2[e] = g.s; g3[e] = g.m; }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int k = threadIdx.x + e * TB;
      if (k < cn) {
        double uv;
        if (pre) uv = g0[e];
        else {
          const double sj = first ? g1[e] : (g1[e] + beta * g2[e]);
          uv = g3[e] * (g0[e] - alpha * sj);
        }
        lprod[k] = eval[e] * uv;
      }
    }
    __syncthreads();
    for (int i = b.r0 + rg; i < b.r1; i += TB / RL) {
      int a0, a1;
      if (bi == (int)blockIdx.x && i == b.r0 + rg) { a0 = rp0; a1 = rp1; }
      else { a0 = c.A.rowptr[i]; a1 = c.A.rowptr[i + 1]; }
      const double acc = row_sum_par(lprod, a0 - b.k0, a1 - b.k0, rlane, RL);
      if (rlane == 0) t[i] = ((bi == (int)blockIdx.x && i == b.r0 + rg) ? prho : c.rhoe[i]) * acc;
    }
    __syncthreads();
  }
  // long rows: one wavefront each
  for (int bi = c.A.nstream + blockIdx.x * (TB / 64) + (threadIdx.x >> 6); bi < c.A.nwave; bi += gridDim.x * (TB / 64)) {
    const RowBlk lb = c.A.blk[bi];
    double acc;
    if (pre) acc = wave_row_dot(c.A, lb.k0, lb.k1, [&](int cc) { return c.ut[cc]; });
    else acc = wave_row_dot(c.A, lb.k0, lb.k1, [&](int cc) {
      const G4 g = gold[cc];
      const double sj = first ? g.w : (g.w + beta * g.s);
      return g.m * (g.r - alpha * sj);
    });
    if ((threadIdx.x & 63) == 0) t[lb.r0] = c.rhoe[lb.r0] * acc;
  }
  // huge rows (a budget constraint over every variable, ...): every workgroup takes a
  // strided slice and leaves one partial; k_huge_reduce adds them in a fixed order
  for (int bi = c.A.nwave; bi < c.A.nblk; ++bi) {
    const RowBlk hb = c.A.blk[bi];
    double s0 = 0.0, s1 = 0.0;
    int k = hb.k0 + blockIdx.x * TB + threadIdx.x;
    const int stride = gridDim.x * TB;
    auto xv = [&](int cc) -> double {
      if (pre) return c.ut[cc];
      const G4 g = gold[cc];
      const double sj = first ? g.w : (g.w + beta * g.s);
      return g.m * (g.r - alpha * sj);
    };
    for (; k + stride < hb.k1; k += 2 * stride) {
      const int c0 = c.A.col[k], c1 = c.A.col[k + stride];
      const double v0 = c.A.val[k], v1 = c.A.val[k + stride];
      s0 += v0 * xv(c0); s1 += v1 * xv(c1);
    }
    if (k < hb.k1) s0 += c.A.val[k] * xv(c.A.col[k]);
    const double tot = block_sum(s0 + s1, red);
    if (threadIdx.x == 0) c.part_h[(size_t)(bi - c.A.nwave) * gridDim.x + blockIdx.x] = tot;
  }
}

// t_i = rho_i * (sum of the k_cg_A partials) for the huge rows of A; one workgroup per row.
__global__ void __launch_bounds__(TB) k_huge_reduce(Ctx c, int flags) {
  const State *st = c.st;
  if (!(flags & 4) && (!st->run || st->done)) return;
  __shared__ double red[16];
  const int row = c.A.blk[c.A.nwave + blockIdx.x].r0;
  const double *part = c.part_h + (size_t)blockIdx.x * c.gridA;
  double s = 0.0;
  for (int i = threadIdx.x; i < c.gridA; i += TB) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) c.ut[c.n + row] = c.rhoe[row] * s;
}

// DENSE: P has dense diagonal blocks (their column walk keeps 64 loads per lane in flight and
// needs ~190 registers; the plain instantiation stays lean for the sparse stream path).
template <bool DENSE, bool FOLD>
__global__ void __launch_bounds__(TB) k_cg_B(Ctx c, int it, int flags) {
  State *st = c.st;
  TL_MARK(c, 3);
  const bool bench = flags & 4;
  if (!bench && it >= (flags >> 8) && (it >= st->iters_last || st->stalled) && (!st->run || st->done)) return;     // see k_cg_A
  const int run = st->run, done = st->done, skip_pre = it < 0 && st->stalled;
  const double sigma = c.prm->sigma;
  const bool has_blk = (int)blockIdx.x < c.Mk.nstream;
  RowBlk b = {0, 0, 0, 0};
  if (has_blk) b = c.Mk.blk[blockIdx.x];
  const int cnt = b.k1 - b.k0;
  const bool small = has_blk;
  double ev[EPT];
  int RL = lanes_for(b.r1 - b.r0);
  int rg = threadIdx.x / RL, rlane = threadIdx.x % RL;
  int rp0 = 0, rp1 = 0;
  G4 *gc = c.g4 + (size_t)(it & 1) * c.n;
  double pu = 0.0, pr = 0.0;           // u_j, r_j of this lane group's first row (off the tail's critical path)
  // huge rows of A folded in: this thread's share of the k_cg_A partials of each (summed below), and the
  // entries hcol_k[j] of this lane group's first row
  double hs[MAX_HUGE_FOLD], ph[MAX_HUGE_FOLD], hrho[MAX_HUGE_FOLD];
#pragma unroll
  for (int k = 0; k < MAX_HUGE_FOLD; ++k) {
    hs[k] = 0.0; ph[k] = 0.0; hrho[k] = 0.0;
    if (FOLD && k < c.nh) {
      hrho[k] = c.rhoe[c.hrow[k]];
      for (int i = threadIdx.x; i < c.gridA; i += TB) hs[k] += c.part_h[(size_t)k * c.gridA + i];
    }
  }
  if (small) {
    if (b.r0 + rg < b.r1) {
      rp0 = c.Mk.rowptr[b.r0 + rg]; rp1 = c.Mk.rowptr[b.r0 + rg + 1];
      pu = c.ut[b.r0 + rg]; pr = gc[b.r0 + rg].r;
#pragma unroll
      for (int k = 0; k < MAX_HUGE_FOLD; ++k) if (FOLD && k < c.nh) ph[k] = c.hcol[(size_t)k * c.n + b.r0 + rg];
    }
    int ecol[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int k = threadIdx.x + e * TB;
      if (k < cnt) { ecol[e] = c.Mk.col[b.k0 + k]; ev[e] = c.Mk.val[b.k0 + k]; }
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int k = threadIdx.x + e * TB;
      if (k < cnt) ev[e] = ev[e] * c.ut[ecol[e]];
    }
  }
  if (!bench && (!run || done || skip_pre)) return;
  LDS_DECL(1);
  double th[MAX_HUGE_FOLD];            // t_h = rho_h * (A u)_h of the folded huge rows, formed by every workgroup itself
#pragma unroll
  for (int k = 0; k < MAX_HUGE_FOLD; ++k) th[k] = (FOLD && k < c.nh) ? hrho[k] * block_sum(hs[k], red) : 0.0;
  auto hterm = [&](int j, bool pref) {
    double s = 0.0;
    if (FOLD) {
#pragma unroll
      for (int k = 0; k < MAX_HUGE_FOLD; ++k) if (k < c.nh) s += (pref ? ph[k] : c.hcol[(size_t)k * c.n + j]) * th[k];
    }
    return s;
  };
  double pg = 0, pd = 0, prr = 0;
  for (int bi = blockIdx.x; bi < c.Mk.nstream; bi += gridDim.x) {
    if (bi != (int)blockIdx.x) { b = c.Mk.blk[bi]; RL = lanes_for(b.r1 - b.r0); rg = threadIdx.x / RL; rlane = threadIdx.x % RL; }
    const int cn = b.k1 - b.k0;
    if (bi == (int)blockIdx.x) {
#pragma unroll
      for (int e = 0; e < EPT; ++e) { const int k = threadIdx.x + e * TB; if (k < cn) lprod[k] = ev[e]; }
    } else stage_products<1>(c.Mk, b, c.ut, nullptr, lprod, nullptr);
    __syncthreads();
    for (int j = b.r0 + rg; j < b.r1; j += TB / RL) {
      int a0, a1;
      if (bi == (int)blockIdx.x && j == b.r0 + rg) { a0 = rp0; a1 = rp1; }
      else { a0 = c.Mk.rowptr[j]; a1 = c.Mk.rowptr[j + 1]; }
      const double acc = row_sum_par(lprod, a0 - b.k0, a1 - b.k0, rlane, RL);
      if (rlane == 0) {
        const bool first = bi == (int)blockIdx.x && j == b.r0 + rg;
        const double uj = first ? pu : c.ut[j], rj = first ? pr : gc[j].r;
        const double wj = (c.nelim && c.erow[j] >= 0) ? 0.0 : (acc + sigma * uj) + hterm(j, first);
        gc[j].w = wj;
        pg += rj * uj; pd += wj * uj; prr += rj * rj;
      }
    }
    __syncthreads();
  }
  // long rows: one wavefront each
  for (int bi = c.Mk.nstream + blockIdx.x * (TB / 64) + (threadIdx.x >> 6); bi < c.Mk.nblk; bi += gridDim.x * (TB / 64)) {
    const RowBlk lb = c.Mk.blk[bi];
    const double acc = wave_row_dot(c.Mk, lb.k0, lb.k1, [&](int cc) { return c.ut[cc]; });
    if ((threadIdx.x & 63) == 0) {
      const int j = lb.r0;
      const double uj = c.ut[j], wj = (acc + sigma * uj) + hterm(j, false), rj = gc[j].r;
      gc[j].w = wj; pg += rj * uj; pd += wj * uj; prr += rj * rj;
    }
  }
  // dense diagonal blocks of P, one workgroup per block
  if (DENSE)
  for (int db = blockIdx.x; db < c.dP.nblk; db += gridDim.x) {
    const DenseBlk d = c.dP.blk[db];
    double acc = dense_block_mv(c.dP, d, c.ut, lprod);
    if ((int)threadIdx.x < d.b) {
      const int jrow = d.c0 + threadIdx.x;
      for (int k = c.Mk.rowptr[jrow]; k < c.Mk.rowptr[jrow + 1]; ++k) acc += c.Mk.val[k] * c.ut[c.Mk.col[k]];   // A' part
      const double uj = lprod[4 * DENSE_MAX + threadIdx.x], wj = (acc + sigma * uj) + hterm(jrow, false), rj = gc[jrow].r;
      gc[jrow].w = wj; pg += rj * uj; pd += wj * uj; prr += rj * rj;
    }
    __syncthreads();
  }
  block_sum3(pg, pd, prr, red);
  if (threadIdx.x == 0) { c.part_gam[blockIdx.x] = pg; c.part_del[blockIdx.x] = pd; c.part_rr[blockIdx.x] = prr; }
}


// Slices of A_i . x for the huge rows of A (every workgroup one strided slice, one partial
// each); the consumer adds the partials in a fixed order.  Launched only when A has huge rows.
__global__ void __launch_bounds__(TB) k_huge_dot(Ctx c, const double *x, int always) {
  if (!always && !c.st->run) return;
  if (!x) {   // x~ as k_admm_finalize will see it (the start vector when no PCG update ran)
    const State *st = c.st;
    x = (c.vx != c.va && st->iters[0] == 0 && st->iters[1] == 0) ? c.vx : c.va;
  }
  __shared__ double red[16];
  for (int bi = c.A.nwave; bi < c.A.nblk; ++bi) {
    const RowBlk hb = c.A.blk[bi];
    double s0 = 0.0, s1 = 0.0;
    int k = hb.k0 + blockIdx.x * TB + threadIdx.x;
    const int stride = gridDim.x * TB;
    for (; k + stride < hb.k1; k += 2 * stride) {
      const int c0 = c.A.col[k], c1 = c.A.col[k + stride];
      s0 += c.A.val[k] * x[c0]; s1 += c.A.val[k + stride] * x[c1];
    }
    if (k < hb.k1) s0 += c.A.val[k] * x[c.A.col[k]];
    const double tot = block_sum(s0 + s1, red);
    if (threadIdx.x == 0) c.part_h[(size_t)(bi - c.A.nwave) * gridDim.x + blockIdx.x] = tot;
  }
}
__device__ __forceinline__ double huge_row_sum(const Ctx &c, int bi, double *red) {
  const double *part = c.part_h + (size_t)(bi - c.A.nwave) * c.gridA;
  double s = 0.0;
  for (int i = threadIdx.x; i < c.gridA; i += TB) s += part[i];
  return block_sum(s, red);
}

// what the next right-hand side carries for row i: rho z - y, minus rho a b_y / D_y where the row has an eliminated variable y
__device__ __forceinline__ double elim_vb(const Ctx &c, const Params &prm, int i, double rho, double vbn, double x_y) {
  const int y = c.ecol[i];
  if (y < 0) return vbn;
  const double a = c.ecoef[i];
  const double by = (prm.use_cvec ? c.cvec[y] : (prm.sigma * x_y - c.q[y])) + a * vbn;
  return vbn - rho * a * by * c.edinv[i];
}

// Last kernel of an ADMM iteration: z~ = A x~, then update_x / update_z (+project)
// / update_y (auxil.c:185-225, proj.c:4-14) and the m-parts of the next
// right-hand side.  If the PCG has not converged within the unrolled
// iterations the iteration is left untouched and `stalled` is raised.
__global__ void __launch_bounds__(TB) k_admm_finalize(Ctx c) {
  State *st = c.st;
  TL_MARK(c, 4);
  TLK_DECL;
  TLK_AT(0, 0); TLK_LAST(0);
  LDS_DECL(1);
  // A launch starts with cold vector L1 and translation caches, so what this kernel costs at config 2 is not its 2.4 MB but its
  // chain of dependent round trips.  The loads are therefore issued in three flights, each as soon as its addresses are known, and
  // the early returns below gate stores only.  The prefetches are unconditional loads at clamped indices (no branch per load: a
  // use the compiler moves into such a branch would wait there), so they are in bounds in every thread of every workgroup
  // whatever the verdict turns out to be; every array of the engine holds at least one element.
  // Flight A (addresses from blockIdx / threadIdx alone): the state, the parameters, this workgroup's first row block, the
  // partials of ||r||^2 and the first round of the x part (both candidates for x~: the choice needs `iters`).
  const int s_run = st->run, s_fail = st->res_fail, s_done = st->done, s_neg = st->neg_curv, s_hist = st->hist_r;
  const int s_it0 = st->iters[0], s_it1 = st->iters[1];
  const double s_tol2 = st->tol2;
  const long long s_admm = st->admm_done, s_total = st->iters_total;
  const int s_max = st->iters_max, s_min = st->iters_min, s_forced = st->forced, s_negseen = st->neg_curv_seen;
  const Params prm = *c.prm;
  const bool ex = c.vx != c.va;
  const bool have = (int)blockIdx.x < c.A.nstream;
  RowBlk b = c.A.blk[max(min((int)blockIdx.x, c.A.nstream - 1), 0)];
  if (!have) b = RowBlk{0, 0, 0, 0};
  TLK_AT(1, b.k1);
  constexpr int NP = MAX_PARTS / TB;
  double fp[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) fp[k] = c.fin_rr[max(min((int)threadIdx.x + k * TB, c.fin_cnt - 1), 0)];
  double *x = c.xy, *y = c.xy + c.n;
  const int j0 = blockIdx.x * TB + threadIdx.x, jc = max(min(j0, c.n - 1), 0);
  const double xo0 = x[jc], xa0 = c.va[jc], xv0 = c.vx[jc], vo0 = c.vold[jc];
  // what update_z / update_y of one row read besides z~
  struct RowIn { double rho, rinv, yo, zo, lo, up, vo, ea, edi, rhe; int ye; };
  auto row_load = [&](int i) {
    RowIn r;
    r.rho = c.rho[i]; r.rinv = c.rhoinv[i]; r.yo = y[i]; r.zo = c.z[i]; r.lo = c.l[i]; r.up = c.u[i];
    r.vo = c.vold[c.n + i];
    r.ye = -1; r.ea = 0.0; r.edi = 0.0; r.rhe = 0.0;
    if (c.nelim) { r.ye = c.ecol[i]; r.ea = c.ecoef[i]; r.edi = c.edinv[i]; r.rhe = c.rhoe[i]; }
    return r;
  };
  // Flight B (addresses from the block descriptor): the chunk's indices and values, the row pointers of the row this thread
  // helps to sum in the first round, and that row's scalars in the lane that will update it.
  constexpr int E = MAX_CHUNK / TB;
  const int cnt = b.k1 - b.k0;
  int cc[E]; double vv[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int kc = max(min(b.k0 + (int)threadIdx.x + e * TB, b.k1 - 1), 0);
    cc[e] = c.A.col[kc]; vv[e] = c.A.val[kc];
  }
  const int RL = lanes_for(b.r1 - b.r0), rg = threadIdx.x / RL, rlane = threadIdx.x % RL;
  const int i0 = b.r0 + rg, ic = max(min(i0, b.r1 - 1), 0);
  const int p0 = c.A.rowptr[ic], p1 = c.A.rowptr[min(ic + 1, c.A.nrows)];
  const RowIn ri0 = row_load(ic);
  const int er0 = (c.nelim ? c.erow : reinterpret_cast<const int *>(c.rho))[c.nelim ? jc : 0];   // (looked at only where c.nelim; no branch, whose merge would wait)
  TLK_AT(2, fp[NP - 1]);
  if (!s_run || s_fail) return;
  // A solve that ended converged (done == 1: every resident launch that did, every k_cg_A that saw its stop test pass) has its
  // verdict already; only done == 0 (the last unrolled iteration's residual is still in the partials) and done == 2 (a forced
  // stop counts as `forced` only if that residual misses the tolerance) read ||r||^2.  s_done is the same in every thread.
  double rr[1] = {0.0};
  if (s_done != 1) {
    // reduce_parts<1> on the prefetched partials: the same additions in the same order
    double s0 = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) s0 = (int)threadIdx.x + k * TB < c.fin_cnt ? s0 + fp[k] : s0;
    for (int i = threadIdx.x + NP * TB; i < c.fin_cnt; i += TB) s0 += c.fin_rr[i];
    rr[0] = block_sum(s0, red);
  }
  TLK_AT(3, rr[0]);
  const int iters = s_it0 > s_it1 ? s_it0 : s_it1;
  const bool conv = s_done == 1 || rr[0] <= s_tol2;
  const bool force = s_done == 2 || iters >= prm.pcg_max_iter || s_neg;
  if (!conv && !force) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st->stalled = 1;
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->stalled = 0;
    st->admm_done = s_admm + 1;
    st->iters_last = iters;
    st->iters_total = s_total + iters;
    if (iters > s_max) st->iters_max = iters;
    if (iters < s_min) st->iters_min = iters;
    if (!conv) st->forced = s_forced + 1;
    if (s_neg) st->neg_curv_seen = s_negseen + 1;
  }
  const double alpha = prm.alpha, oma = 1.0 - prm.alpha;
  // start vector of the next PCG solve: [x~ | rho z~] + theta * (change since the previous ADMM
  // iteration).  No extrapolation in the first iterations after a reset (the iterates still jump),
  // half a step for a while, then the full linear step.  hist_r is advanced by k_pcg_init only.
  const int hist = s_hist;
  const double th = (hist < prm.ex_h0 ? 0.0 : (hist < prm.ex_h1 ? 0.5 : 1.0)) * prm.ex_theta;
  // the start vector itself passed the stop test (no PCG update ran): x~ is the start vector
  const bool from_start = ex && iters == 0;
  const double *xts = from_start ? c.vx : c.va;
  auto x_update = [&](int j, double xo, double xt, double vo) {
    const double xn = alpha * xt + oma * xo;
    c.dxy[j] = xn - xo;
    x[j] = xn;
    // (from_start: the rows below gather x~ from vx in every workgroup while this one runs, so vx must stay what it is -- the next
    // solve then starts from x~ itself; the iterates have all but stopped moving when a start vector passes the stop test)
    if (ex) { if (!from_start) c.vx[j] = xt + th * (xt - vo); c.vold[j] = xt; }
    if (from_start) c.va[j] = xt;
  };
  // (eliminated from the linear system: its row's thread back-substitutes and updates it below)
  if (j0 < c.n && !(c.nelim && er0 >= 0)) x_update(j0, xo0, from_start ? xv0 : xa0, vo0);
  for (int j = j0 + gridDim.x * TB; j < c.n; j += gridDim.x * TB) {
    if (c.nelim && c.erow[j] >= 0) continue;
    x_update(j, x[j], xts[j], c.vold[j]);
  }
  // update_z / update_y of row i given z~_i = (A x~)_i (without the eliminated variable's term), by one thread
  auto row_apply = [&](int i, double zt, const RowIn &r) {
    const double rho = r.rho, rinv = r.rinv, yo = r.yo, zo = r.zo;
    const int ye = r.ye;
    double rz = rho * zt, xny = 0.0;
    if (ye >= 0) {
      // zt so far is (A_X x~_X)_i: the PCG vector is zero at the eliminated variable.  Back substitution
      // x~_y = (b_y - rho a (A_X x~_X)_i) / D_y with the b_y of the system just solved, then the variable's own update_x.
      const double a = r.ea, xoy = x[ye];
      const double by = (prm.use_cvec ? c.cvec[ye] : (prm.sigma * xoy - c.q[ye])) + a * (rho * zo - yo);
      const double xty = (by - rho * a * zt) * r.edi;
      rz = r.rhe * zt;                         // what the operator of the reduced system applies to this row
      zt += a * xty;
      xny = alpha * xty + oma * xoy;
      c.dxy[ye] = xny - xoy; x[ye] = xny; c.xte[i] = xty;
    }
    double v = alpha * zt + oma * zo + rinv * yo;
    v = fmax(v, r.lo);
    const double zn = fmin(v, r.up);
    const double dy = rho * (alpha * zt + oma * zo - zn);
    const double yn = yo + dy;
    c.z[i] = zn; y[i] = yn; c.dy[i] = dy; c.zt[i] = zt;
    c.va[c.n + i] = rz;
    if (ex) { c.vx[c.n + i] = rz + th * (rz - r.vo); c.vold[c.n + i] = rz; }
    c.vb[c.n + i] = ye >= 0 ? elim_vb(c, prm, i, rho, rho * zn - yn, xny) : rho * zn - yn;
  };
  auto row_update = [&](int i, double zt) { row_apply(i, zt, row_load(i)); };
  // stream blocks (whole rows staged through LDS).  This workgroup's first block -- Flight C: the gathers from the vector the
  // verdict selected; then the row sums, and the first round of rows on what flight B brought
  {
    double xg[E];
    TLK_AT(4, cc[E - 1]);
#pragma unroll
    for (int e = 0; e < E; ++e) xg[e] = xts[cc[e]];      // (beyond the chunk: the clamped entry's column again)
    TLK_AT(5, xg[E - 1]);
#pragma unroll
    for (int e = 0; e < E; ++e) { const int k = threadIdx.x + e * TB; if (k < cnt) lprod[k] = vv[e] * xg[e]; }
    __syncthreads();
    TLK_AT(6, 0);
    if (i0 < b.r1) {
      const double zt = row_sum_par(lprod, p0 - b.k0, p1 - b.k0, rlane, RL);
      if (rlane == 0) row_apply(i0, zt, ri0);
    }
    TLK_AT(7, 0);
    for (int i = i0 + TB / RL; i < b.r1; i += TB / RL) {
      const double zt = row_sum_par(lprod, c.A.rowptr[i] - b.k0, c.A.rowptr[i + 1] - b.k0, rlane, RL);
      if (rlane == 0) row_update(i, zt);
    }
    __syncthreads();
  }
  // ... and the blocks beyond the grid, in the plain form
  for (int bi = blockIdx.x + gridDim.x; bi < c.A.nstream; bi += gridDim.x) {
    const RowBlk bb = c.A.blk[bi];
    stage_products<1>(c.A, bb, xts, nullptr, lprod, nullptr);
    __syncthreads();
    const int RLb = lanes_for(bb.r1 - bb.r0), rgb = threadIdx.x / RLb, rlb = threadIdx.x % RLb;
    for (int i = bb.r0 + rgb; i < bb.r1; i += TB / RLb) {
      const double zt = row_sum_par(lprod, c.A.rowptr[i] - bb.k0, c.A.rowptr[i + 1] - bb.k0, rlb, RLb);
      if (rlb == 0) row_update(i, zt);
    }
    __syncthreads();
  }
  // long rows: the whole workgroup per row.  (One wavefront per row as in the PCG kernels is twice as fast on the Lasso's 10 000 rows
  // -- 2 % of its ADMM iteration -- but z~ then differs in its last bits, and a solve at the floor of attainable accuracy
  // (test_tight_tolerance_on_ill_conditioned_system, eps = 1e-9 on a cond 1e6 system) moved from 225 to 325 iterations: not worth it.)
  if (c.fin_wave_rows) {
    // dense-direct engines (dense_direct.h): one wavefront per long row with the PCG kernels' row dot -- there this pass is
    // 40 % of an ADMM iteration (72 -> 2x us at the Lasso's 10 000 rows), and the linear solves no longer stop on a residual
    // that the last bits of z~ could move
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int bi = c.A.nstream + blockIdx.x * (TB / 64) + wv; bi < c.A.nwave; bi += gridDim.x * (TB / 64)) {
      const RowBlk lb = c.A.blk[bi];
      const double zt = wave_row_dot(c.A, lb.k0, lb.k1, [&](int cc) { return xts[cc]; });
      if (lane == 0) row_update(lb.r0, zt);
    }
  } else
  for (int bi = c.A.nstream + blockIdx.x; bi < c.A.nwave; bi += gridDim.x) {
    const RowBlk lb = c.A.blk[bi];
    const double zt = long_row_dot(c.A, lb.k0, lb.k1, xts, red);
    if (threadIdx.x == 0) row_update(lb.r0, zt);
    __syncthreads();
  }
  // huge rows: partials left by k_huge_dot
  for (int bi = c.A.nwave + blockIdx.x; bi < c.A.nblk; bi += gridDim.x) {
    const double zt = huge_row_sum(c, bi, red);
    if (threadIdx.x == 0) row_update(c.A.blk[bi].r0, zt);
    __syncthreads();
  }
  TLK_AT(8, 0); TLK_LAST(1);
  TLK_FLUSH(c, 110, 9);
}
