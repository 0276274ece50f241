// batch_streamed.h -- the streamed-inverse batch engine (OSQP_AMD_BATCH_STREAMED), included by batch.hip.
//
// For members of up to 1024 variables, where K^-1 no longer fits a CU's registers: each member's dense K^-1
// (NP x NP row-major, NP = n rounded up to 32, identity padding) lives in HBM and is streamed once per ADMM
// iteration (twice for refined members) as a GEMV with 16-byte loads.  Only the n- and m-vectors of one member
// live in LDS; the shared pattern is read from global memory (L2 resident) and the member's scaled P and A
// values from its slab io.Wv.  Four kernels, each one launch over the batch:
//   k_bs_setup   one workgroup per member: Ruiz scaling, row classes, workspace (batch.hip phase 0);
//   k_bs_form    grid (NP rows, members): K = P + sigma I + A' diag(rho) A, dense, from a host-built list of
//                (A slot, A slot, row) triples per entry of triu(K): a fixed summation order, no atomics;
//   k_bs_invert  one workgroup per member: Gauss-Jordan in place in HBM without pivoting (K is SPD); a
//                non-positive pivot flags the member (bit 8 of io.flag);
//   k_bs_loop    one workgroup per member: the ADMM loop of k_batch_solve.  A member whose rho moves saves its
//                scaled x, z, y, iteration count and rho and leaves with a rebuild request; the host re-forms and
//                re-inverts those members and relaunches the loop over them (osqp_amd_batch_solve).
// form and invert only touch members whose io.flag has bit 1 set (a rebuild is due), so a launch over the
// whole batch costs nothing for the others.

#define BS_MAX_N 1024      // largest n (k_bs_form's and k_bs_invert's row buffers)
#define BS_MAX_TRIPLES (1 << 26)   // A'A row products of the K pattern (4 bytes x 3 each)
#define BS_NT 512          // loop / setup workgroup: 8 wavefronts
#define BS_NTI 1024        // inversion workgroup: a 32 x 32 grid of entry owners

struct BSPattern {         // K's pattern for the formation kernel (device pointers)
  const int *Ep;           // [nent + 1] triple ranges of the entries of triu(K)
  const int *Eslot;        // [nent] triu(P) slot of the entry, -1 if none
  const int *Ta, *Tb, *Tr; // triples: A slot in column min(i, j), A slot in column max(i, j), row
  const int *Rp, *Rj, *Re; // per row i of K: column j and triu entry of every stored entry (i, j) and (j, i)
};

__device__ __forceinline__ double bs_rho_of(int t, double rho) { return t == -1 ? 1e-6 : (t == 1 ? 1e3 * rho : rho); }

// out_i = sum_j Kinv_ij in_j for i < n.  Sixteen lanes (one DPP row) per row of K^-1, 16-byte loads:
// one load instruction of the sixteen reads 256 contiguous bytes.  in: LDS, zero in [n, NP).
__device__ __forceinline__ void bs_gemv(const double *__restrict__ Kinv, int NP, int n, const double *in, double *out) {
  const int team = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int nc = NP >> 1;                  // double2 per row, a multiple of 16
  for (int i = team; i < n; i += BS_NT / 16) {
    const double2 *row = reinterpret_cast<const double2 *>(Kinv + (long long)i * NP);
    double acc = 0.0;
#pragma unroll 4
    for (int c = l; c < nc; c += 16) {
      const double2 a = row[c];
      const double2 v = *reinterpret_cast<const double2 *>(in + 2 * c);
      acc = __builtin_fma(a.x, v.x, acc);
      acc = __builtin_fma(a.y, v.y, acc);
    }
    acc += quad_xor1(acc); acc += quad_xor2(acc); acc += dpp_mirror(acc, true); acc += dpp_mirror(acc, false);
    if (l == 0) out[i] = acc;
  }
  __syncthreads();
}

// LDS working set (vectors only): 7 n-vectors of NP, 11 m-vectors, 64 + 256 reduction doubles, m ints.
__host__ __device__ __forceinline__ size_t bs_lds_bytes(int NP, int m) {
  const size_t b = sizeof(double) * (7 * (size_t)NP + 11 * (size_t)m + 64 + 256) + sizeof(int) * (size_t)m;
  return (b + 15) & ~(size_t)15;
}

__device__ __forceinline__ BL bs_layout(double *lds, const BPattern &p, const BIO &io, long long qp, int NP) {
  BL s;
  double *w = lds;
  s.NP = NP; s.m = p.m;
  s.nv = w; w += 7 * NP; s.mv = w; w += 11 * p.m;
  s.red = w; w += 64; s.gp = w; w += 256;
  s.rowk = s.colk = nullptr;
  s.ctype = reinterpret_cast<int *>(w);
  s.Pv = io.Wv + qp * ((long long)p.nnzP + p.nnzA); s.Av = s.Pv + p.nnzP;
  s.Pp = p.Pp; s.Pi = p.Pi; s.Pc = p.Pc; s.Fp = p.Fp; s.Fi = p.Fi; s.Fk = p.Fk;
  s.Ap = p.Ap; s.Ai = p.Ai; s.Ac = p.Ac; s.Rp = p.Rp; s.Rj = p.Rj; s.Rk = p.Rk;
  return s;
}

// ---------------------------------------------------------------------------
// setup: k_batch_solve's phase 0 with the matrix values in the member's HBM slab
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BS_NT) k_bs_setup(BPattern p, BSettings st, BIO io, int NP) {
  constexpr int NT = BS_NT, NW = NT / 64;
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const long long qp = blockIdx.x;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  BL s = bs_layout(lds, p, io, qp, NP);
  double cs = 1.0;
  for (int j = tid; j < NP; j += NT) { s_q[j] = 0.0; s_D[j] = 1.0; s_tn[j] = 0.0; }
  for (int i = tid; i < m; i += NT) s_E[i] = 1.0;
  {
    const double *Pg = io.Px + qp * io.strideP, *Ag = io.Ax + qp * io.strideA;
    for (int k = tid; k < p.nnzP; k += NT) s.Pv[k] = Pg[k];
    for (int k = tid; k < p.nnzA; k += NT) s.Av[k] = Ag[k];
  }
  for (int j = tid; j < n; j += NT) s_q[j] = io.Q[qp * n + j];
  for (int i = tid; i < m; i += NT) { s_l[i] = io.L[qp * m + i]; s_u[i] = io.U[qp * m + i]; }
  // The slab is written and re-read by different lanes of this workgroup: every such hand-off below is a
  // fence (the stores reach L2, stale L1 lines go) and a barrier, as in rebuild_kinv.
  __threadfence();
  __syncthreads();
  double *Pv = s.Pv, *Av = s.Av;
  // ---- Ruiz equilibration (scaling.c:44-156), as in k_batch_solve ----
  for (int pass = 0; pass < st.scaling; ++pass) {
    for (int j = tid; j < n; j += NT) {
      double v = 0.0;
      for (int k = s.Fp[j]; k < s.Fp[j + 1]; ++k) v = fmax(v, fabs(Pv[s.Fk[k]]));
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; ++k) v = fmax(v, fabs(Av[k]));
      s_tn[j] = 1.0 / sqrt(clip_scale(v));
    }
    for (int i = tid; i < m; i += NT) {
      double v = 0.0;
      for (int k = s.Rp[i]; k < s.Rp[i + 1]; ++k) v = fmax(v, fabs(Av[s.Rk[k]]));
      s_tm[i] = 1.0 / sqrt(clip_scale(v));
    }
    __syncthreads();
    for (int k = tid; k < p.nnzP; k += NT) Pv[k] = (Pv[k] * s_tn[s.Pi[k]]) * s_tn[s.Pc[k]];
    for (int k = tid; k < p.nnzA; k += NT) Av[k] = (Av[k] * s_tm[s.Ai[k]]) * s_tn[s.Ac[k]];
    for (int j = tid; j < n; j += NT) { s_q[j] = s_q[j] * s_tn[j]; s_D[j] = s_tn[j] * s_D[j]; }
    for (int i = tid; i < m; i += NT) s_E[i] = s_tm[i] * s_E[i];
    __threadfence();
    __syncthreads();
    double cn = 0.0, qn = 0.0;
    for (int j = tid; j < n; j += NT) {
      double v = 0.0;
      for (int k = s.Fp[j]; k < s.Fp[j + 1]; ++k) v = fmax(v, fabs(Pv[s.Fk[k]]));
      s_tn[j] = v;
      qn = fmax(qn, fabs(s_q[j]));
    }
    qn = b_max<NW>(qn, s.red);
    if (tid == 0) { double acc = 0.0; for (int j = 0; j < n; ++j) acc += s_tn[j]; s.red[12] = acc / (double)n; }
    __syncthreads();
    cn = s.red[12];
    double ct = fmax(cn, clip_scale(qn));
    ct = 1.0 / clip_scale(ct);
    for (int k = tid; k < p.nnzP; k += NT) Pv[k] *= ct;
    for (int j = tid; j < n; j += NT) s_q[j] *= ct;
    cs *= ct;
    __threadfence();
    __syncthreads();
  }
  for (int i = tid; i < m; i += NT) { s_l[i] = s_l[i] * s_E[i]; s_u[i] = s_u[i] * s_E[i]; }
  const double rho = fmin(fmax(st.rho, 1e-6), 1e6);
  for (int i = tid; i < m; i += NT) {         // row classes (auxil.c:76-98)
    int t = 0;
    if (s_l[i] < -BINF && s_u[i] > BINF) t = -1;
    else if (s_u[i] - s_l[i] < st.rho_tol) t = 1;
    io.Wt[qp * m + i] = t;
    io.Wl[qp * m + i] = s_l[i]; io.Wu[qp * m + i] = s_u[i]; io.We[qp * m + i] = s_E[i];
    io.Zs[qp * m + i] = 0.0; io.Ys[qp * m + i] = 0.0;
  }
  for (int j = tid; j < n; j += NT) { io.Wq[qp * n + j] = s_q[j]; io.Wd[qp * n + j] = s_D[j]; io.Xs[qp * n + j] = 0.0; }
  if (tid == 0) { io.Wc[qp] = cs; io.rho_io[qp] = rho; io.flag[qp] = 1; }   // 1: K^-1 is due (k_bs_form, k_bs_invert)
}

// ---------------------------------------------------------------------------
// formation of K: block (i, k) writes row i of member list[k]'s K into its K^-1 slot (identity beyond n)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bs_form(BPattern p, BSPattern kp, BIO io, int NP, double sigma, const int *list) {
  __shared__ __attribute__((aligned(16))) double row[1024];
  const long long qp = list ? list[blockIdx.y] : (int)blockIdx.y;
  if (!(io.flag[qp] & 1)) return;
  const int i = blockIdx.x, n = p.n, m = p.m;
  for (int j = threadIdx.x; j < NP; j += 256) row[j] = j == i ? 1.0 : 0.0;
  __syncthreads();
  if (i < n) {
    const double *Pv = io.Wv + qp * ((long long)p.nnzP + p.nnzA), *Av = Pv + p.nnzP;
    const int *ct = io.Wt + qp * m;
    const double rho = io.rho_io[qp];
    for (int k = kp.Rp[i] + threadIdx.x; k < kp.Rp[i + 1]; k += 256) {
      const int j = kp.Rj[k], e = kp.Re[k];
      double acc = 0.0;
      if (kp.Eslot[e] >= 0) acc += Pv[kp.Eslot[e]];
      if (i == j) acc += sigma;
      for (int t = kp.Ep[e]; t < kp.Ep[e + 1]; ++t) acc += bs_rho_of(ct[kp.Tr[t]], rho) * Av[kp.Ta[t]] * Av[kp.Tb[t]];
      row[j] = acc;
    }
  }
  __syncthreads();
  double *out = io.Wk + qp * (long long)NP * NP + (long long)i * NP;
  for (int j = threadIdx.x; j < NP; j += 256) out[j] = row[j];
}

// ---------------------------------------------------------------------------
// Gauss-Jordan inversion in place in HBM without pivoting (invert_tiles, one pivot per step).  Thread (tr, tc)
// of a 32 x 32 grid owns the entries (i, j) with i = tr mod 32, j = tc mod 32 for all pivots, so each entry is
// only ever read and written by its owner; the owners of row k and column k publish them to LDS (double
// buffered, one barrier per pivot).  Only the n x n block is touched: the padding stays the identity.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BS_NTI) k_bs_invert(int n, BIO io, int NP, const int *list) {
  __shared__ double rowk[2][1024], colk[2][1024];
  const long long qp = list ? list[blockIdx.x] : (int)blockIdx.x;
  const int fl = io.flag[qp];
  if (!(fl & 1)) return;
  double *Ka = io.Wk + qp * (long long)NP * NP;
  const int tr = threadIdx.x >> 5, tc = threadIdx.x & 31;
  bool notpd = false;
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    double *rk = rowk[k & 1], *ck = colk[k & 1];
    if (tr == (k & 31)) for (int j = tc; j < n; j += 32) rk[j] = Ka[(long long)k * NP + j];
    if (tc == (k & 31)) for (int i = tr; i < n; i += 32) ck[i] = Ka[(long long)i * NP + k];
    __syncthreads();
    const double akk = rk[k];
    notpd |= !(akk > 0.0);
    const double piv = 1.0 / akk;
    for (int i = tr; i < n; i += 32) {
      const double ci = ck[i];
      double *Ki = Ka + (long long)i * NP;
      if (i == k) {
        for (int j = tc; j < n; j += 32) Ki[j] = j == k ? piv : rk[j] * piv;
      } else {
        for (int j = tc; j < n; j += 32) Ki[j] = j == k ? 0.0 - ci * piv : __builtin_fma(-ci, rk[j] * piv, Ki[j]);
      }
    }
  }
  __syncthreads();
  // bit 1 (rebuild due) cleared, refinement verdict kept, 4: the verdict is re-taken, 8: K not positive definite
  if (threadIdx.x == 0) io.flag[qp] = (fl & 2) | 4 | (notpd ? 8 : 0);
}

// ---------------------------------------------------------------------------
// the ADMM loop: k_batch_solve's phase 1 with K^-1 streamed from HBM
// ---------------------------------------------------------------------------
// list == nullptr: the first round, over the whole batch (in io.order when set), from the stored iterates
// when warm starting; otherwise a resumed round over list[0..gridDim.x): the members continue from the state
// they saved when their rho moved.  A member whose rho moves before max_iter saves its state, sets
// io.flag = 1 | (refinement verdict) and appends itself to rb_list (rb_count).
__global__ void __launch_bounds__(BS_NT) k_bs_loop(BPattern p, BSettings st, BIO io, int NP, const int *list,
                                                   int *rb_count, int *rb_list) {
  constexpr int NT = BS_NT, NW = NT / 64;
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const bool resume = list != nullptr;
  const long long qp = resume ? list[blockIdx.x] : (io.order ? io.order[blockIdx.x] : (int)blockIdx.x);
  extern __shared__ __attribute__((aligned(16))) double lds[];
  BL s = bs_layout(lds, p, io, qp, NP);
  const double *Wk = io.Wk + qp * (long long)NP * NP;

  for (int j = tid; j < NP; j += NT) {
    s_q[j] = 0.0; s_x[j] = 0.0; s_xt[j] = 0.0; s_dx[j] = 0.0; s_D[j] = 1.0; s_tn[j] = 0.0; s_b[j] = 0.0;
  }
  for (int i = tid; i < m; i += NT) { s_z[i] = 0.0; s_y[i] = 0.0; s_E[i] = 1.0; s_dy[i] = 0.0; s_ws[i] = 0.0; }
  __syncthreads();
  for (int j = tid; j < n; j += NT) { s_q[j] = io.Wq[qp * n + j]; s_D[j] = io.Wd[qp * n + j]; }
  for (int i = tid; i < m; i += NT) {
    s_l[i] = io.Wl[qp * m + i]; s_u[i] = io.Wu[qp * m + i]; s_E[i] = io.We[qp * m + i];
    s.ctype[i] = io.Wt[qp * m + i];
  }
  const double cs = io.Wc[qp];
  const double cinv = 1.0 / cs;
  const bool unscaled = st.scaling && !st.scaled_termination;
  double rho = fmin(fmax(io.rho_io[qp], 1e-6), 1e6);
  for (int i = tid; i < m; i += NT) {
    const double r = bs_rho_of(s.ctype[i], rho);
    s_rho[i] = r; s_rinv[i] = 1.0 / r;
  }
  if (st.warm_start || resume) {
    for (int j = tid; j < n; j += NT) s_x[j] = io.Xs[qp * n + j];
    for (int i = tid; i < m; i += NT) { s_z[i] = io.Zs[qp * m + i]; s_y[i] = io.Ys[qp * m + i]; }
  }
  __syncthreads();
  const int qflag = io.flag[qp];
  bool need_refine = (qflag & 2) != 0, check_pending = (qflag & 4) != 0;

  const double alpha = st.alpha, oma = 1.0 - st.alpha, sigma = st.sigma;
  double *sc = s.red + 13;
  enum { S_PRI, S_DUA, S_OBJ, S_NPRI_S, S_NDUA_S, S_NZ_S, S_NAX_S, S_NQ_S, S_NATY_S, S_NPX_S,
         S_NZ, S_NAX, S_NQ, S_NATY, S_NPX, S_STATUS, S_RHO, S_ND, S_LHS, S_NDX, S_QDX, S_COUNT_ };
  enum { F_NORMS = 1, F_STATUS = 2, F_APPROX = 4 };
  if (tid == 0) { for (int k = 0; k < S_COUNT_; ++k) sc[k] = 0.0; sc[S_STATUS] = OSQP_UNSOLVED; sc[S_RHO] = rho; }
  for (int i = tid; i < m; i += NT) s_w[i] = s_rho[i] * s_z[i] - s_y[i];
  __syncthreads();
  int iter = resume ? (int)io.info[qp * 8] : 0, rho_updates = (int)io.info[qp * 8 + 5], stage = 0, probe_until = 0;
  bool norms_fresh = false, rebuild_due = false;

  while (stage != 3) {
    int flags = 0;
    bool checked = false, adapt_due = false;
    if (stage == 0) {
      ++iter;
      {   // b = sigma x - q + A'(rho z - y), four lanes per column
        const int l = tid & 3;
        for (int j = tid >> 2; j < n; j += NT / 4) {
          const double acc = a_col_dot4(s, s_w, j, l);
          if (l == 0) s_b[j] = (sigma * s_x[j] - s_q[j]) + acc;
        }
        __syncthreads();
      }
      bs_gemv(Wk, NP, n, s_b, s_xt);
      const bool probe = !need_refine && (check_pending || iter <= probe_until);
      if (st.refine && (st.refine == 2 || need_refine || probe)) {
        for (int i = tid; i < m; i += NT) s_ws[i] = s_rho[i] * a_row_dot(s, s_xt, i);
        __syncthreads();
        double rmax = 0.0, bmax = 0.0;
        for (int j = tid; j < NP; j += NT) {
          s_tn[j] = j < n ? s_b[j] - (p_row_dot(s, s_xt, j) + sigma * s_xt[j] + a_col_dot(s, s_ws, j)) : 0.0;
          rmax = fmax(rmax, fabs(s_tn[j])); bmax = fmax(bmax, fabs(s_b[j]));
        }
        if (probe) {
          rmax = b_max<NW>(rmax, s.red); bmax = b_max<NW>(bmax, s.red);
          need_refine = rmax > st.refine_tol * bmax;
          if (check_pending) { check_pending = false; probe_until = iter + 3; }
        }
        __syncthreads();
        bs_gemv(Wk, NP, n, s_tn, s_dx);
        for (int j = tid; j < n; j += NT) s_xt[j] += s_dx[j];
        __syncthreads();
      }
      for (int i = tid >> 1; i < m; i += NT / 2) {
        const double zt = a_row_dot2(s, s_xt, i, tid & 1);
        if ((tid & 1) == 0) {
          const double zo = s_z[i], yo = s_y[i], ri = s_rho[i];
          double v = alpha * zt + oma * zo + s_rinv[i] * yo;
          v = fmax(v, s_l[i]);
          const double zn = fmin(v, s_u[i]);
          const double dy = ri * (alpha * zt + oma * zo - zn);
          const double yn = yo + dy;
          s_z[i] = zn; s_dy[i] = dy; s_y[i] = yn;
          s_w[i] = ri * zn - yn;
        }
      }
      for (int j = tid; j < n; j += NT) {
        const double xo = s_x[j];
        const double xn = alpha * s_xt[j] + oma * xo;
        s_dx[j] = xn - xo; s_x[j] = xn;
      }
      __syncthreads();
      norms_fresh = false;
      checked = st.check_termination && (iter % st.check_termination == 0);
      adapt_due = st.adaptive_rho && st.rho_interval && (iter % st.rho_interval == 0);
      if (checked) flags = F_NORMS | F_STATUS;
      else if (adapt_due) flags = F_NORMS;
    } else if (stage == 1) flags = F_STATUS | (norms_fresh ? 0 : F_NORMS);
    else flags = F_STATUS | F_APPROX;

    bool term = false;
    if (flags & F_NORMS) {
      double mx[16], sm[3];
#pragma unroll
      for (int k = 0; k < 16; ++k) mx[k] = 0.0;
      sm[0] = sm[1] = sm[2] = 0.0;
      for (int i = tid >> 1; i < m; i += NT / 2) {
        const double ax = a_row_dot2(s, s_x, i, tid & 1);
        if ((tid & 1) == 0) {
          const double zi = s_z[i], pr = ax + (-1.0) * zi;
          const double ei = unscaled ? 1.0 / s_E[i] : 1.0;
          mx[0] = fmax(mx[0], fabs(ei * pr)); mx[1] = fmax(mx[1], fabs(pr));
          mx[2] = fmax(mx[2], fabs(ei * zi)); mx[3] = fmax(mx[3], fabs(zi));
          mx[4] = fmax(mx[4], fabs(ei * ax)); mx[5] = fmax(mx[5], fabs(ax));
          double dy = s_dy[i];
          const double li = s_l[i], ui = s_u[i];
          if (ui > BINF) { if (li < -BINF) dy = 0.0; else dy = fmin(dy, 0.0); }
          else if (li < -BINF) dy = fmax(dy, 0.0);
          s_ws[i] = dy;
          mx[14] = fmax(mx[14], fabs(unscaled ? s_E[i] * dy : dy));
          sm[1] += ui * fmax(dy, 0.0) + li * fmin(dy, 0.0);
        }
      }
      {   // columns: four lanes each, strided over the workgroup
        const int l = tid & 3;
        for (int j = tid >> 2; j < n; j += NT / 4) {
          const double px = p_row_dot4(s, s_x, j, l);
          const double aty = a_col_dot4(s, s_y, j, l);
          if (l == 0) {
            const double qj = s_q[j], xj = s_x[j], dxj = s_dx[j];
            double dr = qj + px;
            if (m > 0) dr = dr + aty;
            const double di = unscaled ? 1.0 / s_D[j] : 1.0;
            mx[6] = fmax(mx[6], fabs(di * dr)); mx[7] = fmax(mx[7], fabs(dr));
            mx[8] = fmax(mx[8], fabs(di * qj)); mx[9] = fmax(mx[9], fabs(qj));
            mx[10] = fmax(mx[10], fabs(di * aty)); mx[11] = fmax(mx[11], fabs(aty));
            mx[12] = fmax(mx[12], fabs(di * px)); mx[13] = fmax(mx[13], fabs(px));
            sm[0] += xj * (0.5 * px + qj);
            mx[15] = fmax(mx[15], fabs(unscaled ? s_D[j] * dxj : dxj));
            sm[2] += qj * dxj;
          }
        }
      }
      b_reduce_many<NW, 16, 3>(mx, sm, s.gp);
      if (tid == 0) {
        const double *g = s.gp + NW * 19;
        sc[S_PRI] = m == 0 ? 0.0 : (unscaled ? g[0] : g[1]);
        sc[S_NPRI_S] = g[1]; sc[S_NZ] = unscaled ? g[2] : g[3]; sc[S_NZ_S] = g[3];
        sc[S_NAX] = unscaled ? g[4] : g[5]; sc[S_NAX_S] = g[5];
        const double f = unscaled ? cinv : 1.0;
        sc[S_DUA] = unscaled ? g[6] * cinv : g[7]; sc[S_NDUA_S] = g[7];
        sc[S_NQ] = (unscaled ? g[8] : g[9]) * f; sc[S_NQ_S] = g[9];
        sc[S_NATY] = (unscaled ? g[10] : g[11]) * f; sc[S_NATY_S] = g[11];
        sc[S_NPX] = (unscaled ? g[12] : g[13]) * f; sc[S_NPX_S] = g[13];
        sc[S_OBJ] = g[16] * (st.scaling ? cinv : 1.0);
        sc[S_ND] = g[14]; sc[S_LHS] = g[17]; sc[S_NDX] = g[15]; sc[S_QDX] = g[18];
      }
      __syncthreads();
      norms_fresh = true;
    }
    if (flags & F_STATUS) {
      const bool approximate = flags & F_APPROX;
      const double pri_res = sc[S_PRI], dua_res = sc[S_DUA];
      int newstatus = 0;
      double newobj = 0.0;
      if (pri_res > 1e30 || dua_res > 1e30) { newstatus = OSQP_NON_CVX; newobj = OSQP_NAN; }
      else {
        double ea = st.eps_abs, er = st.eps_rel, epi = st.eps_pinf, edi = st.eps_dinf;
        if (approximate) { ea *= 10; er *= 10; epi *= 10; edi *= 10; }
        bool prim_ok = false, dual_ok = false, pinf = false, dinf = false;
        if (m == 0) prim_ok = true;
        else if (pri_res < ea + er * fmax(sc[S_NZ], sc[S_NAX])) prim_ok = true;
        else {
          const double nd = sc[S_ND], lhs = sc[S_LHS];
          if (nd > 1e-30 && lhs < epi * nd) {
            double mxv = 0;
            for (int j = tid; j < n; j += NT) {
              double v = a_col_dot(s, s_ws, j);
              if (unscaled) v = v / s_D[j];
              mxv = fmax(mxv, fabs(v));
            }
            mxv = b_max<NW>(mxv, s.red);
            pinf = mxv < epi * nd;
          }
        }
        if (dua_res < ea + er * fmax(fmax(sc[S_NQ], sc[S_NATY]), sc[S_NPX])) dual_ok = true;
        else {
          const double ndx = sc[S_NDX], qdx = sc[S_QDX];
          const double csc_ = unscaled ? cs : 1.0;
          if (ndx > 1e-30 && qdx < csc_ * edi * ndx) {
            double mxv = 0;
            for (int j = tid; j < n; j += NT) {
              double v = p_row_dot(s, s_dx, j);
              if (unscaled) v = v / s_D[j];
              mxv = fmax(mxv, fabs(v));
            }
            mxv = b_max<NW>(mxv, s.red);
            if (mxv < csc_ * edi * ndx) {
              double viol = 0;
              for (int i = tid; i < m; i += NT) {
                double v = a_row_dot(s, s_dx, i);
                if (unscaled) v = v / s_E[i];
                if ((s_u[i] < BINF && v > edi * ndx) || (s_l[i] > -BINF && v < -edi * ndx)) viol += 1.0;
              }
              viol = b_sum<NW>(viol, s.red);
              dinf = viol == 0.0;
            }
          }
        }
        if (prim_ok && dual_ok) newstatus = approximate ? OSQP_SOLVED_INACCURATE : OSQP_SOLVED;
        else if (pinf) { newstatus = approximate ? OSQP_PRIMAL_INFEASIBLE_INACCURATE : OSQP_PRIMAL_INFEASIBLE; newobj = OSQP_INFTY; }
        else if (dinf) { newstatus = approximate ? OSQP_DUAL_INFEASIBLE_INACCURATE : OSQP_DUAL_INFEASIBLE; newobj = -OSQP_INFTY; }
      }
      __syncthreads();
      if (newstatus != 0) {
        term = true;
        if (tid == 0) { sc[S_STATUS] = newstatus; if (newstatus != OSQP_SOLVED && newstatus != OSQP_SOLVED_INACCURATE) sc[S_OBJ] = newobj; }
      }
      __syncthreads();
    }
    if (stage == 0) {
      if (checked && term) { stage = 3; continue; }
      if (adapt_due) {     // adapt_rho (auxil.c:13-74)
        const double pr = (m ? sc[S_NPRI_S] : 0.0) / (fmax(sc[S_NZ_S], sc[S_NAX_S]) + 1e-30);
        const double du = sc[S_NDUA_S] / (fmax(fmax(sc[S_NQ_S], sc[S_NATY_S]), sc[S_NPX_S]) + 1e-30);
        const double rn = fmin(fmax(rho * sqrt(pr / du), 1e-6), 1e6);
        if (rn > rho * st.adapt_tol || rn < rho / st.adapt_tol) {
          rho = rn; rho_updates++;
          if (iter < st.max_iter) {
            // K^-1 must be rebuilt before the next iteration: save the state and leave it to the host
            for (int j = tid; j < n; j += NT) io.Xs[qp * n + j] = s_x[j];
            for (int i = tid; i < m; i += NT) { io.Zs[qp * m + i] = s_z[i]; io.Ys[qp * m + i] = s_y[i]; }
            if (tid == 0) {
              io.info[qp * 8] = iter; io.info[qp * 8 + 5] = rho_updates; io.rho_io[qp] = rho;
              io.flag[qp] = 1 | (need_refine ? 2 : 0);
              rb_list[atomicAdd(rb_count, 1)] = (int)qp;
            }
            return;
          }
          // at max_iter no further solve with K follows: finish, rebuild after the loop (the host's last pass)
          for (int i = tid; i < m; i += NT) {
            const int t = s.ctype[i];
            if (t == 0) { s_rho[i] = rho; s_rinv[i] = 1.0 / rho; }
            else if (t == 1) { s_rho[i] = 1e3 * rho; s_rinv[i] = 1.0 / s_rho[i]; }
            s_w[i] = s_rho[i] * s_z[i] - s_y[i];
          }
          __syncthreads();
          rebuild_due = true;
        }
      }
      if (iter >= st.max_iter) stage = checked ? 2 : 1;
    } else if (stage == 1) stage = term ? 3 : 2;
    else {
      if (!term && tid == 0) sc[S_STATUS] = OSQP_MAX_ITER_REACHED;
      __syncthreads();
      stage = 3;
    }
  }
  const int status = (int)sc[S_STATUS];
  const double pri_res = sc[S_PRI], dua_res = sc[S_DUA], obj = sc[S_OBJ];
  double rho_est;
  {
    const double pr = (m ? sc[S_NPRI_S] : 0.0) / (fmax(sc[S_NZ_S], sc[S_NAX_S]) + 1e-30);
    const double du = sc[S_NDUA_S] / (fmax(fmax(sc[S_NQ_S], sc[S_NATY_S]), sc[S_NPX_S]) + 1e-30);
    rho_est = fmin(fmax(rho * sqrt(pr / du), 1e-6), 1e6);
  }
  // ---- store_solution (auxil.c:524-562) ----
  const bool has_sol = !(status == OSQP_PRIMAL_INFEASIBLE || status == OSQP_PRIMAL_INFEASIBLE_INACCURATE ||
                         status == OSQP_DUAL_INFEASIBLE || status == OSQP_DUAL_INFEASIBLE_INACCURATE ||
                         status == OSQP_NON_CVX);
  __syncthreads();
  if (has_sol) {
    for (int j = tid; j < n; j += NT) {
      io.Xo[qp * n + j] = st.scaling ? s_x[j] * s_D[j] : s_x[j];
      io.Xs[qp * n + j] = s_x[j];
    }
    for (int i = tid; i < m; i += NT) {
      io.Yo[qp * m + i] = st.scaling ? (s_y[i] * s_E[i]) * cinv : s_y[i];
      io.Ys[qp * m + i] = s_y[i]; io.Zs[qp * m + i] = s_z[i];
    }
  } else {
    for (int j = tid; j < n; j += NT) { io.Xo[qp * n + j] = OSQP_NAN; io.Xs[qp * n + j] = 0.0; }
    for (int i = tid; i < m; i += NT) { io.Yo[qp * m + i] = OSQP_NAN; io.Ys[qp * m + i] = 0.0; io.Zs[qp * m + i] = 0.0; }
    if (status == OSQP_PRIMAL_INFEASIBLE || status == OSQP_PRIMAL_INFEASIBLE_INACCURATE) {
      double mx = 0;
      for (int i = tid; i < m; i += NT) { s_ws[i] = unscaled ? s_ws[i] * s_E[i] : s_ws[i]; mx = fmax(mx, fabs(s_ws[i])); }
      mx = b_max<NW>(mx, s.red);
      for (int i = tid; i < m; i += NT) io.DYo[qp * m + i] = s_ws[i] * (1.0 / mx);
    }
    if (status == OSQP_DUAL_INFEASIBLE || status == OSQP_DUAL_INFEASIBLE_INACCURATE) {
      double mx = 0;
      for (int j = tid; j < n; j += NT) { s_tn[j] = unscaled ? s_dx[j] * s_D[j] : s_dx[j]; mx = fmax(mx, fabs(s_tn[j])); }
      mx = b_max<NW>(mx, s.red);
      for (int j = tid; j < n; j += NT) io.DXo[qp * n + j] = s_tn[j] * (1.0 / mx);
    }
  }
  if (tid == 0) {
    // a rebuild left for after the loop drops the refinement verdict, as k_batch_solve's in-loop rebuild does
    io.flag[qp] = rebuild_due ? 1 : (check_pending ? 4 : (need_refine ? 2 : 0));
    double *inf = io.info + qp * 8;
    inf[0] = iter; inf[1] = status; inf[2] = obj; inf[3] = pri_res; inf[4] = dua_res;
    inf[5] = rho_updates; inf[6] = rho_est; inf[7] = rho;
    io.rho_io[qp] = rho;
  }
}
