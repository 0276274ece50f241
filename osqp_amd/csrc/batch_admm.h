// batch_admm.h -- the per-member OSQP algorithm of the batch engines, included by batch.hip after the
// workgroup helpers and before the engines.  One copy of: Ruiz equilibration with cost and bound scaling
// (src/scaling.c:44-156), row classes and the rho vector (src/auxil.c:76-98), the workspace load / store,
// the iteration (src/osqp.c:356-370), update_info and check_termination with both infeasibility tests
// (src/auxil.c:227-512, 681-786), adapt_rho (src/auxil.c:13-74) and store_solution (src/auxil.c:524-562).
// Everything is a __forceinline__ function over BL / BSettings / BIO for a workgroup of NT threads.
//
// What an engine brings (a plain struct, template parameter K of admm_loop):
//   void solve(const BL &, const double *in, double *out)   out = K^-1 in, ends on a barrier;
//   bool leave(s, p, st, io, qp, a)    rho has just moved: true = the member saved its state and the
//                                      kernel returns now (K^-1 is rebuilt elsewhere);
//   void rho_moved(s, p, st, a)        the rho vectors are updated: bring K^-1 up to date, or note that it is due.
// SLAB (bool): s.Pv / s.Av point at the member's HBM slab io.Wv instead of LDS, so every hand-off of matrix
// values between lanes is a fence plus the barrier, and the workspace load / store skips the values.
// SINGLE_PASS (bool): 4 * NP <= NT, so the four-lanes-per-column passes need no loop (and keep s_b[n..NP) zero).

// uniform scalars of a solve (norms, residuals, status): LDS, s.red + 13
enum { S_PRI, S_DUA, S_OBJ, S_NPRI_S, S_NDUA_S, S_NZ_S, S_NAX_S, S_NQ_S, S_NATY_S, S_NPX_S,
       S_NZ, S_NAX, S_NQ, S_NATY, S_NPX, S_STATUS, S_RHO, S_ND, S_LHS, S_NDX, S_QDX, S_COUNT_ };
enum { F_NORMS = 1, F_STATUS = 2, F_APPROX = 4 };
// The clock of a solve with a time limit (admm_loop<.., CLOCK = true>, bc_solve).  It is looked at only at clock
// iterations: those of a termination check or, with check_termination == 0, every BATCH_CLOCK_INTERVAL-th (the
// reference's default check interval).  The device words of a handle's clock, written by k_clock_start / k_clock_end:
#define BATCH_CLOCK_INTERVAL 25
enum { CK_DEADLINE, CK_START, CK_END, CK_CUT, CK_COUNT_ };   // wall_clock64 ticks: deadline, first and last stamp; members cut
#define S_EXPIRED 40       // s.red slot of the clock's verdict (beyond the reductions' [0, 13) and the scalars from 13)

// Phase time stamps / per-phase accumulators exist only in -DOSQP_AMD_BATCH_DEBUG builds
// (make BATCH_DEBUG=1): they cost ~26 registers and a 2 us s_memrealtime each.
#ifdef OSQP_AMD_BATCH_DEBUG
#define DBG(...) __VA_ARGS__
struct BDbg { unsigned long long tstamp[8], cyc0, pacc[5] = {0, 0, 0, 0, 0}, pt0 = 0, pt1 = 0; };
#define PSTAMP(slot) do { if (st.profile) { dbg.pt1 = wall_clock64(); dbg.pacc[slot] += dbg.pt1 - dbg.pt0; dbg.pt0 = dbg.pt1; } } while (0)
#define ABL(bit) (st.ablate & (bit))
#else
#define DBG(...)
struct BDbg {};
#define PSTAMP(slot) do { } while (0)
#define ABL(bit) 0
#endif

// per-member scalars of a solve (registers)
struct BA {
  double rho, cs;                     // current rho, cost scaling c
  int iter, rho_updates;
  bool need_refine, check_pending;    // refinement verdict (BF_REFINE of io.flag) / still to be taken (BF_OPEN)
  int end_iter;                       // the loop ends with this iteration: max_iter, or the clock iteration that
                                      // found the deadline passed (set before adapt_rho, read by K::leave)
};

// constraint class of a row (auxil.c:76-98): -1 loose, 1 equality, 0 inequality; and its rho
__device__ __forceinline__ int row_class(double l, double u, double rho_tol) {
  if (l < -BINF && u > BINF) return -1;
  return u - l < rho_tol ? 1 : 0;
}
__device__ __forceinline__ double rho_of_class(int t, double rho) { return t == -1 ? 1e-6 : (t == 1 ? 1e3 * rho : rho); }

template <bool SLAB>
__device__ __forceinline__ void handoff() {
  if (SLAB) __threadfence();          // the stores reach L2, stale L1 lines go (as in rebuild_kinv)
  __syncthreads();
}

template <int NT>
__device__ __forceinline__ void clear_vectors(const BL &s) {
  const int tid = threadIdx.x;
  for (int j = tid; j < s.NP; j += NT) {
    s_q[j] = 0.0; s_x[j] = 0.0; s_xt[j] = 0.0; s_dx[j] = 0.0; s_D[j] = 1.0; s_tn[j] = 0.0; s_b[j] = 0.0;
  }
  for (int i = tid; i < s.m; i += NT) { s_z[i] = 0.0; s_y[i] = 0.0; s_E[i] = 1.0; s_dy[i] = 0.0; s_ws[i] = 0.0; }
  __syncthreads();
}

template <int NT>
__device__ __forceinline__ void set_rho_vectors(const BL &s, double rho) {
  for (int i = threadIdx.x; i < s.m; i += NT) {
    const double r = rho_of_class(s.ctype[i], rho);
    s_rho[i] = r; s_rinv[i] = 1.0 / r;
  }
}
// w = rho z - y (each lane reads the rho it wrote itself)
template <int NT>
__device__ __forceinline__ void refresh_w(const BL &s) {
  for (int i = threadIdx.x; i < s.m; i += NT) s_w[i] = s_rho[i] * s_z[i] - s_y[i];
  __syncthreads();
}

// ---------------------------------------------------------------------------
// setup
// ---------------------------------------------------------------------------
template <int NT, bool SLAB>
__device__ __forceinline__ void load_problem(const BL &s, const BPattern &p, const BIO &io, long long qp) {
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const double *Pg = io.Px + qp * io.strideP, *Ag = io.Ax + qp * io.strideA;
  for (int k = tid; k < p.nnzP; k += NT) s.Pv[k] = Pg[k];
  for (int k = tid; k < p.nnzA; k += NT) s.Av[k] = Ag[k];
  for (int j = tid; j < n; j += NT) s_q[j] = io.Q[qp * n + j];
  for (int i = tid; i < m; i += NT) { s_l[i] = io.L[qp * m + i]; s_u[i] = io.U[qp * m + i]; }
  handoff<SLAB>();
}

// Ruiz equilibration (scaling.c:44-156) with cost scaling, then the scaled bounds and their row classes.
// Returns the cost scaling c; D, E, the scaled q, l, u and matrix values are left in s.
// CLASSIFY = false: the scale_data of a matrix update (osqp.c:1254-1257), which keeps the row classes s.ctype holds.
template <int NT, bool SLAB, bool CLASSIFY = true>
__device__ __forceinline__ double ruiz_scale(const BL &s, const BPattern &p, const BSettings &st) {
  constexpr int NW = NT / 64;
  const int n = p.n, m = p.m, tid = threadIdx.x;
  double cs = 1.0;
  for (int pass = 0; pass < st.scaling; ++pass) {
    for (int j = tid; j < n; j += NT) {
      double v = 0.0;
      for (int k = s.Fp[j]; k < s.Fp[j + 1]; ++k) v = fmax(v, fabs(s.Pv[s.Fk[k]]));
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; ++k) v = fmax(v, fabs(s.Av[k]));
      s_tn[j] = 1.0 / sqrt(clip_scale(v));
    }
    for (int i = tid; i < m; i += NT) {
      double v = 0.0;
      for (int k = s.Rp[i]; k < s.Rp[i + 1]; ++k) v = fmax(v, fabs(s.Av[s.Rk[k]]));
      s_tm[i] = 1.0 / sqrt(clip_scale(v));
    }
    __syncthreads();
    for (int k = tid; k < p.nnzP; k += NT) s.Pv[k] = (s.Pv[k] * s_tn[s.Pi[k]]) * s_tn[s.Pc[k]];
    for (int k = tid; k < p.nnzA; k += NT) s.Av[k] = (s.Av[k] * s_tm[s.Ai[k]]) * s_tn[s.Ac[k]];
    for (int j = tid; j < n; j += NT) { s_q[j] = s_q[j] * s_tn[j]; s_D[j] = s_tn[j] * s_D[j]; }
    for (int i = tid; i < m; i += NT) s_E[i] = s_tm[i] * s_E[i];
    handoff<SLAB>();
    // cost normalisation: mean column norm of P (sequential sum, reference order) vs |q|_inf
    double cn = 0.0, qn = 0.0;
    for (int j = tid; j < n; j += NT) {
      double v = 0.0;
      for (int k = s.Fp[j]; k < s.Fp[j + 1]; ++k) v = fmax(v, fabs(s.Pv[s.Fk[k]]));
      s_tn[j] = v;
      qn = fmax(qn, fabs(s_q[j]));
    }
    qn = b_max<NW>(qn, s.red);
    if (tid == 0) { double acc = 0.0; for (int j = 0; j < n; ++j) acc += s_tn[j]; s.red[12] = acc / (double)n; }
    __syncthreads();
    cn = s.red[12];
    double ct = fmax(cn, clip_scale(qn));
    ct = 1.0 / clip_scale(ct);
    for (int k = tid; k < p.nnzP; k += NT) s.Pv[k] *= ct;
    for (int j = tid; j < n; j += NT) s_q[j] *= ct;
    cs *= ct;
    handoff<SLAB>();
  }
  for (int i = tid; i < m; i += NT) {
    s_l[i] = s_l[i] * s_E[i]; s_u[i] = s_u[i] * s_E[i];
    if (CLASSIFY) s.ctype[i] = row_class(s_l[i], s_u[i], st.rho_tol);
  }
  return cs;
}

// the setup workspace of one member: the analogue of the reference's scaled OSQPData, kept across solves.
// FRESH = false (a matrix update): the iterates, the row classes and rho stay what they are, and rho_updates is
// reset as reset_info does in every osqp_update_* (src/auxil.c:632-649).
template <int NT, bool SLAB, bool FRESH = true>
__device__ __forceinline__ void store_workspace(const BL &s, const BPattern &p, const BIO &io, long long qp,
                                                double cs, double rho, int flag) {
  const int n = p.n, m = p.m, tid = threadIdx.x;
  if (!SLAB) {
    double *Wv = io.Wv + qp * ((long long)p.nnzP + p.nnzA);
    for (int k = tid; k < p.nnzP; k += NT) Wv[k] = s.Pv[k];
    for (int k = tid; k < p.nnzA; k += NT) Wv[p.nnzP + k] = s.Av[k];
  }
  for (int j = tid; j < n; j += NT) {
    io.Wq[qp * n + j] = s_q[j]; io.Wd[qp * n + j] = s_D[j];
    if (FRESH) io.Xs[qp * n + j] = 0.0;
  }
  for (int i = tid; i < m; i += NT) {
    io.Wl[qp * m + i] = s_l[i]; io.Wu[qp * m + i] = s_u[i]; io.We[qp * m + i] = s_E[i];
    if (FRESH) { io.Wt[qp * m + i] = s.ctype[i]; io.Zs[qp * m + i] = 0.0; io.Ys[qp * m + i] = 0.0; }
  }
  if (tid == 0) {
    io.Wc[qp] = cs; io.flag[qp] = flag;
    if (FRESH) io.rho_io[qp] = rho; else io.info[qp * 8 + 5] = 0.0;
  }
}

// the row classes of the workspace back into s (a matrix update keeps them)
template <int NT>
__device__ __forceinline__ void load_classes(const BL &s, const BPattern &p, const BIO &io, long long qp) {
  for (int i = threadIdx.x; i < p.m; i += NT) s.ctype[i] = io.Wt[qp * p.m + i];
}

// ---------------------------------------------------------------------------
// solve
// ---------------------------------------------------------------------------
// the workspace back into s (after clear_vectors); returns the cost scaling c
template <int NT, bool SLAB>
__device__ __forceinline__ double load_workspace(const BL &s, const BPattern &p, const BIO &io, long long qp) {
  const int n = p.n, m = p.m, tid = threadIdx.x;
  if (!SLAB) {
    const double *Wv = io.Wv + qp * ((long long)p.nnzP + p.nnzA);
    for (int k = tid; k < p.nnzP; k += NT) s.Pv[k] = Wv[k];
    for (int k = tid; k < p.nnzA; k += NT) s.Av[k] = Wv[p.nnzP + k];
  }
  for (int j = tid; j < n; j += NT) { s_q[j] = io.Wq[qp * n + j]; s_D[j] = io.Wd[qp * n + j]; }
  for (int i = tid; i < m; i += NT) {
    s_l[i] = io.Wl[qp * m + i]; s_u[i] = io.Wu[qp * m + i]; s_E[i] = io.We[qp * m + i];
    s.ctype[i] = io.Wt[qp * m + i];
  }
  return io.Wc[qp];
}

// rho vectors (auxil.c:76-98) and, when warm, the iterates the last solve (or round) left
template <int NT>
__device__ __forceinline__ void init_iterates(const BL &s, const BPattern &p, const BIO &io, long long qp, double rho, bool warm) {
  const int n = p.n, m = p.m, tid = threadIdx.x;
  set_rho_vectors<NT>(s, rho);
  if (warm) {
    for (int j = tid; j < n; j += NT) s_x[j] = io.Xs[qp * n + j];
    for (int i = tid; i < m; i += NT) { s_z[i] = io.Zs[qp * m + i]; s_y[i] = io.Ys[qp * m + i]; }
  }
  __syncthreads();
}

// update_info: residuals and norms (auxil.c:227-318), plus the cheap halves of both infeasibility
// tests (auxil.c:361-512), in two passes and ONE workgroup reduction
template <int NT, bool SINGLE_PASS>
__device__ __forceinline__ void update_info(const BL &s, const BPattern &p, const BSettings &st, double cs) {
  constexpr int NW = NT / 64;
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const bool unscaled = st.scaling && !st.scaled_termination;
  const double cinv = 1.0 / cs;
  double *sc = s.red + 13;
  double mx[16], sm[3];
#pragma unroll
  for (int k = 0; k < 16; ++k) mx[k] = 0.0;
  sm[0] = sm[1] = sm[2] = 0.0;
  for (int i = tid >> 1; i < m; i += NT / 2) {          // rows: two lanes each
    const double ax = a_row_dot2(s, s_x, i, tid & 1);
    if ((tid & 1) == 0) {
      const double zi = s_z[i], pr = ax + (-1.0) * zi;
      const double ei = unscaled ? 1.0 / s_E[i] : 1.0;
      mx[0] = fmax(mx[0], fabs(ei * pr)); mx[1] = fmax(mx[1], fabs(pr));
      mx[2] = fmax(mx[2], fabs(ei * zi)); mx[3] = fmax(mx[3], fabs(zi));
      mx[4] = fmax(mx[4], fabs(ei * ax)); mx[5] = fmax(mx[5], fabs(ax));
      // delta_y projected on the polar of the recession cone (is_primal_infeasible)
      double dy = s_dy[i];
      const double li = s_l[i], ui = s_u[i];
      if (ui > BINF) { if (li < -BINF) dy = 0.0; else dy = fmin(dy, 0.0); }
      else if (li < -BINF) dy = fmax(dy, 0.0);
      s_ws[i] = dy;
      mx[14] = fmax(mx[14], fabs(unscaled ? s_E[i] * dy : dy));
      sm[1] += ui * fmax(dy, 0.0) + li * fmin(dy, 0.0);
    }
  }
  // columns: four lanes each (one trip when SINGLE_PASS: fmax with / adding to the zero above is the value itself)
  for (int j = tid >> 2, l = tid & 3; j < (SINGLE_PASS ? s.NP : n); j += NT / 4) {
    if (j < n) {
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
        mx[15] = fmax(mx[15], fabs(unscaled ? s_D[j] * dxj : dxj));      // is_dual_infeasible: |delta_x|, q'delta_x
        sm[2] += qj * dxj;
      }
    }
  }
  b_reduce_many<NW, 16, 3>(mx, sm, s.gp);
  if (tid == 0) {
    const double *g = s.gp + NW * 19;                 // combined values
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
}

// check_termination (auxil.c:681-786) on the scalars update_info left; true (uniformly) when the member is done
template <int NT>
__device__ __forceinline__ bool check_termination(const BL &s, const BPattern &p, const BSettings &st, double cs, bool approximate) {
  constexpr int NW = NT / 64;
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const bool unscaled = st.scaling && !st.scaled_termination;
  double *sc = s.red + 13;
  const double pri_res = sc[S_PRI], dua_res = sc[S_DUA];
  int newstatus = 0;      // 0 = keep going
  double newobj = 0.0;
  if (pri_res > 1e30 || dua_res > 1e30) { newstatus = OSQP_NON_CVX; newobj = OSQP_NAN; }
  else {
    double ea = st.eps_abs, er = st.eps_rel, epi = st.eps_pinf, edi = st.eps_dinf;
    if (approximate) { ea *= 10; er *= 10; epi *= 10; edi *= 10; }
    bool prim_ok = false, dual_ok = false, pinf = false, dinf = false;
    if (m == 0) prim_ok = true;
    else if (pri_res < ea + er * fmax(sc[S_NZ], sc[S_NAX])) prim_ok = true;
    else {
      // is_primal_infeasible (auxil.c:361-424); the projected delta_y is in ws
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
      // is_dual_infeasible (auxil.c:426-512)
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
  if (newstatus != 0 && tid == 0) {
    sc[S_STATUS] = newstatus;
    if (newstatus != OSQP_SOLVED && newstatus != OSQP_SOLVED_INACCURATE) sc[S_OBJ] = newobj;
  }
  __syncthreads();
  return newstatus != 0;
}

// the rho that adapt_rho would choose (auxil.c:13-74), from the scaled norms of the last update_info
__device__ __forceinline__ double rho_estimate(const double *sc, int m, double rho) {
  const double pr = (m ? sc[S_NPRI_S] : 0.0) / (fmax(sc[S_NZ_S], sc[S_NAX_S]) + 1e-30);
  const double du = sc[S_NDUA_S] / (fmax(fmax(sc[S_NQ_S], sc[S_NATY_S]), sc[S_NPX_S]) + 1e-30);
  return fmin(fmax(rho * sqrt(pr / du), 1e-6), 1e6);
}

// The ADMM loop (osqp.c:354-532) from iteration iter0 + 1, K^-1 current, a.rho / cs / need_refine / check_pending set.
// Uniform scalars (norms, residuals, status) live in LDS (`sc`), not in registers, and the
// residual/termination code has ONE call site: a small stage machine replaces the reference's
// in-loop / post-loop / approximate calls of update_info + check_termination (osqp.c:411-437, 537-581).
// Returns true when the member left for a rebuild of K^-1 (K::leave): the kernel returns at once.
// CLOCK: the solve has a time limit, clk are the handle's clock words.  At a clock iteration, after the termination
// check, ONE thread compares wall_clock64() with the deadline and publishes the verdict through LDS -- wavefronts that
// read the clock themselves could disagree across the deadline and part ways at a barrier.  An expired clock ends the
// loop as max_iter does (which wins when both hold): the approximate test, then OSQP_TIME_LIMIT_REACHED.
template <int NT, bool SINGLE_PASS, bool CLOCK = false, class K>
__device__ __forceinline__ bool admm_loop(const BL &s, const BPattern &p, const BSettings &st, const BIO &io, long long qp,
                                          BA &a, int iter0, K &eng, BDbg &dbg, unsigned long long *clk = nullptr) {
  constexpr int NW = NT / 64;
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const double alpha = st.alpha, oma = 1.0 - st.alpha, sigma = st.sigma;
  double *sc = s.red + 13;
  double &rho = a.rho;
  bool &need_refine = a.need_refine, &check_pending = a.check_pending;
  if (tid == 0) { for (int k = 0; k < S_COUNT_; ++k) sc[k] = 0.0; sc[S_STATUS] = OSQP_UNSOLVED; sc[S_RHO] = rho; }
  refresh_w<NT>(s);
  // rho_updates counts on from the previous solve until an update resets it, like the reference's info
  // (set to 0 by osqp_setup and by reset_info in every osqp_update_*, src/auxil.c:632-649)
  int &iter = a.iter, &rho_updates = a.rho_updates;
  iter = iter0; rho_updates = (int)io.info[qp * 8 + 5];
  a.end_iter = st.max_iter;
  int stage = 0, probe_until = 0;
  bool norms_fresh = false;
  bool cut = false;        // (CLOCK) the clock ended the loop

  while (stage != 3) {
    int flags = 0;
    bool checked = false, adapt_due = false;
    if (stage == 0) {
      ++iter;
      DBG(if (st.profile) dbg.pt0 = wall_clock64();)
      // rhs of the reduced system: b = sigma x - q + A'(rho z - y); w = rho z - y is kept
      // up to date by the z/y update below.  Four lanes per column.
      if (!ABL(1)) {
        for (int j = tid >> 2, l = tid & 3; j < (SINGLE_PASS ? s.NP : n); j += NT / 4) {
          const double acc = j < n ? a_col_dot4(s, s_w, j, l) : 0.0;
          if (l == 0) s_b[j] = j < n ? (sigma * s_x[j] - s_q[j]) + acc : 0.0;
        }
        __syncthreads();
      }
      PSTAMP(0);
      if (!ABL(2)) eng.solve(s, s_b, s_xt);
      PSTAMP(1);
      // One step of iterative refinement, xt += Kinv (b - K xt), for QPs whose K^-1 needs it.
      // Whether it does is probed (relative residual of the solve above refine_tol, fill_settings) in the first
      // four iterations after K^-1 was built; one hit turns refinement on for good (kept per QP
      // across solves).  refine = 2: always on.
      const bool probe = !need_refine && (check_pending || iter <= probe_until);
      if (st.refine && (st.refine == 2 || need_refine || probe)) {
        for (int i = tid; i < m; i += NT) s_ws[i] = s_rho[i] * a_row_dot(s, s_xt, i);
        __syncthreads();
        double rmax = 0.0, bmax = 0.0;
        for (int j = tid; j < s.NP; j += NT) {
          s_tn[j] = j < n ? s_b[j] - (p_row_dot(s, s_xt, j) + sigma * s_xt[j] + a_col_dot(s, s_ws, j)) : 0.0;
          rmax = fmax(rmax, fabs(s_tn[j])); bmax = fmax(bmax, fabs(s_b[j]));
        }
        if (probe) {
          rmax = b_max<NW>(rmax, s.red); bmax = b_max<NW>(bmax, s.red);
          need_refine = rmax > st.refine_tol * bmax;
          if (check_pending) { check_pending = false; probe_until = iter + 3; }
        }
        __syncthreads();
        eng.solve(s, s_tn, s_dx);   // dx is free until the x update below
        for (int j = tid; j < n; j += NT) s_xt[j] += s_dx[j];
        __syncthreads();
      }
      PSTAMP(2);
      // z~ = A x~ ; x, z, y updates (auxil.c:185-225, proj.c:4-14); two lanes per row
      if (!ABL(4))
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
      if (!ABL(8))
      for (int j = tid; j < n; j += NT) {
        const double xo = s_x[j];
        const double xn = alpha * s_xt[j] + oma * xo;
        s_dx[j] = xn - xo; s_x[j] = xn;
      }
      __syncthreads();
      PSTAMP(3);
      norms_fresh = false;
      checked = st.check_termination && (iter % st.check_termination == 0);
      adapt_due = st.adaptive_rho && st.rho_interval && (iter % st.rho_interval == 0);
      if (checked) flags = F_NORMS | F_STATUS;
      else if (adapt_due) flags = F_NORMS;
    } else if (stage == 1) flags = F_STATUS | (norms_fresh ? 0 : F_NORMS);
    else flags = F_STATUS | F_APPROX;

    bool term = false;
    if (flags & F_NORMS) { update_info<NT, SINGLE_PASS>(s, p, st, a.cs); norms_fresh = true; }
    if (flags & F_STATUS) term = check_termination<NT>(s, p, st, a.cs, flags & F_APPROX);
    if (stage == 0) {
      if (checked && term) { stage = 3; continue; }
      if constexpr (CLOCK) {
        if (checked || (!st.check_termination && iter % BATCH_CLOCK_INTERVAL == 0)) {
          // the deadline is loaded here, not before the loop: it holds no register across the K solve
          if (tid == 0) s.red[S_EXPIRED] = wall_clock64() >= *(volatile unsigned long long *)(clk + CK_DEADLINE) ? 1.0 : 0.0;
          __syncthreads();
          if (s.red[S_EXPIRED] != 0.0 && iter < a.end_iter) {
            a.end_iter = iter; cut = true;
            if (tid == 0) atomicAdd(clk + CK_CUT, 1ULL);
          }
        }
      }
      if (adapt_due) {     // adapt_rho (auxil.c:13-74)
        const double rn = rho_estimate(sc, m, rho);
        if (rn > rho * st.adapt_tol || rn < rho / st.adapt_tol) {
          rho = rn; rho_updates++;
          if (eng.leave(s, p, st, io, qp, a)) return true;
          set_rho_vectors<NT>(s, rho);
          refresh_w<NT>(s);
          eng.rho_moved(s, p, st, a);
        }
      }
      if (iter >= a.end_iter) stage = checked ? 2 : 1;
    } else if (stage == 1) stage = term ? 3 : 2;
    else {
      if (!term && tid == 0) sc[S_STATUS] = (CLOCK && cut) ? OSQP_TIME_LIMIT_REACHED : OSQP_MAX_ITER_REACHED;
      __syncthreads();
      stage = 3;
    }
  }
  return false;
}

// store_solution (auxil.c:524-562) with the certificates, the warm-start iterates, io.flag (BF_* bits) and the info record
template <int NT>
__device__ __forceinline__ void store_solution(const BL &s, const BPattern &p, const BSettings &st, const BIO &io, long long qp,
                                               const BA &a, int flag) {
  constexpr int NW = NT / 64;
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const bool unscaled = st.scaling && !st.scaled_termination;
  const double cinv = 1.0 / a.cs;
  const double *sc = s.red + 13;
  const int status = (int)sc[S_STATUS];
  const double pri_res = sc[S_PRI], dua_res = sc[S_DUA], obj = sc[S_OBJ];
  const double rho_est = rho_estimate(sc, m, a.rho);
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
    io.flag[qp] = flag;
    double *inf = io.info + qp * 8;
    inf[0] = a.iter; inf[1] = status; inf[2] = obj; inf[3] = pri_res; inf[4] = dua_res;
    inf[5] = a.rho_updates; inf[6] = rho_est; inf[7] = a.rho;
  }
}
