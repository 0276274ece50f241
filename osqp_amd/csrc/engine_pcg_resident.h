// engine_pcg_resident.h -- included by engine.hip after engine_pcg_steps.h, which ends with k_admm_finalize (it uses cg_step from
// there; Ctx, State and the wavefront / workgroup reductions of engine_device.h).
// The resident PCG (FORM_RESIDENT): the RES_* constants, ResWG / ResCtx, the bounded waits inside a resident launch (res_spin_check,
// res_note, res_slow_note: k_pcg_blockres uses them too), k_form_K, k_form_K_lists and k_pcg_resident.


// ---------------------------------------------------------------------------
// Resident PCG: the whole linear solve of one ADMM iteration in ONE launch.
//
// For problems whose reduced matrix K = P + sigma I + A' diag(rho) A fits the chip's register files
// (n <= 15616, nnz(K) <= 256 workgroups x 448 threads x 64 entries) every workgroup keeps a block of
// rows of K -- values and 16-bit column positions -- in registers for the whole solve, one workgroup per CU:
// wavefronts 1..7 hold the entries and multiply, wavefront 0 owns the rows' vector elements, decides and talks.
// The workgroups exchange vectors through memory INSIDE the launch instead of ending a kernel:
//   (1) an n-vector: every workgroup stores its rows write-through (sc1), drains, raises its flag; wavefront 0
//       polls the 256 flags; then all wavefronts read the vector into LDS with L1-bypassing (sc1) loads -- no
//       fence (MI355X_MICROARCH.md, visibility: the flag/sc1 row).  3.5 us alone (tools/exchange_probe.hip),
//       4.6 us in the loop, against 12.2 us for a k_cg_A/k_cg_B pair;
//   (2) three scalars per workgroup as 8-byte {32 bits, tag} granules, stored and polled with agent-scope atomics.
// Rules the protocol learned the hard way: no 128-byte line of an exchange buffer is written by two
// CUs; a tag never shares a 16-byte store with data it vouches for in the other half; polls are 4- or 8-byte atomic
// loads, never 16-byte buffer loads.
// Recurrences: pipelined CG (Ghysels-Vanroose, ONE exchange per iteration) as long as its true-residual checks
// pass, else Chronopoulos-Gear with a fresh product (the recurrences, scalars and stop rule of k_cg_A / k_cg_B:
// cg_step).  The operator is the explicit K (k_form_K re-forms its values whenever rho, sigma or the matrices change).
// Every wait is bounded in time: if the grid is not co-resident (another process or stream holds CUs) the
// launch gives up, sets State::res_fail, and the host continues with the launch-per-step kernels.
// ---------------------------------------------------------------------------
#define RES_TB 512
#define RES_PT (RES_TB - 64)   // threads that hold entries of K (wavefronts 1..7); wavefront 0 owns the rows and talks
#define RES_MAXROWS 61    // rows per workgroup: they and the three riding partials are stored by the 64 lanes of wavefront 0
#define RES_MAXN (RES_MAXROWS * 256)
#define RES_MAXPAD 16384  // longest exchanged vector (doubles, lines padded)
#define RES_MAXLD (RES_MAXPAD / 2 / RES_TB)   // 16-byte loads per thread that sweep the exchanged vector
#define RES_WAIT_TICKS 2000000LL      // 20 ms of the 100 MHz wall clock: the limit of every wait inside a resident launch (the grid may still be
                                      // arriving in the first one; a later one that long means a workgroup is gone).  Two readings 16 rounds apart
                                      // must both say so, and a reading that cannot be (negative, or hours) restarts the wait's clock.
#define RES_SLOW_TICKS 5000LL         // a wait that ended well after more than 50 us is counted (State::res_slow)
#define AUX_SC1 16
#define AUX_VOL ((int)0x80000000)     // volatile: a poll load the compiler must neither hoist out of its loop nor merge
#define RES_DBG 16                    // ints per workgroup in ResCtx::dbg
#define RES_PRED_WINDOW 16            // solves after which the predicted last trip is judged for this K: more misses than hits switch it off
#define RES_FSTRIDE 32   // 4-byte words between two workgroups' flags: a 128-byte line each
#define RES_GSTRIDE 16   // doubles between two workgroups' granule slots: a 128-byte line each (no line is written by two CUs)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
struct ResWG { int r0, nr, cnt, pos; };   // first row, rows (<= RES_MAXROWS), entries of K, first position in the exchanged vector
struct ResCtx {
  int nwg, E, npad;                  // workgroups, entries per thread, length of the exchanged vector: every workgroup's rows + its three
                                     // dot partials, padded to whole 128-byte lines (a line written by two CUs can lose one of the writes)
  int npw;                           // wavefronts of each workgroup that poll: ceil(nwg / 64), one flag (or one workgroup's granules) per lane
  const unsigned short *rowpos;      // position of row j in that vector
  int pipe;                          // 1: pipelined recurrences where they pass their checks (OSQP_AMD_RESIDENT_PIPE=0: never)
  int predict;                       // 1: the pipelined phase predicts its last trip and sends x - x0 in it (OSQP_AMD_RESIDENT_PREDICT=0: never)
  double pred_margin;                // ... when the extrapolated ||r||^2 is <= pred_margin * tol2 (OSQP_AMD_RESIDENT_PREDICT_MARGIN, default 1)
  int u0_direct;                     // 1: the first product reads u0 from global memory instead of exchanging it
  int inject;                        // test hook (OSQP_AMD_RESIDENT_INJECT=k): in the launch of ADMM iteration k one workgroup walks away,
                                     // the others' waits time out -- the give-up path on demand
  const ResWG *wg;
  const int *ppos;                   // [nwg]: wg[o].pos + wg[o].nr, where workgroup o's three riding partials sit in the exchanged vector
  double *val;                       // [nwg][E][RES_PT]: entry t*E + k of the workgroup's row-major list at (k, t)
  const unsigned short *col;         // same layout: POSITION of the entry's column in the exchanged vector
  const unsigned char *rowl;         // same layout: local row of the entry
  const int *krp, *kcj, *kps, *kdst; // K row by row for k_form_K: row pointers (n + 1), column, slot in M of P(i,j) (-1: none), slot in val
  const unsigned long long *brk;     // [nwg][RES_PT]: bit k set = entry k ends a row segment of this thread
  const unsigned short *slot0;       // [nwg][RES_PT]: first segment slot of the thread
  const unsigned short *segrow;      // [nwg][RES_MAXROWS + 1]: first segment slot of each local row
  double *ubuf;                      // 2 x npad doubles (parity of the tag)
  unsigned *flags;                   // nwg x RES_FSTRIDE words (one 128-byte line each)
  int *dbg;                          // nwg x RES_DBG, written by a launch that gives up: see res_note()
  double *sbuf;                      // 2 x nwg x RES_GSTRIDE 8-byte words: six granules {32 bits of a double, tag} per workgroup, one line each
  double *r0pos;                     // npad doubles: r0 in the exchanged vector's layout, left by k_pcg_init<*, true> (null: r0 and u0 come from
                                     // init_r / init_z, OSQP_AMD_INIT_RESIDENT_STORES=0)
  const int *kcp, *kcm, *kca;        // contribution lists of k_form_K_lists (null: k_form_K forms K): entry e of K (the order of kcj) sums the terms
                                     // kcp[e] .. kcp[e + 1], term q = rhoe[M.col[kcm[q]] - n] * (M.val[kcm[q]] * A.val[kca[q]]), rows of A ascending
};

static __device__ __forceinline__ __amdgpu_buffer_rsrc_t res_rsrc(const void *p, size_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}

// ---- waits inside a resident launch (k_pcg_resident, k_pcg_blockres) ----
// Every wait is a bounded spin of ceil(nwg / 64) wavefronts, one polled workgroup per lane, re-loading only what is still
// missing.  Every 16th round the wave looks at the clock and at the give-up word; every 64th the workgroup stores its own
// flag / granules again (idempotent: should a store ever go missing, the others do not hang on it) -- counted in
// State::res_repub; a wait that ends well after more than 50 us is counted in State::res_slow.
// res_spin_check: 0 = keep polling, 1 = this wait has timed out, 2 = another workgroup gave up.
__device__ __forceinline__ int res_spin_check(State *st, long long &t0, int &late) {
  const long long now = wall_clock64();
  const long long el = now - t0;
  if (el < 0 || el > (1LL << 40)) { t0 = now; late = 0; return 0; }      // not a time: start this wait's clock again
  if (__hip_atomic_load(&st->res_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 2;
  if (el > RES_WAIT_TICKS) { if (late) return 1; late = 1; } else late = 0;
  return 0;
}
// What a workgroup leaves for the host when it gives up (ResCtx::dbg, RES_DBG ints per workgroup):
//   [0] exchange number  [1] mode  [2] PCG iterations          (written at the kernel's exit)
//   [3] 1 / 2: its flag / granule wait timed out, 3: it left because another workgroup had given up
//   [4] first workgroup it still missed (-1: none)   [5] the word it last read from that workgroup (flag, or a granule's tag)
//   [6] ticks it had waited (100 MHz)   [7] XCC id   [8] clock at the give-up (low 32 bits)   [9] rounds   [10] granule index
// Publishing time of a workgroup's last flag = [8] - [6]: its wait started right behind its own store.
__device__ __forceinline__ void res_note(State *st, int *dbg, int g, int verdict, int kind, int nx, int first, unsigned seen, long long t0, unsigned rounds, int gidx) {
  if (verdict == 1 && atomicCAS(&st->res_dbg[0], 0, kind) == 0) { st->res_dbg[1] = nx; st->res_dbg[2] = g; st->res_dbg[3] = first; }
  int *d = dbg + (size_t)RES_DBG * g;
  const long long now = wall_clock64();
  d[3] = verdict == 1 ? kind : 3; d[4] = first; d[5] = (int)seen; d[6] = (int)(now - t0);
  d[7] = (int)__builtin_amdgcn_s_getreg((3 << 11) | 20);        // HW_REG_XCC_ID, bits 3:0
  d[8] = (int)(unsigned)now; d[9] = (int)rounds; d[10] = gidx;
}
__device__ __forceinline__ void res_slow_note(State *st, long long t0, int nx, int g, int missed, int kind) {
  const long long el = wall_clock64() - t0;
  if (el > RES_SLOW_TICKS && el < (1LL << 40)) {
    atomicAdd(&st->res_slow, 1); atomicMax(&st->res_slow_max, (int)(el > 0x7fffffffLL ? 0x7fffffffLL : el));
    atomicAdd(&st->res_slow_hist[el < 20000 ? 0 : (el < 50000 ? 1 : (el < 200000 ? 2 : 3))], 1);
    atomicOr(&st->res_slow_xcc, 1u << (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15));
    st->res_slow_last[0] = nx; st->res_slow_last[1] = g; st->res_slow_last[2] = missed; st->res_slow_last[3] = kind;
  }
}

// K values in the resident layout.  K_ij = P_ij + sigma [i == j] + sum_k rho_k (A_ki A_kj): the sum runs over the rows k
// of A that column i reaches, in ascending k -- the same order and the same products for (i,j) and (j,i), so K is
// symmetric to the bit.  One wavefront per row i of K: each lane keeps up to four entries (i, j) of the row; the
// wavefront walks the rows k of A that column i touches (the A' part of row i of M) and broadcasts their entries
// (k, j') lane by lane; a lane whose j equals j' adds rho_k A_ki A_kj'.  All loads are wavefront-uniform or coalesced:
// 25 us for the 2.09 M entries of config 2 (a two-list merge per entry took 390 us on dependent scattered loads).
__device__ __forceinline__ int lane_int(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__global__ void __launch_bounds__(TB) k_form_K(Ctx c, ResCtx rc) {
  const double sigma = c.prm->sigma;
  if (blockIdx.x == 0 && threadIdx.x == 0) {     // a new K: the pipelined recurrences and the predicted last trip get another chance
    c.st->res_pipe_off = 0;
    c.st->res_pred_off = 0; c.st->res_pred_win[0] = 0; c.st->res_pred_win[1] = 0; c.st->res_pred_win[2] = 0;
  }
  const int lane = threadIdx.x & 63, nwaves = gridDim.x * (TB / 64);
  for (int i = blockIdx.x * (TB / 64) + (threadIdx.x >> 6); i < c.n; i += nwaves) {
    const int e0 = rc.krp[i], e1 = rc.krp[i + 1];
    const int ka = c.M.split[i], kb = c.M.rowptr[i + 1];
    for (int eb = e0; eb < e1; eb += 256) {
      int j[4]; double v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int idx = eb + q * 64 + lane;
        j[q] = -1; v[q] = 0.0;
        if (idx < e1) {
          j[q] = rc.kcj[idx];
          const int ps = rc.kps[idx];
          v[q] = (ps >= 0 ? c.M.val[ps] : 0.0) + (j[q] == i ? sigma : 0.0);
        }
      }
      for (int kc = ka; kc < kb; kc += 64) {
        const bool on = kc + lane < kb;
        const int kk = on ? c.M.col[kc + lane] - c.n : 0;
        const double ai = on ? c.M.val[kc + lane] : 0.0, rk = on ? c.rhoe[kk] : 0.0;     // (rhoe: the rows' effective weights when variables are eliminated, rho itself otherwise)
        const int p0 = on ? c.A.rowptr[kk] : 0, p1 = on ? c.A.rowptr[kk + 1] : 0;
        const int cnt = min(64, kb - kc);
        for (int q = 0; q < cnt; ++q) {
          const double a_i = lane_value(ai, q), r = lane_value(rk, q);
          const int s0 = lane_int(p0, q), s1 = lane_int(p1, q);
          for (int ec = s0; ec < s1; ec += 64) {
            const bool eon = ec + lane < s1;
            const int cj = eon ? c.A.col[ec + lane] : -1;
            const double av = eon ? c.A.val[ec + lane] : 0.0;
            const int len = min(64, s1 - ec);
            for (int e = 0; e < len; ++e) {
              const int cjb = lane_int(cj, e);
              const double t = r * (a_i * lane_value(av, e));
#pragma unroll
              for (int q4 = 0; q4 < 4; ++q4) if (j[q4] == cjb) v[q4] += t;
            }
          }
        }
      }
      // eliminated variables (k_elim_refresh) are not part of the system the launch solves: their rows and columns of K hold
      // nothing but a diagonal entry (the PCG vectors are zero there, so its value never enters a product)
      const bool igone = c.nelim && c.erow[i] >= 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int idx = eb + q * 64 + lane;
        if (idx < e1) {
          const bool gone = c.nelim && (igone || c.erow[j[q]] >= 0);
          rc.val[rc.kdst[idx]] = gone ? (j[q] == i ? 1.0 : 0.0) : v[q];
        }
      }
    }
  }
}

// The same values from contribution lists (build_resident): which rows k of A reach entry (i, j), and where a_ki and a_kj
// sit, depends on the patterns alone, so the merge above is done once on the host and this kernel only streams its result:
// every entry adds its terms in list order (ascending k: the order, the operands and the association of k_form_K, so the
// bits are the same).  The kernel is a chain of dependent loads (offsets -> slots -> values -> weight), so it is laid out for
// few links and many loads per link.  One wavefront per row i of K, four entries per lane.  Nearly every entry has one
// term or none: the first FKL_T terms of all four entries are gathered in one flight per link and added by the lane itself
// (a term the list does not have reads term 0 -- a real slot, one line for all such lanes -- and is not added).  An entry
// with more (the diagonal: as many as column i of A has rows) is finished by the whole wavefront: lane t gathers term t,
// then the products are added in order through readlane.
#define FKL_T 2
__global__ void __launch_bounds__(TB) k_form_K_lists(Ctx c, ResCtx rc) {
  const double sigma = c.prm->sigma;
  if (blockIdx.x == 0 && threadIdx.x == 0) {     // a new K: the pipelined recurrences and the predicted last trip get another chance
    c.st->res_pipe_off = 0;
    c.st->res_pred_off = 0; c.st->res_pred_win[0] = 0; c.st->res_pred_win[1] = 0; c.st->res_pred_win[2] = 0;
  }
  const int lane = threadIdx.x & 63, nwaves = gridDim.x * (TB / 64);
  for (int i = blockIdx.x * (TB / 64) + (threadIdx.x >> 6); i < c.n; i += nwaves) {
    const int e0 = rc.krp[i], e1 = rc.krp[i + 1];
    const bool igone = c.nelim && c.erow[i] >= 0;
    for (int eb = e0; eb < e1; eb += 256) {
      int j[4], ps[4], dst[4], q0[4], len[4]; double v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int idx = min(eb + q * 64 + lane, e1 - 1);          // (lanes past the row read its last entry and store nothing)
        j[q] = rc.kcj[idx]; ps[q] = rc.kps[idx]; dst[q] = rc.kdst[idx];
        q0[q] = rc.kcp[idx]; len[q] = eb + q * 64 + lane < e1 ? rc.kcp[idx + 1] - q0[q] : 0;
      }
      bool any = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = (ps[q] >= 0 ? c.M.val[ps[q]] : 0.0) + (j[q] == i ? sigma : 0.0);
        any = any || len[q] > 0;
      }
      if (__ballot(any)) {                       // (some entry of this pass has a term: the lists are not empty, term 0 exists)
        int pm[4][FKL_T], pa[4][FKL_T], kk[4][FKL_T];
        double am[4][FKL_T], aa[4][FKL_T], rk[4][FKL_T];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < FKL_T; ++t) { const int s = t < len[q] ? q0[q] + t : 0; pm[q][t] = rc.kcm[s]; pa[q][t] = rc.kca[s]; }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < FKL_T; ++t) { kk[q][t] = c.M.col[pm[q][t]] - c.n; am[q][t] = c.M.val[pm[q][t]]; aa[q][t] = c.A.val[pa[q][t]]; }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < FKL_T; ++t) rk[q][t] = c.rhoe[kk[q][t]];     // (rhoe: the rows' effective weights when variables are eliminated, rho itself otherwise)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < FKL_T; ++t) if (t < len[q]) v[q] += rk[q][t] * (am[q][t] * aa[q][t]);
        // the longer lists, one after the other
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          unsigned long long pend = __ballot(len[q] > FKL_T);
          while (pend) {
            const int l = __ffsll((long long)pend) - 1;
            pend &= pend - 1;
            const int s0 = lane_int(q0[q], l) + FKL_T, s1 = s0 - FKL_T + lane_int(len[q], l);
            double acc = lane_value(v[q], l);
            for (int sb = s0; sb < s1; sb += 64) {
              const int s = sb + lane < s1 ? sb + lane : 0;
              const int m_ = rc.kcm[s], a_ = rc.kca[s];
              const int k_ = c.M.col[m_] - c.n;
              const double prod = c.rhoe[k_] * (c.M.val[m_] * c.A.val[a_]);
              const int cnt = min(64, s1 - sb);
              for (int t = 0; t < cnt; ++t) acc += lane_value(prod, t);
            }
            if (lane == l) v[q] = acc;
          }
        }
      }
      // eliminated variables: see k_form_K
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (eb + q * 64 + lane < e1) {
          const bool gone = c.nelim && (igone || c.erow[j[q]] >= 0);
          rc.val[dst[q]] = gone ? (j[q] == i ? 1.0 : 0.0) : v[q];
        }
    }
  }
}

template <int E>
__global__ void __launch_bounds__(RES_TB) k_pcg_resident(Ctx c, ResCtx rc) {
  extern __shared__ __attribute__((aligned(16))) double rlds[];
  State *st = c.st;
  TL_MARK(c, 5);
  // ---- entry: every field of the state, the parameters and the own descriptor in one flight, the returns after one wait ----
  // (none of these loads depends on another; `a || b || c` on three loads is three round trips)
  const int s_stalled = st->stalled, s_run = st->run, s_fail = st->res_fail;
  const unsigned ep0 = st->res_epoch;
  const int s_pipe_off = st->res_pipe_off, s_pred_off = st->res_pred_off, s_admm_done = st->admm_done;
  const Params prm = *c.prm;
  const ResWG w = rc.wg[blockIdx.x];
  if ((s_stalled != 0) | (s_run == 0) | (s_fail != 0)) return;
  double *uv = rlds;                              // npad doubles: the exchanged vector (rows and riding partials of every workgroup)
  double *seg = uv + rc.npad;                     // RES_TB + RES_MAXROWS row-segment sums
  double *sc = seg + RES_TB + RES_MAXROWS;        // 8 doubles: gamma, delta, rr, fail word, verdict; [5] tol2, [6] "the start vector passes" (written once, before the loop)
  double *sval = sc + 8;                          // 3 x 256: the workgroups' dot partials during exchange (2)
#ifdef OSQP_AMD_TIMELINE
  long long *tls = reinterpret_cast<long long *>(sval + 768);   // phase stamps of the first 64 exchanges (workgroup 0)
#define RTL(k) do { if (blockIdx.x == 0 && threadIdx.x == 0 && nx >= 1 && nx <= 64) tls[(nx - 1) * 5 + (k)] = wall_clock64(); } while (0)
  long long *wtl = tls + 5 * 64;                             // [phase][wavefront] stamps of exchange 8 (workgroup 0), then the same of exchange 1
#define WTL(k) do { if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && (nx == 8 || nx == 1)) wtl[(nx == 1 ? 40 : 0) + (k) * 8 + (threadIdx.x >> 6)] = wall_clock64(); } while (0)
  if (blockIdx.x == 0 && threadIdx.x == 0) wtl[80] = wall_clock64();       // kernel entry
#else
#define RTL(k) do { } while (0)
#define WTL(k) do { } while (0)
#endif
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nwg = rc.nwg, npad = rc.npad;
  const bool sabotage = rc.inject > 0 && g == rc.nwg - 1 && s_admm_done + 1 == rc.inject;
  // pipelined recurrences only where a drift would be caught: not in the convexity probe, not after a failed check
  bool pipe = rc.pipe && !s_pipe_off && !prm.no_restart;
  // the predicted last trip (see the loop): wavefront 0 decides, from sums that are the same in every workgroup
  bool predict = pipe && rc.predict && !s_pred_off;
  // ---- own slice of K into registers (issued first: in flight under everything below) ----
  // (wavefronts 1..7; wavefront 0 holds no entries: its loads are the small ones the start-up and the exchanges wait for)
  const bool prod = wv != 0;
  const int tt = t - 64;
  double kv[E]; unsigned short kc[E];
#pragma unroll
  for (int k = 0; k < E; ++k) { kv[k] = 0.0; kc[k] = 0; }
  unsigned long long brk = 0ull;
  int slot0 = 0;
  // u0 = Minv r0 was left in global memory by k_pcg_init (an earlier launch: plain loads see it), in the layout of the exchanged
  // vector: no exchange needed, one coalesced sweep in the form of the exchange's own (every 16-byte load of a thread in flight at
  // once: the register peak the kernel pays there anyway).  It needs nothing but kernel arguments, so wavefronts 1..7 issue it
  // ahead of their entries of K and wavefront 0 behind its start-up sums; a load past the vector's end is dropped by the
  // descriptor's range check.  It lands in LDS before the barrier in front of the loop (uv has no earlier reader).
  const bool u0_direct = rc.u0_direct != 0;
  u32x4 u0v[RES_MAXLD];
  auto u0_issue = [&]() __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t ru = res_rsrc(c.u0pos, (size_t)npad * 8);
#pragma unroll
    for (int q = 0; q < RES_MAXLD; ++q) u0v[q] = __builtin_amdgcn_raw_buffer_load_b128(ru, (q * RES_TB + t) * 16, 0, 0);
  };
  if (prod) {
    if (u0_direct) u0_issue();
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const size_t idx = ((size_t)g * E + k) * RES_PT + tt;
      kv[k] = rc.val[idx]; kc[k] = rc.col[idx];
    }
    brk = rc.brk[(size_t)g * RES_PT + tt];
    slot0 = rc.slot0[(size_t)g * RES_PT + tt];
  }
  int sr0 = 0, sr1 = 0;
  // where the partials of workgroups lane, lane + 64, ... sit in the exchanged vector: wavefront 0 alone reads them (mode 1), so
  // it alone loads them, four loads in one flight at clamped indices (an entry past nwg is never used)
  int ppos[4] = {0, 0, 0, 0};
  // ---- start-up scalars: ||r0||^2, ||b||^2 from k_pcg_init's partials, by wavefront 0 alone ----
  // Wavefront 0 holds no entries of K, so none of these loads queues behind K's.  A lane's partials (lane, lane + 64, ...: at most
  // MAX_PARTS / 64 of each sum) are all in flight at once, at clamped indices, and are added in ascending order from 0.0 (a slot
  // past gridM adds +0.0, which changes no bit of a sum that started at +0.0), then wave_sum: the order the sum has always had.
  // tol2 and the verdict "the start vector already passes" reach the other wavefronts through sc[5], sc[6] at the barrier below.
  constexpr int NPL = MAX_PARTS / 64;
  static_assert(NPL == 16 && NPL * 64 == MAX_PARTS, "k_pcg_resident: a lane of wavefront 0 holds MAX_PARTS / 64 partials of each start-up sum");
  double own_r = 0.0, own_u = 0.0, own_x = 0.0, own_mi = 0.0;
  if (!prod) {
    const int gm = c.gridM;
    double pr[NPL], pb[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) { const int i = min(lane + 64 * q, gm - 1); pr[q] = c.part_rr[i]; pb[q] = c.part_bb[i]; }
#pragma unroll
    for (int q = 0; q < 4; ++q) ppos[q] = rc.ppos[min(lane + 64 * q, nwg - 1)];
    // the own rows in the same flight (clamped: a lane past the workgroup's rows loads a valid element and drops it below)
    // (r0 and u0: from the exchanged vector's layout, where the own rows are w.pos .. w.pos + nr - 1, when k_pcg_init left them there;
    // pointer and index are chosen from kernel arguments alone, so the loads stay in this flight either way)
    const int jc = min(w.r0 + lane, c.n - 1), pc = min(w.pos + lane, npad - 1);
    const bool rpos = rc.r0pos != nullptr;
    const double *rsrc = rpos ? rc.r0pos : c.init_r, *usrc = rpos ? c.u0pos : c.init_z;
    own_r = rsrc[rpos ? (size_t)pc : (size_t)jc * c.init_stride]; own_u = usrc[rpos ? pc : jc]; own_x = c.vx[jc]; own_mi = c.minv[jc];
    sr0 = rc.segrow[(size_t)g * (RES_MAXROWS + 1) + min(lane, RES_MAXROWS)]; sr1 = rc.segrow[(size_t)g * (RES_MAXROWS + 1) + min(lane + 1, RES_MAXROWS)];
    double rr0 = 0.0, bb = 0.0;
#pragma unroll
    for (int q = 0; q < NPL; ++q) { const bool in = lane + 64 * q < gm; rr0 += in ? pr[q] : 0.0; bb += in ? pb[q] : 0.0; }
    rr0 = wave_sum(rr0); bb = wave_sum(bb);
    const double tl2 = fmax(prm.eps_rel * prm.eps_rel * bb, prm.eps_abs * prm.eps_abs);
    if (lane == 0) { sc[3] = 0.0; sc[5] = tl2; sc[6] = rr0 <= tl2 ? 1.0 : 0.0; }
    if (u0_direct) u0_issue();
  }
  // rows of this workgroup live in the lanes of wavefront 0
  const bool own = wv == 0 && lane < w.nr;
  const int j = w.r0 + lane;
  // The eleven doubles of the row state are wavefront 0's alone, and wavefront 0 holds no entries of K: they live in the
  // registers of kv[0..10] (zero in wavefront 0), so that they cost wavefronts 1..7 nothing beside kv[E].  For E < 11 as
  // many as fit, the rest in registers of their own.  EVERY write to one of these names is wavefront 0's (`own`, or
  // `!prod`): in wavefronts 1..7 the same registers are entries of K.
  double rs_rest[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define RES_ROWSTATE(i) (*((i) < E ? &kv[(i) < E ? (i) : 0] : &rs_rest[i]))
  double &r_ = RES_ROWSTATE(0), &u_ = RES_ROWSTATE(1), &w_ = RES_ROWSTATE(2), &p_ = RES_ROWSTATE(3), &s_ = RES_ROWSTATE(4), &x_ = RES_ROWSTATE(5);
  double &mi = RES_ROWSTATE(6), &x0_ = RES_ROWSTATE(7), &r0_ = RES_ROWSTATE(8);
  double &z_ = RES_ROWSTATE(9), &q_ = RES_ROWSTATE(10);     // pipelined recurrences: z = K q, q = Minv s
#undef RES_ROWSTATE
  if (own) { r_ = own_r; u_ = own_u; x_ = own_x; mi = own_mi; x0_ = own_x; r0_ = own_r; }
  else { sr0 = 0; sr1 = 0; }
  if (u0_direct) {
    const int half = npad >> 1;
#pragma unroll
    for (int q = 0; q < RES_MAXLD; ++q) {
      const int i2 = q * RES_TB + t;
      if (i2 < half) { uv[2 * i2] = __hiloint2double((int)u0v[q].y, (int)u0v[q].x); uv[2 * i2 + 1] = __hiloint2double((int)u0v[q].w, (int)u0v[q].z); }
    }
  }
  __syncthreads();
  const double tol2 = sc[5];
  if (sc[6] != 0.0) {                  // the start vector already passes the stop test: all eight wavefronts leave together
    if (g == 0 && t == 0) { st->done = 1; st->tol2 = tol2; }
    return;
  }
  int nx = 0;                          // vector exchanges so far; exchange k carries the tag ep0 + k
  unsigned tag = ep0;
  int par = 0;

  // Exchange (1): every workgroup's rows of one vector (+ 3 doubles riding along) to every workgroup's LDS.
  // Write-through stores, drain, flag; wavefront 0 polls the flags; sc1 sweep.  False when a wait timed out.
  auto vec_exchange = [&](double val, bool ride) __attribute__((always_inline)) -> bool {
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;     // riding partials of (r,u), (w,u), (r,r) when `ride`
    ++nx; tag = ep0 + (unsigned)nx; par = (int)(tag & 1u);
    if (sabotage && nx == 3) return false;     // (test hook: this workgroup walks away without a word)
    RTL(0);
    const __amdgpu_buffer_rsrc_t rs = res_rsrc(rc.ubuf + (size_t)par * npad, (size_t)npad * 8);
    if (wv == 0) {
      // rows at pos .. pos + nr - 1, the three riding partials right behind them: all inside this workgroup's own lines
      if (lane < w.nr) {
        u32x2 d; d.x = (unsigned)__double2loint(val); d.y = (unsigned)__double2hiint(val);
        __builtin_amdgcn_raw_buffer_store_b64(d, rs, (w.pos + lane) * 8, 0, AUX_SC1);
      }
      // (the partials are reduced while the rows are on their way)
      if (ride) { e0 = wave_sum(own ? r_ * u_ : 0.0); e1 = wave_sum(own ? w_ * u_ : 0.0); e2 = wave_sum(own ? r_ * r_ : 0.0); }
      if (lane < 3) {
        const double v = lane == 0 ? e0 : (lane == 1 ? e1 : e2);
        u32x2 d; d.x = (unsigned)__double2loint(v); d.y = (unsigned)__double2hiint(v);
        __builtin_amdgcn_raw_buffer_store_b64(d, rs, (w.pos + w.nr + lane) * 8, 0, AUX_SC1);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(rc.flags + (size_t)g * RES_FSTRIDE, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (wv < rc.npw) {
      // ceil(nwg / 64) wavefronts poll, ONE flag per lane (a lane that polled four flags with atomic loads waited for each
      // before it issued the next), and only until that flag has been seen; the own flag is not polled
      const int o = t;                         // flag of workgroup t
      bool pend = o < nwg && o != g;
      int miss16 = -1;
      unsigned seen = 0, rounds = 0;
      long long t0 = wall_clock64();
      int late = 0;
      bool gave = false;
      while (true) {
        if (pend) {
          seen = __hip_atomic_load(rc.flags + (size_t)o * RES_FSTRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          pend = (int)(seen - tag) < 0;
        }
        if (!__any(pend)) break;
        if (++rounds & 15u) { __builtin_amdgcn_s_sleep(1); continue; }     // clock and give-up word only every 16th round
        const int verdict = res_spin_check(st, t0, late);
        if (verdict) {
          const unsigned long long miss = __ballot(pend);
          const int fl = miss ? (int)__ffsll((long long)miss) - 1 : 0;
          const unsigned sv = (unsigned)__builtin_amdgcn_readlane((int)seen, fl);
          if (lane == 0) { res_note(st, rc.dbg, g, verdict, 1, nx, miss ? 64 * wv + fl : -1, sv, t0, rounds, 0); sc[3] = 1.0; }
          gave = true;
          break;
        }
        if (rounds == 16u) { const unsigned long long ms = __ballot(pend); miss16 = ms ? 64 * wv + (int)__ffsll((long long)ms) - 1 : -1; }
        if ((rounds & 63u) == 0 && wv == 0 && lane == 0) {       // a long wait: say it again
          __hip_atomic_store(rc.flags + (size_t)g * RES_FSTRIDE, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          atomicAdd(&st->res_repub, 1);
        }
        if ((rounds & 255u) == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __builtin_amdgcn_s_sleep(1);
      }
      if (rounds >= 16u && lane == 0 && !gave) res_slow_note(st, t0, nx, g, miss16, 1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __syncthreads();
    RTL(1);
    if (sc[3] != 0.0) return false;
    {
      const int half = npad >> 1;
      u32x4 v[RES_MAXLD];              // every load of the sweep in flight at once
#pragma unroll
      for (int q = 0; q < RES_MAXLD; ++q) { const int i2 = q * RES_TB + t; if (i2 < half) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, i2 * 16, 0, AUX_SC1); }
#pragma unroll
      for (int q = 0; q < RES_MAXLD; ++q) {
        const int i2 = q * RES_TB + t;
        if (i2 < half) { uv[2 * i2] = __hiloint2double((int)v[q].y, (int)v[q].x); uv[2 * i2 + 1] = __hiloint2double((int)v[q].w, (int)v[q].z); }
      }
    }
    __syncthreads();
    RTL(2);
    return true;
  };
  // rows of K times the vector in LDS: E products per thread, row segments through LDS; the own-row value
  // in the lanes of wavefront 0 (ends with the barrier that makes the segments visible)
  auto products_issue = [&]() __attribute__((always_inline)) {
    if (prod) {
      // gathers first (all in flight together; the segment writes below could alias them as far as the compiler knows),
      // half of the entries at a time to stay inside the register budget
      double s = 0.0; int slot = slot0;
      constexpr int H = (E + 1) / 2;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double xv[H];
#pragma unroll
        for (int k = 0; k < H; ++k) if (h * H + k < E) xv[k] = uv[kc[h * H + k]];
#pragma unroll
        for (int k = 0; k < H; ++k)
          if (h * H + k < E) {
            s += kv[h * H + k] * xv[k];
            if ((brk >> (h * H + k)) & 1ull) { seg[slot++] = s; s = 0.0; }
          }
      }
    }
  };
  auto products_finish = [&]() __attribute__((always_inline)) -> double {
    __syncthreads();
    RTL(3);
    double a = 0.0;
    if (own)
      for (int q0 = sr0; q0 < sr1; q0 += 16) {       // 16 independent LDS reads in flight, summed in slot order
        double sv[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) sv[q] = seg[min(q0 + q, sr1 - 1)];     // unconditional: no branch per read
#pragma unroll
        for (int q = 0; q < 16; ++q) a += q0 + q < sr1 ? sv[q] : 0.0;
      }
    return a;
  };
  // Exchange (2): three dot partials per workgroup as tagged granules (the data is the flag); totals in sc[0..2].
  auto scal_exchange = [&](double pg, double pd, double prr) __attribute__((always_inline)) -> bool {
    // granules of 8 bytes {32 bits of data, tag}: six per workgroup, in a line of the workgroup's own, stored with
    // agent-scope atomic stores
    unsigned long long *gb = reinterpret_cast<unsigned long long *>(rc.sbuf) + (size_t)par * nwg * RES_GSTRIDE;
    if (wv == 0) {
      pg = wave_sum(pg); pd = wave_sum(pd); prr = wave_sum(prr);
      if (lane < 6) {
        const double v = lane < 2 ? pg : (lane < 4 ? pd : prr);
        const unsigned half = (lane & 1) ? (unsigned)__double2hiint(v) : (unsigned)__double2loint(v);
        __hip_atomic_store(gb + (size_t)g * RES_GSTRIDE + lane, ((unsigned long long)tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (wv < rc.npw) {
      // ceil(nwg / 64) wavefronts poll, ONE workgroup's six granules per lane, all six loads in flight together
      // (buffer_load_dwordx2 sc1, volatile; six atomic loads went one after the other: 1.9-2.2 us per exchange against
      // 1.5-1.75 at up to 64 workgroups, tools/exchange_probe2.hip), and only the granules still missing.  Each granule vouches
      // for itself; a half arrives in LDS as soon as its tag matches.
      const int o = t;                         // the workgroup whose granules this thread fetches
      const __amdgpu_buffer_rsrc_t rg = res_rsrc(gb, (size_t)nwg * RES_GSTRIDE * 8);
      unsigned pend = o < nwg ? 63u : 0u;
      int miss16 = -1;
      unsigned *svw = reinterpret_cast<unsigned *>(sval) + 6 * o;
      unsigned seen = 0, rounds = 0;
      long long t0 = wall_clock64();
      int late = 0;
      bool gave = false;
      while (true) {
        u32x2 gv[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) if (pend & (1u << q)) gv[q] = __builtin_amdgcn_raw_buffer_load_b64(rg, (o * RES_GSTRIDE + q) * 8, 0, AUX_SC1 | AUX_VOL);
#pragma unroll
        for (int q = 0; q < 6; ++q)
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
          if (lane == 0) { res_note(st, rc.dbg, g, verdict, 2, nx, miss ? 64 * wv + fl : -1, sv, t0, rounds, gi); sc[3] = 1.0; }
          gave = true;
          break;
        }
        if (rounds == 16u) { const unsigned long long ms = __ballot(pend != 0); miss16 = ms ? 64 * wv + (int)__ffsll((long long)ms) - 1 : -1; }
        if ((rounds & 63u) == 0 && wv == 0) {          // a long wait: say it again
          if (lane < 6) {
            const double v = lane < 2 ? pg : (lane < 4 ? pd : prr);
            const unsigned half = (lane & 1) ? (unsigned)__double2hiint(v) : (unsigned)__double2loint(v);
            __hip_atomic_store(gb + (size_t)g * RES_GSTRIDE + lane, ((unsigned long long)tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          if (lane == 0) atomicAdd(&st->res_repub, 1);
        }
        if ((rounds & 255u) == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // a poll that stays unanswered this long: drop whatever this CU still caches
        __builtin_amdgcn_s_sleep(1);
      }
      if (rounds >= 16u && lane == 0 && !gave) res_slow_note(st, t0, nx, g, miss16, 2);
    }
    __syncthreads();
    if (wv == 0) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (lane + 64 * q < nwg) { a0 += sval[3 * (lane + 64 * q)]; a1 += sval[3 * (lane + 64 * q) + 1]; a2 += sval[3 * (lane + 64 * q) + 2]; }
      a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
      if (lane == 0) { sc[0] = a0; sc[1] = a1; sc[2] = a2; }
    }
    __syncthreads();
    RTL(4);
    return sc[3] == 0.0;
  };

  double gam_old = 0.0, alp_old = 0.0;
  int iters = 0;
  bool conv = false, bad = false, failed = false;
  // One loop, one copy of each exchange (four inlined copies cost 88 spilled registers).  Modes:
  //   0  w = K u0 for the pipelined phase           1  pipelined iteration (Ghysels-Vanroose): ONE exchange -- m = Minv w
  //   2  true-residual check r0 - K (x - x0) of        travels with the partials of (r,u), (w,u), (r,r); wavefront 0 forms
  //      EVERY solve that claims convergence           the scalars while the others multiply; w and u follow recurrences
  //   3  Chronopoulos-Gear iteration with a fresh
  //      product (the recurrences of k_cg_A/k_cg_B)
  // The pipelined recurrences drift on ill-conditioned systems, so: out after 64 iterations, out on any breakdown, and
  // every solve that claims convergence is checked against the true residual.  A failed check hands the solve to
  // mode 3 and switches the pipelined phase off until K changes.
  // The predicted last trip.  A pipelined solve of N iterations makes a trip N + 1 whose exchange only delivers the
  // ||r||^2 that says "converged" and whose products nobody uses, and then the check's trip.  When the two latest ||r||^2
  // extrapolate (rr^2 / rr_prev: linear convergence; CG does a little better here, so this errs on the late side) to
  // <= pred_margin * tol2, trip N + 1 sends x - x0 instead of m, with the same three partials riding along:
  //   converged      the products are K (x - x0): straight on to the check's tail -- one trip saved (a hit)
  //   some other stop (breakdown, cap): the check that mode 2 would now run has its product too
  //   goes on        the products are thrown away and NOTHING is touched, neither the row state nor gam_old / alp_old;
  //                  the next trip is an ordinary one with the same partials (a miss: one trip more), and the solve
  //                  predicts no more
  // The iterates are the same bit for bit with or without, hit or miss.  When misses outnumber hits over
  // RES_PRED_WINDOW solves, State::res_pred_off ends it until K changes.
  double rr_prev = 0.0;                // wavefront 0: ||r||^2 of the trip before
  bool pred = false;                   // wavefront 0: the coming trip carries x - x0
  int pred_hit = 0, pred_miss = 0;
  int mode = pipe ? 0 : 3;
  int check_why = 0;                   // 0: the pipelined recurrence says converged, 1: its breakdown / iteration cap, 2: long solve, 3: mode 3 says converged
  int checks3 = 0;                     // failed checks of mode-3 verdicts in this solve
  bool have_u0 = u0_direct;            // the vector k_pcg_init left in global memory, in LDS since the barrier above, is still the u of the recurrences
  while (true) {
    double val = u_, m_ = 0.0;
    if (mode == 1) { m_ = mi * w_; val = pred ? x_ - x0_ : m_; }
    else if (mode == 2) val = x_ - x0_;
    if (have_u0) { ++nx; tag = ep0 + (unsigned)nx; par = (int)(tag & 1u); have_u0 = false; }   // (a fresh tag for the granules of exchange (2))
    else if (!vec_exchange(val, mode == 1)) { failed = true; break; }
    WTL(0);
    products_issue();
    WTL(1);
    CgStep cs{};
    if (mode == 1 && wv == 0) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) if (lane + 64 * q < nwg) { a0 += uv[ppos[q]]; a1 += uv[ppos[q] + 1]; a2 += uv[ppos[q] + 2]; }
      const double gam = wave_sum(a0), del = wave_sum(a1), rr = wave_sum(a2);
      cs = cg_step(rr, gam, del, gam_old, alp_old, tol2, iters, 0, prm, false);
      // (+ 4: this was the predicted trip)
      if (lane == 0) sc[4] = (cs.stop ? (cs.conv ? 1.0 : 2.0) : 0.0) + (pred ? 4.0 : 0.0);
      if (pred) { pred = false; predict = false; }        // one prediction per solve; the scalars stay as they are
      else {
        gam_old = gam; alp_old = cs.alpha;
        // i >= 2: two ||r||^2 on record
        pred = predict && !cs.stop && iters >= 1 && rr * rr <= rc.pred_margin * tol2 * rr_prev;
        rr_prev = rr;
      }
    }
    WTL(2);
    const double kx = products_finish();       // own row of K times the exchanged vector
    WTL(3);
    if (mode == 0) { if (!prod) w_ = kx; mode = 1; continue; }
    if (mode == 1) {
      const int verdict = (int)sc[4];
      if (verdict == 4) { ++pred_miss; continue; }             // predicted, and the solve goes on: this trip did not happen
      if (verdict != 0) {
        check_why = (verdict & 3) == 1 ? 0 : 1; mode = 2;
        if (verdict < 4) continue;                             // (the products of this trip are wasted)
        ++pred_hit;                                            // kx is a row of K (x - x0): on to the tail of mode 2
      }
    }
    if (mode == 1) {
      ++iters;
      if (own) {
        z_ = cs.first ? kx : (kx + cs.beta * z_);
        q_ = cs.first ? m_ : (m_ + cs.beta * q_);
        s_ = cs.first ? w_ : (w_ + cs.beta * s_);
        p_ = cs.first ? u_ : (u_ + cs.beta * p_);
        x_ += cs.alpha * p_;
        r_ -= cs.alpha * s_;
        u_ -= cs.alpha * q_;
        w_ -= cs.alpha * z_;
      }
      WTL(4);
      if (iters >= 64) { check_why = 2; mode = 2; pred = false; }
      continue;
    }
    if (mode == 2) {
      const double rt = r0_ - kx;
      if (!scal_exchange(0.0, 0.0, own ? rt * rt : 0.0)) { failed = true; break; }
      if (sc[2] <= 2.0 * tol2) { conv = true; break; }
      // continue from the true residual with fresh directions; the recurrences are switched off for this K when they
      // had claimed convergence or broken down (not when the solve was merely long)
      if (own) { r_ = rt; u_ = mi * rt; }
      gam_old = 0.0; alp_old = 0.0;
      if (check_why == 3) ++checks3;
      if (g == 0 && t == 0) { if (check_why != 2) st->res_chk_fail += 1; if (check_why < 2) st->res_pipe_off = 1; }   // (a long solve cut at 64 iterations has not failed anything)
      __syncthreads();          // sc[] is rewritten by the next exchange
      mode = 3;
      continue;
    }
    if (!prod) w_ = kx;
    if (!scal_exchange(own ? r_ * u_ : 0.0, own ? w_ * u_ : 0.0, own ? r_ * r_ : 0.0)) { failed = true; break; }
    const double gam = sc[0], del = sc[1], rr = sc[2];
    cs = cg_step(rr, gam, del, gam_old, alp_old, tol2, iters, 0, prm, false);
    if (cs.stop) {
      // a converged solve is checked against the true residual here too (twice at most: on a system whose attainable
      // accuracy sits above the stop the recursive residual's verdict stands, as on the launch-per-step path)
      if (cs.conv && checks3 < 2) { check_why = 3; mode = 2; continue; }
      conv = cs.conv; bad = cs.bad && !cs.conv; break;
    }
    ++iters; gam_old = gam; alp_old = cs.alpha;
    if (own) {
      p_ = cs.first ? u_ : (u_ + cs.beta * p_);
      s_ = cs.first ? w_ : (w_ + cs.beta * s_);
      x_ += cs.alpha * p_;
      r_ -= cs.alpha * s_;
      u_ = mi * r_;
    }
  }
  if (failed) {
    if (t == 0) {
      __hip_atomic_store(&st->res_fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int *d = rc.dbg + (size_t)RES_DBG * g;
      d[0] = nx; d[1] = mode; d[2] = iters;
      if (sabotage) { d[3] = 4; d[7] = (int)__builtin_amdgcn_s_getreg((3 << 11) | 20); d[8] = (int)(unsigned)wall_clock64(); }
    }
    return;
  }
  if (own && iters > 0) c.va[j] = x_;
#ifdef OSQP_AMD_TIMELINE
  if (g == 0 && t == 0) {
    const int cnt = (nx < 64 ? nx : 64) * 5;
    const unsigned long long k0 = atomicAdd(c.tl, (unsigned long long)cnt + 1);
    if (k0 + cnt + 1 < TL_CAP - 2) {
      for (int q = 0; q < cnt; ++q) c.tl[1 + k0 + q] = ((unsigned long long)(10 + q % 5) << 56) | ((unsigned long long)tls[q] & 0x00FFFFFFFFFFFFFFull);
      c.tl[1 + k0 + cnt] = (15ull << 56) | (wall_clock64() & 0x00FFFFFFFFFFFFFFull);
    }
    if (nx >= 8) {
      const unsigned long long k1 = atomicAdd(c.tl, 80ull);
      if (k1 + 80 < TL_CAP - 2) {
        for (int q = 0; q < 40; ++q) c.tl[1 + k1 + q] = ((unsigned long long)(20 + q) << 56) | ((unsigned long long)(wtl[q] - wtl[0]) & 0x00FFFFFFFFFFFFFFull);
        for (int q = 0; q < 40; ++q) c.tl[1 + k1 + 40 + q] = ((unsigned long long)(60 + q) << 56) | ((unsigned long long)(wtl[40 + q] - wtl[80]) & 0x00FFFFFFFFFFFFFFull);   // first trip, since kernel entry
      }
    }
  }
#endif
  if (g == 0 && t == 0) {
    st->iters[0] = iters; st->iters[1] = 0;
    st->done = conv ? 1 : 2;
    if (bad) st->neg_curv = 1;
    st->tol2 = tol2;
    st->res_epoch = ep0 + (unsigned)nx;
    st->res_trips += nx; st->res_solves += 1; st->res_pred_hit += pred_hit; st->res_pred_miss += pred_miss;
    if (rc.predict && !st->res_pred_off) {
      const int ws = st->res_pred_win[0] + 1, wh = st->res_pred_win[1] + pred_hit, wm = st->res_pred_win[2] + pred_miss;
      const bool full = ws >= RES_PRED_WINDOW;
      if (full && wm > wh) st->res_pred_off = 1;
      st->res_pred_win[0] = full ? 0 : ws; st->res_pred_win[1] = full ? 0 : wh; st->res_pred_win[2] = full ? 0 : wm;
    }
  }
}
