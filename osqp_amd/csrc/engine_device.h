// engine_device.h -- included by engine.hip first, right after the system headers and osqp_amd_engine.h (it needs nothing else).
// The device building blocks every solve form shares, and the macros that every later fragment uses: TB, MAX_CHUNK, LONG_ROW,
// HUGE_ROW, MAX_PARTS, MAX_HUGE_FOLD, INF_BOUND and HIPCHK; the descriptors RowBlk / G4 / DevMat / DenseBlk / DenseP / State /
// Params / Ctx; the timeline macros TL_MARK and TLK_* (empty unless -DOSQP_AMD_TIMELINE); the scalar slots SC_* / SCI; the wavefront
// and workgroup reductions (wave_sum, block_sum, block_sum3, reduce_parts, block_max_to); the CSR-stream pieces (stage_products,
// row_sum, row_sum_par), the long-row and dense-block products (long_row_dot, wave_row_dot, dense_block_mv_x, dense_block_mv) and
// LDS_DECL.

#define TB 256            // threads per workgroup (4 wavefronts of 64)
#define MAX_CHUNK 2048    // products staged in LDS per workgroup (x2 for dual stream)
#define LONG_ROW 512      // a row with at least this many entries gets a workgroup of its own (no LDS staging)
#define HUGE_ROW 8192     // A rows this long are sliced over the whole grid in k_cg_A (partials finished by k_huge_reduce)
#define MAX_PARTS 1024    // upper bound on workgroups that emit dot partials
#define MAX_HUGE_FOLD 4   // up to this many huge rows are folded into k_cg_B (more: k_huge_reduce finishes them)
#define INF_BOUND 1e26    // OSQP_INFTY * MIN_SCALING

#define HIPCHK(call)                                                            \
  do {                                                                          \
    hipError_t _e = (call);                                                     \
    if (_e != hipSuccess) {                                                     \
      fprintf(stderr, "osqp_amd: HIP error %s at %s:%d (%s)\n",                 \
              hipGetErrorString(_e), __FILE__, __LINE__, #call);                \
      return HIPENG_ERR_HIP;                                                    \
    }                                                                           \
  } while (0)

// ---------------------------------------------------------------------------
// device-side descriptors
// ---------------------------------------------------------------------------
struct RowBlk { int r0, r1, k0, k1; };
#define IS_LONG(b) ((b).r1 - (b).r0 == 1 && (b).k1 - (b).k0 >= LONG_ROW)
// per-column record gathered by k_cg_A: one 32-byte access instead of four 8-byte
// gathers from four arrays (residual, w = K u, s = K p, Jacobi inverse)
struct __attribute__((aligned(32))) G4 { double r, w, s, m; };

struct DevMat {
  int nrows, nblk;
  int nstream;           // blocks [0,nstream) are multi-row stream blocks, [nstream,nblk) single long rows
  int nwave;             // PCG kernels: long rows [nstream,nwave) take one wavefront each, [nwave,nblk) are huge
  const int    *rowptr;
  const int    *col;
  const unsigned short *col16;   // the same column ids as 16-bit words where every id fits (null otherwise): the long-row passes
                                 // stream 10 instead of 12 bytes per entry (config 3: 26 -> 22 us per pass over A)
  const double *val;
  const int    *split;   // M only: first entry of the A' part of each row
  const RowBlk *blk;
};

// Dense diagonal blocks of P (portfolio-style block-diagonal covariance): such a block is
// kept as a plain dense b x b array (8 B per entry, no index) for the PCG operator kernel;
// everything else of its rows (the A' part) stays in the sparse remainder matrix.
#define DENSE_MAX 128          // lanes cover the block's columns in two 64-lane halves
struct DenseBlk { int c0, b, off, pitch; };   // first row/column, size, offset into val, row pitch in doubles (even, zero padded)
struct DenseP {
  int nblk;                  // dense blocks (0: feature off)
  const DenseBlk *blk;
  const double *val;         // blocks back to back, each b rows of `pitch` doubles (zero padded; row-major = column-major: symmetric)
};

// Written by kernels only; read by the host between windows.
struct State {
  int    run;          // this ADMM iteration is active (written by the first kernel)
  int    done;         // PCG converged (written by k_cg_A)
  int    stalled;      // PCG ran out of unrolled iterations (written by finalize)
  int    neg_curv;     // p'Kp <= 0 seen
  int    iters[2];     // PCG iterations of the current solve (ping-pong on parity)
  int    neg_curv_seen;
  int    iters_last;
  int    iters_max;
  int    iters_min;        // smallest PCG iteration count of a solve since the host last reset it
  int    forced;
  long long iters_total;
  long long admm_done;
  double rz[2];
  double tol2;
  double gam[2], alp[2];   // Chronopoulos-Gear scalars (ping-pong on parity)
  int    hist_r;           // ADMM iterations since the PCG start vector history was reset (k_pcg_init counts)
  long long admm_target;   // k_pcg_init starts no new ADMM iteration once admm_done has reached this
  unsigned res_epoch;      // resident PCG: tag of the last exchange of the previous launch
  int    res_fail;         // resident PCG: a wait timed out (workgroups not co-resident); the host falls back to the launch-per-step path
  int    res_pipe_off;     // resident PCG: the pipelined recurrences failed a true-residual check for this K (k_form_K clears it)
  int    res_chk_fail;     // resident PCG: true-residual checks that failed since create (each continued the solve from the true residual)
  int    res_dbg[4];       // resident PCG, first timed-out wait: 1 = flags / 2 = granules, exchange number, waiting workgroup, first missing workgroup
  int    res_slow;         // resident PCG: waits that ended well but took more than 50 us (the host adds them up: hipeng_resident_info)
  int    res_slow_max;     // ... the longest of them, in ticks of the 100 MHz clock
  int    res_repub;        // ... flags / granules that a workgroup stored again because its own wait went on (every 64th round)
  int    res_slow_hist[4]; // ... slow waits by length: 50-200 us, 200-500 us, 0.5-2 ms, longer
  unsigned res_slow_xcc;   // ... bit k: a wavefront on XCC k had one
  int    res_slow_last[4]; // ... the latest: exchange number, workgroup, first workgroup it had missed at its 16th round, wait kind (1 flags, 2 granules)
  // k_pcg_resident, since create (hipeng_resident_trips): vector trips of its launches, launches that ran a solve, predicted last
  // trips whose products served the true-residual check (hits), predicted last trips that were not the last (misses)
  long long res_trips, res_solves, res_pred_hit, res_pred_miss;
  int    res_pred_win[3];  // the current window of RES_PRED_WINDOW solves on this K: solves, hits, misses
  int    res_pred_off;     // misses outnumbered hits over a window: no predicted trips until K changes (k_form_K clears it)
};

struct Params {          // mutable scalars (host writes, kernels read)
  double sigma, alpha, eps_rel, eps_abs, cinv;
  int    pcg_max_iter, use_cvec, has_scaling, pad0;
  double ex_theta;         // extrapolation of the PCG start vector (0 = plain warm start)
  int    ex_h0, ex_h1;     // no extrapolation before iteration ex_h0 after a reset, half a step before ex_h1
  int    no_restart;       // setup-time convexity probe: any loss of positivity counts as negative curvature
};

struct Ctx {             // static pointers / sizes, passed by value
  int n, m;
  DevMat A, M;
  DevMat Mk;             // what k_cg_B streams: M itself, or its remainder when P has dense blocks
  DenseP dP;
  int nh, hrow[MAX_HUGE_FOLD];     // huge rows of A folded into k_cg_B, and hcol: nh dense vectors hcol_k[j] = A(h_k, j)
  const double *hcol;
  int gridA, gridM;      // launch grids (>=1) of row kernels over A / over M
  double *xy, *z, *zt, *va, *vb, *q, *l, *u, *rho, *rhoinv, *minv, *pdiag;
  double *r, *zz, *kp, *pt0, *pt1, *dxy, *dy, *cvec;
  double *init_r, *init_z;        // where k_pcg_init puts r0 and Minv r0
  double *vx, *vold;               // PCG start vector [x~0 | rho z~0] (extrapolated) and the previous [x~ | rho z~]
  double *pdir, *ut;               // Chronopoulos-Gear PCG: p, [u|t]
  G4     *g4;                      // ... and {r, w, s, Minv} records, ping-ponged on parity (2n)
  int     init_stride;             // element stride of init_r (4 when it points into g4)
  int     fin_wave_rows;           // k_admm_finalize: one wavefront per long row of A (dense-direct engines)
  double *vd;                      // dense-direct engines: vb - vx over all n + m entries (k_vd, before k_pcg_init): the long rows of k_pcg_init then
                                   // gather ONE vector per entry -- they need the residual b - K x~0 only, not b itself
  int     plain_rhs;               // block-direct engines: k_pcg_init leaves b0 = b - S' beta (the right-hand side without the low-rank rows' terms) instead of
  const int *plain_skip;           // the residual b - K x~0: no pass over P.  plain_skip[i] >= 0: row i of A is a coupling row (null: only the folded huge rows are)
  // resident PCG: k_pcg_init also leaves u0 = Minv r0 in the layout of the exchanged vector (position u0map[j] of u0pos), so that
  // the resident launch takes it in with one coalesced sweep instead of a 2-byte-indexed gather (null: not a k_pcg_resident engine)
  const unsigned short *u0map;
  double *u0pos;
  // Slack-like variables eliminated from the linear system (k_elim_refresh): nelim = 0 switches all of it off (rhoe == rho then)
  int     nelim;
  const int *erow, *ecol, *epos;   // [n] row of an eliminated variable (-1: not eliminated); [m] the row's eliminated variable (-1: none), slot of that entry in A.val
  double *rhoe, *ecoef, *edinv, *xte;   // [m] effective rho of the row, A(i, ecol[i]), 1 / D_y, x~ of the row's eliminated variable
  double *D, *Dinv, *E, *Einv;
  double *part_rz, *part_rr, *part_bb, *part_pkp, *part_s0, *part_s1, *part_s2, *part_gam, *part_del;
  const double *fin_rr;  // where k_admm_finalize finds the partials of the last ||r||^2, and how many
  int fin_cnt;
  double *scal;          // reduction outputs (see SC_* below)
  double *part_h;        // huge A rows: [row][workgroup of k_cg_A] partial dots
  State  *st;
  const Params *prm;
#ifdef OSQP_AMD_TIMELINE
  unsigned long long *tl;  // make TIMELINE=1: [0] = count, then one word per kernel start: id << 56 | wall_clock64 (100 MHz)
#endif
};

#ifdef OSQP_AMD_TIMELINE
#define TL_CAP (1 << 20)
#define TL_MARK(c, id) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long k_ = atomicAdd((c).tl, 1ull); \
    if (k_ < TL_CAP - 2) (c).tl[1 + k_] = ((unsigned long long)(id) << 56) | (wall_clock64() & 0x00FFFFFFFFFFFFFFull); } } while (0)
// Stamps inside k_pcg_init / k_admm_finalize (workgroup 0, thread 0): TLK_AT(k, v) reads the clock once v -- the last value a
// flight of loads brings -- is in its register; the kernel's end writes them out as ids base + k (tools/loop_probe.py,
// profiles/iter_kernels_chain_timeline.txt).
// TLK_LAST(k): entry (0) and end (1, after its stores are acknowledged) of the LAST workgroup of the grid, ids base + 20 + k.
#define TLK_N 10
#define TLK_DECL long long tlk_[TLK_N], tll_[2] = {0, 0}; for (int q_ = 0; q_ < TLK_N; ++q_) tlk_[q_] = 0
#define TLK_LAST(k) do { if (k) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) tll_[k] = wall_clock64(); } while (0)
#define TLK_AT(k, v) do { asm volatile("" :: "v"(v)); if (blockIdx.x == 0 && threadIdx.x == 0) tlk_[k] = wall_clock64(); } while (0)
#define TLK_FLUSH(c, base, n) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long k_ = atomicAdd((c).tl, (unsigned long long)(n)); \
    if (k_ + (n) < TL_CAP - 2) for (int q_ = 0; q_ < (n); ++q_) (c).tl[1 + k_ + q_] = ((unsigned long long)((base) + q_) << 56) | ((unsigned long long)tlk_[q_] & 0x00FFFFFFFFFFFFFFull); } \
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) { const unsigned long long k_ = atomicAdd((c).tl, 2ull); \
    if (k_ + 2 < TL_CAP - 2) for (int q_ = 0; q_ < 2; ++q_) (c).tl[1 + k_ + q_] = ((unsigned long long)((base) + 20 + q_) << 56) | ((unsigned long long)tll_[q_] & 0x00FFFFFFFFFFFFFFull); } } while (0)
#else
#define TL_MARK(c, id) do { } while (0)
#define TLK_DECL do { } while (0)
#define TLK_AT(k, v) do { } while (0)
#define TLK_LAST(k) do { } while (0)
#define TLK_FLUSH(c, base, n) do { } while (0)
#endif

enum {  // slots of Ctx::scal (max slots are bit patterns of non-negative doubles)
  SC_PRI_U, SC_PRI_S, SC_Z_U, SC_Z_S, SC_AX_U, SC_AX_S,
  SC_DUA_U, SC_DUA_S, SC_Q_U, SC_Q_S, SC_ATY_U, SC_ATY_S, SC_PX_U, SC_PX_S,
  SC_DYN_U, SC_DYN_S, SC_DXN_U, SC_DXN_S,
  SC_ATDY_U, SC_ATDY_S, SC_PDX_U, SC_PDX_S, SC_ADX_VIOL,
  SC_OBJ, SC_DYLHS, SC_QDX,
  SC_COUNT
};
#define SCI(x) ((x) * 16)   // one 128-byte line per slot: atomics on different slots do not serialise

// ---------------------------------------------------------------------------
// wavefront / workgroup reductions (wave = 64 lanes on gfx950)
// ---------------------------------------------------------------------------
// Sum over the 64 lanes, result in every lane.  Four DPP exchanges inside the 16-lane rows
// (quad xor 1, quad xor 2, half-row mirror, row mirror: no LDS traffic, unlike ds_bpermute
// shuffles), then the four row totals are read out by lane and added in a fixed order.
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_value(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_move<0xB1>(v); v += dpp_move<0x4E>(v); v += dpp_move<0x141>(v); v += dpp_move<0x140>(v);
  return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}

// Sum over the workgroup, result broadcast to every thread.  `red` holds >= 5
// doubles of LDS.  Fixed tree => deterministic.
__device__ __forceinline__ double block_sum(double v, double *red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) red[4] = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return red[4];
}

// Three sums in one pass (one barrier pair instead of three); results broadcast.
// `red` holds >= 16 doubles.
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double *red) {
  a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { red[w] = a; red[4 + w] = b; red[8 + w] = c; }
  __syncthreads();
  a = (red[0] + red[1]) + (red[2] + red[3]);
  b = (red[4] + red[5]) + (red[6] + red[7]);
  c = (red[8] + red[9]) + (red[10] + red[11]);
}

// Re-reduce up to three arrays of per-workgroup partials (same length).
template <int NA>
__device__ __forceinline__ void reduce_parts(const double *a0, const double *a1,
                                             const double *a2, int count,
                                             double *red, double out[NA]) {
  double s0 = 0, s1 = 0, s2 = 0;
  for (int i = threadIdx.x; i < count; i += TB) {
    s0 += a0[i];
    if (NA > 1) s1 += a1[i];
    if (NA > 2) s2 += a2[i];
  }
  if (NA == 1) { out[0] = block_sum(s0, red); return; }
  block_sum3(s0, s1, s2, red);
  out[0] = s0; out[1] = s1;
  if (NA > 2) out[2] = s2;
}

__device__ __forceinline__ void atomic_max_pos(double *slot, double v) {
  // v >= 0: IEEE ordering of non-negative doubles equals unsigned ordering
  atomicMax(reinterpret_cast<unsigned long long *>(slot),
            static_cast<unsigned long long>(__double_as_longlong(v)));
}

__device__ __forceinline__ void block_max_to(double v, double *slot, double *red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) atomic_max_pos(slot, fmax(fmax(red[0], red[1]), fmax(red[2], red[3])));
}

// ---------------------------------------------------------------------------
// CSR-stream building blocks
// ---------------------------------------------------------------------------
// Stage products of the block's entries with one or two input vectors.
// GATHER_P: input 0 is formed on the fly as zz[c] + beta*pold[c] for c < n
// (the PCG direction update fused into the gather).
template <int NV>
__device__ __forceinline__ void stage_products(const DevMat &Mx, const RowBlk b,
                                               const double *in0, const double *in1,
                                               double *l0, double *l1) {
  // all index/value loads of the chunk are issued first, then all gathers, then
  // the LDS writes: up to 2*MAX_CHUNK/TB independent loads in flight per lane
  constexpr int E = MAX_CHUNK / TB;
  const int cnt = b.k1 - b.k0;
  int cc[E]; double vv[E], x0[E], x1[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int k = threadIdx.x + e * TB;
    if (k < cnt) { cc[e] = Mx.col[b.k0 + k]; vv[e] = Mx.val[b.k0 + k]; }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int k = threadIdx.x + e * TB;
    if (k < cnt) { x0[e] = in0[cc[e]]; if (NV == 2) x1[e] = in1[cc[e]]; }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int k = threadIdx.x + e * TB;
    if (k < cnt) { l0[k] = vv[e] * x0[e]; if (NV == 2) l1[k] = vv[e] * x1[e]; }
  }
}

// Sequential (reference-order) sum of one row segment held in LDS.
__device__ __forceinline__ double row_sum(const double *l, int a, int b) {
  double s = 0.0;
  for (int k = a; k < b; ++k) s += l[k];
  return s;
}

// Row segment summed by L adjacent lanes (strided) + xor tree: used by the PCG
// kernels, where the summation order is free; every lane returns the sum.
__device__ __forceinline__ double row_sum_par(const double *l, int a, int b, int lane, int L) {
  double s = 0.0;
  for (int k = a + lane; k < b; k += L) s += l[k];
  // L is a power of two <= 64; the first four butterfly steps stay inside a 16-lane row (DPP)
  if (L >= 2) s += dpp_move<0xB1>(s);
  if (L >= 4) s += dpp_move<0x4E>(s);
  if (L >= 8) s += dpp_move<0x141>(s);
  if (L >= 16) s += dpp_move<0x140>(s);
  if (L >= 32) s += __shfl_xor(s, 16, 64);
  if (L == 64) s += __shfl_xor(s, 32, 64);
  return s;
}
// lanes per row for a block: as many as fit one pass over its rows (1..64)
__device__ __forceinline__ int lanes_for(int nrows) {
  int L = 64;
  while (L > 1 && L * nrows > TB) L >>= 1;
  return L;
}

// A row that does not fit one chunk: whole-workgroup strided reduction of
// sum_k val[k]*in[col[k]] over [ka, kb).  (Summation order differs from the
// sequential reference order; only rows longer than MAX_CHUNK take this path.)
__device__ __forceinline__ double long_row_dot(const DevMat &Mx, int ka, int kb,
                                               const double *in, double *red) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int k = ka + threadIdx.x;
  for (; k + 3 * TB < kb; k += 4 * TB) {          // four independent index/value/gather chains
    const int c0 = Mx.col[k], c1 = Mx.col[k + TB], c2 = Mx.col[k + 2 * TB], c3 = Mx.col[k + 3 * TB];
    const double v0 = Mx.val[k], v1 = Mx.val[k + TB], v2 = Mx.val[k + 2 * TB], v3 = Mx.val[k + 3 * TB];
    s0 += v0 * in[c0]; s1 += v1 * in[c1]; s2 += v2 * in[c2]; s3 += v3 * in[c3];
  }
  for (; k < kb; k += TB) s0 += Mx.val[k] * in[Mx.col[k]];
  return block_sum((s0 + s1) + (s2 + s3), red);
}

// One wavefront per long row; no LDS, no barrier.  The row is taken in chunks of 64 x ROW_U entries: every index and value
// load of a chunk is issued before the first gather, every gather before the first product, lanes beyond the row's end
// are masked (clamped address, zero value).  Measured on the Lasso's pass over A (75 MB with 16-bit column ids): 24.5 us, of which
// 7.7 us are the gathers (16.8 us with the gathered value replaced by a constant: 4.5 TB/s for the stream alone) -- 64 scattered
// 8-byte reads per wave instruction keep the vector L1 busy far longer than their bytes; round 2's form (four chains per lane and
// a one-load-at-a-time remainder loop) took the same time, so neither loop shape is the bound.
#define ROW_U 12
template <bool NARROW, class F>
__device__ __forceinline__ double wave_row_dot_t(const DevMat &Mx, int ka, int kb, F xval) {
  const int lane = threadIdx.x & 63;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int k0 = ka + lane; k0 - lane < kb; k0 += 64 * ROW_U) {
    int cc[ROW_U]; double vv[ROW_U], xx[ROW_U];
#pragma unroll
    for (int q = 0; q < ROW_U; ++q) {
      const int kc = min(k0 + 64 * q, kb - 1);           // (unconditional loads at a clamped address: no branch per entry)
      cc[q] = NARROW ? (int)Mx.col16[kc] : Mx.col[kc];
      vv[q] = Mx.val[kc];
    }
#pragma unroll
    for (int q = 0; q < ROW_U; ++q) xx[q] = xval(cc[q]);
#pragma unroll
    for (int q = 0; q < ROW_U; ++q) if (k0 + 64 * q >= kb) vv[q] = 0.0;
#pragma unroll
    for (int q = 0; q < ROW_U; q += 4) { s0 += vv[q] * xx[q]; s1 += vv[q + 1] * xx[q + 1]; s2 += vv[q + 2] * xx[q + 2]; s3 += vv[q + 3] * xx[q + 3]; }
  }
  return wave_sum((s0 + s1) + (s2 + s3));      // valid in lane 0
}
template <class F>
__device__ __forceinline__ double wave_row_dot(const DevMat &Mx, int ka, int kb, F xval) {
  return Mx.col16 ? wave_row_dot_t<true>(Mx, ka, kb, xval) : wave_row_dot_t<false>(Mx, ka, kb, xval);
}

// y = P_b x_b for one dense diagonal block by the whole workgroup.  P_b is symmetric, so
// y_r = sum_j P_b[j][r] x_j: a lane walks DOWN its columns while the wavefront reads row j contiguously.
// Rows are stored with an even pitch (b rounded up; never a multiple of 32 doubles -- rows that all start on the
// same 256-byte phase camp on a few memory channels: 19.5 instead of 12 us at pitch 128), so one wave instruction
// fetches a whole row with 16-byte loads: lane l owns columns 2l and 2l+1 (measured against 8-byte loads at pitch b and
// against v_mfma_f64_16x16x4_f64 in tools/mfma_dense_probe.hip: 7.65 vs 9.21 vs 9.83 us for the 400 blocks of
// config 5, profiles/r02_mfma_dense_probe.json -- one right-hand side leaves the matrix cores nothing to do).
// Wavefront w takes the rows j = w, w+4, ...; every load of the block is issued before anything is consumed
// (<= 32 rows per wavefront); the four partial vectors meet in LDS.  No index loads, no gathers.
// Returns y_r for r = threadIdx.x < b (0 otherwise); scratch: 5*DENSE_MAX doubles, x_b is left
// in scratch[4*DENSE_MAX ...].  Ends with a barrier; the caller adds one before reusing scratch.
// EARLY: the input element comes out of a chain of dependent loads (k_blk_apply_back).  vmcnt completes in order, so behind the
// 32 block loads every link of the chain would wait for all of them; the chain runs first, alone, and is waited for.
template <bool EARLY = false, class XL>
__device__ __forceinline__ double dense_block_mv_x(const DenseP &dP, const DenseBlk d, XL xload, double *scratch) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double2 *dv = reinterpret_cast<const double2 *>(dP.val + d.off);
  const int hp = d.pitch >> 1;
  double xe = 0.0;
  if (EARLY) {
    if ((int)threadIdx.x < d.b) xe = xload(d.c0 + (int)threadIdx.x);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  double2 v[DENSE_MAX / 4];
#pragma unroll
  for (int q = 0; q < DENSE_MAX / 4; ++q) {
    const int j = w + 4 * q;
    v[q] = (j < d.b && lane < hp) ? dv[(size_t)j * hp + lane] : double2{0.0, 0.0};
  }
  double *xl = scratch + 4 * DENSE_MAX;
  if ((int)threadIdx.x < DENSE_MAX) xl[threadIdx.x] = EARLY ? xe : ((int)threadIdx.x < d.b ? xload(d.c0 + (int)threadIdx.x) : 0.0);
  __syncthreads();
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int q = 0; q < DENSE_MAX / 4; ++q) {
    const double u = xl[min(w + 4 * q, DENSE_MAX - 1)];
    a0 += v[q].x * u; a1 += v[q].y * u;
  }
  scratch[w * DENSE_MAX + 2 * lane] = a0; scratch[w * DENSE_MAX + 2 * lane + 1] = a1;
  __syncthreads();
  const int r = threadIdx.x;
  return r < d.b ? (scratch[r] + scratch[DENSE_MAX + r]) + (scratch[2 * DENSE_MAX + r] + scratch[3 * DENSE_MAX + r]) : 0.0;
}
__device__ __forceinline__ double dense_block_mv(const DenseP &dP, const DenseBlk d, const double *x, double *scratch) {
  return dense_block_mv_x<false>(dP, d, [x](int j) { return x[j]; }, scratch);
}

#define LDS_DECL(NV)                                   \
  __shared__ double lprod[(NV) * MAX_CHUNK];           \
  __shared__ double red[16]
