// batch.hip -- batched OSQP engine for many small QPs with one sparsity pattern
// (MPC-style: BASELINE config 4, 1024 x (n=120, m=240)), gfx950 / MI355X.
//
// One 512-thread workgroup solves one QP from raw data to unscaled solution in
// a single kernel launch; the grid is the batch.  Nothing leaves the CU during
// the ADMM loop:
//   * problem vectors and the (per-QP) scaled matrix values live in LDS;
//   * the KKT solve of update_xz_tilde (reference src/auxil.c:177-183) is a
//     direct one: K = P + sigma I + A' diag(rho) A (n x n, SPD) is formed and
//     inverted in place by Gauss-Jordan with the matrix held in REGISTERS,
//     tiled TR x TC over a 16 x 32 thread grid (n <= 16*TR = 32*TC); every ADMM
//     iteration is then one register-tile GEMV (+ one step of iterative
//     refinement through the sparse operator) -- the per-QP analogue of the
//     reference's factor-once / solve-many LDL^T (qdldl_interface.c:341-376),
//     re-done on every rho update exactly like its re-factorisation (:396-410);
//   * Ruiz equilibration (src/scaling.c:44-156), rho classification
//     (src/auxil.c:76-98), the iteration (src/osqp.c:356-370), residuals and
//     termination incl. infeasibility tests (src/auxil.c:227-512, 681-786), rho
//     adaptation (src/auxil.c:13-74) and solution unscaling (src/scaling.c:177)
//     follow the reference statement by statement, per QP: batch_admm.h, the one copy
//     that the streamed engine (batch_streamed.h, K^-1 in HBM) runs too.  This file adds
//     the tiled engine's LDS layout, its K^-1 (form_K .. rebuild_kinv, TiledK) and the host side.
// Sparsity patterns (shared by the batch) are read from global memory and stay
// L1/L2 resident; per-QP data is read once and written once.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <chrono>
#include <climits>
#include <cmath>
#include <vector>
#include <algorithm>
#include "../../include/osqp_amd.h"
#include "../../include/osqp_amd_batch.h"

#define BT 512            // 8 wavefronts; thread grid 16 (row blocks) x 32 (column blocks)
#define BINF 1e26

#define BCHK(call)                                                              \
  do {                                                                          \
    hipError_t _e = (call);                                                     \
    if (_e != hipSuccess) {                                                     \
      fprintf(stderr, "osqp_amd batch: HIP error %s at %s:%d (%s)\n",           \
              hipGetErrorString(_e), __FILE__, __LINE__, #call);                \
      return -102;                                                              \
    }                                                                           \
  } while (0)

struct BPattern {          // shared sparsity (device pointers)
  int n, m, nnzP, nnzA, nnzPf;
  const int *Pp, *Pi, *Pc;       // triu(P): col ptr, row idx, column of each entry
  const int *Fp, *Fi, *Fk;       // full symmetric P by columns: ptr, row, triu slot
  const int *Ap, *Ai, *Ac;       // A CSC: col ptr, row idx, column of each entry
  const int *Rp, *Rj, *Rk;       // A CSR: row ptr, col idx, CSC slot
  const int *packed;             // all twelve arrays back to back (copied to LDS by the kernel)
};

struct BSettings {
  double rho, sigma, alpha, eps_abs, eps_rel, eps_pinf, eps_dinf, rho_tol, adapt_tol, refine_tol;
  int scaling, adaptive_rho, rho_interval, max_iter, check_termination, scaled_termination,
      warm_start, refine, profile, ablate;
};

struct BIO {               // per-batch arrays (device)
  const double *Px, *Ax;   // shared values, or per-QP values when strideP/strideA != 0
  long long strideP, strideA;
  const double *Q, *L, *U; // [B][n], [B][m], [B][m]
  double *Xs, *Zs, *Ys;    // scaled iterates kept between solves (warm start) [B][..]
  double *Xo, *Yo;         // unscaled solution out
  double *DXo, *DYo;       // certificates out
  double *rho_io;          // current rho per QP (persists between solves)
  // per-QP workspace written by the setup phase (the analogue of the reference's
  // scaled OSQPData + factorisation, kept across solves like its workspace)
  double *Wv;              // [B][nnzP + nnzA] scaled matrix values
  double *Wq, *Wl, *Wu;    // scaled q, l, u
  double *Wd, *We, *Wc;    // D [B][n], E [B][m], c [B]
  double *Wk;              // [B][NP*NP] K^-1 in per-thread tile order
  int    *Wt;              // [B][m] constraint class
  int    *flag;            // [B] BF_* bits
  double *info;            // [B][8]: iter, status, obj, pri, dua, rho_updates, rho_estimate, rho
  const int *order;        // [B] solve phase: workgroup k works on QP order[k] (longest expected first)
};

// The bits of io.flag[qp].  Every writer stores the whole word, so a bit it does not name is cleared.
//   BF_REBUILD  K^-1 no longer matches rho or the row classes.  Set by k_batch_update (a class changed),
//               k_batch_update_rho, the streamed setup (store_workspace) and a streamed member whose rho moved
//               (StreamedK::leave, k_bs_loop's store_solution); cleared by the rebuild: k_bs_invert, or the tiled
//               solve phase, which rebuilds on entry and stores the word without it.
//   BF_REFINE   the member's K solves take a refinement step.  Set or cleared by the probe of admm_loop and stored
//               by store_solution; kept by k_bs_invert and StreamedK::leave; dropped by whoever sets BF_REBUILD alone.
//   BF_OPEN     the refinement verdict is still to be taken.  Set with every new K^-1 (tiled setup and
//               matrix-update phases, k_bs_invert; the tiled solve phase also reads BF_REBUILD as it); cleared
//               by the first probe of admm_loop.
//   BF_NOT_PD   a pivot of K was not positive.  Set by the tiled setup and matrix-update phases and by k_bs_invert,
//               read by the host right after setup or a matrix update, for the members that call touched, and kept
//               there per member (member_not_pd): the next store of the word -- an update_rho, a class-changing
//               update -- clears the bit, not the host's record.
// osqp_amd_batch_rounds counts BF_REFINE; the values are part of what the tests read.
enum { BF_REBUILD = 1, BF_REFINE = 2, BF_OPEN = 4, BF_NOT_PD = 8 };

// ---------------------------------------------------------------------------
// workgroup helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ double b_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ double b_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}
template <int NW>
__device__ __forceinline__ double b_sum(double v, double *red) {
  v = b_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = (red[0] + red[1]) + (red[2] + red[3]);
  if (NW == 8) t += (red[4] + red[5]) + (red[6] + red[7]);
  return t;
}
template <int NW>
__device__ __forceinline__ double b_max(double v, double *red) {
  v = b_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  if (NW == 8) t = fmax(t, fmax(fmax(red[4], red[5]), fmax(red[6], red[7])));
  return t;
}
__device__ __forceinline__ double clip_scale(double v) {
  if (v < 1e-4) v = 1.0;
  if (v > 1e4) v = 1e4;
  return v;
}

// LDS working set of one QP.  n-vectors are NP apart, m-vectors m apart, index
// arrays are one int block: a handful of base pointers instead of ~40.
struct BL {
  double *Pv, *Av;          // scaled matrix values (triu P, CSC A)
  double *nv, *mv;          // n-vector block (stride NP), m-vector block (stride m)
  double *rowk, *colk;      // Gauss-Jordan exchange (2 x 2 x NP)
  double *gp;               // scratch of the fused reductions (256 doubles)
  double *red;
  int *ctype;
  int NP, m;
  // shared sparsity pattern, copied into LDS once per workgroup
  const int *Pp, *Pi, *Pc, *Fp, *Fi, *Fk, *Ap, *Ai, *Ac, *Rp, *Rj, *Rk;
};
#define NV(k) (s.nv + (k) * s.NP)
#define MV(k) (s.mv + (k) * s.m)
#define s_q NV(0)
#define s_x NV(1)
#define s_xt NV(2)
#define s_dx NV(3)
#define s_D NV(4)
#define s_tn NV(5)
#define s_b NV(6)
#define s_l MV(0)
#define s_u MV(1)
#define s_rho MV(2)
#define s_rinv MV(3)
#define s_z MV(4)
#define s_y MV(5)
#define s_ws MV(6)   /* m-scratch: refinement, certificates */
#define s_w MV(7)    /* rho z - y, kept current by the z/y update */
#define s_dy MV(8)
#define s_E MV(9)
#define s_tm MV(10)

// y_i = sum_j A_ij v_j  (row gather through the CSR view of the CSC values)
__device__ __forceinline__ double a_row_dot(const BL &s, const double *v, int i) {
  double acc = 0.0;
  for (int k = s.Rp[i]; k < s.Rp[i + 1]; ++k) acc += s.Av[s.Rk[k]] * v[s.Rj[k]];
  return acc;
}
// (A' v)_j  (column gather)
__device__ __forceinline__ double a_col_dot(const BL &s, const double *v, int j) {
  double acc = 0.0;
  for (int k = s.Ap[j]; k < s.Ap[j + 1]; ++k) acc += s.Av[k] * v[s.Ai[k]];
  return acc;
}
// (P v)_j from the full symmetric pattern
__device__ __forceinline__ double p_row_dot(const BL &s, const double *v, int j) {
  double acc = 0.0;
  for (int k = s.Fp[j]; k < s.Fp[j + 1]; ++k) acc += s.Pv[s.Fk[k]] * v[s.Fi[k]];
  return acc;
}

// ---------------------------------------------------------------------------
// register-tiled K^-1: thread (tr, tc) of a 16 x 16 grid owns rows tr*T.. and
// columns tc*T.. of the (padded) NP x NP matrix, NP = 16*T.
// Sparse dots split over adjacent lanes (the hot loop's rows and columns hold
// 1..6 entries: the serial chain per row, not the flop count, sets the latency).
// Lanes of one quad exchange through DPP quad_perm (no LDS traffic).
__device__ __forceinline__ double quad_xor1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double quad_xor2(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// y_i = sum_j A_ij v_j by the two lanes (l = 0, 1) of a pair; both return the sum
__device__ __forceinline__ double a_row_dot2(const BL &s, const double *v, int i, int l) {
  double acc = 0.0;
  for (int k = s.Rp[i] + l; k < s.Rp[i + 1]; k += 2) acc += s.Av[s.Rk[k]] * v[s.Rj[k]];
  return acc + quad_xor1(acc);
}
// (A' v)_j by the four lanes (l = 0..3) of a quad; all return the sum
__device__ __forceinline__ double a_col_dot4(const BL &s, const double *v, int j, int l) {
  double acc = 0.0;
  for (int k = s.Ap[j] + l; k < s.Ap[j + 1]; k += 4) acc += s.Av[k] * v[s.Ai[k]];
  acc += quad_xor1(acc);
  return acc + quad_xor2(acc);
}

// (P v)_j from the full symmetric pattern by the four lanes of a quad; all return the sum
__device__ __forceinline__ double p_row_dot4(const BL &s, const double *v, int j, int l) {
  double acc = 0.0;
  for (int k = s.Fp[j] + l; k < s.Fp[j + 1]; k += 4) acc += s.Pv[s.Fk[k]] * v[s.Fi[k]];
  acc += quad_xor1(acc);
  return acc + quad_xor2(acc);
}
// Wavefront reductions whose result is uniform: two quad exchanges, two mirror steps inside
// the 16-lane row (DPP, no LDS), then the four row totals are read out by lane.
__device__ __forceinline__ double dpp_mirror(double v, bool half) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  if (half) { lo = __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, true); }
  else      { lo = __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, true); }
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_value(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double wave_all_max(double v) {
  v = fmax(v, quad_xor1(v)); v = fmax(v, quad_xor2(v));
  v = fmax(v, dpp_mirror(v, true)); v = fmax(v, dpp_mirror(v, false));
  return fmax(fmax(lane_value(v, 0), lane_value(v, 16)), fmax(lane_value(v, 32), lane_value(v, 48)));
}
__device__ __forceinline__ double wave_all_sum(double v) {
  v += quad_xor1(v); v += quad_xor2(v);
  v += dpp_mirror(v, true); v += dpp_mirror(v, false);
  return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}
// NMAX maxima and NSUM sums over the workgroup with two barriers; the combined values are
// left in buf[NW*(NMAX+NSUM) ...] (maxima first).  buf: >= (NW+1)*(NMAX+NSUM) doubles of LDS.
template <int NW, int NMAX, int NSUM>
__device__ __forceinline__ void b_reduce_many(double (&mx)[NMAX], double (&sm)[NSUM], double *buf) {
  constexpr int K = NMAX + NSUM;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NMAX; ++k) { const double r = wave_all_max(mx[k]); if (lane == 0) buf[w * K + k] = r; }
#pragma unroll
  for (int k = 0; k < NSUM; ++k) { const double r = wave_all_sum(sm[k]); if (lane == 0) buf[w * K + NMAX + k] = r; }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    const int k = threadIdx.x;
    double r;
    if (k < NMAX) { r = buf[k]; for (int q = 1; q < NW; ++q) r = fmax(r, buf[q * K + k]); }
    else {
      r = (buf[k] + buf[K + k]) + (buf[2 * K + k] + buf[3 * K + k]);
      if (NW == 8) r += (buf[4 * K + k] + buf[5 * K + k]) + (buf[6 * K + k] + buf[7 * K + k]);
    }
    buf[NW * K + k] = r;
  }
  __syncthreads();
}

#include "batch_admm.h"

// ---------------------------------------------------------------------------
template <int TR, int TC, int GC>
__device__ __forceinline__ void form_K(double (&a)[TR][TC], int n, const BL &s, double sigma) {
  const int tr = threadIdx.x / GC, tc = threadIdx.x % GC;
  const double *rho = s_rho;
#pragma unroll 1
  for (int r = 0; r < TR; ++r) {
    double v[TC];
#pragma unroll 1
    for (int c = 0; c < TC; ++c) {
      const int i = tr * TR + r, j = tc * TC + c;
      double acc = 0.0;
      if (i < n && j < n) {
        // P_ij from the upper triangle: column max(i,j), row min(i,j)
        const int cj = i > j ? i : j, ri = i > j ? j : i;
        for (int k = s.Pp[cj]; k < s.Pp[cj + 1]; ++k) if (s.Pi[k] == ri) acc += s.Pv[k];
        if (i == j) acc += sigma;
        // sum_t rho_t A_ti A_tj : merge of the two sorted columns
        int ka = s.Ap[i], kb = s.Ap[j];
        const int ea = s.Ap[i + 1], eb = s.Ap[j + 1];
        while (ka < ea && kb < eb) {
          const int ra = s.Ai[ka], rb = s.Ai[kb];
          if (ra == rb) { acc += rho[ra] * s.Av[ka] * s.Av[kb]; ++ka; ++kb; }
          else if (ra < rb) ++ka; else ++kb;
        }
      } else if (i == j) acc = 1.0;    // identity padding keeps the inverse well defined
#pragma unroll
      for (int cc = 0; cc < TC; ++cc) if (cc == c) v[cc] = acc;
    }
#pragma unroll
    for (int rr = 0; rr < TR; ++rr)
#pragma unroll
      for (int cc = 0; cc < TC; ++cc) if (rr == r) a[rr][cc] = v[cc];
  }
}

// In-place Gauss-Jordan inversion without pivoting (K is SPD).  One barrier per
// pivot: the pivot row / column are exchanged through double-buffered LDS.
// Returns true (uniformly: every lane reads every pivot) when a pivot was not
// positive -- NaN included.  The pivots are the D of K = L D L', so all of them
// are positive exactly when K is positive definite (Sylvester); the setup phase
// turns this into OSQP_NONCVX_ERROR, the solve phase ignores it.
template <int TR, int TC, int GC>
__device__ __forceinline__ bool invert_tiles(double (&a)[TR][TC], const BL &s, int n) {
  // The pivot loop is unrolled by TR (a multiple of TC) so that the pivot's
  // position inside a tile (ko, kco) is a compile-time constant: the register
  // tile is only ever indexed statically.  Per pivot: owners publish row k and
  // column k to LDS, one barrier, one FMA per tile element, then the owners of
  // row k / column k overwrite their strip with the Gauss-Jordan special cases.
  static_assert(TR % TC == 0, "tile shape");
  constexpr int NP = 16 * TR;
  const int tr = threadIdx.x / GC, tc = threadIdx.x % GC;
  const int nkb = (n + TR - 1) / TR;    // padded rows/columns are identity: nothing to eliminate
  bool notpd = false;
#pragma unroll 1
  for (int kb = 0; kb < nkb; ++kb) {
#pragma unroll
    for (int ko = 0; ko < TR; ++ko) {
      const int k = kb * TR + ko;
      const int kco = ko % TC;               // static after unrolling
      const int kc = k / TC;                 // column block that owns column k
      double *rowk = s.rowk + (k & 1) * NP, *colk = s.colk + (k & 1) * NP;
      if (tr == kb) {
#pragma unroll
        for (int c = 0; c < TC; ++c) rowk[c * GC + tc] = a[ko][c];   // [c][tc]: lane stride 8 B
      }
      if (tc == kc) {
#pragma unroll
        for (int r = 0; r < TR; ++r) colk[tr * TR + r] = a[r][kco];
      }
      __syncthreads();
      const double akk = rowk[kco * GC + kc];
      notpd |= !(akk > 0.0);
      const double piv = 1.0 / akk;
      double rk[TC];
#pragma unroll
      for (int c = 0; c < TC; ++c) rk[c] = rowk[c * GC + tc] * piv;
#pragma unroll
      for (int r = 0; r < TR; ++r) {
        const double ci = colk[tr * TR + r];
#pragma unroll
        for (int c = 0; c < TC; ++c) a[r][c] = __builtin_fma(-ci, rk[c], a[r][c]);
      }
      if (tc == kc) {          // column k: a_ik <- -a_ik / a_kk
#pragma unroll
        for (int r = 0; r < TR; ++r) a[r][kco] = 0.0 - colk[tr * TR + r] * piv;
      }
      if (tr == kb) {          // row k: a_kj <- a_kj / a_kk, a_kk <- 1 / a_kk
#pragma unroll
        for (int c = 0; c < TC; ++c) a[ko][c] = (tc * TC + c == k) ? piv : rk[c];
      }
    }
  }
  __syncthreads();
  return notpd;
}

// K^-1 for the per-iteration GEMV lives in a second register layout ("G"): eight adjacent
// lanes share a group of RG = NP/64 rows, lane q of the eight holds the columns
// {16k + 2q, 16k + 2q + 1}.  The eight partial sums of a row meet through three DPP exchanges
// (no LDS round trip, one barrier per GEMV), and for a fixed k the eight lanes read 128
// contiguous bytes of the input vector.  The Gauss-Jordan tiles (layout "I") are converted
// once per inversion through the per-QP K^-1 array in HBM, which is stored in G order.
template <int NP> struct GL { static constexpr int RG = NP / 64, CG = NP / 8; };

// out_i = sum_j Kinv_ij in_j ; in / out are LDS vectors of length >= NP
template <int NP>
__device__ __forceinline__ void tile_gemv(const double (&ag)[GL<NP>::RG][GL<NP>::CG], const double *in, double *out) {
  constexpr int RG = GL<NP>::RG, CG = GL<NP>::CG;
  const int g = threadIdx.x >> 3, q = threadIdx.x & 7;
  double acc[RG];
#pragma unroll
  for (int r = 0; r < RG; ++r) acc[r] = 0.0;
#pragma unroll
  for (int k = 0; k < CG / 2; ++k) {
    const double2 bv = *reinterpret_cast<const double2 *>(in + 16 * k + 2 * q);
#pragma unroll
    for (int r = 0; r < RG; ++r) {
      acc[r] = __builtin_fma(ag[r][2 * k], bv.x, acc[r]);
      acc[r] = __builtin_fma(ag[r][2 * k + 1], bv.y, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < RG; ++r) {
    double v = acc[r];
    v += quad_xor1(v); v += quad_xor2(v); v += dpp_mirror(v, true);
    if (q == 0) out[g * RG + r] = v;
  }
  __syncthreads();
}
// element (i, j) of K^-1 -> position in the per-QP array (G order, slot-major so that the
// loads of the solve phase are coalesced).  Host and device: osqp_amd_batch_member un-permutes with it.
template <int NP, int NT>
__host__ __device__ __forceinline__ int g_index(int i, int j) {
  constexpr int RG = GL<NP>::RG, CG = GL<NP>::CG;
  const int tg = (i / RG) * 8 + ((j & 15) >> 1);
  const int sg = (i % RG) * CG + ((j >> 4) << 1) + (j & 1);
  return sg * NT + tg;
}
template <int TR, int TC, int GC>
__device__ __forceinline__ void store_kinv(const double (&a)[TR][TC], double *Wk) {
  constexpr int NP = 16 * TR, NT = 16 * GC;
  const int tr = threadIdx.x / GC, tc = threadIdx.x % GC;
#pragma unroll
  for (int r = 0; r < TR; ++r)
#pragma unroll
    for (int c = 0; c < TC; ++c) Wk[g_index<NP, NT>(tr * TR + r, tc * TC + c)] = a[r][c];
}
// (agent-scope loads: inside the loop the array was just rewritten by other lanes of this workgroup)
template <int NP, int NT>
__device__ __forceinline__ void load_kinv(double (&ag)[GL<NP>::RG][GL<NP>::CG], double *Wk) {
#pragma unroll
  for (int r = 0; r < GL<NP>::RG; ++r)
#pragma unroll
    for (int c = 0; c < GL<NP>::CG; ++c)
      ag[r][c] = __hip_atomic_load(Wk + (r * GL<NP>::CG + c) * NT + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// form K, invert it in the Gauss-Jordan tile layout and leave it in HBM in GEMV order;
// true when K was not positive definite (invert_tiles)
template <int TR, int TC, int GC>
__device__ __forceinline__ bool rebuild_kinv(int n, const BL &s, double sigma, double *Wk) {
  double a[TR][TC];
  form_K<TR, TC, GC>(a, n, s, sigma);
  const bool notpd = invert_tiles<TR, TC, GC>(a, s, n);
  store_kinv<TR, TC, GC>(a, Wk);
  __threadfence();               // the stores are re-read by other lanes of this workgroup
  __syncthreads();
  return notpd;
}

// ---------------------------------------------------------------------------
// the tiled engine: LDS layout, its K solve, the kernel
// ---------------------------------------------------------------------------
// LDS working set: matrix values (+1: the n-vectors are read 16 bytes at a time by the GEMV), 7 n-vectors of
// NP, 11 m-vectors, the Gauss-Jordan exchange (4 NP), 64 + 256 reduction doubles, m class ints (+4) and the
// twelve pattern arrays.
__host__ __device__ __forceinline__ size_t bt_lds_bytes(const BPattern &p, int NP) {
  const size_t b = sizeof(double) * ((size_t)p.nnzP + p.nnzA + 1 + 7 * NP + 11 * (size_t)p.m + 4 * NP + 64 + 256) +
                   sizeof(int) * ((size_t)p.m + 4 + 3 * ((size_t)p.n + 1) + 2 * (size_t)p.nnzP + 2 * (size_t)p.nnzPf +
                                  4 * (size_t)p.nnzA + (size_t)p.m + 1);
  return (b + 15) & ~(size_t)15;
}
// (also copies the shared pattern into LDS: visible after the next barrier)
template <int NP, int NT>
__device__ __forceinline__ BL bt_layout(double *lds, const BPattern &p) {
  BL s;
  const int n = p.n, m = p.m;
  double *w = lds;
  s.NP = NP; s.m = m;
  s.Pv = w; w += p.nnzP; s.Av = w; w += p.nnzA;
  w += (p.nnzP + p.nnzA) & 1;
  s.nv = w; w += 7 * NP; s.mv = w; w += 11 * m;
  s.rowk = w; w += 2 * NP; s.colk = w; w += 2 * NP; s.red = w; w += 64; s.gp = w; w += 256;
  int *iw = reinterpret_cast<int *>(w);
  s.ctype = iw; iw += m;
  int *ib = iw;
  s.Pp = iw; iw += n + 1; s.Pi = iw; iw += p.nnzP; s.Pc = iw; iw += p.nnzP;
  s.Fp = iw; iw += n + 1; s.Fi = iw; iw += p.nnzPf; s.Fk = iw; iw += p.nnzPf;
  s.Ap = iw; iw += n + 1; s.Ai = iw; iw += p.nnzA; s.Ac = iw; iw += p.nnzA;
  s.Rp = iw; iw += m + 1; s.Rj = iw; iw += p.nnzA; s.Rk = iw; iw += p.nnzA;
  // the host packs the twelve index arrays back to back in this order
  const int tot = (int)(iw - ib);
  for (int k = threadIdx.x; k < tot; k += NT) ib[k] = p.packed[k];
  return s;
}

// K^-1 in registers.  A rho move re-forms and re-inverts K inside the loop, exactly like the reference's
// re-factorisation, and the refinement verdict is taken again.
template <int TR, int TC, int GC>
struct TiledK {
  static constexpr int NP = 16 * TR, NT = 16 * GC;
  double ag[GL<NP>::RG][GL<NP>::CG];     // K^-1 in the GEMV layout
  double *Wk;
  __device__ __forceinline__ void solve(const BL &, const double *in, double *out) const { tile_gemv<NP>(ag, in, out); }
  __device__ __forceinline__ bool leave(const BL &, const BPattern &, const BSettings &, const BIO &, long long, const BA &) const { return false; }
  __device__ __forceinline__ void rho_moved(const BL &s, const BPattern &p, const BSettings &st, BA &a) {
    rebuild_kinv<TR, TC, GC>(p.n, s, st.sigma, Wk);
    load_kinv<NP, NT>(ag, Wk);
    a.check_pending = true;
  }
};

// PH = 0: setup phase (scale, classify, build K^-1, store the workspace);
// PH = 1: solve phase (load the workspace, ADMM loop, store the solution);
// PH = 2: matrix-update phase (osqp_update_P_A, osqp.c:1171-1279): the setup phase on the current raw data with
//         the member's row classes, rho and iterates kept; one workgroup per listed member with `list` (qp = list[blockIdx.x],
//         osqp_amd_batch_update_matrices_members), which no other phase reads;
// PH = 3: the solve phase of a solve with a time limit (admm_loop<.., CLOCK = true>): an instantiation of its own, so
//         that PH = 1 -- 256 registers and spills at tile 8 -- carries no clock statement.  clk: the clock words (PH = 3).
#ifndef BATCH_WAVES_PER_SIMD
#define BATCH_WAVES_PER_SIMD 2   // 4 (two workgroups per CU, <= 128 registers) was measured slower: spills lengthen the slowest QP
#endif
template <int TR, int TC, int GC, int PH>
__global__ void __launch_bounds__(16 * GC, PH == 1 || PH == 3 ? BATCH_WAVES_PER_SIMD : 2)
k_batch_solve(BPattern p, BSettings st, BIO io, unsigned long long *clk, const int *list) {
  constexpr int NP = 16 * TR, NT = 16 * GC;
  static_assert(GC * TC == NP, "tile shape");
  static_assert(4 * NP <= NT, "the GEMV reduction and the column dots use four lanes per row/column");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const long long qp = ((PH == 1 || PH == 3) && io.order) ? io.order[blockIdx.x]
                       : (PH == 2 && list) ? list[blockIdx.x] : (int)blockIdx.x;
  const BL s = bt_layout<NP, NT>(lds, p);
  double *Wk = io.Wk + qp * (long long)(NP * NP);
  BDbg dbg;
  DBG(dbg.tstamp[0] = wall_clock64(); dbg.cyc0 = clock64();)
  clear_vectors<NT>(s);
  if (PH == 0) {
    load_problem<NT, false>(s, p, io, qp);
    const double cs = ruiz_scale<NT, false>(s, p, st);
    const double rho = fmin(fmax(st.rho, 1e-6), 1e6);
    set_rho_vectors<NT>(s, rho);
    __syncthreads();
    const bool notpd = rebuild_kinv<TR, TC, GC>(p.n, s, st.sigma, Wk);
    store_workspace<NT, false>(s, p, io, qp, cs, rho, notpd ? BF_OPEN | BF_NOT_PD : BF_OPEN);
    return;
  }
  if (PH == 2) {
    load_problem<NT, false>(s, p, io, qp);
    load_classes<NT>(s, p, io, qp);
    const double cs = ruiz_scale<NT, false, false>(s, p, st);
    const double rho = fmin(fmax(io.rho_io[qp], 1e-6), 1e6);
    __syncthreads();
    set_rho_vectors<NT>(s, rho);
    __syncthreads();
    const bool notpd = rebuild_kinv<TR, TC, GC>(p.n, s, st.sigma, Wk);
    store_workspace<NT, false, false>(s, p, io, qp, cs, rho, notpd ? BF_OPEN | BF_NOT_PD : BF_OPEN);
    return;
  }
  TiledK<TR, TC, GC> eng;
  eng.Wk = Wk;
  BA a;
  a.cs = load_workspace<NT, false>(s, p, io, qp);
  DBG(dbg.tstamp[1] = dbg.tstamp[2] = wall_clock64();)
  a.rho = fmin(fmax(io.rho_io[qp], 1e-6), 1e6);
  init_iterates<NT>(s, p, io, qp, a.rho, st.warm_start);
  DBG(dbg.tstamp[3] = wall_clock64();)
  // refinement is applied only to QPs whose K^-1 left a relative residual above refine_tol in the
  // first solves after it was (re)built; the verdict is kept in BF_REFINE
  const int qflag = io.flag[qp];
  a.need_refine = (qflag & BF_REFINE) != 0;
  a.check_pending = (qflag & (BF_REBUILD | BF_OPEN)) != 0;
  if (qflag & BF_REBUILD) rebuild_kinv<TR, TC, GC>(p.n, s, st.sigma, Wk);   // (the verdict on K is dropped: not covered in-loop)
  DBG(dbg.tstamp[4] = wall_clock64();)
  load_kinv<NP, NT>(eng.ag, Wk);
  DBG(dbg.tstamp[5] = wall_clock64();)
  admm_loop<NT, true, PH == 3>(s, p, st, io, qp, a, 0, eng, dbg, clk);
  DBG(dbg.tstamp[6] = wall_clock64();)
  store_solution<NT>(s, p, st, io, qp, a, a.check_pending ? BF_OPEN : (a.need_refine ? BF_REFINE : 0));
  DBG(if (st.profile && tid == 0) {
    const int n = p.n;
    dbg.tstamp[7] = wall_clock64();
    for (int k = 0; k < 8; ++k) io.DXo[qp * n + k] = (double)(dbg.tstamp[k] - dbg.tstamp[0]);
    for (int k = 0; k < 4; ++k) io.DXo[qp * n + 8 + k] = (double)dbg.pacc[k];
    io.DXo[qp * n + 12] = (double)(clock64() - dbg.cyc0);
    io.DXo[qp * n + 13] = (double)dbg.tstamp[0]; io.DXo[qp * n + 14] = (double)dbg.tstamp[7];
  })
  if (tid == 0 && io.rho_io) io.rho_io[qp] = a.rho;
}

// the clamp of BatchOSQP.update (np.maximum(L, -OSQP_INFTY), np.minimum(U, OSQP_INFTY)); a NaN stays a NaN
__device__ __forceinline__ double clamp_lower(double v) { return v < -OSQP_INFTY ? -OSQP_INFTY : v; }
__device__ __forceinline__ double clamp_upper(double v) { return v > OSQP_INFTY ? OSQP_INFTY : v; }

#define BD_NT 256
#define BD_MAX_BLOCKS 1024
// *bad += the number of k in [0, cnt) with clamp(L[k]) > clamp(U[k]) (osqp.c:815-822 for every QP).  Grid-stride;
// the workgroup's count meets in LDS and at most one atomicAdd per workgroup leaves it.
__global__ void __launch_bounds__(BD_NT) k_batch_check_bounds(long long cnt, const double *L, const double *U, int *bad) {
  __shared__ int wsum[BD_NT / 64];
  int c = 0;
  for (long long k = (long long)blockIdx.x * BD_NT + threadIdx.x; k < cnt; k += (long long)gridDim.x * BD_NT)
    c += clamp_lower(L[k]) > clamp_upper(U[k]) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    if (t) atomicAdd(bad, t);
  }
}

// osqp_update_lin_cost / osqp_update_bounds for every QP of the batch
// (src/osqp.c:765-846): new raw vectors are scaled with the stored D, E, c; rows
// are re-classified and a changed class requests a rebuild of K^-1
// (update_rho_vec, src/auxil.c:100-142).
// One workgroup per member of the call: qp = list[blockIdx.x], or blockIdx.x itself without a list; Q, L, U hold that
// member's new row at blockIdx.x.  With rawQ, rawL, rawU (every form of osqp_amd_batch_update) the raw row -- clamped to
// +-OSQP_INFTY where clamp is set, the device route's -- goes into the handle's raw arrays first; without them (setup of
// the common-K engine) Q, L, U are those arrays.
__global__ void __launch_bounds__(256) k_batch_update(int n, int m, BIO io, const double *Q, const double *L,
                                                      const double *U, double rho_tol, const int *list, double *rawQ,
                                                      double *rawL, double *rawU, int clamp) {
  const long long qp = list ? list[blockIdx.x] : blockIdx.x, src = blockIdx.x;
  __shared__ int changed;
  if (threadIdx.x == 0) changed = 0;
  __syncthreads();
  if (Q) {
    const double c = io.Wc[qp];
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
      const double v = Q[src * n + j];
      if (rawQ) rawQ[qp * n + j] = v;
      io.Wq[qp * n + j] = (v * io.Wd[qp * n + j]) * c;
    }
  }
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    const double e = io.We[qp * m + i];
    if (L) {
      double v = L[src * m + i];
      if (rawL) { if (clamp) v = clamp_lower(v); rawL[qp * m + i] = v; }
      io.Wl[qp * m + i] = v * e;
    }
    if (U) {
      double v = U[src * m + i];
      if (rawU) { if (clamp) v = clamp_upper(v); rawU[qp * m + i] = v; }
      io.Wu[qp * m + i] = v * e;
    }
    if (L || U) {
      const int t = row_class(io.Wl[qp * m + i], io.Wu[qp * m + i], rho_tol);
      if (t != io.Wt[qp * m + i]) { io.Wt[qp * m + i] = t; changed = 1; }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && changed) io.flag[qp] = BF_REBUILD;   // the refinement verdict is re-taken after the rebuild
  if (threadIdx.x == 0) io.info[qp * 8 + 5] = 0.0;      // reset_info: rho_updates (src/auxil.c:647)
}

// Rows of a member-major array into a compact one: dst[k][j] = src[list[k]][j], k < count, j < width.  One thread per
// (k, j), j fastest, as k_batch_scatter: the reads run along a member's row and the writes are contiguous.
__global__ void __launch_bounds__(256) k_batch_gather(double *dst, const double *src, long long width, const int *list,
                                                      long long count) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= width * count) return;
  const long long k = t / width, j = t - k * width;
  dst[t] = src[(long long)list[k] * width + j];
}

// New matrix values into the raw value array of the batch: slot idx[k] (k itself when idx is null) of every member
// receives src[k] (shared values) or src[member][k].  dstride = 0: the raw array is shared and so is src.  One
// thread per (member, k), k fastest: the reads are coalesced, and so are the writes of a full update.
// list (null: every member): `members` listed ones, row b of src -- or its one row -- goes to member list[b].
__global__ void __launch_bounds__(256) k_batch_scatter(double *dst, long long dstride, const double *src, long long sstride,
                                                       const int *idx, long long cnt, long long members, const int *list) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= cnt * members) return;
  const long long b = t / cnt, k = t - b * cnt;
  dst[(list ? list[b] : b) * dstride + (idx ? idx[k] : k)] = src[b * sstride + k];
}

// osqp_update_rho for every QP (osqp.c:1281-1332): the clipped value, and a rebuild of K^-1 at the start of the next
// solve, after which the refinement verdict is re-taken (as after a class change in k_batch_update)
// list (null: every member): the B listed members only, rho compact (rho[k] for member list[k]).
__global__ void __launch_bounds__(256) k_batch_update_rho(long long B, BIO io, const double *rho, int per_member,
                                                          const int *list) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= B) return;
  const long long qp = list ? list[k] : k;
  io.rho_io[qp] = fmin(fmax(rho[per_member ? k : 0], 1e-6), 1e6);
  io.flag[qp] = BF_REBUILD;
}

// osqp_warm_start / _x / _y for every QP (osqp.c:942-1010): x = D^-1 x, z = A x with the scaled A, y = c E^-1 y.
// One workgroup per QP; the scaled x is handed from its writers to the row sums through LDS.
#define BW_MAX_N 1024      // largest n of either engine
// list (null: every member): one workgroup per listed member, X and Y compact (row blockIdx.x).
__global__ void __launch_bounds__(256) k_batch_warm_start(BPattern p, BIO io, const double *X, const double *Y, const int *list) {
  __shared__ double xs[BW_MAX_N];
  const long long qp = list ? list[blockIdx.x] : blockIdx.x, src = blockIdx.x;
  const int n = p.n, m = p.m;
  if (X) {
    for (int j = threadIdx.x; j < n; j += 256) {
      const double v = (1.0 / io.Wd[qp * n + j]) * X[src * n + j];
      xs[j] = v; io.Xs[qp * n + j] = v;
    }
    __syncthreads();
    const double *Av = io.Wv + qp * ((long long)p.nnzP + p.nnzA) + p.nnzP;
    for (int i = threadIdx.x; i < m; i += 256) {
      double acc = 0.0;
      for (int k = p.Rp[i]; k < p.Rp[i + 1]; ++k) acc += Av[p.Rk[k]] * xs[p.Rj[k]];
      io.Zs[qp * m + i] = acc;
    }
  }
  if (Y) {
    const double c = io.Wc[qp];
    for (int i = threadIdx.x; i < m; i += 256) io.Ys[qp * m + i] = ((1.0 / io.We[qp * m + i]) * Y[src * m + i]) * c;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// Dispatch order of the next solve: QPs sorted by the iteration count of the solve
// that just finished, longest first.  Workgroups are handed to CUs in blockIdx
// order as CUs free up, so this is longest-processing-time-first list scheduling
// and the batch no longer ends on a late-started slow QP.  (The order only moves
// work between CUs; every QP's arithmetic is untouched, so the order inside a bucket
// may vary from run to run.)  Counting sort in one workgroup: 1024 buckets over
// [0, max iterations], histogram, exclusive scan, scatter through bucket cursors.
__global__ void __launch_bounds__(1024) k_batch_order(long long B, const double *info, int *order) {
  __shared__ int hist[1024], wmax[16];
  const int tid = threadIdx.x;
  int mx = 1;
  for (long long b = tid; b < B; b += 1024) mx = max(mx, (int)info[b * 8]);
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_down(mx, o, 64));
  hist[tid] = 0;
  if ((tid & 63) == 0) wmax[tid >> 6] = mx;
  __syncthreads();
  mx = wmax[0];
  for (int k = 1; k < 16; ++k) mx = max(mx, wmax[k]);
  const double sc = 1023.0 / (double)mx;
  for (long long b = tid; b < B; b += 1024) atomicAdd(&hist[1023 - (int)(info[b * 8] * sc)], 1);
  __syncthreads();
  // exclusive scan of the 1024 bucket counts (bucket 0 = most iterations): wavefront scans + 16 totals
  const int cnt = hist[tid];
  int incl = cnt;
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl += t; }
  if ((tid & 63) == 63) wmax[tid >> 6] = incl;
  __syncthreads();
  int base = incl - cnt;
  for (int k = 0; k < (tid >> 6); ++k) base += wmax[k];
  __syncthreads();
  hist[tid] = base;                         // now the bucket's write cursor
  __syncthreads();
  for (long long b = tid; b < B; b += 1024) order[atomicAdd(&hist[1023 - (int)(info[b * 8] * sc)], 1)] = (int)b;
}

// The clock of a solve with a time limit, one thread each on the handle's stream: k_clock_start, first in the solve,
// writes the absolute deadline, the start stamp and a zero count of cut members; k_clock_end, after the last loop
// kernel, the end stamp.
__global__ void k_clock_start(unsigned long long *clk, unsigned long long ticks) {
  const unsigned long long now = wall_clock64();
  clk[CK_DEADLINE] = now + ticks; clk[CK_START] = now; clk[CK_END] = now; clk[CK_CUT] = 0;
}
__global__ void k_clock_end(unsigned long long *clk) { clk[CK_END] = wall_clock64(); }

#include "batch_streamed.h"
#include "batch_common.h"
#include "batch_polish.h"
#include "batch_adjoint.h"
#include "batch_tangent.h"
#include "batch_common_kkt.h"
#include "batch_verify.h"

struct osqp_amd_batch {
  int engine = OSQP_AMD_BATCH_TILED;
  int NPs = 0;              // streamed engine: padded order of K^-1 (n rounded up to 32)
  BSPattern kpat{};         // streamed engine: pattern of K for k_bs_form
  int *d_count = nullptr, *d_list[2] = {nullptr, nullptr};   // streamed engine: rebuild requests of a round
  int last_rounds = 0;
  // common-K engine (batch_common.h): one K^-1 (io.Wk), one rho and one refinement verdict, kept on the host
  BCT ct{};
  double bc_rho = 0.0;      // the batch's rho
  double *bc_wk2 = nullptr; // the second NP x NP buffer of the inversion (k_bc_pivot); io.Wk and it swap roles
  double *bc_qhat = nullptr; // [n] q^ of a model update (k_bc_qhat), allocated by the first one
  int bc_pivot2 = 1;        // OSQP_AMD_BATCH_MODEL_PIVOT2 (0: a model update inverts K, then H, with k_bc_pivot)
  bool bc_rebuild = false;  // K^-1 no longer matches rho or the row classes
  bool bc_refine = false;   // the K^-1 solves take the refinement step (the verdict of the last probe)
  bool bc_open = false;     // the verdict is to be taken again: K^-1 is new
  std::vector<char> bc_probed;   // [B] the member was listed in a solve that probed this K^-1 (cleared with every new K^-1)
  int bc_pack = 1;          // OSQP_AMD_BATCH_COMMON_PACK (0: the columns of a solve stay where they started)
  int bc_cols[3] = {0, 0, 0};   // of the last solve: columns it started with, packs, columns in use when it ended
  BKkt bk{};                // the shared KKT pieces (batch_common_kkt.h), built by osqp_amd_batch_common_kkt
  int device = 0, tile = 8, threads = 512;
  long long B = 0;
  int n = 0, m = 0, nnzP = 0, nnzA = 0;
  hipStream_t stream = nullptr;
  BPattern pat{};
  BSettings st{};
  BIO io{};
  std::vector<void *> allocs;
  size_t lds_bytes = 0;
  int solves = 0;
  std::vector<double> h_info;
  double *dQ = nullptr, *dL = nullptr, *dU = nullptr;   // the raw q, l, u (io.Q, io.L, io.U), written by updates
  double *dPx = nullptr, *dAx = nullptr;                // the raw matrix values (io.Px, io.Ax), written by matrix updates
  double *d_vals = nullptr, *d_rho = nullptr;           // staging of update_matrices / update_rho / warm_start
  int *d_idx = nullptr;
  size_t vals_cap = 0, idx_cap = 0;
  bool noncvx = false;      // some member's K is indefinite since its last matrix update: solve refuses
  std::vector<char> member_not_pd;   // ... per member: written by a matrix update for the members it re-inverts, and by nothing else
  int *d_order = nullptr;   // dispatch order for the next solve (k_batch_order)
  int lpt = 1;
  // the limits of a solve (osqp_amd_batch_solve_limited)
  unsigned long long *d_clock = nullptr;   // [CK_COUNT_] the clock words, allocated by the first solve with a time limit
  int clock_khz = 0;        // hipDeviceAttributeWallClockRate, read with them
  double report[4] = {0, 0, 0, 0};   // osqp_amd_batch_solve_report of the last solve
  std::chrono::steady_clock::time_point clock_t0;   // when k_clock_start was enqueued (the common-K engine's clock)
  // polish (batch_polish.h)
  double pol_delta = 0.0;   // settings->delta
  int pol_refine = 0;       // settings->polish_refine_iter
  size_t pol_cap = 0;       // largest KKT buffer in bytes (OSQP_AMD_BATCH_POLISH_CAP_BYTES)
  size_t pol_bytes = 0;     // size of pol.K as allocated
  BPol pol{};
  int *d_plist = nullptr;   // [B] the solved members, in index order
  bool solved = false;      // the iterates and info on the device are those of a solve of the current problem
  std::vector<char> member_solved;   // ... per member (a solve of chosen members sets its own); solved = all of them
  bool polished = false;    // ... and polish has already run on them
  std::vector<char> member_polished;   // polish has run on the member since its last solve, by osqp_amd_batch_polish or _polish_members
  // the _members calls: the call's list on the device, uploaded once per call, and each listed member's place in it
  int *d_mlist = nullptr, *d_mpos = nullptr;   // [B], [B]
  // adjoint and tangent (batch_adjoint.h, batch_tangent.h): the one staging set of the derivative calls.  Each of
  // them returns with the stream synchronised, so nothing is queued on it between calls.  in, out and mat grow with
  // ncot / ndir (freed by cleanup); the rest is allocated at the first call.
  struct {
    double *in = nullptr;    // the vector inputs of the host route: dl/dx, dl/dy, or the tangents dQ, dL, dU
    double *out = nullptr;   // dQ, dL, dU of the adjoint, or dX, dY of the tangent
    double *mat = nullptr;   // the matrix slab: dPx, dAx the adjoint returns, or the tangent's on the host route
    size_t in_cap = 0, out_cap = 0, mat_cap = 0;   // in doubles
    int *act = nullptr, *stat = nullptr, *piv = nullptr;   // [B][m], [B], [B] (the inversion's verdict)
  } bd;
  int *d_bad = nullptr;     // device-array updates (bounds_cross_dev): count of l > u pairs of k_batch_check_bounds
  // the kept KKT inversion (bd_run): what a one-chunk adjoint / adjoint_multi / tangent call built -- pol.map, rows,
  // mred, nlow, d_plist, the inverses in pol.K and the pivot verdicts -- stays for the later calls on the same solve
  int kkt_cache = 1;        // OSQP_AMD_BATCH_KKT_CACHE (0: every call builds its own)
  bool kkt_valid = false;   // dropped by a polish that does work and by a regrowth of pol.K
  int kkt_epoch = 0;        // b->solves when it was built: a later solve outdates it (kkt_kept)
  int kkt_NPOL = 0, kkt_NS = 0;   // (NS: the order of the per-member S^-1 on a common-K handle with the shared pieces)
  size_t kkt_count = 0;     // the members in it
  std::vector<int> kkt_members;   // the list of the _members call that built it (empty: a whole-batch call)
  int *kkt_piv = nullptr;   // [B] 0, or -1 where k_bp_invert met a pivot of the wrong sign
  long long kkt_builds = 0; // passes of k_bp_form + k_bp_invert over the solved members since setup, polish's included
};

static void batch_launch(osqp_amd_batch *b, int phase, const BSettings *st = nullptr, unsigned long long *clk = nullptr,
                         const int *list = nullptr, long long count = 0);

// the problem or the stored iterates have changed: no member's results are those of a solve of what the handle holds
static void mark_unsolved(osqp_amd_batch *b) {
  b->solved = false;
  std::fill(b->member_solved.begin(), b->member_solved.end(), (char)0);
  std::fill(b->member_polished.begin(), b->member_polished.end(), (char)0);
}
// ... of the listed members only (the _members form of an update or a warm start); a kept KKT inversion goes with them
static void mark_members_unsolved(osqp_amd_batch *b, const c_int *members, c_int count) {
  b->solved = false;
  b->kkt_valid = false;
  for (c_int k = 0; k < count; k++) b->member_solved[(size_t)members[k]] = b->member_polished[(size_t)members[k]] = 0;
}

template <typename Tp>
static int balloc(osqp_amd_batch *b, Tp **p, size_t cnt) {
  void *q = nullptr;
  if (!cnt) cnt = 1;
  BCHK(hipMalloc(&q, cnt * sizeof(Tp)));
  BCHK(hipMemsetAsync(q, 0, cnt * sizeof(Tp), b->stream));
  b->allocs.push_back(q);
  *p = static_cast<Tp *>(q);
  return 0;
}
template <typename Tp>
static int bupload(osqp_amd_batch *b, const Tp **dst, const std::vector<Tp> &src) {
  Tp *d = nullptr;
  if (balloc(b, &d, src.size())) return -102;
  if (!src.empty()) BCHK(hipMemcpyAsync(d, src.data(), src.size() * sizeof(Tp), hipMemcpyHostToDevice, b->stream));
  *dst = d;
  return 0;
}

// *p once: a call that follows a failed allocation asks only for what is still missing
template <typename Tp>
static int balloc_once(osqp_amd_batch *b, Tp **p, size_t cnt) { return *p ? 0 : balloc(b, p, cnt); }

// The forms of a call: host arrays or device arrays (dev), every member or the listed ones (members, count).  Each call
// has one body, <name>_call(b, dev, members /*null: every member*/, count, ...); its entry points are wrappers that
// check the handle and the list and hand a list of all B members on as null, so count == B runs the whole-batch code.

// OSQP_DATA_VALIDATION_ERROR unless p is device memory of the handle's device as this process's HIP runtime knows it:
// a host pointer, managed or registered host memory, another device's memory and an address of another runtime's
// allocation (two HIP runtimes mapped side by side) are all refused.  Only asks the runtime; touches no GPU memory.
static c_int dev_ptr_check(const osqp_amd_batch *b, const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return OSQP_DATA_VALIDATION_ERROR;
  }
  return (at.type == hipMemoryTypeDevice && at.device == b->device) ? 0 : OSQP_DATA_VALIDATION_ERROR;
}
static c_int dev_ptrs_check(const osqp_amd_batch *b, std::initializer_list<const void *> ps) {
  for (const void *p : ps) if (p && dev_ptr_check(b, p)) return OSQP_DATA_VALIDATION_ERROR;
  return 0;
}

// a member list: host, `count` in [1, B] indices, strictly ascending, each in [0, B)
static c_int members_check(const osqp_amd_batch *b, const c_int *members, c_int count) {
  if (!members || count < 1 || count > b->B) return OSQP_DATA_VALIDATION_ERROR;
  for (c_int k = 0; k < count; k++)
    if (members[k] < 0 || members[k] >= b->B || (k && members[k] <= members[k - 1])) return OSQP_DATA_VALIDATION_ERROR;
  return 0;
}
// The list of a _members call on the device: d_mlist[k] = list[k] and, with pos, d_mpos[list[k]] = k.  One upload per
// call; the wait is for the host vectors.
static int members_upload(osqp_amd_batch *b, const int *list, size_t count, bool pos) {
  const size_t B = (size_t)b->B;
  if (balloc_once(b, &b->d_mlist, B) || balloc_once(b, &b->d_mpos, B)) { (void)hipGetLastError(); return -102; }
  BCHK(hipMemcpyAsync(b->d_mlist, list, count * sizeof(int), hipMemcpyHostToDevice, b->stream));
  std::vector<int> at;
  if (pos) {
    at.assign(B, 0);
    for (size_t k = 0; k < count; k++) at[(size_t)list[k]] = (int)k;
    BCHK(hipMemcpyAsync(b->d_mpos, at.data(), B * sizeof(int), hipMemcpyHostToDevice, b->stream));
  }
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}
// the list of a call's body on the device (null: nothing to do, the kernels take every member)
static int members_put(osqp_amd_batch *b, const c_int *members, c_int count) {
  if (!members) return 0;
  const std::vector<int> sel(members, members + count);
  return members_upload(b, sel.data(), sel.size(), false);
}
// the solved and polished flags of the members of a call that changes their data or their stored iterates
static void mark_call_unsolved(osqp_amd_batch *b, const c_int *members, c_int count) {
  if (members) mark_members_unsolved(b, members, count);
  else mark_unsolved(b);
}

// A kernel may use more than 64 KiB of dynamic LDS only after its limit was raised.  The limit is a property of the
// kernel function on the current device, not of a batch: another handle of another size may have set it to its own,
// smaller value since.  So it is set before every launch that needs it.
static void set_dynamic_lds(const void *fn, size_t bytes) {
  if (bytes > 64 * 1024) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
#define KFN(...) reinterpret_cast<const void *>(&__VA_ARGS__)   // (variadic: a template-id carries commas)

// io.flag of every member as the launches queued so far leave it
static int read_flags(osqp_amd_batch *b, std::vector<int> &h) {
  h.resize((size_t)b->B);
  BCHK(hipGetLastError());
  BCHK(hipMemcpyAsync(h.data(), b->io.flag, h.size() * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}
// the first member whose K was not positive definite (BF_NOT_PD), B when there is none, -1 after a HIP error
static long long first_not_pd(osqp_amd_batch *b) {
  std::vector<int> h;
  if (read_flags(b, h)) return -1;
  long long q = 0;
  while (q < b->B && !(h[q] & BF_NOT_PD)) q++;
  return q;
}

static void fill_settings(osqp_amd_batch *b, const OSQPSettings *s) {
  BSettings &t = b->st;
  t.rho = s->rho; t.sigma = s->sigma; t.alpha = s->alpha; t.eps_abs = s->eps_abs; t.eps_rel = s->eps_rel;
  t.eps_pinf = s->eps_prim_inf; t.eps_dinf = s->eps_dual_inf; t.rho_tol = RHO_TOL;
  t.adapt_tol = s->adaptive_rho_tolerance;
  t.scaling = (int)s->scaling; t.adaptive_rho = (int)s->adaptive_rho;
  t.rho_interval = (int)s->adaptive_rho_interval;
  if (t.adaptive_rho && !t.rho_interval)   // deterministic stand-in for the timing rule (osqp.c:267-279)
    t.rho_interval = s->check_termination ? 4 * (int)s->check_termination : 100;
  t.max_iter = (int)s->max_iter; t.check_termination = (int)s->check_termination;
  b->report[0] = t.max_iter;                     // (before the first solve: the cap a plain one will run with)
  t.scaled_termination = (int)s->scaled_termination; t.warm_start = (int)s->warm_start;
  const char *e = getenv("OSQP_AMD_BATCH_REFINE");
  t.refine = e ? atoi(e) : 1;
  // Refine when the explicit-inverse solve leaves a relative residual above ~50 eps.  The reference's LDL'
  // solve leaves O(eps); a GEMV with K^-1 leaves up to eps cond(K), and ADMM carries that difference into
  // y (equality rows multiply it by 1e3 rho every iteration).  At 1e-12, unscaled members with equality rows
  // (cond(K) ~ 1e4) were left unrefined and missed the parity bar; the MPC batch stays below 5e-15.
  e = getenv("OSQP_AMD_BATCH_REFINE_TOL");
  t.refine_tol = e ? atof(e) : 1e-14;
  e = getenv("OSQP_AMD_BATCH_PROFILE");
  t.profile = e ? atoi(e) : 0;
  e = getenv("OSQP_AMD_BATCH_ABLATE");   // timing experiments only: skip phases of the loop (results are garbage)
  t.ablate = e ? atoi(e) : 0;
  e = getenv("OSQP_AMD_BATCH_LPT");
  b->lpt = e ? atoi(e) : 1;   // phase time stamps (wall_clock64 ticks) written into DX[0..7]
  b->pol_delta = s->delta; b->pol_refine = (int)s->polish_refine_iter;
  // cap of the polish buffer (osqp_amd_batch_polish works through the solved members in chunks that fit it);
  // read here, once per handle
  e = getenv("OSQP_AMD_BATCH_POLISH_CAP_BYTES");
  b->pol_cap = e ? (size_t)strtoull(e, nullptr, 10) : (size_t)8 << 30;
  // 0: adjoint, adjoint_multi and tangent build the KKT inversion anew in every call (the two routes give the same
  // bits; the switch exists to compare them)
  e = getenv("OSQP_AMD_BATCH_KKT_CACHE");
  b->kkt_cache = e ? atoi(e) : 1;
  // 0: a model update of a common-K handle with the shared pieces runs the two pivot sequences one after the other (the
  // same bits; the switch exists to time them against k_bc_pivot2)
  e = getenv("OSQP_AMD_BATCH_MODEL_PIVOT2");
  b->bc_pivot2 = e ? atoi(e) : 1;
  // 0: a solve of a common-K handle never packs its running columns (the same bits; the switch exists to compare and
  // to time the two)
  e = getenv("OSQP_AMD_BATCH_COMMON_PACK");
  b->bc_pack = e ? atoi(e) : 1;
}

static int bs_build_kpattern(osqp_amd_batch *b, const std::vector<int> &Pp, const std::vector<int> &Pi,
                             const std::vector<int> &Rp, const std::vector<int> &Rc, const std::vector<int> &Rk);
static int bs_setup_launch(osqp_amd_batch *b, bool update, const int *list = nullptr, long long count = 0);
static int bc_alloc(osqp_amd_batch *b);
static int stage_reserve(osqp_amd_batch *b, size_t vals, size_t idx);
static int bc_setup_launch(osqp_amd_batch *b, const c_float *Q);

static c_int batch_setup(osqp_amd_batch **out, c_int engine, c_int batch, const csc *P, const csc *A,
                         const c_float *Px_all, const c_float *Ax_all,
                         const c_float *Q, const c_float *L, const c_float *U,
                         const OSQPSettings *settings, c_int device) {
  if (!out || !P || !A || !Q || !settings || batch <= 0) return OSQP_DATA_VALIDATION_ERROR;
  if (engine != OSQP_AMD_BATCH_TILED && engine != OSQP_AMD_BATCH_STREAMED && engine != OSQP_AMD_BATCH_COMMON)
    return OSQP_SETTINGS_VALIDATION_ERROR;
  const bool common = engine == OSQP_AMD_BATCH_COMMON;
  const bool streamed = engine == OSQP_AMD_BATCH_STREAMED || common;   // K^-1 dense in HBM, formed by k_bs_form
  const char *ename = common ? "common-K" : "streamed";
  *out = nullptr;
  const int n = (int)P->n, m = (int)A->m;
  if (P->m != P->n || A->n != P->n || n <= 0 || (m > 0 && (!L || !U))) return OSQP_DATA_VALIDATION_ERROR;
  for (c_int j = 0; j < n; j++)
    for (c_int k = P->p[j]; k < P->p[j + 1]; k++) if (P->i[k] > j) return OSQP_DATA_VALIDATION_ERROR;
  if (settings->adaptive_rho_tolerance < 1.0) return OSQP_SETTINGS_VALIDATION_ERROR;
  if (settings->rho <= 0 || settings->sigma <= 0 || settings->alpha <= 0 || settings->alpha >= 2 ||
      settings->max_iter <= 0 || settings->scaling < 0 || settings->check_termination < 0)
    return OSQP_SETTINGS_VALIDATION_ERROR;
  // the solve has no polish step (polish is a call of its own on a solved handle, osqp_amd_batch_polish) and a clock
  // only per call (osqp_amd_batch_solve_limited): refusing beats an answer the caller did not ask for
  if (settings->polish || settings->time_limit > 0) {
    fprintf(stderr, "osqp_amd batch: %s is not implemented by the batched engine\n",
            settings->polish ? "polish" : "time_limit");
    return OSQP_SETTINGS_VALIDATION_ERROR;
  }
  if (!streamed && n > 128) {
    fprintf(stderr, "osqp_amd batch: n = %d > 128 is not supported by the register-tiled engine; "
                    "use one osqp_setup workspace per QP (one-QP-per-stream)\n", n);
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  if (streamed && n > BS_MAX_N) {
    fprintf(stderr, "osqp_amd batch: n = %d > %d is not supported by the %s engine\n", n, BS_MAX_N, ename);
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  if (streamed && !common && batch > 65535) {   // k_bs_form's grid: y = members
    fprintf(stderr, "osqp_amd batch: %lld members > 65535 are not supported by the streamed engine\n", (long long)batch);
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  const int NPs = (n + 31) & ~31;
  if (streamed && bs_lds_bytes(NPs, m) > 160 * 1024) {
    fprintf(stderr, "osqp_amd batch: problem needs %zu B of LDS per QP (> 160 KiB) in the %s engine\n",
            bs_lds_bytes(NPs, m), ename);
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  if (streamed && m > 0) {   // products of the A'A term of K: sum over rows of c (c + 1) / 2, c entries per row
    std::vector<size_t> rc_(m, 0);
    for (c_int k = 0; k < A->p[n]; k++) rc_[A->i[k]]++;
    size_t ntri = 0;
    for (size_t c : rc_) ntri += c * (c + 1) / 2;
    if (ntri > (size_t)BS_MAX_TRIPLES) {
      fprintf(stderr, "osqp_amd batch: A'A has %zu row products (> %d) -- A's rows are too dense for the %s "
                      "engine\n", ntri, BS_MAX_TRIPLES, ename);
      return OSQP_LINSYS_SOLVER_INIT_ERROR;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fprintf(stderr, "osqp_amd batch: no HIP device available -- there is no CPU fallback\n");
    return OSQP_LINSYS_SOLVER_LOAD_ERROR;
  }
  osqp_amd_batch *b = new (std::nothrow) osqp_amd_batch();
  if (!b) return OSQP_MEM_ALLOC_ERROR;
  b->device = (int)device; b->B = batch; b->n = n; b->m = m;
  b->member_solved.assign((size_t)batch, (char)0);
  b->member_polished.assign((size_t)batch, (char)0);
  b->member_not_pd.assign((size_t)batch, (char)0);
  b->engine = (int)engine; b->NPs = streamed ? NPs : 0;
  b->nnzP = (int)P->p[n]; b->nnzA = (int)A->p[n];
  b->tile = n <= 64 ? 4 : 8;
  b->threads = 512;   // 8x4 (n <= 128) or 4x2 (n <= 64) register tiles; 256-thread variants (8x8 tiles) spill
  if (hipSetDevice(b->device) != hipSuccess || hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
    delete b; return OSQP_LINSYS_SOLVER_LOAD_ERROR;
  }
  fill_settings(b, settings);

  // ---- shared patterns -------------------------------------------------------
  std::vector<int> Pp(n + 1), Pi(b->nnzP), Pc(b->nnzP), Ap(n + 1), Ai(b->nnzA), Ac(b->nnzA);
  for (int j = 0; j <= n; j++) { Pp[j] = (int)P->p[j]; Ap[j] = (int)A->p[j]; }
  for (int j = 0; j < n; j++) {
    for (int k = Pp[j]; k < Pp[j + 1]; k++) { Pi[k] = (int)P->i[k]; Pc[k] = j; }
    for (int k = Ap[j]; k < Ap[j + 1]; k++) { Ai[k] = (int)A->i[k]; Ac[k] = j; }
  }
  // full symmetric pattern of P by columns, each column in the reference's
  // summation order: rows >= ... (upper part: entries (j, c>=j) come from row j
  // of triu) then the column's own strictly-upper entries
  std::vector<int> cnt(n, 0);
  for (int k = 0; k < b->nnzP; k++) { cnt[Pi[k]]++; if (Pi[k] != Pc[k]) cnt[Pc[k]]++; }
  std::vector<int> Fp(n + 1, 0);
  for (int j = 0; j < n; j++) Fp[j + 1] = Fp[j] + cnt[j];
  std::vector<int> Fi(Fp[n]), Fk(Fp[n]), nx(Fp.begin(), Fp.end() - 1);
  for (int j = 0; j < n; j++)           // upper part of row i: ascending column
    for (int k = Pp[j]; k < Pp[j + 1]; k++) { int i = Pi[k]; Fi[nx[i]] = j; Fk[nx[i]] = k; nx[i]++; }
  for (int j = 0; j < n; j++)           // lower part of row j: the column's own entries
    for (int k = Pp[j]; k < Pp[j + 1]; k++) if (Pi[k] != j) { Fi[nx[j]] = Pi[k]; Fk[nx[j]] = k; nx[j]++; }
  // CSR view of A
  std::vector<int> Rp(m + 1, 0);
  for (int k = 0; k < b->nnzA; k++) Rp[Ai[k] + 1]++;
  for (int i = 0; i < m; i++) Rp[i + 1] += Rp[i];
  std::vector<int> Rj(b->nnzA), Rk(b->nnzA), rn(Rp.begin(), Rp.end() - 1);
  for (int j = 0; j < n; j++)
    for (int k = Ap[j]; k < Ap[j + 1]; k++) { int d = rn[Ai[k]]++; Rj[d] = j; Rk[d] = k; }

  BPattern &pt = b->pat;
  pt.n = n; pt.m = m; pt.nnzP = b->nnzP; pt.nnzA = b->nnzA; pt.nnzPf = Fp[n];
  int rc = 0;
  rc |= bupload(b, &pt.Pp, Pp); rc |= bupload(b, &pt.Pi, Pi); rc |= bupload(b, &pt.Pc, Pc);
  rc |= bupload(b, &pt.Fp, Fp); rc |= bupload(b, &pt.Fi, Fi); rc |= bupload(b, &pt.Fk, Fk);
  rc |= bupload(b, &pt.Ap, Ap); rc |= bupload(b, &pt.Ai, Ai); rc |= bupload(b, &pt.Ac, Ac);
  rc |= bupload(b, &pt.Rp, Rp); rc |= bupload(b, &pt.Rj, Rj); rc |= bupload(b, &pt.Rk, Rk);
  {
    std::vector<int> pk;
    for (const std::vector<int> *v : {&Pp, &Pi, &Pc, &Fp, &Fi, &Fk, &Ap, &Ai, &Ac, &Rp, &Rj, &Rk})
      pk.insert(pk.end(), v->begin(), v->end());
    rc |= bupload(b, &pt.packed, pk);
  }

  // ---- values and per-QP arrays ----------------------------------------------
  BIO &io = b->io;
  const size_t B = (size_t)batch;
  double *dPx = nullptr, *dAx = nullptr, *dQ = nullptr, *dL = nullptr, *dU = nullptr;
  io.strideP = Px_all ? b->nnzP : 0; io.strideA = Ax_all ? b->nnzA : 0;
  rc |= balloc(b, &dPx, Px_all ? B * b->nnzP : (size_t)b->nnzP);
  rc |= balloc(b, &dAx, Ax_all ? B * b->nnzA : (size_t)b->nnzA);
  rc |= balloc(b, &dQ, B * n); rc |= balloc(b, &dL, B * m); rc |= balloc(b, &dU, B * m);
  rc |= balloc(b, &io.Xs, B * n); rc |= balloc(b, &io.Zs, B * m); rc |= balloc(b, &io.Ys, B * m);
  rc |= balloc(b, &io.Xo, B * n); rc |= balloc(b, &io.Yo, B * m);
  rc |= balloc(b, &io.DXo, B * n); rc |= balloc(b, &io.DYo, B * m);
  rc |= balloc(b, &io.rho_io, B); rc |= balloc(b, &io.info, B * 8);
  { int *ord = nullptr; rc |= balloc(b, &ord, B); b->d_order = ord; }
  {
    const size_t NPk = streamed ? (size_t)b->NPs : (size_t)16 * b->tile;
    const size_t Bk = common ? 1 : B;            // the common-K engine: one slab of scaled values, one K^-1
    rc |= balloc(b, &io.Wv, Bk * ((size_t)b->nnzP + b->nnzA));
    rc |= balloc(b, &io.Wq, B * n); rc |= balloc(b, &io.Wl, B * m); rc |= balloc(b, &io.Wu, B * m);
    rc |= balloc(b, &io.Wd, B * n); rc |= balloc(b, &io.We, B * m); rc |= balloc(b, &io.Wc, B);
    rc |= balloc(b, &io.Wk, Bk * NPk * NPk); rc |= balloc(b, &io.Wt, B * m); rc |= balloc(b, &io.flag, B);
    if (common) rc |= bc_alloc(b);
    else if (streamed) { rc |= balloc(b, &b->d_count, 1); rc |= balloc(b, &b->d_list[0], B); rc |= balloc(b, &b->d_list[1], B); }
  }
  if (rc) { osqp_amd_batch_cleanup(b); return OSQP_MEM_ALLOC_ERROR; }
  io.Px = dPx; io.Ax = dAx; io.Q = dQ; io.L = dL; io.U = dU;
  b->dPx = dPx; b->dAx = dAx; b->dQ = dQ; b->dL = dL; b->dU = dU;
  auto up = [&](double *d, const c_float *s, size_t cnt) -> int {
    if (cnt && s && hipMemcpyAsync(d, s, cnt * sizeof(double), hipMemcpyHostToDevice, b->stream) != hipSuccess) return 1;
    return 0;
  };
  rc |= up(dPx, Px_all ? Px_all : P->x, Px_all ? B * b->nnzP : (size_t)b->nnzP);
  rc |= up(dAx, Ax_all ? Ax_all : A->x, Ax_all ? B * b->nnzA : (size_t)b->nnzA);
  rc |= up(dQ, Q, B * n); rc |= up(dL, L, B * m); rc |= up(dU, U, B * m);
  if (rc || hipStreamSynchronize(b->stream) != hipSuccess) { osqp_amd_batch_cleanup(b); return OSQP_LINSYS_SOLVER_INIT_ERROR; }

  if (streamed) {
    const int krc = bs_build_kpattern(b, Pp, Pi, Rp, Rj, Rk);
    if (krc) { osqp_amd_batch_cleanup(b); return krc; }
    b->lds_bytes = bs_lds_bytes(b->NPs, m);
  } else {
    b->lds_bytes = bt_lds_bytes(pt, 16 * b->tile);
    if (b->lds_bytes > 160 * 1024) {
      fprintf(stderr, "osqp_amd batch: problem needs %zu B of LDS per QP (> 160 KiB)\n", b->lds_bytes);
      osqp_amd_batch_cleanup(b);
      return OSQP_LINSYS_SOLVER_INIT_ERROR;
    }
  }
  b->h_info.assign(B * 8, 0.0);
  // setup phase on the device: Ruiz scaling, rho classes, K^-1 (one workgroup per QP)
  if (common) {
    const int crc = bc_setup_launch(b, Q);
    if (crc) { osqp_amd_batch_cleanup(b); return crc; }
  } else if (streamed) (void)bs_setup_launch(b, false);
  else batch_launch(b, 0);
  // a non-positive Gauss-Jordan pivot: K = P + sigma I + A' rho A is not positive definite, which
  // the reference's LDL' inertia check rejects at osqp_setup (qdldl_interface.c:93-99)
  const long long bad = first_not_pd(b);
  if (bad != batch) {
    if (bad >= 0) fprintf(stderr, "osqp_amd batch: QP %zu of the batch is non-convex (K = P + sigma I + A' rho A is not "
                                  "positive definite)\n", (size_t)bad);
    osqp_amd_batch_cleanup(b);
    return bad < 0 ? OSQP_LINSYS_SOLVER_INIT_ERROR : OSQP_NONCVX_ERROR;
  }
  *out = b;
  return 0;
}

extern "C" c_int osqp_amd_batch_setup(osqp_amd_batch **out, c_int batch, const csc *P, const csc *A,
                                     const c_float *Px_all, const c_float *Ax_all,
                                     const c_float *Q, const c_float *L, const c_float *U,
                                     const OSQPSettings *settings, c_int device) {
  return batch_setup(out, OSQP_AMD_BATCH_TILED, batch, P, A, Px_all, Ax_all, Q, L, U, settings, device);
}

extern "C" c_int osqp_amd_batch_setup_engine(osqp_amd_batch **out, c_int engine, c_int batch, const csc *P, const csc *A,
                                            const c_float *Px_all, const c_float *Ax_all,
                                            const c_float *Q, const c_float *L, const c_float *U,
                                            const OSQPSettings *settings, c_int device) {
  if (out) *out = nullptr;
  if (engine == OSQP_AMD_BATCH_COMMON) engine = -1;   // that engine has an entry of its own (no per-member values): unknown here
  return batch_setup(out, engine, batch, P, A, Px_all, Ax_all, Q, L, U, settings, device);
}

// ---------------------------------------------------------------------------
// streamed engine: host side
// ---------------------------------------------------------------------------
// The pattern of K = P + sigma I + A' diag(rho) A for k_bs_form.  Every entry (i <= j) of triu(K) -- the diagonal,
// triu(P) and triu(A'A) -- gets its triu(P) slot and the list of (A slot in column i, A slot in column j, row)
// triples of its A'A term in ascending row order; each row of K lists its stored entries (i, j) and (j, i).  Both
// halves of K sum the same triples in the same order, so K is symmetric to the bit.
static int bs_build_kpattern(osqp_amd_batch *b, const std::vector<int> &Pp, const std::vector<int> &Pi,
                             const std::vector<int> &Rp, const std::vector<int> &Rc, const std::vector<int> &Rk) {
  const int n = b->n, m = b->m;
  std::vector<int> eid((size_t)n * n, -1);          // (i, j), i <= j -> entry
  std::vector<int> ei, ej;
  auto entry = [&](int i, int j) {
    int &e = eid[(size_t)i * n + j];
    if (e < 0) { e = (int)ei.size(); ei.push_back(i); ej.push_back(j); }
    return e;
  };
  for (int j = 0; j < n; j++) entry(j, j);
  for (int j = 0; j < n; j++)
    for (int k = Pp[j]; k < Pp[j + 1]; k++) entry(Pi[k], j);
  // rows of A (CSR view: column Rc and CSC slot Rk, slots in column order) -> triples, counted first then
  // filled in ascending row order
  size_t ntri = 0;
  for (int r = 0; r < m; r++) {
    const size_t c = (size_t)(Rp[r + 1] - Rp[r]);
    ntri += c * (c + 1) / 2;
  }
  for (int r = 0; r < m; r++)   // (ntri <= BS_MAX_TRIPLES: checked by batch_setup)
    for (int a = Rp[r]; a < Rp[r + 1]; a++)
      for (int c = a; c < Rp[r + 1]; c++) entry(Rc[a], Rc[c]);
  const int nent = (int)ei.size();
  std::vector<int> Ep(nent + 1, 0), slot(nent, -1);
  for (int j = 0; j < n; j++)
    for (int k = Pp[j]; k < Pp[j + 1]; k++) slot[eid[(size_t)Pi[k] * n + j]] = k;
  for (int r = 0; r < m; r++)
    for (int a = Rp[r]; a < Rp[r + 1]; a++)
      for (int c = a; c < Rp[r + 1]; c++) Ep[eid[(size_t)Rc[a] * n + Rc[c]] + 1]++;
  for (int e = 0; e < nent; e++) Ep[e + 1] += Ep[e];
  std::vector<int> Ta(ntri), Tb(ntri), Tr(ntri), tx(Ep.begin(), Ep.end() - 1);
  for (int r = 0; r < m; r++)
    for (int a = Rp[r]; a < Rp[r + 1]; a++)
      for (int c = a; c < Rp[r + 1]; c++) {
        const int t = tx[eid[(size_t)Rc[a] * n + Rc[c]]]++;
        Ta[t] = Rk[a]; Tb[t] = Rk[c]; Tr[t] = r;       // Rc[a] <= Rc[c]: slot of the smaller column first
      }
  // rows of K: entry (i, j) is stored in row i and, off the diagonal, in row j
  std::vector<int> Kp(n + 1, 0);
  for (int e = 0; e < nent; e++) { Kp[ei[e] + 1]++; if (ei[e] != ej[e]) Kp[ej[e] + 1]++; }
  for (int i = 0; i < n; i++) Kp[i + 1] += Kp[i];
  std::vector<int> Kj(Kp[n]), Ke(Kp[n]), kx(Kp.begin(), Kp.end() - 1);
  for (int e = 0; e < nent; e++) {
    int d = kx[ei[e]]++; Kj[d] = ej[e]; Ke[d] = e;
    if (ei[e] != ej[e]) { d = kx[ej[e]]++; Kj[d] = ei[e]; Ke[d] = e; }
  }
  BSPattern &kp = b->kpat;
  int rc = 0;
  rc |= bupload(b, &kp.Ep, Ep); rc |= bupload(b, &kp.Eslot, slot);
  rc |= bupload(b, &kp.Ta, Ta); rc |= bupload(b, &kp.Tb, Tb); rc |= bupload(b, &kp.Tr, Tr);
  rc |= bupload(b, &kp.Rp, Kp); rc |= bupload(b, &kp.Rj, Kj); rc |= bupload(b, &kp.Re, Ke);
  return rc ? OSQP_MEM_ALLOC_ERROR : 0;
}

// form and invert K for the members of list[0..count) (the whole batch when list is null) that have a rebuild due
static void bs_rebuild(osqp_amd_batch *b, const int *list, long long count) {
  hipLaunchKernelGGL(k_bs_form, dim3((unsigned)b->NPs, (unsigned)count), dim3(256), 0, b->stream,
                     b->pat, b->kpat, b->io, b->NPs, b->st.sigma, list);
  hipLaunchKernelGGL(k_bs_invert, dim3((unsigned)count), dim3(BS_NTI), 0, b->stream, b->n, b->io, b->NPs, list);
}

// update = true: the re-equilibration of a matrix update; K is re-formed and re-inverted for every member either way.
// list (device, with update only; null: every member): for the `count` listed members alone.
static int bs_setup_launch(osqp_amd_batch *b, bool update, const int *list, long long count) {
  const void *fn = update ? KFN(k_bs_setup<true>) : KFN(k_bs_setup<false>);
  int NP = b->NPs;
  if (!list) count = b->B;
  void *args[] = {&b->pat, &b->st, &b->io, &NP, &list};
  set_dynamic_lds(fn, b->lds_bytes);
  (void)hipLaunchKernel(fn, dim3((unsigned)count), dim3(BS_NT), args, b->lds_bytes, b->stream);
  bs_rebuild(b, list, count);
  return 0;
}

// The streamed engine's part of a solve: rounds of the ADMM loop.  Round 0 runs every member; a member whose rho
// moves leaves with a rebuild request, and the next round re-forms and re-inverts K for those members and
// resumes them.  One counter is read back per round; rounds <= rho updates of the slowest member + 1.
// st: the settings of this call (b->st, or a copy with the call's max_iter); clk: the clock words of a solve with a
// time limit (k_bs_loop<true>), null without one.
static int bs_solve(osqp_amd_batch *b, const BSettings &st, unsigned long long *clk) {
  bs_rebuild(b, nullptr, b->B);                  // members whose class changed in an update, or rho at max_iter
  const int *list = nullptr;
  long long count = b->B;
  int cur = 0, rounds = 0;
  for (;;) {
    BCHK(hipMemsetAsync(b->d_count, 0, sizeof(int), b->stream));
    const void *fn = clk ? KFN(k_bs_loop<true>) : KFN(k_bs_loop<false>);
    int NP = b->NPs;
    int *rb_list = b->d_list[cur];
    void *args[] = {&b->pat, const_cast<BSettings *>(&st), &b->io, &NP, &list, &b->d_count, &rb_list, &clk};
    set_dynamic_lds(fn, b->lds_bytes);
    (void)hipLaunchKernel(fn, dim3((unsigned)count), dim3(BS_NT), args, b->lds_bytes, b->stream);
    BCHK(hipGetLastError());
    int h = 0;
    BCHK(hipMemcpyAsync(&h, b->d_count, sizeof(int), hipMemcpyDeviceToHost, b->stream));
    BCHK(hipStreamSynchronize(b->stream));
    rounds++;
    if (h == 0) break;
    list = b->d_list[cur];
    count = h;
    bs_rebuild(b, list, count);
    cur ^= 1;
  }
  if (clk) hipLaunchKernelGGL(k_clock_end, dim3(1), dim3(1), 0, b->stream, clk);
  bs_rebuild(b, nullptr, b->B);                  // rho moved in the last iteration: K^-1 follows it, as in k_batch_solve
  b->last_rounds = rounds;
  return 0;
}

// ---------------------------------------------------------------------------
// common-K engine: host side (kernels: batch_common.h)
// ---------------------------------------------------------------------------
static int bc_alloc(osqp_amd_batch *b) {
  BCT &t = b->ct;
  const size_t B = (size_t)b->B, Bp = (B + 15) & ~(size_t)15, NP = (size_t)b->NPs, m = (size_t)b->m;
  t.Bp = (int)Bp;
  int rc = 0;
  for (double **v : {&t.q, &t.x, &t.dx, &t.R, &t.Xt, &t.Rr}) rc |= balloc(b, v, NP * Bp);
  for (double **v : {&t.l, &t.u, &t.z, &t.y, &t.w, &t.dy, &t.T}) rc |= balloc(b, v, m * Bp);
  rc |= balloc(b, &t.done, B); rc |= balloc(b, &t.verdict, B); rc |= balloc(b, &t.est, B);
  rc |= balloc(b, &t.count, 1); rc |= balloc(b, &t.bad, B + 1);
  rc |= balloc(b, &t.mem, Bp); rc |= balloc(b, &t.src, B);
  rc |= balloc(b, &b->bc_wk2, NP * NP);
  return rc;
}

// form and invert the one K with the batch's rho; the refinement verdict is taken again on the new K^-1
static void bc_rebuild(osqp_amd_batch *b) {
  const int NP = b->NPs;
  hipLaunchKernelGGL(k_bc_mark, dim3(1), dim3(64), 0, b->stream, b->io, b->bc_rho);
  hipLaunchKernelGGL(k_bs_form, dim3((unsigned)NP, 1), dim3(256), 0, b->stream, b->pat, b->kpat, b->io, NP, b->st.sigma,
                     (const int *)nullptr);
  // Gauss-Jordan, one launch per pivot between the two buffers; K^-1 ends in whichever the last pivot wrote
  for (int k = 0; k < b->n; k++) {
    hipLaunchKernelGGL(k_bc_pivot, dim3((unsigned)((NP + 63) / 64), (unsigned)((NP + 15) / 16)), dim3(64, 4), 0, b->stream,
                       (const double *)b->io.Wk, b->bc_wk2, b->n, NP, k, b->io);
    std::swap(b->io.Wk, b->bc_wk2);
  }
  b->bc_rebuild = false;
  b->bc_open = true;
  b->bc_probed.assign((size_t)b->B, 0);
}

// Do the bounds L, U (device, raw, [B][m]; null = keep) leave every row with one class over the batch?  0: yes
// (*moved: some row's common class changes); 1: no, stderr names the first member and row; nothing is written.
// members (with d_list, the same list on the device; null: every member): L, U are compact [count][m], and a listed
// member's rows must keep the class the handle holds, which the unlisted members keep.
static int bc_check_classes(osqp_amd_batch *b, const double *L, const double *U, int clamp, bool *moved, const char *what,
                            const c_int *members = nullptr, size_t count = 0, const int *d_list = nullptr) {
  const size_t B = (size_t)b->B;
  std::vector<int> h(B + 1);
  BCHK(hipMemsetAsync(b->ct.bad, 0, (B + 1) * sizeof(int), b->stream));
  hipLaunchKernelGGL(k_bc_classes, dim3((unsigned)(members ? count : B)), dim3(256), 0, b->stream, b->m, b->B, b->io, L, U,
                     clamp, (double)RHO_TOL, b->ct.bad, d_list);
  BCHK(hipGetLastError());
  BCHK(hipMemcpyAsync(h.data(), b->ct.bad, (B + 1) * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  BCHK(hipStreamSynchronize(b->stream));
  for (size_t k = 0; members && k < count; k++)
    if (h[k] >= 0) {
      fprintf(stderr, "osqp_amd batch: %s: row %d of member %zu would get another class (loose / inequality / equality) "
                      "than the handle holds for it -- the common-K engine needs one class per row over the batch\n",
              what, h[k], (size_t)members[k]);
      return 1;
    }
  for (size_t q = 0; !members && q < B; q++)
    if (h[q] >= 0) {
      fprintf(stderr, "osqp_amd batch: %s: row %d of member %zu has another class (loose / inequality / equality) than in "
                      "member 0 -- the common-K engine needs one class per row over the batch\n", what, h[q], q);
      return 1;
    }
  if (moved) *moved = h[B] != 0;
  return 0;
}

// Setup: k_bs_setup on the one-member image (q^, L[0], U[0]), q^_j = max_b |Q[b][j]| -- D, E, c, the scaled values and
// the row classes --, the same for every member (k_bc_spread), the class agreement (k_bc_classes), every member's
// scaled q, l, u (k_batch_update: the reference's osqp_update_lin_cost / _bounds with the kept scaling), the one K^-1.
static int bc_setup_launch(osqp_amd_batch *b, const c_float *Q) {
  const size_t B = (size_t)b->B, n = (size_t)b->n;
  std::vector<double> qhat(n, 0.0);
  for (size_t q = 0; q < B; q++)
    for (size_t j = 0; j < n; j++) qhat[j] = std::max(qhat[j], std::fabs((double)Q[q * n + j]));
  const double *d_qhat = nullptr;
  if (bupload(b, &d_qhat, qhat)) return OSQP_MEM_ALLOC_ERROR;
  if (hipStreamSynchronize(b->stream) != hipSuccess) return OSQP_LINSYS_SOLVER_INIT_ERROR;   // qhat leaves scope
  BIO io1 = b->io;
  io1.Q = d_qhat;
  int NP = b->NPs;
  const int *every = nullptr;
  void *args[] = {&b->pat, &b->st, &io1, &NP, &every};
  set_dynamic_lds(KFN(k_bs_setup<false>), b->lds_bytes);
  (void)hipLaunchKernel(KFN(k_bs_setup<false>), dim3(1), dim3(BS_NT), args, b->lds_bytes, b->stream);
  if (B > 1) hipLaunchKernelGGL(k_bc_spread, dim3((unsigned)(B - 1)), dim3(256), 0, b->stream, b->n, b->m, b->io);
  const int crc = bc_check_classes(b, b->dL, b->dU, 0, nullptr, "setup");
  if (crc) return crc == 1 ? OSQP_DATA_VALIDATION_ERROR : OSQP_LINSYS_SOLVER_INIT_ERROR;
  hipLaunchKernelGGL(k_batch_update, dim3((unsigned)B), dim3(256), 0, b->stream, b->n, b->m, b->io,
                     (const double *)b->dQ, (const double *)b->dL, (const double *)b->dU, (double)RHO_TOL, (const int *)nullptr,
                     (double *)nullptr, (double *)nullptr, (double *)nullptr, 0);
  b->bc_rho = fmin(fmax(b->st.rho, 1e-6), 1e6);
  bc_rebuild(b);
  return 0;
}

// The batch's rho estimate from the running columns' (est > 0; a finished one carries -1), in column order -- which is
// member order, before and after a pack --: the value itself when all agree, the geometric mean otherwise; clipped as
// the reference clips.  0: nobody is running.
static double bc_batch_estimate(const std::vector<double> &est, size_t cols) {
  double first = 0.0, sumlog = 0.0;
  size_t cnt = 0;
  bool equal = true;
  for (size_t c = 0; c < cols; c++) {
    const double e = est[c];
    if (!(e > 0.0)) continue;
    if (!cnt) first = e; else if (e != first) equal = false;
    sumlog += std::log(e); cnt++;
  }
  if (!cnt) return 0.0;
  const double v = equal ? first : std::exp(sumlog / (double)cnt);
  return fmin(fmax(v, 1e-6), 1e6);
}

// The common-K engine's part of a solve: the ADMM loop of admm_loop, an iteration = a few launches over the columns.
// members: the `count` members to solve, ascending (null: all B, column = member).  Column c starts as member
// members[c]; C, the columns in use, starts at count and falls at every pack (batch_common.h).
// st: the settings of this call.  limit > 0: the call's time limit in seconds, the host's to watch -- the columns move in
// lockstep --: at a clock iteration (BATCH_CLOCK_INTERVAL), once the stream is synchronised and the termination check
// has been made, the time since k_clock_start was enqueued (b->clock_t0) is compared with it, and an expiry makes the
// iteration the last; *cut: the members running then.
static int bc_solve(osqp_amd_batch *b, const BSettings &st, const c_int *members, long long count, double limit, long long *cut) {
  BCT t = b->ct;
  const int n = b->n, m = b->m, NP = b->NPs, Bp = t.Bp;
  const dim3 eb(BC_TX, BC_TY);
  auto ey = [](int cnt) { return (unsigned)((cnt + BC_TY - 1) / BC_TY); };
  auto groups = [](long long cols) { return (unsigned)((cols + BC_TX - 1) / BC_TX); };   // (BC_TX = BC_TILE = 64)
  t.C = (int)count;
  unsigned gx = groups(t.C), g256 = (unsigned)((t.C + 255) / 256);
  dim3 gg((unsigned)((((t.C + 15) & ~15) + BC_TILE - 1) / BC_TILE), (unsigned)((NP + BC_TILE - 1) / BC_TILE));
  b->bc_cols[0] = b->bc_cols[2] = t.C; b->bc_cols[1] = 0;
  if (b->bc_rebuild) bc_rebuild(b);              // a class changed in an update, rho was set, or rho moved at max_iter
  // A verdict of "off" binds only the members that were probed under this K^-1: a solve that lists one that was not
  // probes through its first four iterations, as the first solve after the inversion does.  A window counts for every
  // member of the list, finished columns included (k_bc_probe skips them): full solves keep the launches they had.
  auto member_of = [&](long long c) { return (size_t)(members ? members[c] : c); };
  if (!b->bc_refine && !b->bc_open)
    for (long long c = 0; c < count; c++) if (!b->bc_probed[member_of(c)]) { b->bc_open = true; break; }
  auto mark_probed = [&]() { for (long long c = 0; c < count; c++) b->bc_probed[member_of(c)] = 1; };
  BCHK(hipMemsetAsync(t.count, 0, sizeof(int), b->stream));
  // the one host list behind t.src: the members first, the source columns of every pack later -- rewritten only after a
  // synchronisation that follows the copy of its last content
  std::vector<int> list;
  if (members) {
    list.assign(members, members + count);
    BCHK(hipMemcpyAsync(t.src, list.data(), (size_t)count * sizeof(int), hipMemcpyHostToDevice, b->stream));
  }
  hipLaunchKernelGGL(k_bc_load, dim3(gx, ey(std::max(std::max(n, m), 1))), eb, 0, b->stream, n, m, b->io, t,
                     members ? (const int *)t.src : (const int *)nullptr, b->bc_rho, st.warm_start);
  std::vector<double> est((size_t)count);
  std::vector<int> verdict((size_t)count), flags((size_t)count);
  bool verdict_pending = false;
  auto take_verdict = [&]() -> int {
    BCHK(hipMemcpyAsync(verdict.data(), t.verdict, (size_t)t.C * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    BCHK(hipStreamSynchronize(b->stream));
    for (int c = 0; c < t.C; c++) if (verdict[(size_t)c]) b->bc_refine = true;
    verdict_pending = false;
    return 0;
  };
  set_dynamic_lds(KFN(k_bc_check), b->lds_bytes);
  long long running = count;
  int iter = 0, rounds = 1, probe_until = 0;
  while (running > 0) {
    ++iter;
    const double rho = b->bc_rho;
    hipLaunchKernelGGL(k_bc_rhs, dim3(gx, ey(n)), eb, 0, b->stream, b->pat, b->io, t, st.sigma);
    hipLaunchKernelGGL(k_bc_gemm, gg, dim3(256), 0, b->stream, (const double *)b->io.Wk, (const double *)t.R, t.Xt,
                       (const double *)nullptr, NP, Bp, t.C);
    // the refinement rule of admm_loop with one verdict for the batch: probed in the first four iterations after an
    // inversion (refinement is applied while probing), one hit of any running member turns it on for good
    const bool probe = !b->bc_refine && (b->bc_open || iter <= probe_until);
    if (st.refine && (st.refine == 2 || b->bc_refine || probe)) {
      if (m) hipLaunchKernelGGL(k_bc_rows, dim3(gx, ey(m)), eb, 0, b->stream, b->pat, b->io, t, rho);
      hipLaunchKernelGGL(k_bc_resid, dim3(gx, ey(n)), eb, 0, b->stream, b->pat, b->io, t, st.sigma);
      if (probe) {
        hipLaunchKernelGGL(k_bc_probe, dim3(g256), dim3(256), 0, b->stream, n, t, st.refine_tol);
        verdict_pending = true;
        if (b->bc_open) { b->bc_open = false; probe_until = iter + 3; mark_probed(); }
      }
      hipLaunchKernelGGL(k_bc_gemm, gg, dim3(256), 0, b->stream, (const double *)b->io.Wk, (const double *)t.Rr, t.Xt,
                         (const double *)t.Xt, NP, Bp, t.C);
      if (verdict_pending && iter == probe_until) if (const int rc = take_verdict()) return rc;
    }
    hipLaunchKernelGGL(k_bc_step, dim3(gx, ey(n + m)), eb, 0, b->stream, b->pat, b->io, t, rho, st.alpha);
    const int checked = st.check_termination && (iter % st.check_termination == 0);
    const int adapt = st.adaptive_rho && st.rho_interval && (iter % st.rho_interval == 0);
    bool last = iter >= st.max_iter, expired = false;
    const bool clock_iter = limit > 0 && !last && (checked || (!st.check_termination && iter % BATCH_CLOCK_INTERVAL == 0));
    auto read_clock = [&]() {
      if (clock_iter && std::chrono::duration<double>(std::chrono::steady_clock::now() - b->clock_t0).count() >= limit)
        last = expired = true;
    };
    if (checked || adapt) {
      hipLaunchKernelGGL(k_bc_check, dim3((unsigned)t.C), dim3(BS_NT), b->lds_bytes, b->stream, b->pat, st, b->io, t, NP,
                         rho, iter, checked, adapt, 0);
      BCHK(hipGetLastError());
      // a pack needs more than one group of columns; the flags it is made from come over with the count
      const bool may_pack = b->bc_pack && !last && groups(t.C) > 1;
      int done = 0;
      BCHK(hipMemcpyAsync(&done, t.count, sizeof(int), hipMemcpyDeviceToHost, b->stream));
      if (adapt) BCHK(hipMemcpyAsync(est.data(), t.est, (size_t)t.C * sizeof(double), hipMemcpyDeviceToHost, b->stream));
      if (may_pack) BCHK(hipMemcpyAsync(flags.data(), t.done, (size_t)t.C * sizeof(int), hipMemcpyDeviceToHost, b->stream));
      BCHK(hipStreamSynchronize(b->stream));
      running = count - done;
      read_clock();
      const double rn = (adapt && running > 0) ? bc_batch_estimate(est, (size_t)t.C) : 0.0;
      if (rn > 0.0 && (rn > rho * st.adapt_tol || rn < rho / st.adapt_tol)) {     // adapt_rho (auxil.c:13-74)
        b->bc_rho = rn;
        hipLaunchKernelGGL(k_bc_adopt, dim3(g256), dim3(256), 0, b->stream, b->io, t);
        b->bc_rebuild = true;
        if (!last) {                             // (after the last iteration no solve with K follows: the rebuild ends the solve)
          if (verdict_pending) if (const int rc = take_verdict()) return rc;
          bc_rebuild(b); rounds++;
          hipLaunchKernelGGL(k_bc_load_w, dim3(gx, ey(std::max(m, 1))), eb, 0, b->stream, m, b->io, t, rn);
        }
      }
      // Pack once a whole group of 64 columns -- a workgroup column of every kernel -- is saved.  A verdict still open
      // is taken first: it is read by column.  (Taking it early changes no iterate: refinement is applied while probing.)
      if (may_pack && !last && running > 0 && groups(running) < groups(t.C)) {
        if (verdict_pending) if (const int rc = take_verdict()) return rc;
        list.clear();
        for (int c = 0; c < t.C; c++) if (!flags[(size_t)c]) list.push_back(c);
        if ((long long)list.size() != running) return -102;
        BCHK(hipMemcpyAsync(t.src, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(k_bc_pack, dim3((unsigned)std::max(std::max(n, m), 1), 10), dim3(256), 0, b->stream, n, m, t,
                           (int)running);
        t.C = (int)running;
        gx = groups(t.C); g256 = (unsigned)((t.C + 255) / 256);
        gg.x = (unsigned)((((t.C + 15) & ~15) + BC_TILE - 1) / BC_TILE);
        b->bc_cols[1]++; b->bc_cols[2] = t.C;
      }
    } else if (clock_iter) {
      BCHK(hipStreamSynchronize(b->stream));
      read_clock();
    }
    if (last && running > 0) {
      hipLaunchKernelGGL(k_bc_check, dim3((unsigned)t.C), dim3(BS_NT), b->lds_bytes, b->stream, b->pat, st, b->io, t, NP,
                         b->bc_rho, iter, checked, 0, expired ? 2 : 1);
      if (expired) *cut = running;
      running = 0;
    }
  }
  if (limit > 0) hipLaunchKernelGGL(k_clock_end, dim3(1), dim3(1), 0, b->stream, b->d_clock);
  if (verdict_pending) if (const int rc = take_verdict()) return rc;
  if (b->bc_rebuild) bc_rebuild(b);              // rho moved in the last iteration: K^-1 follows it
  BCHK(hipStreamSynchronize(b->stream));         // (`list` leaves scope: its last copy has been made)
  b->last_rounds = rounds;
  return 0;
}

// the one instantiation of k_batch_solve for (tile, phase)
static const void *batch_kernel(int tile, int phase) {
  if (phase == 2) return tile == 8 ? KFN((k_batch_solve<8, 4, 32, 2>)) : KFN((k_batch_solve<4, 2, 32, 2>));
  if (phase == 3) return tile == 8 ? KFN((k_batch_solve<8, 4, 32, 3>)) : KFN((k_batch_solve<4, 2, 32, 3>));
  if (tile == 8) return phase ? KFN((k_batch_solve<8, 4, 32, 1>)) : KFN((k_batch_solve<8, 4, 32, 0>));
  return phase ? KFN((k_batch_solve<4, 2, 32, 1>)) : KFN((k_batch_solve<4, 2, 32, 0>));
}
// st: the settings of a solve phase's call (null: b->st); clk: the clock words of phase 3; list (device, phase 2 only;
// null: every member): the `count` listed members of a matrix update
static void batch_launch(osqp_amd_batch *b, int phase, const BSettings *st, unsigned long long *clk, const int *list,
                         long long count) {
  const void *fn = batch_kernel(b->tile, phase);
  set_dynamic_lds(fn, b->lds_bytes);
  void *args[] = {&b->pat, st ? const_cast<BSettings *>(st) : &b->st, &b->io, &clk, &list};
  (void)hipLaunchKernel(fn, dim3((unsigned)(list ? count : b->B)), dim3(BT), args, b->lds_bytes, b->stream);
}

// the calls the common-K engine does not serve: the handle is left untouched and usable
static c_int bc_refuse(const char *call, bool hint) {
  fprintf(stderr, "osqp_amd batch: %s is not served by the common-K engine (OSQP_AMD_BATCH_COMMON)%s; use the tiled or "
                  "the streamed engine\n", call, hint ? " without its shared KKT pieces (osqp_amd_batch_common_kkt)" : "");
  return OSQP_LINSYS_SOLVER_INIT_ERROR;
}
// BC_UNSERVED: a common-K handle without the shared KKT pieces; BC_NEVER: any common-K handle
#define BC_UNSERVED(b, call) do { if ((b) && (b)->engine == OSQP_AMD_BATCH_COMMON && !(b)->bk.H) return bc_refuse(call, true); } while (0)
#define BC_NEVER(b, call) do { if ((b) && (b)->engine == OSQP_AMD_BATCH_COMMON) return bc_refuse(call, false); } while (0)

extern "C" c_int osqp_amd_batch_setup_common(osqp_amd_batch **out, c_int batch, const csc *P, const csc *A,
                                            const c_float *Q, const c_float *L, const c_float *U,
                                            const OSQPSettings *settings, c_int device) {
  if (out) *out = nullptr;
  return batch_setup(out, OSQP_AMD_BATCH_COMMON, batch, P, A, nullptr, nullptr, Q, L, U, settings, device);
}

extern "C" void osqp_amd_batch_cleanup(osqp_amd_batch *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  for (void *p : b->allocs) (void)hipFree(p);
  if (b->pol.K) (void)hipFree(b->pol.K);
  for (double *p : {b->bk.H, b->bk.Wt}) if (p) (void)hipFree(p);
  for (double *p : {b->bd.in, b->bd.mat, b->bd.out}) if (p) (void)hipFree(p);
  b->kkt_valid = false;
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

// 1 when some pair of the cnt device pairs has l > u after the clamp to +-OSQP_INFTY, 0 when none has: k_batch_check_bounds
// and one 4-byte read-back, before anything of the handle is written
static c_int bounds_cross_dev(osqp_amd_batch *b, const double *L, const double *U, size_t cnt) {
  if (balloc_once(b, &b->d_bad, 1)) { (void)hipGetLastError(); return OSQP_MEM_ALLOC_ERROR; }
  int bad = 0;
  BCHK(hipMemsetAsync(b->d_bad, 0, sizeof(int), b->stream));
  const unsigned blocks = (unsigned)std::min<size_t>((cnt + BD_NT - 1) / BD_NT, BD_MAX_BLOCKS);
  hipLaunchKernelGGL(k_batch_check_bounds, dim3(blocks), dim3(BD_NT), 0, b->stream, (long long)cnt, L, U, b->d_bad);
  BCHK(hipGetLastError());
  BCHK(hipMemcpyAsync(&bad, b->d_bad, sizeof(int), hipMemcpyDeviceToHost, b->stream));
  BCHK(hipStreamSynchronize(b->stream));
  return bad ? 1 : 0;
}

// osqp_amd_batch_update in its four forms; Q, L, U are [R][.], R = count with a list and B without (null = keep).  The
// rows are read in place on the device route and go through the staging on the host route; k_batch_update writes the
// raw rows of the call's members (clamped on the device route) and scales them.
static c_int update_call(osqp_amd_batch *b, bool dev, const c_int *members, c_int count, const c_float *Q, const c_float *L,
                         const c_float *U) {
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {Q, L, U})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t R = members ? (size_t)count : (size_t)b->B, n = (size_t)b->n, m = (size_t)b->m, cnt = R * m;
  if (!m) L = U = nullptr;
  if (dev && L && U) { if (const c_int rc = bounds_cross_dev(b, L, U, cnt)) return rc; }
  if (!dev && L && U)
    for (size_t k = 0; k < cnt; k++) if (L[k] > U[k]) return 1;   // osqp.c:815-822
  if (members_put(b, members, count)) return OSQP_MEM_ALLOC_ERROR;
  const int *list = members ? b->d_mlist : nullptr;
  const double *sQ = Q, *sL = L, *sU = U;
  if (!dev) {
    if (stage_reserve(b, (Q ? R * n : 0) + (L ? cnt : 0) + (U ? cnt : 0), 0)) return OSQP_MEM_ALLOC_ERROR;
    double *at = b->d_vals;
    for (const double **v : {&sQ, &sL, &sU}) {
      if (!*v) continue;
      const size_t len = v == &sQ ? R * n : cnt;
      BCHK(hipMemcpyAsync(at, *v, len * sizeof(double), hipMemcpyHostToDevice, b->stream));
      *v = at; at += len;
    }
  }
  // common-K, one class per row over the batch, before any write: a whole-batch update may move a row's class in every
  // member (the one K^-1 is rebuilt); the unlisted members of a list keep theirs, so the listed ones must too
  if (b->engine == OSQP_AMD_BATCH_COMMON && (sL || sU)) {
    bool moved = false;
    if (const int rc = bc_check_classes(b, sL, sU, dev ? 1 : 0, members ? nullptr : &moved, members ? "update_members" : "update",
                                        members, R, list)) return rc;
    if (moved) b->bc_rebuild = true;
  }
  mark_call_unsolved(b, members, count);
  hipLaunchKernelGGL(k_batch_update, dim3((unsigned)R), dim3(256), 0, b->stream, b->n, b->m, b->io, sQ, sL, sU, (double)RHO_TOL,
                     list, b->dQ, b->dL, b->dU, dev ? 1 : 0);
  BCHK(hipGetLastError());
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_update(osqp_amd_batch *b, const c_float *Q, const c_float *L, const c_float *U) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return update_call(b, false, nullptr, 0, Q, L, U);
}

// ---------------------------------------------------------------------------
// matrix-value, rho and warm-start updates
// ---------------------------------------------------------------------------
static int stage_reserve(osqp_amd_batch *b, size_t vals, size_t idx) {
  if (vals > b->vals_cap) { if (balloc(b, &b->d_vals, vals)) return -102; b->vals_cap = vals; }
  if (idx > b->idx_cap) { if (balloc(b, &b->d_idx, idx)) return -102; b->idx_cap = idx; }
  return 0;
}

// One of P, A: new values into the raw value array (switched to per-member storage first when the handle holds
// shared values and the update brings per-member ones, or values for a list of members).  at / iat: where this
// matrix's values and indices sit in the staging buffers.  dev: vals is a device array
// (osqp_amd_batch_update_matrices_dev): it is copied device to device where the layouts match and read in place by
// k_batch_scatter otherwise; idx is a host list either way.  list (device; null: every member): vals is one [cnt] array
// for each of the `count` listed members, or with per_member compact [count][cnt]; the other members' rows stay.
static int patch_values(osqp_amd_batch *b, double **raw, const double **io_raw, long long *stride, int nnz,
                        const c_float *vals, const c_int *idx, c_int cnt, c_int per_member, size_t at, size_t iat,
                        bool dev = false, const int *list = nullptr, long long count = 0) {
  const long long B = b->B;
  if ((per_member || list) && !*stride) {
    double *all = nullptr;
    if (balloc(b, &all, (size_t)B * nnz)) return -102;
    if (nnz) hipLaunchKernelGGL(k_batch_scatter, dim3((unsigned)((B * nnz + 255) / 256)), dim3(256), 0, b->stream,
                                all, (long long)nnz, *raw, 0LL, (const int *)nullptr, (long long)nnz, B, (const int *)nullptr);
    *raw = all; *io_raw = all; *stride = nnz;   // (the shared array stays in b->allocs until cleanup)
  }
  if (!cnt) return 0;
  const size_t tot = per_member ? (size_t)(list ? count : B) * cnt : (size_t)cnt;
  if (!list && !idx && (per_member || !*stride)) {       // same layout as the raw array: straight in
    BCHK(hipMemcpyAsync(*raw, vals, tot * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, b->stream));
    return 0;
  }
  const double *src = dev ? vals : b->d_vals + at;
  if (!dev) BCHK(hipMemcpyAsync(b->d_vals + at, vals, tot * sizeof(double), hipMemcpyHostToDevice, b->stream));
  if (idx) {
    std::vector<int> h(idx, idx + cnt);
    BCHK(hipMemcpyAsync(b->d_idx + iat, h.data(), (size_t)cnt * sizeof(int), hipMemcpyHostToDevice, b->stream));
    BCHK(hipStreamSynchronize(b->stream));      // h goes out of scope
  }
  const long long members = list ? count : (*stride ? B : 1);
  hipLaunchKernelGGL(k_batch_scatter, dim3((unsigned)((members * cnt + 255) / 256)), dim3(256), 0, b->stream,
                     *raw, *stride, src, per_member ? (long long)cnt : 0LL,
                     idx ? b->d_idx + iat : (const int *)nullptr, (long long)cnt, members, list);
  return 0;
}

// osqp_amd_batch_update_matrices in its four forms: with dev the value arrays are device arrays (the index lists are
// host lists either way); with members the values go to the `count` listed members -- one [k] array for each of them,
// or with *_per_member compact [count][k] -- and only they are re-equilibrated, re-formed and re-inverted.
static c_int update_matrices_call(osqp_amd_batch *b, bool dev, const c_int *members, c_int count,
                                  const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                  const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member) {
  // nothing is written before every argument has passed (osqp.c:1197-1222; the index range is this project's check)
  if (Px && Px_idx && P_n > b->nnzP) return 1;
  if (Ax && Ax_idx && A_n > b->nnzA) return 2;
  if ((Px && Px_idx && P_n < 0) || (Ax && Ax_idx && A_n < 0)) return OSQP_DATA_VALIDATION_ERROR;
  if (Px && Px_idx) for (c_int k = 0; k < P_n; k++) if (Px_idx[k] < 0 || Px_idx[k] >= b->nnzP) return OSQP_DATA_VALIDATION_ERROR;
  if (Ax && Ax_idx) for (c_int k = 0; k < A_n; k++) if (Ax_idx[k] < 0 || Ax_idx[k] >= b->nnzA) return OSQP_DATA_VALIDATION_ERROR;
  if (!Px && !Ax) return 0;
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {Px, Ax})) return OSQP_DATA_VALIDATION_ERROR;
  if (members_put(b, members, count)) return OSQP_MEM_ALLOC_ERROR;
  const int *list = members ? b->d_mlist : nullptr;
  mark_call_unsolved(b, members, count);
  const c_int pc = Px ? (Px_idx ? P_n : (c_int)b->nnzP) : 0, ac = Ax ? (Ax_idx ? A_n : (c_int)b->nnzA) : 0;
  const size_t R = members ? (size_t)count : (size_t)b->B;   // (the device route stages the index lists only)
  const size_t pv = dev ? 0 : (size_t)pc * (Px_per_member ? R : 1), av = dev ? 0 : (size_t)ac * (Ax_per_member ? R : 1);
  if (stage_reserve(b, pv + av, (size_t)pc + ac)) return OSQP_MEM_ALLOC_ERROR;
  if (Px && patch_values(b, &b->dPx, &b->io.Px, &b->io.strideP, b->nnzP, Px, Px_idx, pc, Px_per_member, 0, 0, dev, list, count))
    return OSQP_MEM_ALLOC_ERROR;
  if (Ax && patch_values(b, &b->dAx, &b->io.Ax, &b->io.strideA, b->nnzA, Ax, Ax_idx, ac, Ax_per_member, pv, (size_t)pc, dev, list,
                         count))
    return OSQP_MEM_ALLOC_ERROR;
  // re-equilibrate from the raw data, re-form and re-invert K with each member's current rho and classes
  if (b->engine == OSQP_AMD_BATCH_STREAMED) (void)bs_setup_launch(b, true, list, count);
  else batch_launch(b, 2, nullptr, nullptr, list, count);
  // the verdict of the members this call re-inverted goes into the host's record; an unlisted member that an earlier
  // call left non-convex still is, whatever has stored its flag word since
  std::vector<int> fl;
  if (read_flags(b, fl)) return -102;
  for (size_t k = 0; k < R; k++) {
    const size_t q = members ? (size_t)members[k] : k;
    b->member_not_pd[q] = (fl[q] & BF_NOT_PD) ? 1 : 0;
  }
  const long long bad = std::find(b->member_not_pd.begin(), b->member_not_pd.end(), (char)1) - b->member_not_pd.begin();
  b->noncvx = bad != b->B;
  if (b->noncvx) {
    fprintf(stderr, "osqp_amd batch: the new K of QP %zu of the batch is not positive definite (K = P + sigma I + "
                    "A' rho A with the updated values); solves are refused until a matrix update succeeds\n", (size_t)bad);
    return OSQP_NONCVX_ERROR;
  }
  return 0;
}

extern "C" c_int osqp_amd_batch_update_matrices(osqp_amd_batch *b,
                                                const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                                const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member) {
  BC_NEVER(b, "osqp_amd_batch_update_matrices");
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return update_matrices_call(b, false, nullptr, 0, Px, Px_idx, P_n, Px_per_member, Ax, Ax_idx, A_n, Ax_per_member);
}

// osqp_amd_batch_update_rho and its _members form: rho is one value, or with per_member [R], R = count with a list and B
// without
static c_int update_rho_call(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *rho, c_int per_member) {
  if (!rho) return OSQP_DATA_VALIDATION_ERROR;
  const size_t R = members ? (size_t)count : (size_t)b->B, cnt = per_member ? R : 1;
  for (size_t k = 0; k < cnt; k++) if (!(rho[k] > 0)) return 1;   // osqp.c:1288-1293
  if (b->engine == OSQP_AMD_BATCH_COMMON) {
    if (per_member || members) {
      fprintf(stderr, "osqp_amd batch: the common-K engine has one rho for the batch: osqp_amd_batch_update_rho%s\n",
              members ? "_members takes all of its members (count = batch)" : " takes a scalar (per_member = 0)");
      return 1;
    }
    b->bc_rho = fmin(fmax(rho[0], 1e-6), 1e6);
    b->bc_rebuild = true;
  }
  BCHK(hipSetDevice(b->device));
  if (members_put(b, members, count)) return OSQP_MEM_ALLOC_ERROR;
  mark_call_unsolved(b, members, count);
  if (balloc_once(b, &b->d_rho, (size_t)b->B)) return OSQP_MEM_ALLOC_ERROR;
  BCHK(hipMemcpyAsync(b->d_rho, rho, cnt * sizeof(double), hipMemcpyHostToDevice, b->stream));
  hipLaunchKernelGGL(k_batch_update_rho, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, b->stream,
                     (long long)R, b->io, b->d_rho, (int)(per_member != 0), members ? b->d_mlist : (const int *)nullptr);
  BCHK(hipGetLastError());
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_update_rho(osqp_amd_batch *b, const c_float *rho, c_int per_member) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return update_rho_call(b, nullptr, 0, rho, per_member);
}

// osqp_amd_batch_warm_start in its four forms; X, Y are [R][.], R = count with a list and B without (null = keep)
static c_int warm_start_call(osqp_amd_batch *b, bool dev, const c_int *members, c_int count, const c_float *X, const c_float *Y) {
  if (X || Y) BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {X, Y})) return OSQP_DATA_VALIDATION_ERROR;
  b->st.warm_start = 1;                          // osqp.c:948
  if (!X && !Y) return 0;
  const size_t R = members ? (size_t)count : (size_t)b->B, nx = X ? R * b->n : 0, ny = Y ? R * b->m : 0;
  if (members_put(b, members, count)) return OSQP_MEM_ALLOC_ERROR;
  const int *list = members ? b->d_mlist : nullptr;
  const double *sX = X, *sY = Y;
  if (!dev) {
    if (stage_reserve(b, nx + ny, 0)) return OSQP_MEM_ALLOC_ERROR;
    if (nx) BCHK(hipMemcpyAsync(b->d_vals, X, nx * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (ny) BCHK(hipMemcpyAsync(b->d_vals + nx, Y, ny * sizeof(double), hipMemcpyHostToDevice, b->stream));
    sX = X ? b->d_vals : nullptr; sY = Y ? b->d_vals + nx : nullptr;
  }
  mark_call_unsolved(b, members, count);         // the stored iterates are the caller's now, not a solve's
  const auto fn = b->engine == OSQP_AMD_BATCH_COMMON ? k_bc_warm_start : k_batch_warm_start;
  hipLaunchKernelGGL(fn, dim3((unsigned)R), dim3(256), 0, b->stream, b->pat, b->io, sX, sY, list);
  BCHK(hipGetLastError());
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_warm_start(osqp_amd_batch *b, const c_float *X, const c_float *Y) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return warm_start_call(b, false, nullptr, 0, X, Y);
}

// A solve of all members (members = null) or of `count` chosen ones: what osqp_amd_batch_solve and
// osqp_amd_batch_solve_members share once their arguments have passed.  The solved flags of the members it is about to
// solve are cleared first and set when it has ended; `solved` is all of them.
// max_iter > 0: the iteration cap of this call -- it runs with a copy of b->st, so everything max_iter does follows;
// time_limit > 0: its time limit in seconds, counted from k_clock_start (osqp_amd_batch_solve_limited).
static c_int batch_solve_run(osqp_amd_batch *b, const c_int *members, long long count, int max_iter = 0, double time_limit = 0.0) {
  BCHK(hipSetDevice(b->device));
  BSettings st = b->st;
  if (max_iter > 0) st.max_iter = max_iter;
  unsigned long long *clk = nullptr;
  long long cut = 0;
  if (time_limit > 0) {
    if (!b->d_clock) {
      BCHK(hipDeviceGetAttribute(&b->clock_khz, hipDeviceAttributeWallClockRate, b->device));
      if (b->clock_khz <= 0) return -102;
      if (balloc_once(b, &b->d_clock, (size_t)CK_COUNT_)) return OSQP_MEM_ALLOC_ERROR;
    }
    clk = b->d_clock;
  }
  b->solved = b->polished = false;
  if (!members) mark_unsolved(b);
  else for (long long k = 0; k < count; k++) b->member_solved[(size_t)members[k]] = b->member_polished[(size_t)members[k]] = 0;
  b->io.order = (b->lpt && b->solves > 0) ? b->d_order : nullptr;   // first solve: no history, index order
  if (clk) {
    const double ticks = time_limit * 1e3 * (double)b->clock_khz;
    hipLaunchKernelGGL(k_clock_start, dim3(1), dim3(1), 0, b->stream, clk, ticks < 0x1p62 ? (unsigned long long)ticks : 1ULL << 62);
    b->clock_t0 = std::chrono::steady_clock::now();
  }
  if (b->engine == OSQP_AMD_BATCH_COMMON) { if (const int rc = bc_solve(b, st, members, count, time_limit, &cut)) return rc; }
  else if (b->engine != OSQP_AMD_BATCH_STREAMED) {
    batch_launch(b, clk ? 3 : 1, &st, clk);
    if (clk) hipLaunchKernelGGL(k_clock_end, dim3(1), dim3(1), 0, b->stream, clk);
  }
  else if (const int rc = bs_solve(b, st, clk)) return rc;
  if (b->lpt && b->engine != OSQP_AMD_BATCH_COMMON) hipLaunchKernelGGL(k_batch_order, dim3(1), dim3(1024), 0, b->stream, b->B, b->io.info, b->d_order);
  BCHK(hipGetLastError());
  BCHK(hipStreamSynchronize(b->stream));
  b->solves++;                                   // (a kept KKT inversion is of an earlier solve now: kkt_kept)
  b->report[0] = st.max_iter; b->report[1] = time_limit; b->report[2] = b->report[3] = 0.0;
  if (clk) {                                     // the stamps and the count, once (a plain solve reads nothing extra)
    unsigned long long w[CK_COUNT_];
    BCHK(hipMemcpy(w, clk, sizeof(w), hipMemcpyDeviceToHost));
    b->report[2] = (double)(w[CK_END] - w[CK_START]) / (1e3 * (double)b->clock_khz);
    b->report[3] = b->engine == OSQP_AMD_BATCH_COMMON ? (double)cut : (double)w[CK_CUT];
  }
  if (!members) std::fill(b->member_solved.begin(), b->member_solved.end(), (char)1);
  else for (long long k = 0; k < count; k++) b->member_solved[(size_t)members[k]] = 1;
  b->solved = std::find(b->member_solved.begin(), b->member_solved.end(), (char)0) == b->member_solved.end();
  return 0;
}

extern "C" c_int osqp_amd_batch_solve(osqp_amd_batch *b) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (b->noncvx) return OSQP_NONCVX_ERROR;
  return batch_solve_run(b, nullptr, b->B);
}

// the refusals of a member list given to a solve: the engine's, then the list's
static c_int solve_members_check(osqp_amd_batch *b, const c_int *members, c_int count) {
  if (b->engine != OSQP_AMD_BATCH_COMMON) {
    fprintf(stderr, "osqp_amd batch: osqp_amd_batch_solve_members is a call of the common-K engine (OSQP_AMD_BATCH_COMMON); "
                    "the %s engine solves all members (osqp_amd_batch_solve)\n",
            b->engine == OSQP_AMD_BATCH_STREAMED ? "streamed" : "tiled");
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  return members_check(b, members, count);
}

extern "C" c_int osqp_amd_batch_solve_members(osqp_amd_batch *b, const c_int *members, c_int count) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (const c_int rc = solve_members_check(b, members, count)) return rc;
  if (b->noncvx) return OSQP_NONCVX_ERROR;
  // all B members, ascending: the identity, and the full solve to the bit
  return batch_solve_run(b, count == b->B ? nullptr : members, count);
}

extern "C" c_int osqp_amd_batch_solve_limited(osqp_amd_batch *b, const c_int *members, c_int count, c_int max_iter,
                                             c_float time_limit) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (max_iter < 0 || max_iter > INT_MAX || !std::isfinite(time_limit) || time_limit < 0) return OSQP_SETTINGS_VALIDATION_ERROR;
  if (members) if (const c_int rc = solve_members_check(b, members, count)) return rc;
  if (b->noncvx) return OSQP_NONCVX_ERROR;
  const bool all = !members || count == b->B;
  return batch_solve_run(b, all ? nullptr : members, all ? b->B : count, (int)max_iter, time_limit);
}

extern "C" c_int osqp_amd_batch_solve_report(osqp_amd_batch *b, c_float out[4]) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!out) return OSQP_DATA_VALIDATION_ERROR;
  for (int k = 0; k < 4; k++) out[k] = b->report[k];
  return 0;
}

// Of the last solve of a common-K handle: the columns it started with, its packs, the columns in use when it ended.
// Touches no GPU memory.
extern "C" c_int osqp_amd_batch_common_columns(osqp_amd_batch *b, c_int out[3]) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!out) return OSQP_DATA_VALIDATION_ERROR;
  if (b->engine != OSQP_AMD_BATCH_COMMON) {
    fprintf(stderr, "osqp_amd batch: osqp_amd_batch_common_columns is a call of the common-K engine (OSQP_AMD_BATCH_COMMON)\n");
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  for (int k = 0; k < 3; k++) out[k] = b->bc_cols[k];
  return 0;
}

// the row maps, counts and status of polish and the list of solved members, allocated at the first polish or adjoint
static int bp_reserve_maps(osqp_amd_batch *b) {
  if (b->d_plist) return 0;
  const size_t B = (size_t)b->B, m = (size_t)b->m;
  BPol &pl = b->pol;
  if (balloc_once(b, &pl.map, B * m) || balloc_once(b, &pl.rows, B * m) || balloc_once(b, &pl.mred, B) ||
      balloc_once(b, &pl.nlow, B) || balloc_once(b, &pl.stat, B) || balloc_once(b, &b->d_plist, B)) {
    (void)hipGetLastError();
    return -102;
  }
  return 0;
}
// the KKT buffer of at least `bytes` (it only grows)
static int bp_reserve_K(osqp_amd_batch *b, size_t bytes) {
  BPol &pl = b->pol;
  if (bytes <= b->pol_bytes) return 0;
  if (pl.K) (void)hipFree(pl.K);
  pl.K = nullptr; b->pol_bytes = 0;
  b->kkt_valid = false;                          // a kept inversion went with the buffer
  void *k = nullptr;
  if (hipMalloc(&k, bytes) != hipSuccess) { (void)hipGetLastError(); return -102; }
  pl.K = static_cast<double *>(k); b->pol_bytes = bytes;
  return 0;
}

// What polish and adjoint share before their own kernel: the active rows of every solved member (k_bp_active with
// pl, whose stat is the caller's status array), the list of solved members on the device, the padded order NPOL,
// the refusals, the KKT buffer and the members per chunk.  lds_of: the caller's kernel's LDS for (n, m, NPOL).
// On a common-K handle with the shared pieces the buffer holds S^-1 of order NS per member, not the whole matrix of
// order NPOL; NPOL stays the length of the kernels' LDS vectors [x; nu], and lds includes BlockK's scratch.
struct BPlan { size_t count = 0, chunk = 0, lds = 0, ilds = 0; int NPOL = 0, NS = 0; };
static BlockK bk_solver(const osqp_amd_batch *b, int NS) { return BlockK{b->bk.H, b->bk.Wt, b->NPs, NS}; }
// sel (null: every member): the members the call is about, ascending, already on the device in b->d_mlist
// (members_upload); k_bp_active runs over them alone, and NPOL and NS come from their largest mred.
static c_int bp_plan(osqp_amd_batch *b, BPol &pl, const char *what, size_t (*lds_of)(int, int, int), BPlan *out,
                     const std::vector<int> *sel = nullptr) {
  const size_t B = (size_t)b->B;
  const int n = b->n, m = b->m;
  hipLaunchKernelGGL(k_bp_active, dim3((unsigned)(sel ? sel->size() : B)), dim3(256), 0, b->stream, m, b->io, pl,
                     sel ? (const int *)b->d_mlist : (const int *)nullptr);
  BCHK(hipGetLastError());
  std::vector<int> h(B), list;
  BCHK(hipMemcpyAsync(h.data(), pl.mred, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  BCHK(hipStreamSynchronize(b->stream));
  int mmax = 0;
  for (size_t q = 0; !sel && q < B; q++) if (h[q] >= 0) { list.push_back((int)q); mmax = std::max(mmax, h[q]); }
  for (size_t k = 0; sel && k < sel->size(); k++) {
    const int q = (*sel)[k];
    if (h[(size_t)q] >= 0) { list.push_back(q); mmax = std::max(mmax, h[(size_t)q]); }
  }
  *out = BPlan{};
  if (list.empty()) return 0;
  const int NPOL = (n + mmax + 31) & ~31;
  const bool blk = b->bk.H != nullptr;
  const int NS = blk ? std::max(32, (mmax + 31) & ~31) : 0, KN = blk ? NS : NPOL;
  const size_t lds = lds_of(n, m, NPOL) + (blk ? bk_scratch_bytes(b->NPs, NS) : 0);
  if (NPOL > BP_MAX_N || lds > 160 * 1024) {
    fprintf(stderr, "osqp_amd batch: %s needs a KKT matrix of order n + active rows = %d (> %d) or %zu B of LDS "
                    "(> 160 KiB) for some member\n", what, n + mmax, BP_MAX_N, lds);
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  const size_t per = (size_t)KN * KN * sizeof(double);
  const size_t chunk = std::min(std::min(list.size(), (size_t)65535), std::max((size_t)1, b->pol_cap / per));
  if (bp_reserve_K(b, chunk * per)) return OSQP_MEM_ALLOC_ERROR;
  pl.K = b->pol.K;
  BCHK(hipMemcpyAsync(b->d_plist, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
  BCHK(hipStreamSynchronize(b->stream));         // (list goes out of scope)
  out->count = list.size(); out->chunk = chunk; out->lds = lds; out->ilds = 4 * (size_t)KN * sizeof(double); out->NPOL = NPOL; out->NS = NS;
  return 0;
}
static size_t bp_lds_of(int n, int m, int NPOL) { return bp_lds_bytes(n, m, NPOL); }
static size_t bd_lds_of(int n, int m, int NPOL) { return bd_lds_bytes(n, m, NPOL); }

// The planned chunks of solved members: the KKT matrix of each member of a chunk (k_bp_form), its inverse
// (k_bp_invert), then the caller's kernel fn, launched by third(members of the chunk, their list) with pn.lds
// bytes of LDS.  Nothing is waited for.
template <class Third>
static int bp_run_chunks(osqp_amd_batch *b, const BPol &pl, const BPlan &pn, const void *fn, Third third) {
  const bool blk = b->bk.H != nullptr;
  set_dynamic_lds(blk ? KFN(k_bk_invert) : KFN(k_bp_invert), pn.ilds);
  set_dynamic_lds(fn, pn.lds);
  if (pn.count) b->kkt_builds++;
  for (size_t c0 = 0; c0 < pn.count; c0 += pn.chunk) {
    const unsigned cnt = (unsigned)std::min(pn.chunk, pn.count - c0);
    const int *lp = b->d_plist + c0;
    if (blk) {
      hipLaunchKernelGGL(k_bk_form, dim3((unsigned)pn.NS, cnt), dim3(256), 0, b->stream, b->pat, b->io, pl, b->bk, b->NPs, pn.NS, b->pol_delta, lp);
      hipLaunchKernelGGL(k_bk_invert, dim3(cnt), dim3(BS_NTI), pn.ilds, b->stream, pl, pn.NS, lp);
    } else {
      hipLaunchKernelGGL(k_bp_form, dim3((unsigned)pn.NPOL, cnt), dim3(256), 0, b->stream, b->pat, b->io, pl, pn.NPOL, b->pol_delta, lp);
      hipLaunchKernelGGL(k_bp_invert, dim3(cnt), dim3(BS_NTI), pn.ilds, b->stream, b->n, pl, pn.NPOL, lp);
    }
    third(cnt, lp);
    BCHK(hipGetLastError());
  }
  return 0;
}

// Whether the inversion a derivative call left in pol.K still belongs to the handle's point.  Every call that reads
// it has passed `b->solved`, which only osqp_amd_batch_solve sets, together with b->solves; every update and warm
// start that withdraws the permission to call clears it until the next solve.  So the epoch outdates what a solve,
// or an update followed by a solve, has overtaken.
// An inversion built by a _members call is kept with its list (kkt_members) and belongs to a later _members call with
// the identical list, whose members have all passed their solved flags; a whole-batch call reuses only a whole-batch
// build.  kkt_kept: something is kept and still belongs to the handle's point (osqp_amd_batch_kkt_info);
// kkt_kept_for: ... and to the asking call, whose list is sel (null: a whole-batch call).
static bool kkt_kept(const osqp_amd_batch *b) {
  if (!b->kkt_valid || b->kkt_epoch != b->solves) return false;
  if (b->kkt_members.empty()) return b->solved;
  for (int q : b->kkt_members) if (!b->member_solved[(size_t)q]) return false;
  return true;
}
static bool kkt_kept_for(const osqp_amd_batch *b, const std::vector<int> *sel) {
  return kkt_kept(b) && (sel ? b->kkt_members == *sel : b->kkt_members.empty());
}
// What adjoint, adjoint_multi and tangent share around their own kernel fn, which third(plan, members, their list)
// launches with pn.lds bytes of LDS; pl.stat is the call's array of pivot verdicts.  While an inversion is kept,
// only the verdicts are copied and fn launched.  Otherwise bp_plan and bp_run_chunks as polish runs them; when the
// plan is one chunk (and OSQP_AMD_BATCH_KKT_CACHE is not 0) the verdicts are saved after k_bp_invert and what was
// built is kept.  Either way fn sees the same maps, list, inverses and verdicts: the same bits.  Nothing is waited for.
template <class Third>
static c_int bd_run(osqp_amd_batch *b, BPol &pl, const char *what, size_t (*lds_of)(int, int, int), const void *fn, Third third,
                    const std::vector<int> *sel = nullptr) {
  const size_t B = (size_t)b->B;
  BPlan pn;
  if (kkt_kept_for(b, sel)) {
    pn.count = pn.chunk = b->kkt_count; pn.NPOL = b->kkt_NPOL; pn.NS = b->kkt_NS;
    pn.lds = lds_of(b->n, b->m, pn.NPOL) + (b->bk.H ? bk_scratch_bytes(b->NPs, pn.NS) : 0);
    if (pn.lds > 160 * 1024) {
      fprintf(stderr, "osqp_amd batch: %s needs %zu B of LDS (> 160 KiB) for some member\n", what, pn.lds);
      return OSQP_LINSYS_SOLVER_INIT_ERROR;
    }
    pl.K = b->pol.K;
    BCHK(hipMemcpyAsync(pl.stat, b->kkt_piv, B * sizeof(int), hipMemcpyDeviceToDevice, b->stream));
    set_dynamic_lds(fn, pn.lds);
    third(pn, (unsigned)pn.count, (const int *)b->d_plist);
    BCHK(hipGetLastError());
    return 0;
  }
  b->kkt_valid = false;                          // k_bp_active rewrites the maps
  const c_int rc = bp_plan(b, pl, what, lds_of, &pn, sel);
  if (rc) return rc;
  const bool keep = b->kkt_cache && pn.count && pn.count <= pn.chunk;
  if (keep && balloc_once(b, &b->kkt_piv, B)) { (void)hipGetLastError(); return OSQP_MEM_ALLOC_ERROR; }
  if (bp_run_chunks(b, pl, pn, fn, [&](unsigned cnt, const int *lp) {
        if (keep) (void)hipMemcpyAsync(b->kkt_piv, pl.stat, B * sizeof(int), hipMemcpyDeviceToDevice, b->stream);
        third(pn, cnt, lp);
      })) return -102;
  if (keep) {
    b->kkt_valid = true; b->kkt_epoch = b->solves; b->kkt_NPOL = pn.NPOL; b->kkt_NS = pn.NS; b->kkt_count = pn.count;
    if (sel) b->kkt_members = *sel; else b->kkt_members.clear();
  }
  return 0;
}

// polish's plan and chunks for every member (sel null) or the members of sel (bp_plan), and the wait for them
static c_int bp_polish_run(osqp_amd_batch *b, const std::vector<int> *sel) {
  BPol &pl = b->pol;
  BPlan pn;
  b->kkt_valid = false;   // polish overwrites pol.K and may move the point: it neither reads nor leaves a kept inversion
  const c_int rc = bp_plan(b, pl, "polish", bp_lds_of, &pn, sel);
  if (rc) return rc;
  const bool blk = b->bk.H != nullptr;
  if (bp_run_chunks(b, pl, pn, blk ? KFN(k_bp_polish<BlockK, BlockK>) : KFN(k_bp_polish<FullK>), [&](unsigned cnt, const int *lp) {
        if (blk) hipLaunchKernelGGL((k_bp_polish<BlockK, BlockK>), dim3(cnt), dim3(BP_NT), pn.lds, b->stream, b->pat, b->st, b->io, pl, pn.NPOL, b->pol_refine, lp, bk_solver(b, pn.NS));
        else hipLaunchKernelGGL(k_bp_polish<FullK>, dim3(cnt), dim3(BP_NT), pn.lds, b->stream, b->pat, b->st, b->io, pl, pn.NPOL, b->pol_refine, lp);
      })) return -102;
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// status_polish[k] (null: not asked for) of member members[k], or of member k without a list, as polish left it
static c_int polish_status_out(osqp_amd_batch *b, const c_int *members, c_int count, c_int *status_polish) {
  if (!status_polish) return 0;
  std::vector<int> h((size_t)b->B);
  BCHK(hipMemcpyAsync(h.data(), b->pol.stat, h.size() * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  BCHK(hipStreamSynchronize(b->stream));
  for (c_int k = 0; k < count; k++) status_polish[k] = h[(size_t)(members ? members[k] : k)];
  return 0;
}

// polish for the solved members, in chunks of at most pol_cap bytes of KKT matrices (batch_polish.h)
extern "C" c_int osqp_amd_batch_polish(osqp_amd_batch *b, c_int *status_polish) {
  BC_UNSERVED(b, "osqp_amd_batch_polish");
  if (!b || !b->solved) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  BCHK(hipSetDevice(b->device));
  if (bp_reserve_maps(b)) return OSQP_MEM_ALLOC_ERROR;
  if (!b->polished) {       // (a second call without a solve in between finds the work done and reports it again)
    if (const c_int rc = bp_polish_run(b, nullptr)) return rc;
    b->polished = true;
    std::fill(b->member_polished.begin(), b->member_polished.end(), (char)1);
  }
  return polish_status_out(b, nullptr, b->B, status_polish);
}

// For the tests and tools: builds of the KKT inversion since setup, whether one is kept, its NPOL and its members.
// Touches no GPU memory.
extern "C" c_int osqp_amd_batch_kkt_info(osqp_amd_batch *b, c_int out[4]) {
  BC_UNSERVED(b, "osqp_amd_batch_kkt_info");
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!out) return OSQP_DATA_VALIDATION_ERROR;
  const bool kept = kkt_kept(b);
  out[0] = (c_int)b->kkt_builds; out[1] = kept ? 1 : 0;
  out[2] = kept ? (b->bk.H ? b->kkt_NS : b->kkt_NPOL) : 0; out[3] = kept ? (c_int)b->kkt_count : 0;
  return 0;
}

// The shared KKT pieces of a common-K handle (batch_common_kkt.h).  on: H = (P~ + delta I)^-1 by k_bk_hform and the
// k_bc_pivot sequence of bc_rebuild between two buffers of the call's own -- the pivot kernel sees a BIO whose flag is
// the call's own word, so io.flag[0] and io.Wk stay as they are -- then Wt = A~ H.  off: both are freed.  Either way a
// kept inversion is dropped: it belongs to the route that built it.
static void bk_free(osqp_amd_batch *b) {
  for (double **p : {&b->bk.H, &b->bk.Wt}) { if (*p) (void)hipFree(*p); *p = nullptr; }
}
// H and Wt from the scaled values the handle holds now, into b->bk's allocations where it has them (a model update)
// and into new ones otherwise (osqp_amd_batch_common_kkt).  On any failure both are freed.
static c_int bk_build(osqp_amd_batch *b) {
  const int n = b->n, m = b->m, NP = b->NPs;
  const size_t sq = (size_t)NP * NP * sizeof(double);
  // word: the pivots' verdict.  It is not cleared here: pivot 0 of k_bc_pivot stores the whole word (BF_OPEN) before any
  // pivot ORs BF_NOT_PD into it, and n >= 1 on every handle, so it is written before it is read.
  void *h2 = nullptr, *word = nullptr;
  auto fail = [&](c_int rc) { bk_free(b); if (h2) (void)hipFree(h2); if (word) (void)hipFree(word); (void)hipGetLastError(); return rc; };
  if ((!b->bk.H && hipMalloc((void **)&b->bk.H, sq) != hipSuccess) || hipMalloc(&h2, sq) != hipSuccess ||
      hipMalloc(&word, sizeof(int)) != hipSuccess ||
      (m > 0 && !b->bk.Wt && hipMalloc((void **)&b->bk.Wt, (size_t)m * NP * sizeof(double)) != hipSuccess))
    return fail(OSQP_MEM_ALLOC_ERROR);
  BIO io = b->io;
  io.flag = static_cast<int *>(word);
  double *cur = b->bk.H, *other = static_cast<double *>(h2);
  hipLaunchKernelGGL(k_bk_hform, dim3((unsigned)NP), dim3(256), 0, b->stream, b->pat, b->io, NP, b->pol_delta, cur);
  for (int k = 0; k < n; k++) {
    hipLaunchKernelGGL(k_bc_pivot, dim3((unsigned)((NP + 63) / 64), (unsigned)((NP + 15) / 16)), dim3(64, 4), 0, b->stream,
                       (const double *)cur, other, n, NP, k, io);
    std::swap(cur, other);
  }
  int verdict = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&verdict, word, sizeof(int), hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
      hipStreamSynchronize(b->stream) != hipSuccess) return fail(-102);
  b->bk.H = cur; h2 = other;                     // the inverse is in whichever buffer the last pivot wrote
  if (verdict & BF_NOT_PD) {
    fprintf(stderr, "osqp_amd batch: osqp_amd_batch_common_kkt: a pivot of P + delta I is not positive\n");
    return fail(OSQP_NONCVX_ERROR);
  }
  if (m > 0) hipLaunchKernelGGL(k_bk_wt, dim3((unsigned)m), dim3(256), 0, b->stream, b->pat, b->io, NP, (const double *)b->bk.H, b->bk.Wt);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess) return fail(-102);
  (void)hipFree(h2); (void)hipFree(word);
  return 0;
}
extern "C" c_int osqp_amd_batch_common_kkt(osqp_amd_batch *b, c_int on) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (b->engine != OSQP_AMD_BATCH_COMMON) {
    fprintf(stderr, "osqp_amd batch: osqp_amd_batch_common_kkt is a call of the common-K engine (OSQP_AMD_BATCH_COMMON); the "
                    "tiled and the streamed engine serve polish, adjoint and tangent as they are\n");
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  if (on && b->bk.H) return 0;
  BCHK(hipSetDevice(b->device));
  BCHK(hipStreamSynchronize(b->stream));
  b->kkt_valid = false;
  if (!on) { bk_free(b); return 0; }
  return bk_build(b);
}

// bc_rebuild and bk_build of a model update on a handle with the shared pieces, side by side: k_bc_pivot2 advances K and
// P~ + delta I in one launch per pivot.  *kflag: K's flag word.  Where K fails, H's verdict is not read and the pieces
// stay allocated (the call that repairs K rebuilds them); where only H fails, bk_build's outcome.
static c_int bc_rebuild_pair(osqp_amd_batch *b, int *kflag) {
  const int n = b->n, m = b->m, NP = b->NPs;
  const size_t sq = (size_t)NP * NP * sizeof(double);
  void *h2 = nullptr, *word = nullptr;
  auto fail = [&](c_int rc) { bk_free(b); if (h2) (void)hipFree(h2); if (word) (void)hipFree(word); (void)hipGetLastError(); return rc; };
  if (hipMalloc(&h2, sq) != hipSuccess || hipMalloc(&word, sizeof(int)) != hipSuccess) return fail(OSQP_MEM_ALLOC_ERROR);
  hipLaunchKernelGGL(k_bc_mark, dim3(1), dim3(64), 0, b->stream, b->io, b->bc_rho);
  hipLaunchKernelGGL(k_bs_form, dim3((unsigned)NP, 1), dim3(256), 0, b->stream, b->pat, b->kpat, b->io, NP, b->st.sigma,
                     (const int *)nullptr);
  hipLaunchKernelGGL(k_bk_hform, dim3((unsigned)NP), dim3(256), 0, b->stream, b->pat, b->io, NP, b->pol_delta, b->bk.H);
  BCPair a;
  a.in[0] = b->io.Wk; a.out[0] = b->bc_wk2; a.flag[0] = b->io.flag;
  a.in[1] = b->bk.H; a.out[1] = static_cast<double *>(h2); a.flag[1] = static_cast<int *>(word);
  for (int k = 0; k < n; k++) {
    hipLaunchKernelGGL(k_bc_pivot2, dim3((unsigned)((NP + 63) / 64), (unsigned)((NP + 15) / 16), 2), dim3(64, 4), 0, b->stream,
                       a, n, NP, k);
    for (int s = 0; s < 2; s++) { double *t = const_cast<double *>(a.in[s]); a.in[s] = a.out[s]; a.out[s] = t; }
  }
  b->io.Wk = const_cast<double *>(a.in[0]); b->bc_wk2 = a.out[0];
  b->bk.H = const_cast<double *>(a.in[1]); h2 = a.out[1];      // each inverse is in whichever buffer the last pivot wrote
  b->bc_rebuild = false;
  b->bc_open = true;
  b->bc_probed.assign((size_t)b->B, 0);
  int verdict = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(kflag, b->io.flag, sizeof(int), hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
      hipMemcpyAsync(&verdict, word, sizeof(int), hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
      hipStreamSynchronize(b->stream) != hipSuccess) return fail(-102);
  if (!(*kflag & BF_NOT_PD)) {
    if (verdict & BF_NOT_PD) {
      fprintf(stderr, "osqp_amd batch: osqp_amd_batch_common_kkt: a pivot of P + delta I is not positive\n");
      return fail(OSQP_NONCVX_ERROR);
    }
    if (m > 0) hipLaunchKernelGGL(k_bk_wt, dim3((unsigned)m), dim3(256), 0, b->stream, b->pat, b->io, NP, (const double *)b->bk.H, b->bk.Wt);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess) return fail(-102);
  }
  (void)hipFree(h2); (void)hipFree(word);
  return 0;
}

// New values for the one model of a common-K handle: osqp_update_P / _A / _P_A on the shared raw arrays, then
// setup's scale_data on the one-member image (q^, L[0], U[0]) with the classes kept (k_bs_setup<true>), D, E, c for
// every member (k_bc_spread), every member's scaled q, l, u from its stored raw ones (k_bc_rescale), the one K^-1 with
// the batch's rho as it stands, and H / Wt where the handle carries them.  dev: Px / Ax are device arrays.
static c_int bc_update_model(osqp_amd_batch *b, bool dev, const char *call, const c_float *Px, const c_int *Px_idx, c_int P_n,
                             const c_float *Ax, const c_int *Ax_idx, c_int A_n) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (b->engine != OSQP_AMD_BATCH_COMMON) {
    fprintf(stderr, "osqp_amd batch: %s is a call of the common-K engine (OSQP_AMD_BATCH_COMMON); the tiled and the streamed "
                    "engine take new matrix values through osqp_amd_batch_update_matrices\n", call);
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  // nothing is written before every argument has passed: osqp_amd_batch_update_matrices' refusals in its order
  if (Px && Px_idx && P_n > b->nnzP) return 1;
  if (Ax && Ax_idx && A_n > b->nnzA) return 2;
  if ((Px && Px_idx && P_n < 0) || (Ax && Ax_idx && A_n < 0)) return OSQP_DATA_VALIDATION_ERROR;
  if (Px && Px_idx) for (c_int k = 0; k < P_n; k++) if (Px_idx[k] < 0 || Px_idx[k] >= b->nnzP) return OSQP_DATA_VALIDATION_ERROR;
  if (Ax && Ax_idx) for (c_int k = 0; k < A_n; k++) if (Ax_idx[k] < 0 || Ax_idx[k] >= b->nnzA) return OSQP_DATA_VALIDATION_ERROR;
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {Px, Ax})) return OSQP_DATA_VALIDATION_ERROR;
  if (!Px && !Ax) return 0;
  mark_unsolved(b);                             // (a kept KKT inversion goes with it: kkt_kept)
  b->kkt_valid = false;
  const c_int pc = Px ? (Px_idx ? P_n : (c_int)b->nnzP) : 0, ac = Ax ? (Ax_idx ? A_n : (c_int)b->nnzA) : 0;
  const size_t n = (size_t)b->n, B = (size_t)b->B;
  if (stage_reserve(b, dev ? 0 : (size_t)pc + ac, (size_t)pc + ac) || balloc_once(b, &b->bc_qhat, n)) return OSQP_MEM_ALLOC_ERROR;
  if (Px && patch_values(b, &b->dPx, &b->io.Px, &b->io.strideP, b->nnzP, Px, Px_idx, pc, 0, 0, 0, dev)) return OSQP_MEM_ALLOC_ERROR;
  if (Ax && patch_values(b, &b->dAx, &b->io.Ax, &b->io.strideA, b->nnzA, Ax, Ax_idx, ac, 0, (size_t)pc, (size_t)pc, dev))
    return OSQP_MEM_ALLOC_ERROR;
  hipLaunchKernelGGL(k_bc_qhat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, b->n, b->B, (const double *)b->dQ,
                     b->bc_qhat);
  BIO io1 = b->io;
  io1.Q = b->bc_qhat;
  int NP = b->NPs;
  const int *every = nullptr;
  void *args[] = {&b->pat, &b->st, &io1, &NP, &every};
  set_dynamic_lds(KFN(k_bs_setup<true>), b->lds_bytes);
  (void)hipLaunchKernel(KFN(k_bs_setup<true>), dim3(1), dim3(BS_NT), args, b->lds_bytes, b->stream);
  if (B > 1) hipLaunchKernelGGL(k_bc_spread, dim3((unsigned)(B - 1)), dim3(256), 0, b->stream, b->n, b->m, b->io);
  hipLaunchKernelGGL(k_bc_rescale, dim3((unsigned)B), dim3(256), 0, b->stream, b->n, b->m, b->io);
  b->bc_refine = false;                          // the verdict belonged to the old K; the rebuild re-opens it
  int flag = 0;
  c_int hrc = 0;
  const bool pair = b->bk.H && b->bc_pivot2;
  if (pair) hrc = bc_rebuild_pair(b, &flag);
  else {
    bc_rebuild(b);
    BCHK(hipGetLastError());
    BCHK(hipMemcpyAsync(&flag, b->io.flag, sizeof(int), hipMemcpyDeviceToHost, b->stream));
    BCHK(hipStreamSynchronize(b->stream));
  }
  if (hrc && hrc != OSQP_NONCVX_ERROR) return hrc;
  b->noncvx = (flag & BF_NOT_PD) != 0;
  if (b->noncvx) {                               // (H and Wt wait for the call that repairs K)
    fprintf(stderr, "osqp_amd batch: the new K of the batch is not positive definite (K = P + sigma I + A' rho A with the "
                    "updated values); solves are refused until a matrix update succeeds\n");
    return OSQP_NONCVX_ERROR;
  }
  if (pair) return hrc;
  return b->bk.H ? bk_build(b) : 0;
}
extern "C" c_int osqp_amd_batch_common_update_model(osqp_amd_batch *b, const c_float *Px, const c_int *Px_idx, c_int P_n,
                                                    const c_float *Ax, const c_int *Ax_idx, c_int A_n) {
  return bc_update_model(b, false, "osqp_amd_batch_common_update_model", Px, Px_idx, P_n, Ax, Ax_idx, A_n);
}

// For the tests: the shared pieces and, of the kept inversion, member qp's S^-1 as stored.
extern "C" c_int osqp_amd_batch_common_kkt_peek(osqp_amd_batch *b, c_float *H, c_float *Wt, c_int qp, c_int *mred, c_int *NS, c_float *Sinv) {
  if (!b || !b->bk.H) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  const size_t B = (size_t)b->B, NP = (size_t)b->NPs;
  const bool member = mred || NS || Sinv;
  if (member && (qp < 0 || (size_t)qp >= B)) return OSQP_DATA_VALIDATION_ERROR;
  if (member && !kkt_kept(b)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  BCHK(hipSetDevice(b->device));
  if (H) BCHK(hipMemcpyAsync(H, b->bk.H, NP * NP * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  if (Wt && b->m) BCHK(hipMemcpyAsync(Wt, b->bk.Wt, (size_t)b->m * NP * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  if (member) {
    std::vector<int> h(B);
    BCHK(hipMemcpyAsync(h.data(), b->pol.mred, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    BCHK(hipStreamSynchronize(b->stream));
    if (h[(size_t)qp] < 0) return OSQP_DATA_VALIDATION_ERROR;   // not a solved member: it has no slot
    size_t slot = 0;                             // the solved members sit in the buffer in index order
    for (size_t q = 0; q < (size_t)qp; q++) if (h[q] >= 0) slot++;
    const size_t ns = (size_t)b->kkt_NS;
    if (mred) *mred = h[(size_t)qp];
    if (NS) *NS = (c_int)ns;
    if (Sinv) BCHK(hipMemcpyAsync(Sinv, b->pol.K + slot * ns * ns, ns * ns * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  }
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// a staging buffer of the derivative calls of at least cnt doubles (it only grows; nothing is queued on it between
// calls)
static int bd_reserve(double **p, size_t *cap, size_t cnt) {
  if (cnt <= *cap) return 0;
  if (*p) (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  void *q = nullptr;
  if (hipMalloc(&q, cnt * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return -102; }
  *p = static_cast<double *>(q); *cap = cnt;
  return 0;
}

// What the adjoint and the tangent do before bd_run.  The handle's staging for this call: nout doubles of output and
// nmat of matrix output, both zeroed with `active` and the status (members that are skipped or rejected report
// zeros), and room for the inputs.  *pl: polish's buffers with the call's own pivot verdicts; polish's status array
// stays polish's.  ins: the inputs (null = none); *slot is where the kernel reads each -- in place on the device
// route, from the staging (vectors in `in`, matrices in `mat`) on the host route.
struct BDIn { const c_float *src; size_t cnt; const double **slot; bool mat; };
// R: the rows of the call's arrays -- B, or the listed members of a _members call -- which size what is zeroed.
static c_int bd_stage(osqp_amd_batch *b, BPol *pl, bool dev, std::initializer_list<BDIn> ins, size_t nout, size_t nmat, size_t R) {
  const size_t B = (size_t)b->B, m = (size_t)b->m;
  auto &sg = b->bd;
  if (bp_reserve_maps(b)) return OSQP_MEM_ALLOC_ERROR;
  if (balloc_once(b, &sg.act, B * m) || balloc_once(b, &sg.stat, B) || balloc_once(b, &sg.piv, B)) {
    (void)hipGetLastError();
    return OSQP_MEM_ALLOC_ERROR;
  }
  size_t nin = 0, nmat_in = 0;                   // (the input staging is the host route's alone)
  if (!dev) for (const BDIn &t : ins) if (t.src) (t.mat ? nmat_in : nin) += t.cnt;
  nout = std::max((size_t)1, nout);
  if (bd_reserve(&sg.out, &sg.out_cap, nout) || bd_reserve(&sg.in, &sg.in_cap, nin) ||
      bd_reserve(&sg.mat, &sg.mat_cap, std::max(nmat, nmat_in)))
    return OSQP_MEM_ALLOC_ERROR;
  *pl = b->pol;
  pl->stat = sg.piv;
  double *vec = sg.in, *mat = sg.mat;
  for (const BDIn &t : ins) {
    *t.slot = t.src;
    if (dev || !t.src) continue;
    double *&dst = t.mat ? mat : vec;
    BCHK(hipMemcpyAsync(dst, t.src, t.cnt * sizeof(double), hipMemcpyHostToDevice, b->stream));
    *t.slot = dst;
    dst += t.cnt;
  }
  BCHK(hipMemsetAsync(sg.out, 0, nout * sizeof(double), b->stream));
  BCHK(hipMemsetAsync(sg.act, 0, std::max((size_t)1, R * m) * sizeof(int), b->stream));
  BCHK(hipMemsetAsync(sg.stat, 0, R * sizeof(int), b->stream));
  if (nmat) BCHK(hipMemsetAsync(sg.mat, 0, nmat * sizeof(double), b->stream));
  return 0;
}

// What a derivative call hands back, each a (destination, staging, count) with null or 0 skipped, and the wait for the
// stream.  dev: device-to-device copies.  Otherwise to the host, where the ints arrive as int and are widened to
// c_int after the wait.
struct BDOut { void *dst; const void *src; size_t cnt; };
static c_int bd_deliver(osqp_amd_batch *b, bool dev, std::initializer_list<BDOut> floats, std::initializer_list<BDOut> ints) {
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  for (const BDOut &t : floats)
    if (t.dst && t.cnt) BCHK(hipMemcpyAsync(t.dst, t.src, t.cnt * sizeof(double), kind, b->stream));
  size_t total = 0;
  for (const BDOut &t : ints) if (t.dst) total += t.cnt;
  std::vector<int> h(dev ? 0 : total);
  int *hp = h.data();
  for (const BDOut &t : ints) {
    if (!t.dst || !t.cnt) continue;
    BCHK(hipMemcpyAsync(dev ? t.dst : (void *)hp, t.src, t.cnt * sizeof(int), kind, b->stream));
    if (!dev) hp += t.cnt;
  }
  BCHK(hipStreamSynchronize(b->stream));
  if (dev) return 0;
  hp = h.data();
  for (const BDOut &t : ints) {
    if (!t.dst) continue;
    for (size_t k = 0; k < t.cnt; k++) static_cast<c_int *>(t.dst)[k] = hp[k];
    hp += t.cnt;
  }
  return 0;
}


// adjoint derivatives for the solved members (batch_adjoint.h), ncot cotangents per member: polish's active rows, KKT
// matrix and inversion on polish's buffers, in the same chunks, one inversion for the ncot cotangents of a member;
// nothing of the solve state is written.  What the four entry points below share; dev: every array is on the device,
// dX and dY are read in place.
// the precondition of polish, adjoint and tangent: every member (members null), or every listed one, is solved on the
// current problem
static bool members_solved(const osqp_amd_batch *b, const c_int *members, c_int count) {
  if (!members) return b->solved;
  for (c_int k = 0; k < count; k++) if (!b->member_solved[(size_t)members[k]]) return false;
  return true;
}
// members (null: every member; a list the caller has checked): the _members form -- every array is compact, [count][.],
// the listed members must be solved on the current problem, and the staging is sized by count.
static c_int adjoint_call(osqp_amd_batch *b, bool dev, const char *what, c_int ncot, const c_float *dX, const c_float *dY,
                          c_float *dQ, c_float *dL, c_float *dU, c_float *dPx, c_float *dAx, void *active, void *status,
                          const c_int *members = nullptr, c_int count = 0) {
  if (!b || !members_solved(b, members, count)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (ncot < 1 || ncot > 65535) return OSQP_DATA_VALIDATION_ERROR;
  if (!dX || !dQ || (b->m > 0 && (!dL || !dU))) return OSQP_DATA_VALIDATION_ERROR;
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {dX, dY, dQ, dL, dU, dPx, dAx, active, status})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t B = members ? (size_t)count : (size_t)b->B, D = (size_t)ncot;   // (B: the rows of the call's arrays)
  const size_t n = (size_t)b->n, m = (size_t)b->m, nnzP = (size_t)b->nnzP, nnzA = (size_t)b->nnzA;
  const size_t nP = dPx ? B * D * nnzP : 0, nA = dAx ? B * D * nnzA : 0;   // only what the call asked for
  if (!m) dY = nullptr;
  const std::vector<int> sel(members, members + (members ? count : 0));
  if (members && members_upload(b, sel.data(), sel.size(), true)) return OSQP_MEM_ALLOC_ERROR;
  BPol pl;
  BAdj ad{};
  ad.ncot = (int)ncot;
  if (const c_int rc = bd_stage(b, &pl, dev, {{dX, B * D * n, &ad.gx, false}, {dY, B * D * m, &ad.gy, false}},
                                B * D * (n + 2 * m), nP + nA, B)) return rc;
  if (members) pl.pos = b->d_mpos;
  ad.dQ = b->bd.out; ad.dL = ad.dQ + B * D * n; ad.dU = ad.dL + B * D * m;
  ad.dPx = nP ? b->bd.mat : nullptr; ad.dAx = nA ? b->bd.mat + nP : nullptr;
  ad.active = b->bd.act; ad.stat = b->bd.stat;
  const bool blk = b->bk.H != nullptr;
  if (const c_int rc = bd_run(b, pl, what, bd_lds_of, blk ? KFN(k_ba_adjoint<BlockK, BlockK>) : KFN(k_ba_adjoint<FullK>), [&](const BPlan &pn, unsigned cnt, const int *lp) {
        if (blk) hipLaunchKernelGGL((k_ba_adjoint<BlockK, BlockK>), dim3(cnt, (unsigned)ncot), dim3(BP_NT), pn.lds, b->stream, b->pat, b->io, pl, ad, pn.NPOL, b->pol_refine, lp, bk_solver(b, pn.NS));
        else hipLaunchKernelGGL(k_ba_adjoint<FullK>, dim3(cnt, (unsigned)ncot), dim3(BP_NT), pn.lds, b->stream, b->pat, b->io, pl, ad, pn.NPOL, b->pol_refine, lp);
      }, members ? &sel : nullptr)) return rc;
  return bd_deliver(b, dev, {{dQ, ad.dQ, B * D * n}, {dL, ad.dL, B * D * m}, {dU, ad.dU, B * D * m}, {dPx, ad.dPx, nP}, {dAx, ad.dAx, nA}},
                    {{active, ad.active, B * m}, {status, ad.stat, B}});
}

extern "C" c_int osqp_amd_batch_adjoint(osqp_amd_batch *b, const c_float *dX, const c_float *dY,
                                        c_float *dQ, c_float *dL, c_float *dU, c_float *dPx, c_float *dAx,
                                        c_int *active, c_int *status_adjoint) {
  BC_UNSERVED(b, "osqp_amd_batch_adjoint");
  return adjoint_call(b, false, "adjoint", 1, dX, dY, dQ, dL, dU, dPx, dAx, active, status_adjoint);
}
extern "C" c_int osqp_amd_batch_adjoint_dev(osqp_amd_batch *b, const c_float *dX, const c_float *dY,
                                            c_float *dQ, c_float *dL, c_float *dU, c_float *dPx, c_float *dAx,
                                            int *active, int *status_adjoint) {
  BC_UNSERVED(b, "osqp_amd_batch_adjoint_dev");
  return adjoint_call(b, true, "adjoint", 1, dX, dY, dQ, dL, dU, dPx, dAx, active, status_adjoint);
}
extern "C" c_int osqp_amd_batch_adjoint_multi(osqp_amd_batch *b, c_int ncot, const c_float *dX, const c_float *dY,
                                              c_float *dQ, c_float *dL, c_float *dU, c_float *dPx, c_float *dAx,
                                              c_int *active, c_int *status_adjoint) {
  BC_UNSERVED(b, "osqp_amd_batch_adjoint_multi");
  return adjoint_call(b, false, "adjoint_multi", ncot, dX, dY, dQ, dL, dU, dPx, dAx, active, status_adjoint);
}
extern "C" c_int osqp_amd_batch_adjoint_multi_dev(osqp_amd_batch *b, c_int ncot, const c_float *dX, const c_float *dY,
                                                  c_float *dQ, c_float *dL, c_float *dU, c_float *dPx, c_float *dAx,
                                                  int *active, int *status_adjoint) {
  BC_UNSERVED(b, "osqp_amd_batch_adjoint_multi_dev");
  return adjoint_call(b, true, "adjoint_multi", ncot, dX, dY, dQ, dL, dU, dPx, dAx, active, status_adjoint);
}

// forward sensitivities for the solved members (batch_tangent.h): the adjoint's route, one inversion for the ndir
// directions of a member; nothing of the solve state is written.  dev: every array is on the device, the tangents
// are read in place.
static c_int tangent_call(osqp_amd_batch *b, bool dev, c_int ndir, const c_float *dQ, const c_float *dL, const c_float *dU,
                          const c_float *dPx, const c_float *dAx, c_float *dX, c_float *dY, void *active, void *status,
                          const c_int *members = nullptr, c_int count = 0) {
  if (!b || !members_solved(b, members, count)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (ndir < 1 || ndir > 65535 || !dX) return OSQP_DATA_VALIDATION_ERROR;
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {dQ, dL, dU, dPx, dAx, dX, dY, active, status})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t B = members ? (size_t)count : (size_t)b->B, D = (size_t)ndir;   // (B: the rows of the call's arrays)
  const size_t n = (size_t)b->n, m = (size_t)b->m, nnzP = (size_t)b->nnzP, nnzA = (size_t)b->nnzA;
  if (!m) dL = dU = nullptr;
  if (!nnzP) dPx = nullptr;
  if (!nnzA) dAx = nullptr;
  const std::vector<int> sel(members, members + (members ? count : 0));
  if (members && members_upload(b, sel.data(), sel.size(), true)) return OSQP_MEM_ALLOC_ERROR;
  BPol pl;
  BTan tg{};
  tg.ndir = (int)ndir;
  if (const c_int rc = bd_stage(b, &pl, dev, {{dQ, B * D * n, &tg.dQ, false}, {dL, B * D * m, &tg.dL, false}, {dU, B * D * m, &tg.dU, false},
                                              {dPx, B * D * nnzP, &tg.dPx, true}, {dAx, B * D * nnzA, &tg.dAx, true}},
                                B * D * (n + m), 0, B)) return rc;
  if (members) pl.pos = b->d_mpos;
  tg.dX = b->bd.out; tg.dY = tg.dX + B * D * n;
  tg.active = b->bd.act; tg.stat = b->bd.stat;
  const bool blk = b->bk.H != nullptr;
  if (const c_int rc = bd_run(b, pl, "tangent", bd_lds_of, blk ? KFN(k_bt_tangent<BlockK, BlockK>) : KFN(k_bt_tangent<FullK>), [&](const BPlan &pn, unsigned cnt, const int *lp) {
        if (blk) hipLaunchKernelGGL((k_bt_tangent<BlockK, BlockK>), dim3(cnt, (unsigned)ndir), dim3(BP_NT), pn.lds, b->stream, b->pat, b->io, pl, tg, pn.NPOL, b->pol_refine, lp, bk_solver(b, pn.NS));
        else hipLaunchKernelGGL(k_bt_tangent<FullK>, dim3(cnt, (unsigned)ndir), dim3(BP_NT), pn.lds, b->stream, b->pat, b->io, pl, tg, pn.NPOL, b->pol_refine, lp);
      }, members ? &sel : nullptr)) return rc;
  return bd_deliver(b, dev, {{dX, tg.dX, B * D * n}, {dY, tg.dY, B * D * m}}, {{active, tg.active, B * m}, {status, tg.stat, B}});
}

extern "C" c_int osqp_amd_batch_tangent(osqp_amd_batch *b, c_int ndir, const c_float *dQ, const c_float *dL, const c_float *dU,
                                        const c_float *dPx, const c_float *dAx, c_float *dX, c_float *dY,
                                        c_int *active, c_int *status_tangent) {
  BC_UNSERVED(b, "osqp_amd_batch_tangent");
  return tangent_call(b, false, ndir, dQ, dL, dU, dPx, dAx, dX, dY, active, status_tangent);
}
extern "C" c_int osqp_amd_batch_tangent_dev(osqp_amd_batch *b, c_int ndir, const c_float *dQ, const c_float *dL,
                                            const c_float *dU, const c_float *dPx, const c_float *dAx, c_float *dX,
                                            c_float *dY, int *active, int *status_tangent) {
  BC_UNSERVED(b, "osqp_amd_batch_tangent_dev");
  return tangent_call(b, true, ndir, dQ, dL, dU, dPx, dAx, dX, dY, active, status_tangent);
}

// osqp_amd_batch_get in its four forms; the arrays are [R][.], R = count with a list and B without (null = not asked
// for).  Without a list: one copy per array.  With one: k_batch_gather writes the listed rows into the caller's device
// array, or into the staging, from where one copy per array takes them to the host.
static c_int get_call(osqp_amd_batch *b, bool dev, const c_int *members, c_int count, c_float *X, c_float *Y, c_float *info8,
                      c_float *DX, c_float *DY) {
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {X, Y, info8, DX, DY})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t R = members ? (size_t)count : (size_t)b->B, n = (size_t)b->n, m = (size_t)b->m;
  const struct { c_float *dst; const double *src; size_t width; } rows[] = {
      {X, b->io.Xo, n}, {Y, b->io.Yo, m}, {info8, b->io.info, 8}, {DX, b->io.DXo, n}, {DY, b->io.DYo, m}};
  size_t total = 0;
  for (const auto &r : rows) if (r.dst) total += R * r.width;
  if (!total) return 0;
  if (members_put(b, members, count)) return OSQP_MEM_ALLOC_ERROR;
  if (members && !dev && stage_reserve(b, total, 0)) return OSQP_MEM_ALLOC_ERROR;
  const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  double *at = b->d_vals;
  for (const auto &r : rows) {
    const size_t len = R * r.width;
    if (!r.dst || !len) continue;
    const double *src = r.src;
    if (members) {
      hipLaunchKernelGGL(k_batch_gather, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, b->stream, dev ? r.dst : at, r.src,
                         (long long)r.width, (const int *)b->d_mlist, (long long)R);
      BCHK(hipGetLastError());
      src = at; at += len;
    }
    if (!members || !dev) BCHK(hipMemcpyAsync(r.dst, src, len * sizeof(double), out, b->stream));
  }
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_get(osqp_amd_batch *b, c_float *X, c_float *Y, c_float *info8,
                                   c_float *DX, c_float *DY) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return get_call(b, false, nullptr, 0, X, Y, info8, DX, DY);
}

// osqp_amd_batch_verify in its four forms (batch_verify.h): the 16-slot record of every member, or of the listed ones,
// on the raw data the handle holds now.  X, Y, DX, DY are [R][.], R = count with a list and B without; NULL = the
// handle's own io.Xo, io.Yo, io.DXo, io.DYo at the member's row.  The given arrays are read in place on the device route
// and go through the staging of the derivative calls on the host route; k_batch_verify writes the records into that
// staging, from where one copy takes them to V.  Needs no solve and writes nothing of the handle.
static c_int verify_call(osqp_amd_batch *b, bool dev, const c_int *members, c_int count, const c_float *X, const c_float *Y,
                         const c_float *DX, const c_float *DY, c_float eps_abs, c_float eps_rel, c_float *V) {
  if (!V || !std::isfinite(eps_abs) || !std::isfinite(eps_rel)) return OSQP_DATA_VALIDATION_ERROR;
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {X, Y, DX, DY, V})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t R = members ? (size_t)count : (size_t)b->B, n = (size_t)b->n, m = (size_t)b->m;
  if (members_put(b, members, count)) return OSQP_MEM_ALLOC_ERROR;
  BVer v{};
  v.eps_abs = eps_abs < 0 ? b->st.eps_abs : eps_abs; v.eps_rel = eps_rel < 0 ? b->st.eps_rel : eps_rel;
  v.eps_pinf = b->st.eps_pinf; v.eps_dinf = b->st.eps_dinf;
  const struct { const c_float *given; const double *own; const double **slot; size_t width; } ins[] = {
      {X, b->io.Xo, &v.X, n}, {m ? Y : nullptr, b->io.Yo, &v.Y, m}, {DX, b->io.DXo, &v.DX, n}, {m ? DY : nullptr, b->io.DYo, &v.DY, m}};
  size_t nin = 0;
  if (!dev) for (const auto &t : ins) if (t.given) nin += R * t.width;
  auto &sg = b->bd;
  if (bd_reserve(&sg.in, &sg.in_cap, nin) || bd_reserve(&sg.out, &sg.out_cap, R * BV_SLOTS)) return OSQP_MEM_ALLOC_ERROR;
  double *at = sg.in;
  for (int k = 0; k < 4; k++) {
    const auto &t = ins[k];
    *t.slot = t.given;
    if (!t.given) { *t.slot = t.own; v.own |= 1 << k; continue; }
    if (dev || !t.width) continue;
    BCHK(hipMemcpyAsync(at, t.given, R * t.width * sizeof(double), hipMemcpyHostToDevice, b->stream));
    *t.slot = at; at += R * t.width;
  }
  v.V = sg.out;
  const size_t lds = bv_lds_bytes(b->n, b->m);
  const int *list = members ? b->d_mlist : nullptr;
  set_dynamic_lds(KFN(k_batch_verify), lds);
  hipLaunchKernelGGL(k_batch_verify, dim3((unsigned)R), dim3(BV_NT), lds, b->stream, b->pat, b->io, v, list);
  BCHK(hipGetLastError());
  BCHK(hipMemcpyAsync(V, sg.out, R * BV_SLOTS * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, b->stream));
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_verify(osqp_amd_batch *b, const c_float *X, const c_float *Y, const c_float *DX,
                                       const c_float *DY, c_float eps_abs, c_float eps_rel, c_float *V) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return verify_call(b, false, nullptr, 0, X, Y, DX, DY, eps_abs, eps_rel, V);
}

// Test hook: one member's workspace as the last setup / update / solve left it (K^-1 un-permuted
// from the GEMV order on the host with the kernel's own g_index).
extern "C" c_int osqp_amd_batch_member(osqp_amd_batch *b, c_int qp, c_float *D, c_float *E, c_float *c, c_float *rho,
                                      c_int *ctype, c_float *Pv, c_float *Av, c_float *Kinv, c_int *NPo) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (qp < 0 || qp >= b->B) return OSQP_DATA_VALIDATION_ERROR;
  BCHK(hipSetDevice(b->device));
  const bool common = b->engine == OSQP_AMD_BATCH_COMMON;     // one slab of values, one K^-1, one rho: for any qp
  const bool streamed = b->engine == OSQP_AMD_BATCH_STREAMED || common;
  const int n = b->n, m = b->m, NP = streamed ? b->NPs : 16 * b->tile;
  const long long q = qp, qk = common ? 0 : qp, nv = (long long)b->nnzP + b->nnzA;
  std::vector<int> t(m);
  std::vector<double> wk(Kinv ? (size_t)NP * NP : 0);
  auto get = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream) : hipSuccess;
  };
  if (D) BCHK(get(D, b->io.Wd + q * n, n * sizeof(double)));
  if (E) BCHK(get(E, b->io.We + q * m, m * sizeof(double)));
  if (c) BCHK(get(c, b->io.Wc + q, sizeof(double)));
  if (rho && common) *rho = b->bc_rho;
  else if (rho) BCHK(get(rho, b->io.rho_io + q, sizeof(double)));
  if (ctype) BCHK(get(t.data(), b->io.Wt + q * m, m * sizeof(int)));
  if (Pv) BCHK(get(Pv, b->io.Wv + qk * nv, b->nnzP * sizeof(double)));
  if (Av) BCHK(get(Av, b->io.Wv + qk * nv + b->nnzP, b->nnzA * sizeof(double)));
  if (Kinv) BCHK(get(wk.data(), b->io.Wk + qk * NP * NP, wk.size() * sizeof(double)));
  BCHK(hipStreamSynchronize(b->stream));
  if (ctype) for (int i = 0; i < m; i++) ctype[i] = t[i];
  if (Kinv && streamed) {
    std::copy(wk.begin(), wk.end(), Kinv);      // row-major already
  } else if (Kinv) {
    for (int i = 0; i < NP; i++)
      for (int j = 0; j < NP; j++)
        Kinv[(size_t)i * NP + j] = wk[b->tile == 8 ? g_index<128, BT>(i, j) : g_index<64, BT>(i, j)];
  }
  if (NPo) *NPo = NP;
  return 0;
}

extern "C" c_int osqp_amd_batch_shape(osqp_amd_batch *b, c_int *engine, c_int *NP) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (engine) *engine = b->engine;
  if (NP) *NP = b->engine != OSQP_AMD_BATCH_TILED ? b->NPs : 16 * b->tile;
  return 0;
}

extern "C" c_int osqp_amd_batch_rounds(osqp_amd_batch *b, c_int *rounds, c_int *refined) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (rounds) *rounds = b->engine != OSQP_AMD_BATCH_TILED ? b->last_rounds : (b->solves ? 1 : 0);
  if (refined && b->engine == OSQP_AMD_BATCH_COMMON) *refined = b->bc_refine ? b->B : 0;   // one verdict for the batch
  else if (refined) {
    BCHK(hipSetDevice(b->device));
    std::vector<int> f;
    if (read_flags(b, f)) return -102;
    c_int c = 0;
    for (int v : f) c += (v & BF_REFINE) ? 1 : 0;
    *refined = c;
  }
  return 0;
}

// device pointers of the result arrays (for device-side gathers: RCCL all_gather)
extern "C" c_int osqp_amd_batch_device_ptrs(osqp_amd_batch *b, void **X, void **Y, void **info8) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (X) *X = b->io.Xo;
  if (Y) *Y = b->io.Yo;
  if (info8) *info8 = b->io.info;
  return 0;
}

#include "batch_devio.h"
#include "batch_members.h"
