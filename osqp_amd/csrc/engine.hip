// engine.hip -- device-resident OSQP ADMM engine for gfx950 (MI355X, CDNA4).
//
// What runs here (all fp64, int32 indices, one HIP stream per engine):
//   * the ADMM iteration of osqp_solve (reference src/osqp.c:356-370,
//     src/auxil.c:161-225, src/proj.c:4-14) as hipGraph replays of
//       k_pcg_init -> k_cg_A, k_cg_B (operator on u0) -> K x { k_cg_A, k_cg_B } -> k_admm_finalize
//   * the linear solve of update_xz_tilde as an indirect method: Jacobi-PCG on
//       (P + sigma I + A' diag(rho) A) x~ = sigma x - q + A'(rho.z - y)
//     (docs/solver/index.rst:50-55 in the reference), then z~ = A x~
//   * residual / tolerance / rho-estimate / infeasibility reductions of
//     update_info + check_termination (src/auxil.c:13-52, 227-512)
//
// Data layout in HBM:
//   A      : CSR (row gather for A x), built from the CSC the API hands over
//   M      : fused row matrix [P_full | A'] (n rows, n+m columns).  Row j holds
//            P(j, j..n) ascending, then P(j, 0..j) ascending, then column j of
//            A with column ids n+i -- i.e. exactly the summation order of the
//            reference's mat_vec + mat_tpose_vec(skip_diag) + mat_tpose_vec
//            (lin_alg.c:241-322), so P x and A' y are reproduced bit for bit.
//   vectors: [x | y], [x~ | rho z~], [0 | rho z - y], [p | t] (x2) are stored
//            contiguously so one fused SpMV over M consumes "n-part | m-part".
//
// SpMV scheme (all matrices): row blocks of <= chunk non-zeros are streamed
// with fully coalesced index/value loads, the products val*x[col] are staged in
// LDS, then each row segment is summed sequentially from LDS by one lane
// (CSR-stream).  Rows longer than a chunk are reduced by the whole workgroup
// with 64-lane wavefront shuffles.  Dot products are written as one partial
// per workgroup and re-reduced in a fixed order by every workgroup of the next
// kernel, so results are bitwise reproducible and PCG scalars never visit the
// host.
//
// What stays in this file: the host side.  All device code, the dense-direct form's host side and the test hooks stand in
// fragments, each included exactly once at the place where its text belongs.  They are pieces of this file, not headers that
// compile alone; each opens with where it is included, what it holds and what must stand before it.  In include order:
//  device, ahead of the host side
//   engine_device.h         constants, HIPCHK, RowBlk / G4 / DevMat / DenseP / State / Params / Ctx, timeline macros, scalar slots,
//                           reductions, the stream / long-row / dense-block SpMV pieces, LDS_DECL
//   engine_pcg_steps.h      launch-per-step PCG: k_vd, k_pcg_init, cg_step, k_cg_A, k_huge_reduce, k_cg_B, k_huge_dot, k_admm_finalize
//   engine_pcg_resident.h   resident PCG: ResCtx, the bounded waits, k_form_K, k_form_K_lists, k_pcg_resident
//   engine_pcg_blockres.h   block-resident PCG: BrCtx, k_pcg_blockres
//   engine_block_direct.h   block-direct solve: BdCtx, k_blk_*, k_cpl_*, k_cap_diag, k_cap_step
//   dense_direct.h          dense-direct solve: DdCtx, k_dd_*
//   engine_block_check.h    block-direct solve: k_blk_check, k_cap_check (they use dense_direct.h's probe vector)
//   engine_aux_kernels.h    k_elim_refresh, k_elim_split, k_precond, k_refresh_m, k_spmv
//   engine_check_kernels.h  k_residuals, k_final_sums, k_certificates
//   engine_ruiz_kernels.h   Ruiz equilibration: k_ruiz_*
//   engine_util_kernels.h   k_fill, k_fill_ranges, k_start_reset, k_window_begin, k_repack
//  inside and behind the host side
//   dense_direct_host.h     build_dense_direct, dd_refresh, launch_dense_direct, the dense-direct test hooks
//   engine_hooks.h          entry points for tests and measurements
//   kkt_sens.h              derivatives of the solution (k_sens_*)
//   verify.h                a point against the raw problem (k_ver_*)
//   rowpart_native.h        one QP over several GPUs by rows (k_rp_*)
// The order is pinned: the kernels, and the instantiations of the kernel templates, stand in the code object in the order of
// the text (host text included: a host launch instantiates its kernel template), the hand-tuned kernels are sensitive to their
// place there, and the check of a change that only moves text is that the device assembly of this translation unit stays what it
// was.  A new fragment goes where its text would have gone.  Macros cross the seams (HIPCHK, TB and the other constants, TL_MARK /
// TLK_*, LDS_DECL): the header of a fragment that uses one names the fragment that defines it.

#include <hip/hip_runtime.h>
#include <cstdio>
#include <new>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <climits>
#include <limits>
#include <cmath>
#include <vector>
#include <map>
#include <algorithm>
#include <mutex>
#include <condition_variable>
#include <thread>
#include <atomic>
#include <chrono>
#include "../../include/osqp_amd_engine.h"

// device (the map above says what each fragment holds)
#include "engine_device.h"
#include "engine_pcg_steps.h"
#include "engine_pcg_resident.h"
#include "engine_pcg_blockres.h"
#include "engine_block_direct.h"
#include "dense_direct.h"
#include "engine_block_check.h"
#include "engine_aux_kernels.h"
#include "engine_check_kernels.h"
#include "engine_ruiz_kernels.h"
#include "engine_util_kernels.h"

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct HostMat {         // host image of a device CSR matrix
  int nrows = 0, ncols = 0, nstream = 0, nwave = 0;
  std::vector<int> rowptr, col, split;
  std::vector<double> val;
  std::vector<RowBlk> blk;
  int *d_rowptr = nullptr, *d_col = nullptr, *d_split = nullptr;
  unsigned short *d_col16 = nullptr;
  double *d_val = nullptr;
  RowBlk *d_blk = nullptr;
};

// ---- the OSQP_AMD_* switches of the single-QP engine: one row each, one reader, one struct ----
// read_switches() is the only place of this translation unit that looks at the environment, and a pure function of it.  Every hipeng
// takes its values when it is made (hipeng::sw, a member initialiser: the plan temporaries of the CPU hooks have them too), and
// every use site reads e->sw.  A clamp that depends on the problem (RESIDENT_NWG, BLOCK_FIN_DOTS) stays at its use site.
enum SwKind : int { SW_FLAG = 0, SW_INT = 1, SW_DOUBLE = 2, SW_INT_PAIR = 3, SW_TEXT = 4 };   // atoi != 0 / atoi / atof / sscanf "%d,%d" / the string itself
enum SwRange : int { SW_ANY = 0, SW_CLAMP = 1, SW_IGNORE = 2 };    // a value outside [lo, hi] is taken as it is / clamped / ignored (the switch then reads as not set)
constexpr int SW_UNSET = -1;     // what the field of an `unset is distinct` row holds while its variable is not set: the use site works out the default
struct Switches {
  int resident, resident_min_n, resident_all_cus, resident_nwg, resident_banks, resident_pipe, resident_predict;
  double resident_predict_margin;
  int resident_inject, resident_u0, resident_fine, resident_blocks, init_resident_stores, form_k_lists;
  double form_k_list_mb;
  int setup_threads, block_direct, block_coupled_max, block_fin_dots, block_plain;
  int dense_p, dense_direct, dense_small, dense_symv, dense_one_gather, dense_chol, dense_gemm_lds;
  int elim, hfold, split, chunk, fin_grid, fused_check;
  double extrap;
  int extrap_sched[2];
  int khead, graph_segs, trace;
  char trace_maps[PATH_MAX];
};
struct SwRow { const char *name; SwKind kind; size_t field; double def, def2; SwRange range; double lo, hi; bool unset_distinct; const char *what; };
#define SW(field) offsetof(Switches, field)
#define SW_NAME(x) "OSQP_AMD_" x
constexpr double SW_INF = std::numeric_limits<double>::infinity(), SW_TINY = std::numeric_limits<double>::denorm_min();    // [SW_TINY, SW_INF]: v > 0
static const SwRow SW_TABLE[] = {
  // name                                  kind         field                         default  range      lo   hi         unset distinct
  {SW_NAME("RESIDENT"),                    SW_FLAG,     SW(resident),                 1, 0,    SW_ANY,    0, 0,           false, "0: never a one-launch form (resident PCG, block-resident PCG, block-direct solve)"},
  {SW_NAME("RESIDENT_MIN_N"),              SW_INT,      SW(resident_min_n),           256, 0,  SW_ANY,    0, 0,           false, "smallest n that takes the resident PCG"},
  {SW_NAME("RESIDENT_ALL_CUS"),            SW_FLAG,     SW(resident_all_cus),         0, 0,    SW_ANY,    0, 0,           false, "1: a resident grid may take every CU (default: one per XCD stays free)"},
  {SW_NAME("RESIDENT_NWG"),                SW_INT,      SW(resident_nwg),             0, 0,    SW_ANY,    0, 0,           false, "> 0: at least this many workgroups per resident launch, at most the plan's CUs (0: sized to the problem)"},
  {SW_NAME("RESIDENT_BANKS"),              SW_FLAG,     SW(resident_banks),           1, 0,    SW_ANY,    0, 0,           false, "0: a thread's entries of K in row order instead of spread over the LDS bank pairs"},
  {SW_NAME("RESIDENT_PIPE"),               SW_FLAG,     SW(resident_pipe),            1, 0,    SW_ANY,    0, 0,           false, "0: Chronopoulos-Gear recurrences only, never the pipelined ones"},
  {SW_NAME("RESIDENT_PREDICT"),            SW_FLAG,     SW(resident_predict),         1, 0,    SW_ANY,    0, 0,           false, "0: no predicted last trip in the pipelined phase"},
  {SW_NAME("RESIDENT_PREDICT_MARGIN"),     SW_DOUBLE,   SW(resident_predict_margin),  1.0, 0,  SW_IGNORE, SW_TINY, SW_INF, false, "last trip predicted at |r|^2 <= margin x tol^2; taken only if > 0"},
  {SW_NAME("RESIDENT_INJECT"),             SW_INT,      SW(resident_inject),          0, 0,    SW_ANY,    0, 0,           false, "test hook: the resident launch of ADMM iteration k gives up"},
  {SW_NAME("RESIDENT_U0"),                 SW_FLAG,     SW(resident_u0),              1, 0,    SW_ANY,    0, 0,           false, "0: exchange the first vector instead of reading it from memory"},
  {SW_NAME("RESIDENT_FINE"),               SW_INT,      SW(resident_fine),            2, 0,    SW_ANY,    0, 0,           false, "polled words in uncached (2), fine-grained (1) or ordinary (0) device memory"},
  {SW_NAME("RESIDENT_BLOCKS"),             SW_FLAG,     SW(resident_blocks),          1, 0,    SW_ANY,    0, 0,           false, "0: neither block form"},
  {SW_NAME("INIT_RESIDENT_STORES"),        SW_FLAG,     SW(init_resident_stores),     1, 0,    SW_ANY,    0, 0,           false, "0: k_pcg_init of the resident graphs also stores r0 and u0 where the launch-per-step kernels want them"},
  {SW_NAME("FORM_K_LISTS"),                SW_FLAG,     SW(form_k_lists),             1, 0,    SW_ANY,    0, 0,           false, "0: k_form_K (merge on the device) instead of k_form_K_lists"},
  {SW_NAME("FORM_K_LIST_MB"),              SW_DOUBLE,   SW(form_k_list_mb),           128.0, 0, SW_CLAMP, 0.0, 1e6,       false, "budget of the contribution lists in MiB"},
  {SW_NAME("SETUP_THREADS"),               SW_INT,      SW(setup_threads),            0, 0,    SW_CLAMP,  1, 64,          true,  "host threads of the resident set-up (unset: min(8, cores))"},
  {SW_NAME("BLOCK_DIRECT"),                SW_FLAG,     SW(block_direct),             1, 0,    SW_ANY,    0, 0,           false, "0: the block-resident PCG instead of the block-direct solve"},
  {SW_NAME("BLOCK_COUPLED_MAX"),           SW_INT,      SW(block_coupled_max),        CPL_MAX, 0, SW_CLAMP, 0, CPL_MAX,   false, "most coupling rows of A the block-direct solve carries as its low-rank term"},
  {SW_NAME("BLOCK_FIN_DOTS"),              SW_FLAG,     SW(block_fin_dots),           1, 0,    SW_ANY,    0, 0,           false, "0: a k_huge_dot launch per iteration even where the block-direct kernels could leave the partials"},
  {SW_NAME("BLOCK_PLAIN"),                 SW_FLAG,     SW(block_plain),              0, 0,    SW_ANY,    0, 0,           false, "1: block-direct solve on the right-hand side with the low-rank rows' terms split off"},
  {SW_NAME("DENSE_P"),                     SW_FLAG,     SW(dense_p),                  1, 0,    SW_ANY,    0, 0,           false, "0: no kernel path of their own for dense diagonal blocks of P"},
  {SW_NAME("DENSE_DIRECT"),                SW_INT,      SW(dense_direct),             1, 0,    SW_ANY,    0, 0,           false, "dense-direct solve: 0 never, 1 where it pays, 2 whenever it fits"},
  {SW_NAME("DENSE_SMALL"),                 SW_INT,      SW(dense_small),              1024, 0, SW_CLAMP,  0, INT_MAX,     false, "most dense unknowns that take the dense-direct solve ahead of the resident PCG (0: none)"},
  {SW_NAME("DENSE_SYMV"),                  SW_FLAG,     SW(dense_symv),               0, 0,    SW_ANY,    0, 0,           true,  "dense-direct solve from the inverse's lower tiles (1) or all its entries (0) (unset: tiles from 2048 unknowns up)"},
  {SW_NAME("DENSE_ONE_GATHER"),            SW_FLAG,     SW(dense_one_gather),         1, 0,    SW_ANY,    0, 0,           false, "0: dense-direct engines gather vb and vx separately in k_pcg_init"},
  {SW_NAME("DENSE_CHOL"),                  SW_FLAG,     SW(dense_chol),               0, 0,    SW_ANY,    0, 0,           true,  "1: blocked Cholesky inversion at once (unset: the caller's default -- 0 in an engine's refresh, 1 in hipeng_dense_invert_selftest)"},
  {SW_NAME("DENSE_GEMM_LDS"),              SW_FLAG,     SW(dense_gemm_lds),           1, 0,    SW_ANY,    0, 0,           false, "0: the dense-direct GEMM kernel that feeds the MFMAs from global memory"},
  {SW_NAME("ELIM"),                        SW_FLAG,     SW(elim),                     1, 0,    SW_ANY,    0, 0,           false, "0: no slack-like variable is eliminated from the linear system"},
  {SW_NAME("HFOLD"),                       SW_FLAG,     SW(hfold),                    1, 0,    SW_ANY,    0, 0,           false, "0: huge rows of A finish their sums in k_huge_reduce instead of inside k_cg_B"},
  {SW_NAME("SPLIT"),                       SW_FLAG,     SW(split),                    0, 0,    SW_ANY,    0, 0,           true,  "vector update and operator apply as two launches (unset: when most of A sits in long rows)"},
  {SW_NAME("CHUNK"),                       SW_INT,      SW(chunk),                    0, 0,    SW_IGNORE, 64, MAX_CHUNK,  true,  "products per row block (unset or outside [64, 2048]: pick_chunk)"},
  {SW_NAME("FIN_GRID"),                    SW_INT,      SW(fin_grid),                 0, 0,    SW_CLAMP,  1, INT_MAX,     true,  "workgroups of k_admm_finalize (unset: computed from the problem)"},
  {SW_NAME("FUSED_CHECK"),                 SW_FLAG,     SW(fused_check),              1, 0,    SW_ANY,    0, 0,           false, "0: a window that ends in a check waits twice; prologue and resets one operation per field"},
  {SW_NAME("EXTRAP"),                      SW_DOUBLE,   SW(extrap),                   1.0, 0,  SW_ANY,    0, 0,           false, "theta of the extrapolated PCG start (0: plain warm start)"},
  {SW_NAME("EXTRAP_SCHED"),                SW_INT_PAIR, SW(extrap_sched),             5, 12,   SW_ANY,    0, 0,           false, "h0,h1: history lengths of the extrapolated start"},
  {SW_NAME("KHEAD"),                       SW_INT,      SW(khead),                    1, 0,    SW_ANY,    0, 0,           false, "unrolled PCG slots beyond the last window's maximum"},
  {SW_NAME("GRAPH_SEGS"),                  SW_INT,      SW(graph_segs),               5, 0,    SW_CLAMP,  1, 32,          false, "ADMM iterations captured per hipGraph"},
  {SW_NAME("TRACE"),                       SW_INT,      SW(trace),                    0, 0,    SW_CLAMP,  1, INT_MAX,     false, "set: 1 = one line per window, 2 = every HIP call of the run loop"},
  {SW_NAME("TRACE_MAPS"),                  SW_TEXT,     SW(trace_maps),               0, 0,    SW_ANY,    0, 0,           false, "with TRACE >= 2: file that receives /proc/self/maps once per process"},
};
#undef SW_NAME
#undef SW
constexpr int SW_COUNT = (int)(sizeof(SW_TABLE) / sizeof(SW_TABLE[0]));
static Switches read_switches() {
  Switches sw{};
  for (const SwRow &r : SW_TABLE) {
    char *at = reinterpret_cast<char *>(&sw) + r.field;
    int *iv = reinterpret_cast<int *>(at);
    double *dv = reinterpret_cast<double *>(at);
    const char *x = getenv(r.name);
    if (r.kind == SW_TEXT) { if (x) snprintf(at, PATH_MAX, "%s", x); continue; }
    if (r.kind == SW_INT_PAIR) { iv[0] = (int)r.def; iv[1] = (int)r.def2; if (x) sscanf(x, "%d,%d", &iv[0], &iv[1]); continue; }
    if (r.kind == SW_DOUBLE) {
      double v = x ? atof(x) : r.def;
      if (x && r.range == SW_CLAMP) v = std::max(r.lo, std::min(r.hi, v));
      if (x && r.range == SW_IGNORE && !(v >= r.lo && v <= r.hi)) v = r.def;
      *dv = v;
      continue;
    }
    const int unset = r.unset_distinct ? SW_UNSET : (int)r.def;
    int v = unset;
    if (x) {
      v = r.kind == SW_FLAG ? atoi(x) != 0 : atoi(x);
      if (r.range == SW_CLAMP) v = std::max((int)r.lo, std::min((int)r.hi, v));
      if (r.range == SW_IGNORE && (v < (int)r.lo || v > (int)r.hi)) v = unset;
    }
    *iv = v;
  }
  return sw;
}

// How an engine solves the linear system of an ADMM iteration (the values are hipeng_resident_info [9]): launch-per-step PCG kernels only,
// k_pcg_resident, k_pcg_blockres, block-direct solve (k_blk_apply / k_blk_finish), dense-direct solve (dense_direct.h)
enum SolveForm : int { FORM_STEPS = 0, FORM_RESIDENT = 1, FORM_BLOCKRES = 2, FORM_BLOCK_DIRECT = 3, FORM_DENSE_DIRECT = 4 };
struct hipeng {
  Switches sw = read_switches();       // the environment as it was when this engine was made
  int device = 0;
  int n = 0, m = 0;
  hipStream_t stream = nullptr;
  HostMat A, M, Mr;                    // Mr: remainder of M outside P's dense blocks (empty: no dense blocks)
  std::vector<int> Mr_src, dP_src;     // slot in M of every Mr entry / dense entry (-1: structural zero)
  std::vector<int> hrows, hcol_src;    // huge rows of A folded into k_cg_B; slot in M of hcol_k[j] (-1: zero)
  int *d_hcol_src = nullptr;
  double *d_hcol = nullptr;
  std::vector<DenseBlk> dP_blks;
  int *d_Mr_src = nullptr, *d_dP_src = nullptr;
  DenseBlk *d_dP_blks = nullptr;
  double *d_dP_val = nullptr;
  std::vector<int> A_csc2csr;          // CSC slot of A -> CSR slot
  std::vector<int> P_toM_up, P_toM_lo; // triu(P) slot -> slots in M (lo = -1 on the diagonal)
  std::vector<int> A_toM;              // CSC slot of A -> slot in M
  std::vector<double> pdiag;
  Ctx c{};
  Params prm{};
  Params *d_prm = nullptr;
  std::vector<void *> allocs;
  std::map<int, hipGraphExec_t> graphs;
  int K = 8;
  int spec_lo = 0;           // unrolled slots below this prefetch without a look at the flags (smallest count of the last window); pcg_count_will_jump()
  bool split = false;     // large A: vector update and operator apply as two launches (plain 8-byte gathers)
  int rlA = 8, rlM = 8;   // lanes per row segment in the PCG kernels
  bool calibrated = false;   // a window has sized K since the PCG iteration count last jumped: pcg_count_will_jump() (the host-call table)
  double ex_theta0 = 1.0;    // OSQP_AMD_EXTRAP (0 disables the extrapolated PCG start)
  bool start_dirty = true;   // the PCG start history is void: start_history_void(), hipeng_run_admm consumes it (the host-call table)
  long long admm_total = 0;            // host copy of State::admm_done
  State *h_state = nullptr;            // pinned staging for the state read-back and the target upload
  long long *h_target = nullptr;
  // sw.fused_check (default 1): a window that ends in a check enqueues the residual pass behind its graphs and waits once
  // (hipeng_run_admm_check); the window's prologue, hipeng_cold_start and reset_start are one launch each.  0: one operation per field / array.
  double *h_check = nullptr;           // pinned: the scalars' lines followed by State, as they lie on the device (one D2H copy)
  hipeng_stats stats{};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  long long admm_done_seen = 0;
  SolveForm form = FORM_STEPS;   // what set-up built (direct_disable takes an engine back to FORM_STEPS for good)
  bool res_use = false;      // ... and in use (a launch that gave up suspends it)
  int res_fails = 0;         // launches that gave up waiting, in a row (one sends the rest of the run_admm call to the launch-per-step
                             // kernels; the third in a row sends the engine there for good; a call without one starts the count again)
  long long res_gave_up = 0; // ... since create
  int res_cus = 248;         // CUs a process's resident launches may hold together on this device (all but one per XCD)
  long long res_slow = 0, res_slow_max = 0, res_repub = 0;   // State::res_slow / res_slow_max / res_repub added up over the windows
  long long res_slow_hist[4] = {0, 0, 0, 0}; unsigned res_slow_xcc = 0; int res_slow_last[4] = {0, 0, 0, 0};
  ResCtx rc{};
  BrCtx bc{};                // FORM_BLOCKRES
  BdCtx bd{};                // FORM_BLOCK_DIRECT
  DdCtx dd{};                // FORM_DENSE_DIRECT
  double *dd_init_r = nullptr; int dd_init_stride = 4; double dd_check = 0.0; bool dd_chol = false;   // what direct_disable restores; the last inverse's check; the Cholesky route was needed
  bool elim_rhs_dirty = false;   // the m-part of the right-hand side (with eliminated variables: their q_y and coefficients, elim_vb) must be formed again: rhs_m_stale(), the host-call table
  std::vector<double> h_rho; // host copy of rho (the capacitance matrix of the block-direct form needs the huge rows' entries)
  std::vector<int> erow, ecol, epos;   // host images of Ctx::erow / ecol / epos (empty: no variable is eliminated)
  size_t res_lds = 0;
  long long res_nnz = 0;
  bool fk_lists = false;     // resident PCG: k_form_K_lists forms K (else k_form_K); terms, bytes of the lists, their budget in bytes
  long long fk_terms = 0, fk_bytes = 0, fk_budget = 0;
  bool explicit_inverse() const { return form == FORM_BLOCK_DIRECT || form == FORM_DENSE_DIRECT; }
  bool one_launch() const { return form == FORM_RESIDENT || form == FORM_BLOCKRES; }      // one launch per solve: it needs the CU lease
  bool resident_available() const { return form != FORM_STEPS && res_fails < 3; }         // (a launch that gave up suspends the mode for the rest of that call only)
  int one_launch_grid() const { return form == FORM_BLOCKRES ? bc.nwg : rc.nwg; }         // grid, debug buffer and exchange buffer of the one-launch forms
  int *one_launch_dbg() const { return form == FORM_BLOCKRES ? bc.dbg : rc.dbg; }
  const double *one_launch_sbuf() const { return form == FORM_BLOCKRES ? bc.sbuf : rc.sbuf; }
};

static int elem_grid(int cnt) { return std::max(1, std::min((cnt + TB - 1) / TB, MAX_PARTS)); }
// ---- the launches that several host calls share ----
static void launch_spmv(hipeng *e, const DevMat &Mx, const double *in, double *out, int sel) { hipLaunchKernelGGL(k_spmv, dim3(std::min(MAX_PARTS, std::max(1, Mx.nblk))), dim3(TB), 0, e->stream, Mx, in, out, sel); }
static void launch_precond(hipeng *e) { hipLaunchKernelGGL(k_precond, dim3(elem_grid(e->n)), dim3(TB), 0, e->stream, e->c); }
static void launch_elim_refresh(hipeng *e) { if (e->c.nelim) hipLaunchKernelGGL(k_elim_refresh, dim3(elem_grid(e->m)), dim3(TB), 0, e->stream, e->c); }
// ---- what a host call leaves to do: each function is the only writer of its fields (hipeng_run_admm, the consumer, clears them);
// which entry point calls which is the host-call table of DESIGN 2 ----
static void pcg_count_will_jump(hipeng *e) { e->calibrated = false; e->spec_lo = 0; }   // two iterations to see where it lands, then whole windows
static void start_history_void(hipeng *e) { e->start_dirty = true; }                    // [x~ | rho z~] was rewritten from outside the loop: reset_start
static void rhs_m_stale(hipeng *e) { e->elim_rhs_dirty = true; }
// k_refresh_m forms the m-parts of the PCG input vectors again; a caller that rewrites the start vector's m-part with it voids the history
enum StartHistory { START_HISTORY_KEPT, START_HISTORY_VOID };
static void launch_refresh_m(hipeng *e, int zt_partial, StartHistory h) {
  hipLaunchKernelGGL(k_refresh_m, dim3(elem_grid(e->m)), dim3(TB), 0, e->stream, e->c, zt_partial);
  if (h == START_HISTORY_VOID) start_history_void(e);
}

template <typename T>
static int dev_alloc(hipeng *e, T **p, size_t count) {
  void *q = nullptr;
  if (count == 0) count = 1;
  HIPCHK(hipMalloc(&q, count * sizeof(T)));
  HIPCHK(hipMemsetAsync(q, 0, count * sizeof(T), e->stream));
  e->allocs.push_back(q);
  *p = static_cast<T *>(q);
  return 0;
}

// Words that one CU polls while another writes them (exchange flags, tagged granules) live in UNCACHED device memory
// (hipDeviceMallocUncached): in ordinary memory an XCD's L2 can keep an old copy of such a line for good (a whole XCD
// then polls the old value while the others have moved on: seen about once in 1e5 exchanges on small problems, with
// every kind of load); uncached polls are also faster (143.6 against 149.8 us per ADMM iteration at config 2).
// OSQP_AMD_RESIDENT_FINE=1: fine-grained (coherent) but cacheable; =0: like everything else.
template <typename T>
static int dev_alloc_polled(hipeng *e, T **p, size_t count) {
  const int fine = e->sw.resident_fine;
  if (!fine) return dev_alloc(e, p, count);
  void *q = nullptr;
  if (count == 0) count = 1;
  HIPCHK(hipExtMallocWithFlags(&q, count * sizeof(T), fine == 2 ? hipDeviceMallocUncached : hipDeviceMallocFinegrained));
  HIPCHK(hipMemsetAsync(q, 0, count * sizeof(T), e->stream));
  e->allocs.push_back(q);
  *p = static_cast<T *>(q);
  return 0;
}

// Greedy row blocks: as many whole rows as fit `chunk` products (at least one
// row; a single row may exceed MAX_CHUNK and then takes the long-row path).
static void build_blocks(HostMat &H, int chunk, bool huge_ok, const std::vector<char> *skip = nullptr, int long_row = LONG_ROW) {
  // stream blocks first (runs of consecutive short rows, at most `chunk` products),
  // then one block per long row: the PCG kernels give each long row a wavefront
  H.blk.clear();
  std::vector<RowBlk> longs, huges;
  int r = 0;
  while (r < H.nrows) {
    if (skip && (*skip)[r]) { r++; continue; }     // rows served by another path (dense blocks of P)
    const int k0 = H.rowptr[r];
    if (H.rowptr[r + 1] - k0 >= long_row) {
      ((huge_ok && H.rowptr[r + 1] - k0 >= HUGE_ROW) ? huges : longs).push_back({r, r + 1, k0, H.rowptr[r + 1]});
      r++; continue;
    }
    int r1 = r + 1;
    while (r1 < H.nrows && !(skip && (*skip)[r1]) && H.rowptr[r1 + 1] - H.rowptr[r1] < long_row &&
           H.rowptr[r1 + 1] - k0 <= chunk && (r1 - r) < 8 * TB) r1++;
    H.blk.push_back({r, r1, k0, H.rowptr[r1]});
    r = r1;
  }
  H.nstream = (int)H.blk.size();
  H.blk.insert(H.blk.end(), longs.begin(), longs.end());
  H.nwave = (int)H.blk.size();
  H.blk.insert(H.blk.end(), huges.begin(), huges.end());
}

static int pick_chunk(const Switches &sw, long long nnz) {
  // about one to two workgroups per CU on small problems (every workgroup of a
  // consumer kernel re-reduces one dot partial per producer workgroup, so the
  // grid is kept near the CU count), full 2048-product chunks on large ones
  int chunk = 256;
  while (chunk < MAX_CHUNK && nnz / chunk > 640) chunk <<= 1;
  if (sw.chunk != SW_UNSET) chunk = sw.chunk;   // tuning experiments
  return chunk;
}

static int upload_mat(hipeng *e, HostMat &H) {
  if (dev_alloc(e, &H.d_rowptr, H.rowptr.size())) return HIPENG_ERR_HIP;
  if (dev_alloc(e, &H.d_col, H.col.size())) return HIPENG_ERR_HIP;
  if (dev_alloc(e, &H.d_val, H.val.size())) return HIPENG_ERR_HIP;
  if (dev_alloc(e, &H.d_blk, H.blk.size())) return HIPENG_ERR_HIP;
  HIPCHK(hipMemcpyAsync(H.d_rowptr, H.rowptr.data(), H.rowptr.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (!H.col.empty()) {
    HIPCHK(hipMemcpyAsync(H.d_col, H.col.data(), H.col.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(H.d_val, H.val.data(), H.val.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  }
  if (!H.blk.empty())
    HIPCHK(hipMemcpyAsync(H.d_blk, H.blk.data(), H.blk.size() * sizeof(RowBlk), hipMemcpyHostToDevice, e->stream));
  if (H.nwave > H.nstream && !H.col.empty() && *std::max_element(H.col.begin(), H.col.end()) <= 0xffff) {
    // long rows (one wavefront each in the PCG kernels) and every column id fits 16 bits: a second, narrower index array
    std::vector<unsigned short> c16(H.col.begin(), H.col.end());
    if (dev_alloc(e, &H.d_col16, c16.size())) return HIPENG_ERR_HIP;
    HIPCHK(hipMemcpyAsync(H.d_col16, c16.data(), c16.size() * sizeof(unsigned short), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));       // (the source is a local)
  }
  if (!H.split.empty()) {
    if (dev_alloc(e, &H.d_split, H.split.size())) return HIPENG_ERR_HIP;
    HIPCHK(hipMemcpyAsync(H.d_split, H.split.data(), H.split.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  }
  return 0;
}

static DevMat dev_view(const HostMat &H) {
  DevMat d;
  d.nrows = H.nrows; d.nblk = (int)H.blk.size(); d.nstream = H.nstream; d.nwave = H.nwave;
  d.rowptr = H.d_rowptr; d.col = H.d_col; d.col16 = H.d_col16; d.val = H.d_val; d.split = H.d_split; d.blk = H.d_blk;
  return d;
}

// CSC (int64) -> CSR (int32) of A, columns ascending inside each row.
static void build_A(hipeng *e, const csc *A) {
  const int n = e->n, m = e->m;
  const long long nnz = A->p[n];
  HostMat &H = e->A;
  H.nrows = m; H.ncols = n;
  H.rowptr.assign(m + 1, 0);
  for (long long k = 0; k < nnz; k++) H.rowptr[A->i[k] + 1]++;
  for (int i = 0; i < m; i++) H.rowptr[i + 1] += H.rowptr[i];
  H.col.assign(nnz, 0); H.val.assign(nnz, 0.0);
  e->A_csc2csr.assign(nnz, 0);
  std::vector<int> nxt(H.rowptr.begin(), H.rowptr.end() - 1);
  for (int j = 0; j < n; j++)
    for (long long k = A->p[j]; k < A->p[j + 1]; k++) {
      const int dst = nxt[A->i[k]]++;
      H.col[dst] = j; H.val[dst] = A->x[k];
      e->A_csc2csr[k] = dst;
    }
  build_blocks(H, pick_chunk(e->sw, nnz), true);     // k_cg_A slices huge rows over the grid
}

// Fused row matrix M = [P_full | A'] with the reference's summation order.
static void build_M(hipeng *e, const csc *P, const csc *A) {
  const int n = e->n;
  const long long nnzP = P->p[n], nnzA = A->p[n];
  HostMat &H = e->M;
  H.nrows = n; H.ncols = n + e->m;
  std::vector<int> up(n, 0), lo(n, 0);
  for (int j = 0; j < n; j++)
    for (long long k = P->p[j]; k < P->p[j + 1]; k++) {
      const int i = (int)P->i[k];
      up[i]++;                 // entry (i,j), j >= i : upper part of row i
      if (i != j) lo[j]++;     // mirrored entry (j,i), i < j : lower part of row j
    }
  H.rowptr.assign(n + 1, 0); H.split.assign(n, 0);
  for (int j = 0; j < n; j++) {
    H.split[j] = H.rowptr[j] + up[j] + lo[j];
    H.rowptr[j + 1] = H.split[j] + (int)(A->p[j + 1] - A->p[j]);
  }
  const long long tot = H.rowptr[n];
  H.col.assign(tot, 0); H.val.assign(tot, 0.0);
  e->P_toM_up.assign(nnzP, -1); e->P_toM_lo.assign(nnzP, -1); e->A_toM.assign(nnzA, -1);
  e->pdiag.assign(n, 0.0);
  std::vector<int> nu(n), nl(n);
  for (int j = 0; j < n; j++) { nu[j] = H.rowptr[j]; nl[j] = H.rowptr[j] + up[j]; }
  // scanning columns in ascending order fills each row's upper part in
  // ascending column order; a column's own entries (ascending rows) fill the
  // lower part of row j in ascending column order
  for (int j = 0; j < n; j++)
    for (long long k = P->p[j]; k < P->p[j + 1]; k++) {
      const int i = (int)P->i[k];
      int d = nu[i]++;
      H.col[d] = j; H.val[d] = P->x[k]; e->P_toM_up[k] = d;
      if (i != j) { d = nl[j]++; H.col[d] = i; H.val[d] = P->x[k]; e->P_toM_lo[k] = d; }
      else e->pdiag[j] = P->x[k];
    }
  for (int j = 0; j < n; j++) {
    int d = H.split[j];
    for (long long k = A->p[j]; k < A->p[j + 1]; k++, d++) {
      H.col[d] = n + (int)A->i[k]; H.val[d] = A->x[k]; e->A_toM[k] = d;
    }
  }
  build_blocks(H, pick_chunk(e->sw, tot), false);    // rows of M need their full sum inside k_cg_B
}

// Dense diagonal blocks of P (BASELINE config 5: block-diagonal covariance).  Column j
// starts a block iff no later column of triu(P) reaches above row j; a block of 32..128
// rows that is at least half full becomes a dense array for k_cg_B, the rest of M becomes the
// remainder matrix Mr.  Values of both are gathered from M on the device (k_repack), so
// every path that changes M (scaling, osqp_update_P/A) only has to repack.
static void build_dense(hipeng *e, const csc *P) {
  const int n = e->n;
  if (n == 0) return;
  std::vector<char> dense(n, 0);
  const HostMat &M = e->M;
  long long off = 0;
  if (!e->sw.dense_p) goto build_remainder;
  {
  std::vector<int> lo(n), smin(n + 1, n);
  for (int j = 0; j < n; j++) {
    lo[j] = j;
    for (long long k = P->p[j]; k < P->p[j + 1]; k++) lo[j] = std::min(lo[j], (int)P->i[k]);
  }
  for (int j = n - 1; j >= 0; j--) smin[j] = std::min(smin[j + 1], lo[j]);
  int s0 = 0;
  for (int j = 1; j <= n; j++) {
    if (j < n && smin[j] < j) continue;          // column j (or a later one) still reaches into the block
    const long long b = j - s0, nnz = P->p[j] - P->p[s0];
    long long pitch = (b + 1) & ~1ll;
    if (pitch % 32 == 0 && pitch < DENSE_MAX) pitch += 2;
    if (b >= 32 && b <= DENSE_MAX && 2 * nnz - b >= (b * b) / 2 && off + b * pitch < (1ll << 31)) {
      for (int i = s0; i < j; i++) dense[i] = 1;
      e->dP_blks.push_back({s0, (int)b, (int)off, (int)pitch});
      off += b * pitch;
    }
    s0 = j;
  }
  }
build_remainder:
  // Huge rows of A (sliced over the grid in k_cg_A): their entries leave the A' part of the matrix k_cg_B streams
  // and become dense n-vectors hcol_k[j] = A(h_k, j); k_cg_B adds hcol_k[j] * t_{h_k} to row j with
  // t_{h_k} = rho * (sum of the k_cg_A partials) formed by every workgroup itself -- no k_huge_reduce launch.
  e->hrows.clear();
  for (int q = e->A.nwave; q < (int)e->A.blk.size(); q++) e->hrows.push_back(e->A.blk[q].r0);
  if ((int)e->hrows.size() > MAX_HUGE_FOLD) e->hrows.clear();        // many huge rows: keep the k_huge_reduce path
  if (!e->sw.hfold) e->hrows.clear();   // tuning experiments
  if (e->dP_blks.empty() && e->hrows.empty()) return;
  std::vector<int> hidx(e->m > 0 ? e->m : 1, -1);
  for (size_t k = 0; k < e->hrows.size(); k++) hidx[e->hrows[k]] = (int)k;
  e->hcol_src.assign(e->hrows.size() * (size_t)n, -1);
  e->dP_src.assign((size_t)off, -1);
  for (const DenseBlk &d : e->dP_blks)
    for (int i = d.c0; i < d.c0 + d.b; i++)
      for (int k = M.rowptr[i]; k < M.split[i]; k++)     // P part of the row: all inside the block
        e->dP_src[(size_t)d.off + (size_t)(i - d.c0) * d.pitch + (M.col[k] - d.c0)] = k;
  HostMat &R = e->Mr;
  R.nrows = n; R.ncols = M.ncols;
  R.rowptr.assign(n + 1, 0);
  R.col.clear(); R.val.clear(); e->Mr_src.clear();
  for (int i = 0; i < n; i++) {
    for (int k = dense[i] ? M.split[i] : M.rowptr[i]; k < M.rowptr[i + 1]; k++) {
      if (k >= M.split[i] && hidx[M.col[k] - n] >= 0) { e->hcol_src[(size_t)hidx[M.col[k] - n] * n + i] = k; continue; }
      R.col.push_back(M.col[k]); R.val.push_back(M.val[k]); e->Mr_src.push_back(k);
    }
    R.rowptr[i + 1] = (int)R.col.size();
  }
  build_blocks(R, pick_chunk(e->sw, std::max(1, R.rowptr[n])), false, e->dP_blks.empty() ? nullptr : &dense);
}

// refresh the dense rows and the remainder matrix from the values of M (device side)
static int repack_dense(hipeng *e) {
  if (e->dP_blks.empty() && e->hrows.empty()) return 0;
  const long long nr = (long long)e->Mr_src.size(), nd = (long long)e->dP_src.size(), nh = (long long)e->hcol_src.size();
  if (nr) hipLaunchKernelGGL(k_repack, dim3((unsigned)std::min<long long>(4096, (nr + TB - 1) / TB)), dim3(TB), 0, e->stream,
                             e->M.d_val, e->d_Mr_src, e->Mr.d_val, nr);
  if (nd) hipLaunchKernelGGL(k_repack, dim3((unsigned)std::min<long long>(4096, (nd + TB - 1) / TB)), dim3(TB), 0, e->stream,
                             e->M.d_val, e->d_dP_src, e->d_dP_val, nd);
  if (nh) hipLaunchKernelGGL(k_repack, dim3((unsigned)std::min<long long>(4096, (nh + TB - 1) / TB)), dim3(TB), 0, e->stream,
                             e->M.d_val, e->d_hcol_src, e->d_hcol, nh);
  HIPCHK(hipGetLastError());
  return 0;
}


// ---- resident PCG: symbolic K, row partition, register layout --------------------------------------
// Resident launches need their workgroups co-resident, one per CU.  With grids sized to the problem several engines of one process
// can be inside resident windows at the same time as long as their grids fit the device together: a per-device budget of CUs
// (all but one per XCD), taken for the span launch ... sync of a window and handed back afterwards.  (Round 2 had a mutex here:
// "one QP per stream" then meant one resident QP at a time.)  Across processes there is no such book-keeping: a launch that
// finds CUs taken waits for them -- its first wait has 20 ms -- and gives up otherwise.
struct CuBudget { std::mutex mu; std::condition_variable cv; int avail = -1; };
static CuBudget g_res_cu[16];
struct CuLease {
  CuBudget *b = nullptr; int n = 0;
  void take(int device, int total, int want) {
    b = &g_res_cu[device & 15]; n = std::min(want, total);
    std::unique_lock<std::mutex> lk(b->mu);
    if (b->avail < 0) b->avail = total;
    b->cv.wait(lk, [&] { return b->avail >= n; });
    b->avail -= n;
  }
  void give() { if (b) { { std::lock_guard<std::mutex> lk(b->mu); b->avail += n; } b->cv.notify_all(); b = nullptr; } }
  ~CuLease() { give(); }
};
static const int RES_E_LIST[] = {8, 16, 20, 24, 32, 48, 64};

template <int E> static int res_set_lds(size_t lds) {
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_pcg_resident<E>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}
static void launch_dense_direct(hipeng *e);
static void launch_resident(hipeng *e) {
  const dim3 g(e->one_launch_grid()), b(RES_TB);
  const int gb = std::max(1, std::min(1024, e->c.dP.nblk));       // (block-direct)
  switch (e->form) {
    case FORM_STEPS: return;       // (no caller: get_graph asks for K = 0 only while res_use holds, which a FORM_STEPS engine never sets)
    case FORM_BLOCKRES:       // (ahead of FORM_RESIDENT: the instantiations of the two kernel templates keep their order in the code object)
      switch (e->c.nh) {
        case 0: hipLaunchKernelGGL(k_pcg_blockres<0>, g, b, 0, e->stream, e->c, e->bc); break;
        case 1: hipLaunchKernelGGL(k_pcg_blockres<1>, g, b, 0, e->stream, e->c, e->bc); break;
        case 2: hipLaunchKernelGGL(k_pcg_blockres<2>, g, b, 0, e->stream, e->c, e->bc); break;
        case 3: hipLaunchKernelGGL(k_pcg_blockres<3>, g, b, 0, e->stream, e->c, e->bc); break;
        default: hipLaunchKernelGGL(k_pcg_blockres<4>, g, b, 0, e->stream, e->c, e->bc); break;
      }
      return;
    case FORM_RESIDENT:
      switch (e->rc.E) {
        case 8:  hipLaunchKernelGGL(k_pcg_resident<8>,  g, b, e->res_lds, e->stream, e->c, e->rc); break;
        case 16: hipLaunchKernelGGL(k_pcg_resident<16>, g, b, e->res_lds, e->stream, e->c, e->rc); break;
        case 20: hipLaunchKernelGGL(k_pcg_resident<20>, g, b, e->res_lds, e->stream, e->c, e->rc); break;
        case 24: hipLaunchKernelGGL(k_pcg_resident<24>, g, b, e->res_lds, e->stream, e->c, e->rc); break;
        case 32: hipLaunchKernelGGL(k_pcg_resident<32>, g, b, e->res_lds, e->stream, e->c, e->rc); break;
        case 48: hipLaunchKernelGGL(k_pcg_resident<48>, g, b, e->res_lds, e->stream, e->c, e->rc); break;
        default: hipLaunchKernelGGL(k_pcg_resident<64>, g, b, e->res_lds, e->stream, e->c, e->rc); break;
      }
      return;
    case FORM_BLOCK_DIRECT:
      hipLaunchKernelGGL(k_blk_apply, dim3(gb), dim3(TB), 0, e->stream, e->c, e->bd, (const double *)e->c.init_r, e->bd.t, 1);
      if (e->bd.kc) {
        hipLaunchKernelGGL(k_cpl_dot, dim3(e->bd.kc), dim3(TB), 0, e->stream, e->c, e->bd, (const double *)e->bd.t, e->bd.cs, 1, 1, 0ll, 0ll, 1);
        hipLaunchKernelGGL(k_cpl_solve, dim3((e->bd.kc + TB / 64 - 1) / (TB / 64)), dim3(TB), 0, e->stream, e->c, e->bd);
        hipLaunchKernelGGL(k_blk_apply_back, dim3(gb), dim3(TB), 0, e->stream, e->c, e->bd);
      } else hipLaunchKernelGGL(k_blk_finish, dim3(std::max(1, std::min(256, (e->n + TB - 1) / TB))), dim3(TB), 0, e->stream, e->c, e->bd);
      return;
    case FORM_DENSE_DIRECT: launch_dense_direct(e); return;
  }
}

// Host-side set-up work of the resident PCG (symbolic K, register layout) is independent per row / per workgroup: a few threads.
template <class F>
static void parallel_chunks(const Switches &sw, int count, int min_chunk, F fn) {
  int T = sw.setup_threads != SW_UNSET ? sw.setup_threads : (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency()));
  T = std::min(T, std::max(1, count / min_chunk));
  if (T <= 1) { fn(0, count, 0, 1); return; }
  std::vector<std::thread> th;
  for (int k = 0; k < T; k++) th.emplace_back([=, &fn] { fn((int)((long long)count * k / T), (int)((long long)count * (k + 1) / T), k, T); });
  for (auto &t : th) t.join();
}

// Returns 0 (with e->form = FORM_RESIDENT when the problem qualifies) or a HIPENG error.  Not qualifying is not an error.
#define RES_NO(why) do { if (e->sw.trace) fprintf(stderr, "[osqp_amd] resident PCG not used: %s\n", why); return 0; } while (0)
// What build_resident works out on the host before anything is uploaded (hipeng_resident_plan hands it to the CPU tests).
struct ResPlanOut {
  bool ok = false; int nwg = 0, E = 0, npad = 0; long long nnzK = 0;
  std::vector<ResWG> wg; std::vector<int> Kptr, Kcol, kdst; std::vector<unsigned short> rowpos, col; std::vector<unsigned long long> brk;
  bool lists = false; std::vector<int> Kcp, Kcm, Kca;     // the contribution lists of k_form_K_lists, where they are in use
};
static int build_resident(hipeng *e, int plan_nwg = 0, ResPlanOut *po = nullptr) {
  const int n = e->n;       // (called on an engine that is still FORM_STEPS)
  if (!e->sw.resident) RES_NO("OSQP_AMD_RESIDENT=0");
  if (n < e->sw.resident_min_n || n > RES_MAXN) RES_NO("n outside [OSQP_AMD_RESIDENT_MIN_N, 15616]");
  if (!e->hrows.empty() || e->A.nwave < (int)e->A.blk.size()) RES_NO("A has rows of 8192 or more entries");   // (their outer products alone overflow the register files)
  int nwg = plan_nwg < 0 ? -plan_nwg : plan_nwg;      // (plan mode: nwg > 0 keeps that grid, nwg < 0 sizes the grid for a machine of -nwg CUs)
  const bool fixed_grid = po && plan_nwg > 0;
  if (!po) {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, e->device));
    // One CU per XCD stays free.  A grid that takes EVERY CU can be preempted in mid-launch when anything else wants a CU:
    // measured (profiles/r03_resident_slow_waits.txt) as waits of 1.05-1.10 ms, always the 32 workgroups of XCC 0 at once,
    // about once per 20-30 s of 256-workgroup launches and never with a smaller grid -- the time it takes to save and
    // restore an XCD's 32 x 570 KB of registers and LDS.  (Round 2's 1 ms wait limit turned each of them into a give-up.)
    nwg = std::min(256, prop.multiProcessorCount) - 8;
    if (e->sw.resident_all_cus) nwg += 8;
    e->res_cus = nwg;
    if (prop.sharedMemPerBlock < 64 * 1024) RES_NO("too little LDS");
  }
  if (nwg <= 0 || nwg > 256 || (long long)nwg * RES_MAXROWS < n) RES_NO("too few CUs");
  const HostMat &M = e->M, &A = e->A;
  const auto tb0 = std::chrono::steady_clock::now();
  for (int i = 0; i < n; i++)
    for (int k = M.split[i] + 1; k < M.rowptr[i + 1]; k++) if (M.col[k] <= M.col[k - 1]) RES_NO("a column of A is not sorted by row (or repeats one)");   // the merge in k_form_K wants ascending rows
  // pattern of K, row by row (sorted), with the slot of P(i,j) in M
  const size_t cap_total = (size_t)nwg * RES_PT * 64;
  std::vector<int> Kptr(n + 1, 0), Kcol, Kps;
  // Contribution lists for k_form_K_lists: for entry e of K, in the order of Kcol, the terms Kcp[e] .. Kcp[e + 1]; term q is row
  // k of A with a_ki at slot Kcm[q] of M and a_kj at slot Kca[q] of A, rows ascending (the order of column i in M).  Every pair
  // of entries of a row of A is one term: sum_k nnz(A_k)^2 of them, known before the pass, so that the budget
  // (OSQP_AMD_FORM_K_LIST_MB, 8 bytes per term + 4 per entry of K) decides the same for any number of threads.
  std::vector<int> Kcp, Kcm, Kca;
  long long fk_terms = 0;
  const long long fk_budget = (long long)e->sw.form_k_list_mb << 20;
  bool fk_lists = e->sw.form_k_lists != 0;
  for (int k = 0; k < e->m; k++) { const long long len = A.rowptr[k + 1] - A.rowptr[k]; fk_terms += len * len; }
  auto fk_bytes = [&](long long entries) { return 8 * fk_terms + 4 * (entries + 1); };
  if (fk_terms > 0x7fffffffLL || fk_bytes(n) > fk_budget) fk_lists = false;      // (K has n entries at least: the diagonal)
  {
    // rows in contiguous chunks, one thread each with its own scratch; the chunks' lists are joined in order afterwards
    std::vector<std::vector<int>> cKcol(64), cKps(64), cLen(64), cCnt(64), cCm(64), cCa(64);
    std::atomic<int> bad{0};
    int used = 1;
    parallel_chunks(e->sw, n, 256, [&](int lo, int hi, int tid, int T) {
      if (tid == 0) used = T;
      std::vector<int> mark(n, -1), pslot(n, -1);
      std::vector<int> &kc = cKcol[tid], &kp = cKps[tid], &ln = cLen[tid], &cn = cCnt[tid], &cm = cCm[tid], &ca = cCa[tid];
      std::vector<size_t> fill;
      kc.reserve((size_t)(hi - lo) * 64); ln.reserve(hi - lo);
      for (int i = lo; i < hi && !bad.load(std::memory_order_relaxed); i++) {
        const size_t start = kc.size();
        auto add = [&](int j) { if (mark[j] != i) { mark[j] = i; pslot[j] = -1; kc.push_back(j); } };
        add(i);
        for (int k = M.rowptr[i]; k < M.split[i]; k++) {
          const int j = M.col[k];
          add(j);
          if (pslot[j] != -1) { bad = 1; break; }
          pslot[j] = k;
        }
        for (int k = M.split[i]; k < M.rowptr[i + 1]; k++) {
          const int row = M.col[k] - n;
          for (int q = A.rowptr[row]; q < A.rowptr[row + 1]; q++) add(A.col[q]);
        }
        if (kc.size() > cap_total) { bad = 2; break; }
        std::sort(kc.begin() + start, kc.end());
        kp.resize(kc.size());
        for (size_t q = start; q < kc.size(); q++) kp[q] = pslot[kc[q]];
        ln.push_back((int)(kc.size() - start));
        if (fk_lists) {
          // the terms of this row's entries: counted per entry, then filled in the order of column i (ascending k)
          const size_t len = kc.size() - start, cstart = cn.size(), tstart = cm.size();
          for (size_t q = start; q < kc.size(); q++) pslot[kc[q]] = (int)(q - start);      // (pslot has served: now the entry's place in the row)
          cn.resize(cstart + len, 0);
          size_t terms = 0;
          for (int k = M.split[i]; k < M.rowptr[i + 1]; k++) {
            const int row = M.col[k] - n;
            for (int q = A.rowptr[row]; q < A.rowptr[row + 1]; q++) cn[cstart + pslot[A.col[q]]]++;
            terms += A.rowptr[row + 1] - A.rowptr[row];
          }
          fill.resize(len);
          size_t at = tstart;
          for (size_t q = 0; q < len; q++) { fill[q] = at; at += cn[cstart + q]; }
          cm.resize(tstart + terms); ca.resize(tstart + terms);
          for (int k = M.split[i]; k < M.rowptr[i + 1]; k++) {
            const int row = M.col[k] - n;
            for (int q = A.rowptr[row]; q < A.rowptr[row + 1]; q++) { const size_t d = fill[pslot[A.col[q]]]++; cm[d] = k; ca[d] = q; }
          }
        }
      }
    });
    if (bad.load() == 1) RES_NO("P repeats an entry");
    size_t tot = 0;
    for (int k = 0; k < used; k++) tot += cKcol[k].size();
    if (bad.load() == 2 || tot > cap_total) RES_NO("K has more entries than the register files hold");
    Kcol.reserve(tot); Kps.reserve(tot);
    int row = 0;
    for (int k = 0; k < used; k++) {
      Kcol.insert(Kcol.end(), cKcol[k].begin(), cKcol[k].end());
      Kps.insert(Kps.end(), cKps[k].begin(), cKps[k].end());
      for (int len : cLen[k]) { Kptr[row + 1] = Kptr[row] + len; row++; }
    }
    if (fk_lists && fk_bytes((long long)tot) > fk_budget) fk_lists = false;
    if (fk_lists) {
      Kcp.reserve(tot + 1); Kcm.reserve((size_t)fk_terms); Kca.reserve((size_t)fk_terms);
      Kcp.push_back(0);
      for (int k = 0; k < used; k++) {
        for (int cnt : cCnt[k]) Kcp.push_back(Kcp.back() + cnt);
        Kcm.insert(Kcm.end(), cCm[k].begin(), cCm[k].end());
        Kca.insert(Kca.end(), cCa[k].begin(), cCa[k].end());
      }
    }
  }
  const long long nnzK = Kptr[n];
  const auto tb1 = std::chrono::steady_clock::now();
  // contiguous row blocks, at most RES_MAXROWS rows and C entries each: smallest C that needs <= nwg blocks
  auto packs = [&](long long C) -> int {
    int g = 0, rows = 0; long long cnt = 0;
    for (int i = 0; i < n; i++) {
      const int len = Kptr[i + 1] - Kptr[i];
      if (len > C) return 1 << 30;
      if (rows > 0 && (cnt + len > C || rows == RES_MAXROWS)) { g++; cnt = 0; rows = 0; }
      cnt += len; rows++;
    }
    return g + 1;
  };
  // The grid is sized to the problem: every exchange is an all-to-all between the participating CUs and costs 2.3 us among
  // 4, 3.6 among 16, 4.2 among 64, 6.5 among 256 (profiles/r03_exchange_probe2.txt), while a thread's E entries cost about
  // 0.06 us each per product.  So: the smallest grid that keeps E <= 16 (halving E from 16 no longer pays for the doubled
  // grid), at most `nwg_max` = the CUs of the device; beyond that E grows (20, 24, ... at config 2: 256 workgroups, E = 20).
  // OSQP_AMD_RESIDENT_NWG overrides (tests, probes).
  const int nwg_max = nwg;
  long long maxrow = 1;
  for (int i = 0; i < n; i++) maxrow = std::max<long long>(maxrow, Kptr[i + 1] - Kptr[i]);
  if (packs(std::max<long long>(nnzK, 1)) > nwg_max) RES_NO("more than 61 rows per workgroup");
  int E = 0;
  long long C = 0;
  const int force_nwg = std::max(0, std::min(nwg_max, e->sw.resident_nwg));
  for (int cand : RES_E_LIST) {
    const long long cap = (long long)cand * RES_PT;
    if (cap < maxrow) continue;
    const int need = packs(cap);
    if (need > nwg_max) continue;
    if (!po && force_nwg > 0 && need > force_nwg) continue;
    E = cand; nwg = need;
    if (cand >= 16 || fixed_grid) break;
    // E = 8 fits: keep it only if E = 16 would not halve the grid (tiny problems: the rows, not the entries, set the grid)
    const int need16 = packs(16LL * RES_PT);
    if (need16 * 2 > need) break;
  }
  if (!E) RES_NO("a row block of K exceeds 448 x 64 entries");
  if (fixed_grid) nwg = nwg_max;               // (a plan for the CPU tests that keeps the grid it was asked for)
  else if (force_nwg > nwg) nwg = force_nwg;
  {
    // smallest block capacity that still needs no more than nwg blocks: balances the workgroups
    long long lo = maxrow, hi = (long long)E * RES_PT;
    while (lo < hi) { const long long mid = (lo + hi) / 2; if (packs(mid) <= nwg) hi = mid; else lo = mid + 1; }
    C = lo;
    if (fixed_grid) { E = 0; for (int cand : RES_E_LIST) if ((long long)cand * RES_PT >= C) { E = cand; break; } if (!E) RES_NO("a row block of K exceeds 448 x 64 entries"); }
  }
  std::vector<ResWG> wg(nwg, ResWG{n, 0, 0, 0});
  {
    int g = 0, rows = 0; long long cnt = 0; wg[0].r0 = 0;
    for (int i = 0; i < n; i++) {
      const int len = Kptr[i + 1] - Kptr[i];
      if (rows > 0 && (cnt + len > C || rows == RES_MAXROWS)) { wg[g].nr = rows; wg[g].cnt = (int)cnt; g++; wg[g].r0 = i; cnt = 0; rows = 0; }
      cnt += len; rows++;
    }
    wg[g].nr = rows; wg[g].cnt = (int)cnt;
  }
  // positions in the exchanged vector: a workgroup's rows, then its three dot partials, in lines of its own
  std::vector<unsigned short> rowpos(n, 0);
  int npad = 0;
  for (int g = 0; g < nwg; g++) {
    wg[g].pos = npad;
    for (int r = 0; r < wg[g].nr; r++) rowpos[wg[g].r0 + r] = (unsigned short)(npad + r);
    npad += ((wg[g].nr + 3 + 15) / 16) * 16;
  }
  if (npad > RES_MAXPAD) RES_NO("the exchanged vector (rows padded to whole lines) exceeds 16384 doubles");
  const size_t slots = (size_t)nwg * E * RES_PT;
  const bool bank_sched = e->sw.resident_banks != 0;
  std::vector<unsigned short> col(slots, 0), slot0((size_t)nwg * RES_PT, 0), segrow((size_t)nwg * (RES_MAXROWS + 1), 0);
  std::vector<unsigned char> rowl(slots, 0);
  std::vector<int> kdst((size_t)nnzK, 0);
  std::vector<unsigned long long> brk((size_t)nwg * RES_PT, 0ull);
  std::atomic<int> seg_over{0};
  parallel_chunks(e->sw, nwg, 4, [&](int g_lo, int g_hi, int, int) {        // workgroups write disjoint parts of every array
  for (int g = g_lo; g < g_hi; g++) {
    const ResWG &w = wg[g];
    if (w.nr == 0) continue;
    const int base = Kptr[w.r0];
    std::vector<int> rowof(w.cnt);
    for (int r = 0; r < w.nr; r++)
      for (int q = Kptr[w.r0 + r] - base; q < Kptr[w.r0 + r + 1] - base; q++) rowof[q] = r;
    // Order of the entries inside each thread's chunk.  One wave instruction of the product loop gathers 64 doubles from
    // LDS at the columns of the lanes' k-th entries; random columns pile up to ~6 lanes on one of the 32 bank pairs.
    // A chunk that lies inside one row may be summed in any order, so its entries are dealt to the E slots such that
    // each slot spreads over the bank pairs (a greedy deal, deterministic; pairwise swaps on top of it cost 0.3 s of setup
    // at config 2 for nothing measurable).
    std::vector<int> ord((size_t)RES_PT * E, -1);
    for (int le = 0; le < w.cnt; le++) ord[le] = le;
    if (bank_sched)
    for (int wq = 0; wq < RES_PT / 64; wq++) {
      int cntb[64][32];                           // [slot][bank pair] over the 64 lanes of this wavefront
      for (int k = 0; k < E; k++) for (int b = 0; b < 32; b++) cntb[k][b] = 0;
      bool freec[64];
      for (int l = 0; l < 64; l++) {
        const int t = wq * 64 + l, a = t * E;
        freec[l] = a + E <= w.cnt && rowof[a] == rowof[a + E - 1];
        if (!freec[l]) for (int k = 0; k < E && a + k < w.cnt; k++) cntb[k][rowpos[Kcol[base + a + k]] & 31]++;
      }
      for (int k = 0; k < E; k++)                 // deal: slot by slot, every free lane gives the entry whose bank pair is emptiest
        for (int l = 0; l < 64; l++) {
          if (!freec[l]) continue;
          const int a = (wq * 64 + l) * E;
          int best = k, bc = 1 << 30;
          for (int q = k; q < E; q++) { const int c = cntb[k][rowpos[Kcol[base + ord[a + q]]] & 31]; if (c < bc) { bc = c; best = q; } }
          std::swap(ord[a + k], ord[a + best]);
          cntb[k][rowpos[Kcol[base + ord[a + k]]] & 31]++;
        }
    }
    int nseg = 0, next_row = 0;
    for (int t = 0; t < RES_PT; t++) {
      slot0[(size_t)g * RES_PT + t] = (unsigned short)nseg;
      unsigned long long b = 0;
      for (int k = 0; k < E; k++) {
        if (t * E + k >= w.cnt) break;
        const int le = ord[t * E + k];
        const size_t sl = ((size_t)g * E + k) * RES_PT + t;
        col[sl] = rowpos[Kcol[base + le]]; rowl[sl] = (unsigned char)rowof[le]; kdst[base + le] = (int)sl;
        while (next_row <= rowof[le]) segrow[(size_t)g * (RES_MAXROWS + 1) + next_row++] = (unsigned short)nseg;   // first segment of the row
        const bool last = k == E - 1 || t * E + k + 1 >= w.cnt || rowof[ord[t * E + k + 1]] != rowof[le];
        if (last) { b |= 1ull << k; nseg++; }
      }
      brk[(size_t)g * RES_PT + t] = b;
    }
    for (int r = next_row; r <= RES_MAXROWS; r++) segrow[(size_t)g * (RES_MAXROWS + 1) + r] = (unsigned short)nseg;
    if (nseg > RES_TB + RES_MAXROWS) seg_over = 1;   // cannot happen (one segment per thread plus one per row change)
  }
  });
  if (seg_over.load()) return 0;
  const auto tb2 = std::chrono::steady_clock::now();
  if (po) {                      // plan only (no device): hand the layout out
    po->ok = true; po->nwg = nwg; po->E = E; po->npad = npad; po->nnzK = nnzK;
    po->wg = wg; po->Kptr = Kptr; po->Kcol = Kcol; po->kdst = kdst; po->rowpos = rowpos; po->col = col; po->brk = brk;
    po->lists = fk_lists; po->Kcp = Kcp; po->Kcm = Kcm; po->Kca = Kca;
    return 0;
  }
  ResCtx rc{};
  rc.nwg = nwg; rc.E = E; rc.npad = npad;
  rc.npw = (nwg + 63) / 64;
  rc.pipe = e->sw.resident_pipe;
  rc.predict = e->sw.resident_predict; rc.pred_margin = e->sw.resident_predict_margin;
  rc.u0_direct = e->sw.resident_u0;
  rc.inject = e->sw.resident_inject;
  unsigned short *d_rowpos = nullptr;
  std::vector<int> ppos(wg.size());
  for (size_t o = 0; o < wg.size(); o++) ppos[o] = wg[o].pos + wg[o].nr;
  int *d_ppos = nullptr;
  ResWG *d_wg = nullptr; unsigned short *d_col = nullptr, *d_slot0 = nullptr, *d_segrow = nullptr; unsigned char *d_rowl = nullptr;
  int *d_krp = nullptr, *d_kcj = nullptr, *d_kps = nullptr, *d_kdst = nullptr; unsigned long long *d_brk = nullptr;
  if (dev_alloc(e, &d_wg, wg.size()) || dev_alloc(e, &d_ppos, ppos.size()) || dev_alloc(e, &rc.val, slots) || dev_alloc(e, &d_col, slots) || dev_alloc(e, &d_rowl, slots) ||
      dev_alloc(e, &d_krp, Kptr.size()) || dev_alloc(e, &d_kcj, Kcol.size()) || dev_alloc(e, &d_kps, Kps.size()) || dev_alloc(e, &d_kdst, kdst.size()) ||
      dev_alloc(e, &d_brk, brk.size()) || dev_alloc(e, &d_slot0, slot0.size()) ||
      dev_alloc(e, &d_segrow, segrow.size()) || dev_alloc(e, &d_rowpos, rowpos.size()) || dev_alloc(e, &rc.ubuf, (size_t)2 * rc.npad) ||
      dev_alloc_polled(e, &rc.flags, (size_t)nwg * RES_FSTRIDE) || dev_alloc(e, &rc.dbg, (size_t)nwg * RES_DBG) || dev_alloc_polled(e, &rc.sbuf, (size_t)2 * nwg * RES_GSTRIDE)) return HIPENG_ERR_HIP;
#define UP(dst, src) HIPCHK(hipMemcpyAsync(dst, (src).data(), (src).size() * sizeof((src)[0]), hipMemcpyHostToDevice, e->stream))
  if (fk_lists) {
    int *d_kcp = nullptr, *d_kcm = nullptr, *d_kca = nullptr;
    if (dev_alloc(e, &d_kcp, Kcp.size()) || dev_alloc(e, &d_kcm, Kcm.size()) || dev_alloc(e, &d_kca, Kca.size())) return HIPENG_ERR_HIP;
    UP(d_kcp, Kcp); UP(d_kcm, Kcm); UP(d_kca, Kca);
    rc.kcp = d_kcp; rc.kcm = d_kcm; rc.kca = d_kca;
  }
  e->fk_lists = fk_lists; e->fk_terms = fk_terms; e->fk_bytes = fk_lists ? fk_bytes(nnzK) : 0; e->fk_budget = fk_budget;
  UP(d_wg, wg); UP(d_ppos, ppos); UP(d_rowpos, rowpos); UP(d_col, col); UP(d_rowl, rowl); UP(d_krp, Kptr); UP(d_kcj, Kcol); UP(d_kps, Kps); UP(d_kdst, kdst); UP(d_brk, brk); UP(d_slot0, slot0); UP(d_segrow, segrow);
#undef UP
  HIPCHK(hipStreamSynchronize(e->stream));       // the sources are locals
  {
    double *d_u0pos = nullptr;
    if (dev_alloc(e, &d_u0pos, (size_t)rc.npad)) return HIPENG_ERR_HIP;       // (zeroed: the padding positions are read, never written)
    e->c.u0map = d_rowpos; e->c.u0pos = d_u0pos;
    // OSQP_AMD_INIT_RESIDENT_STORES (default 1): k_pcg_init of the resident graphs stores r0 beside u0 in this layout and nothing else
    rc.r0pos = nullptr;
    if (e->sw.init_resident_stores && dev_alloc(e, &rc.r0pos, (size_t)rc.npad)) return HIPENG_ERR_HIP;
  }
  rc.wg = d_wg; rc.ppos = d_ppos; rc.rowpos = d_rowpos; rc.col = d_col; rc.rowl = d_rowl; rc.krp = d_krp; rc.kcj = d_kcj; rc.kps = d_kps; rc.kdst = d_kdst; rc.brk = d_brk; rc.slot0 = d_slot0; rc.segrow = d_segrow;
  e->rc = rc;
  e->res_lds = ((size_t)rc.npad + RES_TB + RES_MAXROWS + 3 + 16 + 768 + 5 * 64 + 96) * sizeof(double);   // + phase stamps of the TIMELINE build
  int rcode = 0;
  switch (E) {
    case 8: rcode = res_set_lds<8>(e->res_lds); break;   case 16: rcode = res_set_lds<16>(e->res_lds); break;
    case 20: rcode = res_set_lds<20>(e->res_lds); break; case 24: rcode = res_set_lds<24>(e->res_lds); break;
    case 32: rcode = res_set_lds<32>(e->res_lds); break; case 48: rcode = res_set_lds<48>(e->res_lds); break;
    default: rcode = res_set_lds<64>(e->res_lds); break;
  }
  if (rcode) RES_NO("the launch's LDS request was refused");
  e->res_nnz = nnzK;
  e->form = FORM_RESIDENT; e->res_use = true;
  if (e->sw.trace) {
    const auto tb3 = std::chrono::steady_clock::now();
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[osqp_amd] resident PCG: nnz(K)=%lld, %d workgroups x %d threads x %d entries, %zu B LDS; host: pattern %.0f ms, layout %.0f ms, upload %.0f ms\n",
            nnzK, nwg, RES_TB, E, e->res_lds, ms(tb0, tb1), ms(tb1, tb2), ms(tb2, tb3));
  }
  return 0;
}


// P consists of dense diagonal blocks only: they tile 0..n, none above DENSE_MAX.
static bool blocks_tile(hipeng *e) {
  if (e->dP_blks.empty()) return false;
  int next = 0;
  for (const DenseBlk &d : e->dP_blks) { if (d.c0 != next || d.b > DENSE_MAX) return false; next += d.b; }
  return next == e->n;
}
// What the block-resident PCG (k_pcg_blockres) and the plain block-direct form (k_blk_invert / k_blk_apply / k_blk_finish) accept.
static bool blocks_eligible(hipeng *e) {
  if (!blocks_tile(e)) return false;
  // rows of A: one entry each, except the folded huge rows (all of the huge ones must be folded)
  if ((int)e->A.blk.size() - e->A.nwave != (int)e->hrows.size()) return false;
  std::vector<char> ishuge(std::max(1, e->m), 0);
  for (int hr : e->hrows) ishuge[hr] = 1;
  for (int i = 0; i < e->m; i++) if (!ishuge[i] && e->A.rowptr[i + 1] - e->A.rowptr[i] != 1) return false;
  return true;
}
// Coupled form of the block-direct solve: the blocks tile 0..n and at most CPL_MAX rows of A have two or more entries (any
// length, any pattern).  `rows` receives them.
static bool blocks_coupled_eligible(hipeng *e, std::vector<int> &rows) {
  if (!blocks_tile(e)) return false;
  const int cap = e->sw.block_coupled_max;
  rows.clear();
  for (int i = 0; i < e->m; i++) if (e->A.rowptr[i + 1] - e->A.rowptr[i] >= 2) { if ((int)rows.size() >= cap) return false; rows.push_back(i); }
  return !rows.empty();
}
static int build_blockdirect(hipeng *e) {
  if (!e->sw.resident || !e->sw.resident_blocks || !e->sw.block_direct) return 0;
  std::vector<int> crows;
  const bool plain = blocks_eligible(e);
  if (!plain && !blocks_coupled_eligible(e, crows)) return 0;
  BdCtx bd{};
  if (!plain) {
    int *d_crow = nullptr, *d_cidx = nullptr, *d_chuge = nullptr;
    const size_t kc = crows.size();
    std::vector<int> chuge(kc, -1);
    for (size_t r = 0; r < kc; r++) for (size_t h = 0; h < e->hrows.size(); h++) if (e->hrows[h] == crows[r]) chuge[r] = (int)h;
    std::vector<int> cidx((size_t)std::max(1, e->m), -1);
    for (size_t r = 0; r < kc; r++) cidx[crows[r]] = (int)r;
    if (dev_alloc(e, &d_crow, kc) || dev_alloc(e, &d_chuge, kc) || dev_alloc(e, &d_cidx, cidx.size()) || dev_alloc(e, &bd.cs, kc) || dev_alloc(e, &bd.cc, kc) ||
        dev_alloc(e, &bd.cap, kc * kc) || dev_alloc(e, &bd.cap2, kc * kc) || dev_alloc(e, &bd.cap0, kc * kc) || dev_alloc(e, &bd.wm, (size_t)16 * e->n)) return HIPENG_ERR_HIP;
    HIPCHK(hipMemcpyAsync(d_crow, crows.data(), kc * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_cidx, cidx.data(), cidx.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_chuge, chuge.data(), kc * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));          // (the sources are locals)
    bd.kc = (int)kc; bd.crow = d_crow; bd.cidx = d_cidx; bd.chuge = d_chuge;
    {
      std::vector<int> cbptr((size_t)e->n + 1, 0);
      std::vector<int2> cbent;
      for (int j = 0; j < e->n; j++) {
        for (int k = e->M.split[j]; k < e->M.rowptr[j + 1]; k++) { const int q = cidx[e->M.col[k] - e->n]; if (q >= 0) cbent.push_back(int2{q, k}); }
        cbptr[j + 1] = (int)cbent.size();
      }
      int *d_ptr = nullptr; int2 *d_ent = nullptr;
      if (dev_alloc(e, &d_ptr, cbptr.size()) || dev_alloc(e, &d_ent, std::max<size_t>(1, cbent.size()))) return HIPENG_ERR_HIP;
      HIPCHK(hipMemcpyAsync(d_ptr, cbptr.data(), cbptr.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
      if (!cbent.empty()) HIPCHK(hipMemcpyAsync(d_ent, cbent.data(), cbent.size() * sizeof(int2), hipMemcpyHostToDevice, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      bd.cbptr = d_ptr; bd.cbent = d_ent;
    }
  }
  const size_t nd = e->dP_src.size(), n = (size_t)e->n, nb = e->dP_blks.size();
  if (dev_alloc(e, &bd.binv, nd) || dev_alloc(e, &bd.t, n) || dev_alloc(e, &bd.wh, (size_t)MAX_HUGE_FOLD * n) ||
      dev_alloc(e, &bd.cinv, (size_t)MAX_HUGE_FOLD * MAX_HUGE_FOLD) || dev_alloc(e, &bd.part, (size_t)MAX_HUGE_FOLD * nb) || dev_alloc(e, &bd.flag, 4) || dev_alloc(e, &bd.chk, (size_t)2)) return HIPENG_ERR_HIP;
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_blk_invert), hipFuncAttributeMaxDynamicSharedMemorySize, DENSE_MAX * DENSE_MAX * (int)sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    return 0;                        // not an error: the block-resident PCG takes over
  }
  {
    // A x~ of the folded huge rows from the kernel that writes x~ (instead of a k_huge_dot launch per ADMM iteration): every
    // huge row folded, and that kernel's grid within the gridA partial slots k_admm_finalize sums
    const int fin_grid = bd.kc ? std::max(1, std::min(1024, (int)nb)) : std::max(1, std::min(256, (e->n + TB - 1) / TB));
    bd.fin_dots = !e->hrows.empty() && (int)e->A.blk.size() - e->A.nwave == (int)e->hrows.size() && fin_grid <= e->c.gridA;
    bd.fin_dots = bd.fin_dots && e->sw.block_fin_dots;
  }
  {
    // Opt-in (OSQP_AMD_BLOCK_PLAIN=1), not the default: exact algebra, 46 -> 37 us per ADMM iteration at config 5, and x~ as accurate
    // entry by entry -- but a' x~ = a' t0 - c a' W is then a difference of two numbers of size 1e4: 1e-12 of noise in the budget row's
    // constraint value, times rho_h in y_h (1e-10), which moves the dual residual norm by 1e-7 relative, the next rho estimate with
    // it, and the trajectory by 1e-7: config 5's golden objective is then off by 2.4e-6 (bar 1e-6).  tools/plain_check.py.
    const int plain = e->sw.block_plain;
    e->c.plain_rhs = plain;
    e->c.plain_skip = (plain && bd.kc) ? bd.cidx : nullptr;
  }
  e->bd = bd;
  // the solve kernels read the residual as a plain n-vector
  e->dd_init_r = e->c.init_r; e->dd_init_stride = e->c.init_stride;       // (what the launch-per-step kernels use: direct_disable puts them back)
  e->c.init_r = e->c.r; e->c.init_stride = 1;
  e->form = FORM_BLOCK_DIRECT; e->res_use = true;
  if (e->sw.trace) fprintf(stderr, "[osqp_amd] block-direct solve: %zu dense blocks inverted explicitly, %d %s of A as a Woodbury term\n", nb,
                        bd.kc ? bd.kc : (int)e->hrows.size(), bd.kc ? "coupling rows" : "huge rows");
  return 0;
}
// A direct form whose fresh inverse cannot be trusted leaves: this engine goes on with the launch-per-step PCG kernels for good.
static void direct_disable(hipeng *e, const char *what, const char *why, double err) {
  if (e->sw.trace) fprintf(stderr, "[osqp_amd] %s solve dropped (%s, check %.2e): the PCG kernels take over\n", what, why, err);
  for (auto &g : e->graphs) (void)hipGraphExecDestroy(g.second);      // (they hold the Ctx by value)
  e->graphs.clear();
  e->c.init_r = e->dd_init_r; e->c.init_stride = e->dd_init_stride; e->c.fin_wave_rows = 0; e->c.plain_rhs = 0; e->c.plain_skip = nullptr; e->c.vd = nullptr;
  if (e->form == FORM_DENSE_DIRECT) launch_precond(e);       // (refresh_operator leaves it out on a dense-direct engine)
  e->form = FORM_STEPS; e->res_use = false;
  pcg_count_will_jump(e); start_history_void(e);
}
// The verdict on the inverses blk_refresh has just formed (k_blk_check, k_cap_check): Gauss-Jordan has an error ~ cond^2 eps; fine on
// the blocks this form was built for (cond ~ 20), not on every block-diagonal P.  A pivot that was not positive stays what it was: the
// sign of an indefinite block (State::neg_curv).
#define BLK_CHECK 1e-6
static int blk_check(hipeng *e) {
  double chk[2] = {0.0, 0.0}; int flag = 0;
  HIPCHK(hipMemcpyAsync(chk, e->bd.chk, sizeof(chk), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&flag, e->bd.flag, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->dd_check = std::max(chk[0], chk[1]);
  if (e->sw.trace) fprintf(stderr, "[osqp_amd] block-direct refresh: inverse blocks off by %.2e, capacitance inverse by %.2e (probe vector of size 1..2)\n", chk[0], chk[1]);
  if (!flag && !(e->dd_check <= BLK_CHECK)) direct_disable(e, "block-direct", chk[0] > BLK_CHECK ? "the inverse blocks failed their check" : "the capacitance inverse failed its check", e->dd_check);
  return 0;
}
// New rho, sigma or matrix values: invert the blocks again, W = B^-1 A_h', capacitance matrix R_h^-1 + A_h W and its inverse.
static int blk_refresh(hipeng *e) {
  const Ctx &c = e->c;
  const int nh = c.nh, nb = c.dP.nblk, n = e->n;
  HIPCHK(hipMemsetAsync(e->bd.flag, 0, 4 * sizeof(int), e->stream));
  int bmax = 1;
  for (const DenseBlk &d : e->dP_blks) bmax = std::max(bmax, d.b);
  hipLaunchKernelGGL(k_blk_invert, dim3(std::min(nb, 1024)), dim3(INV_TB), (size_t)bmax * bmax * sizeof(double), e->stream, e->c, e->bd);
  HIPCHK(hipMemsetAsync(e->bd.chk, 0, 2 * sizeof(double), e->stream));
  hipLaunchKernelGGL(k_blk_check, dim3(std::min(nb, 1024)), dim3(TB), 0, e->stream, e->c, e->bd);
  if (e->bd.kc) {
    // capacitance matrix, rows r0 .. r0 + 15 = S (B^-1 S_g')': one block pass on the matrix cores and 16 kc row dots per group,
    // then the diagonal and kc pivot steps; everything on the stream
    const int kc = e->bd.kc;
    for (int r0 = 0; r0 < kc; r0 += 16) {
      hipLaunchKernelGGL(k_blk_apply_multi, dim3(std::min(nb, 1024)), dim3(TB), 0, e->stream, e->c, e->bd, r0, e->bd.wm);
      hipLaunchKernelGGL(k_cpl_dot, dim3(kc, 16), dim3(TB), 0, e->stream, e->c, e->bd, (const double *)e->bd.wm, e->bd.cap + (size_t)r0 * kc, 0, 0,
                         (long long)n, (long long)kc, std::min(16, kc - r0));
    }
    hipLaunchKernelGGL(k_cap_diag, dim3((kc + TB - 1) / TB), dim3(TB), 0, e->stream, e->c, e->bd);
    HIPCHK(hipMemcpyAsync(e->bd.cap0, e->bd.cap, (size_t)kc * kc * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    double *src = e->bd.cap, *dst = e->bd.cap2;
    const unsigned gs = (unsigned)(((long long)kc * kc + TB - 1) / TB);
    for (int p = 0; p < kc; p++) { hipLaunchKernelGGL(k_cap_step, dim3(gs), dim3(TB), 0, e->stream, e->bd, (const double *)src, dst, p); std::swap(src, dst); }
    if (src != e->bd.cap) HIPCHK(hipMemcpyAsync(e->bd.cap, src, (size_t)kc * kc * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    hipLaunchKernelGGL(k_cap_check, dim3(1), dim3(TB), 0, e->stream, e->bd);
    HIPCHK(hipGetLastError());
    return blk_check(e);
  }
  std::vector<double> C((size_t)MAX_HUGE_FOLD * MAX_HUGE_FOLD, 0.0), part((size_t)MAX_HUGE_FOLD * nb);
  for (int h = 0; h < nh; h++) {
    hipLaunchKernelGGL(k_blk_apply, dim3(std::min(nb, 1024)), dim3(TB), 0, e->stream, e->c, e->bd, (const double *)(c.hcol + (size_t)h * n), e->bd.wh + (size_t)h * n, 0);
    HIPCHK(hipMemcpyAsync(part.data(), e->bd.part, part.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int h2 = 0; h2 < nh; h2++) { double s = 0.0; for (int q = 0; q < nb; q++) s += part[(size_t)h2 * nb + q]; C[(size_t)h2 * MAX_HUGE_FOLD + h] = s; }   // (A_h2 W_h)
  }
  HIPCHK(hipGetLastError());
  bool bad = false;
  for (int h = 0; h < nh; h++) {
    const double rho = e->h_rho.size() > (size_t)c.hrow[h] ? e->h_rho[(size_t)c.hrow[h]] : 0.0;
    if (!(rho > 0.0)) bad = true; else C[(size_t)h * MAX_HUGE_FOLD + h] += 1.0 / rho;
  }
  // inverse of the nh x nh capacitance matrix (symmetric positive definite when K is): Gauss-Jordan on the host
  std::vector<double> I((size_t)MAX_HUGE_FOLD * MAX_HUGE_FOLD, 0.0);
  for (int h = 0; h < nh; h++) I[(size_t)h * MAX_HUGE_FOLD + h] = 1.0;
  for (int p = 0; p < nh && !bad; p++) {
    const double piv = C[(size_t)p * MAX_HUGE_FOLD + p];
    if (!(piv > 0.0)) { bad = true; break; }
    for (int j = 0; j < nh; j++) { C[(size_t)p * MAX_HUGE_FOLD + j] /= piv; I[(size_t)p * MAX_HUGE_FOLD + j] /= piv; }
    for (int i = 0; i < nh; i++) if (i != p) {
      const double f = C[(size_t)i * MAX_HUGE_FOLD + p];
      for (int j = 0; j < nh; j++) { C[(size_t)i * MAX_HUGE_FOLD + j] -= f * C[(size_t)p * MAX_HUGE_FOLD + j]; I[(size_t)i * MAX_HUGE_FOLD + j] -= f * I[(size_t)p * MAX_HUGE_FOLD + j]; }
    }
  }
  if (bad) { const int one = 1; for (double &v : I) v = 0.0; HIPCHK(hipMemcpyAsync(e->bd.flag, &one, sizeof(int), hipMemcpyHostToDevice, e->stream)); }
  HIPCHK(hipMemcpyAsync(e->bd.cinv, I.data(), I.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  return blk_check(e);
}

// Block-resident form (k_pcg_blockres): P = dense diagonal blocks only, rows of A single-entry or folded huge rows.
static int build_blockres(hipeng *e) {
  if (!e->sw.resident || !e->sw.resident_blocks || !blocks_eligible(e)) return 0;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, e->device));
  const int nwg = std::min(256, prop.multiProcessorCount) - 8;       // one CU per XCD stays free (see build_resident)
  e->res_cus = nwg;
  const int nb = (int)e->dP_blks.size();
  if (nb > 2 * nwg) RES_NO("more than two dense blocks per CU");
  // contiguous blocks, at most two and at most 256 rows per workgroup, spread evenly
  std::vector<int> blk0(nwg + 1, nb);
  {
    int q = 0;
    for (int g = 0; g < nwg; g++) {
      blk0[g] = q;
      const int upto = (int)(((long long)nb * (g + 1) + nwg - 1) / nwg);
      int rows = 0, cnt = 0;
      while (q < nb && q < upto && cnt < 2 && rows + e->dP_blks[q].b <= 256) { rows += e->dP_blks[q].b; q++; cnt++; }
    }
    blk0[nwg] = q;
    if (q != nb) RES_NO("the dense blocks do not fit two per workgroup");
  }
  BrCtx bc{};
  bc.nwg = nwg;
  int *d_blk0 = nullptr;
  if (dev_alloc(e, &d_blk0, blk0.size()) || dev_alloc_polled(e, &bc.sbuf, (size_t)2 * nwg * RES_GSTRIDE) || dev_alloc(e, &bc.dbg, (size_t)nwg * RES_DBG)) return HIPENG_ERR_HIP;
  HIPCHK(hipMemcpyAsync(d_blk0, blk0.data(), blk0.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  bc.blk0 = d_blk0;
  e->bc = bc;
  e->form = FORM_BLOCKRES; e->res_use = true;
  if (e->sw.trace) fprintf(stderr, "[osqp_amd] block-resident PCG: %d dense blocks over %d workgroups, %d huge rows of A as rank-one terms\n", nb, nwg, (int)e->hrows.size());
  return 0;
}

// Everything derived from (P, A, rho, sigma): the Jacobi preconditioner.
static int dd_refresh(hipeng *e);
static void refresh_operator(hipeng *e) {
  rhs_m_stale(e);
  launch_elim_refresh(e);
  // (the Jacobi preconditioner: one thread per column -- 1.3 ms on the Lasso's 1 500-entry columns -- and of no use to a dense-direct
  // engine; direct_disable forms it when such an engine goes back to the PCG kernels)
  switch (e->form) {
    case FORM_STEPS: case FORM_BLOCKRES: launch_precond(e); break;
    case FORM_RESIDENT:
      launch_precond(e);
      if (e->rc.kcp) hipLaunchKernelGGL(k_form_K_lists, dim3((e->n + 3) / 4), dim3(TB), 0, e->stream, e->c, e->rc);
      else hipLaunchKernelGGL(k_form_K, dim3(std::min(2048, (e->n + 3) / 4)), dim3(TB), 0, e->stream, e->c, e->rc);
      break;
    case FORM_BLOCK_DIRECT: launch_precond(e); if (blk_refresh(e)) fprintf(stderr, "osqp_amd: the block-direct solve could not be refreshed\n"); break;
    case FORM_DENSE_DIRECT: if (dd_refresh(e)) fprintf(stderr, "osqp_amd: the dense-direct solve could not be refreshed\n"); break;
  }
}

// The PCG start vector history is void (cold/warm start from the host, new rho, new matrices):
// start from [x~ | rho z~] as it stands and extrapolate again once a few iterations are on record.
static int reset_start(hipeng *e) {
  if (e->c.vx != e->c.va && e->sw.fused_check && e->n + e->m > 0) {      // (both copies and the count in one launch)
    hipLaunchKernelGGL(k_start_reset, dim3(elem_grid(e->n + e->m)), dim3(TB), 0, e->stream, e->c, e->n + e->m);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (e->c.vx != e->c.va) {
    HIPCHK(hipMemcpyAsync(e->c.vx, e->c.va, (size_t)std::max(1, e->n + e->m) * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    // ... and the "previous" vector with it: what vold held was formed with the rho and A from before the call, so a schedule that
    // extrapolates at the first k_admm_finalize after a reset (OSQP_AMD_EXTRAP_SCHED with ex_h0 <= 1) would mix two operators into
    // the m-part of the next start vector.  The default schedule multiplies that difference by theta = 0 and is not changed by this.
    HIPCHK(hipMemcpyAsync(e->c.vold, e->c.va, (size_t)std::max(1, e->n + e->m) * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
  }
  HIPCHK(hipMemsetAsync(&e->c.st->hist_r, 0, sizeof(int), e->stream));
  return 0;
}

static int upload_vec(hipeng *e, double *dst, const c_float *src, size_t cnt) {
  if (cnt == 0 || !src) return 0;
  HIPCHK(hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyHostToDevice, e->stream));
  return 0;
}

static int push_params(hipeng *e) {
  HIPCHK(hipMemcpyAsync(e->d_prm, &e->prm, sizeof(Params), hipMemcpyHostToDevice, e->stream));
  // the source is host-pageable and may be reused right away
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// Which variables can be eliminated from the linear system (see k_elim_refresh): exactly one entry in their column of A,
// no off-diagonal entry in P, at most one such variable per row, the row not a huge one.  Launch-per-step engines and the
// resident PCG (k_form_K forms the reduced operator then); not the block forms.  OSQP_AMD_ELIM=0 switches it off.
static int build_elim(hipeng *e, const csc *P, const csc *A) {
  Ctx &c = e->c;
  c.nelim = 0; c.erow = c.ecol = c.epos = nullptr; c.rhoe = c.rho; c.ecoef = c.edinv = c.xte = nullptr;
  const int n = e->n, m = e->m;
  if (!e->sw.elim) return 0;
  if (e->form == FORM_BLOCKRES || e->form == FORM_BLOCK_DIRECT || m == 0 || n == 0) return 0;      // (the block forms of the portfolio family hold their own operator; the other forms are built after this)
  std::vector<char> coupled(n, 0);
  for (int j = 0; j < n; j++)
    for (long long k = P->p[j]; k < P->p[j + 1]; k++) if (P->i[k] != j) { coupled[j] = 1; coupled[(int)P->i[k]] = 1; }
  std::vector<int> erow(n, -1), ecol(m, -1), epos(m, 0);
  int cnt = 0;
  for (int j = 0; j < n; j++) {
    if (coupled[j] || A->p[j + 1] - A->p[j] != 1) continue;
    const long long k = A->p[j];
    const int i = (int)A->i[k];
    if (ecol[i] >= 0) continue;
    if (e->A.rowptr[i + 1] - e->A.rowptr[i] >= HUGE_ROW) continue;
    erow[j] = i; ecol[i] = j; epos[i] = e->A_csc2csr[k]; cnt++;
  }
  if (cnt == 0) return 0;
  int *d_erow = nullptr, *d_ecol = nullptr, *d_epos = nullptr;
  if (dev_alloc(e, &d_erow, (size_t)n) || dev_alloc(e, &d_ecol, (size_t)m) || dev_alloc(e, &d_epos, (size_t)m) ||
      dev_alloc(e, &c.rhoe, (size_t)m) || dev_alloc(e, &c.ecoef, (size_t)m) || dev_alloc(e, &c.edinv, (size_t)m) || dev_alloc(e, &c.xte, (size_t)m)) return HIPENG_ERR_HIP;
  HIPCHK(hipMemcpyAsync(d_erow, erow.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(d_ecol, ecol.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(d_epos, epos.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  c.erow = d_erow; c.ecol = d_ecol; c.epos = d_epos; c.nelim = cnt;
  e->erow = erow; e->ecol = ecol; e->epos = epos;
  if (e->sw.trace) fprintf(stderr, "[osqp_amd] %d of %d variables eliminated from the linear system (one row of A each, no coupling in P)\n", cnt, n);
  return 0;
}

#include "dense_direct_host.h"

extern "C" int hipeng_create(hipeng **out, const csc *P, const csc *A, const c_float *q,
                             const c_float *l, const c_float *u, const c_float *rho_vec,
                             const hipeng_params *prm, int device) {
  if (!out || !P || !A || !prm) return HIPENG_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fprintf(stderr, "osqp_amd: no HIP device available -- the HIP engine has no CPU fallback\n");
    return HIPENG_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) return HIPENG_ERR_ARG;
  if (P->n > 0x7ffffff0LL || A->m > 0x7ffffff0LL || P->p[P->n] + A->p[A->n] + P->p[P->n] > 0x7ffffff0LL)
    return HIPENG_ERR_ARG;   // int32 device indices
  hipeng *e = new (std::nothrow) hipeng();
  if (!e) return HIPENG_ERR_ALLOC;
  e->device = device; e->n = (int)P->n; e->m = (int)A->m;
  const int n = e->n, m = e->m;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreate(&e->ev0));
  HIPCHK(hipEventCreate(&e->ev1));
  build_A(e, A);
  build_M(e, P, A);
  build_dense(e, P);
  auto pick_rl = [](const HostMat &H) {
    int maxrows = 1;
    for (const RowBlk &b : H.blk) maxrows = std::max(maxrows, b.r1 - b.r0);
    int rl = 8;
    while (rl > 1 && TB / rl < maxrows) rl >>= 1;   // one pass over the block's rows if possible
    return rl;
  };
  e->rlA = pick_rl(e->A); e->rlM = pick_rl(e->M);
  {
    // when most of A sits in long rows, a 32-byte record gather per entry dominates k_cg_A:
    // do the vector update in its own (tiny) launch and gather plain 8-byte u instead
    long long lnnz = 0;
    for (size_t q = (size_t)e->A.nstream; q < (size_t)e->A.nwave; q++) lnnz += e->A.blk[q].k1 - e->A.blk[q].k0;
    e->split = 2 * lnnz >= (long long)e->A.val.size() && !e->A.val.empty();
  }
  if (e->sw.split != SW_UNSET) e->split = e->sw.split != 0;
  if (upload_mat(e, e->A) || upload_mat(e, e->M)) return HIPENG_ERR_HIP;
  Ctx &c = e->c;
  c.n = n; c.m = m;
  c.A = dev_view(e->A); c.M = dev_view(e->M);
  c.Mk = c.M; c.dP = DenseP{0, nullptr, nullptr}; c.nh = 0; c.hcol = nullptr;
  if (!e->dP_blks.empty() || !e->hrows.empty()) {
    if (upload_mat(e, e->Mr)) return HIPENG_ERR_HIP;
    if (dev_alloc(e, &e->d_Mr_src, e->Mr_src.size()) || dev_alloc(e, &e->d_dP_src, e->dP_src.size()) ||
        dev_alloc(e, &e->d_dP_blks, e->dP_blks.size()) || dev_alloc(e, &e->d_dP_val, e->dP_src.size()) ||
        dev_alloc(e, &e->d_hcol_src, e->hcol_src.size()) || dev_alloc(e, &e->d_hcol, e->hcol_src.size())) return HIPENG_ERR_HIP;
    if (!e->Mr_src.empty())
      HIPCHK(hipMemcpyAsync(e->d_Mr_src, e->Mr_src.data(), e->Mr_src.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    if (!e->dP_src.empty()) {
      HIPCHK(hipMemcpyAsync(e->d_dP_src, e->dP_src.data(), e->dP_src.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
      HIPCHK(hipMemcpyAsync(e->d_dP_blks, e->dP_blks.data(), e->dP_blks.size() * sizeof(DenseBlk), hipMemcpyHostToDevice, e->stream));
    }
    if (!e->hcol_src.empty())
      HIPCHK(hipMemcpyAsync(e->d_hcol_src, e->hcol_src.data(), e->hcol_src.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    c.Mk = dev_view(e->Mr);
    if (!e->dP_blks.empty()) c.dP = DenseP{(int)e->dP_blks.size(), e->d_dP_blks, e->d_dP_val};
    c.nh = (int)e->hrows.size(); c.hcol = e->d_hcol;
    for (int k = 0; k < MAX_HUGE_FOLD; k++) c.hrow[k] = k < c.nh ? e->hrows[k] : 0;
    if (repack_dense(e)) return HIPENG_ERR_HIP;
  }
  const int cap = MAX_PARTS;
  c.gridM = std::min(cap, std::max(1, c.M.nblk));
  c.gridA = std::min(cap, std::max(std::max(1, c.A.nblk), std::min(elem_grid(n), 256)));
#define DA(field, cnt) if (dev_alloc(e, &c.field, (size_t)(cnt))) return HIPENG_ERR_HIP
  DA(xy, n + m); DA(z, m); DA(zt, m); DA(va, n + m); DA(vb, n + m);
  DA(q, n); DA(l, m); DA(u, m); DA(rho, m); DA(rhoinv, m); DA(minv, n); DA(pdiag, n);
  DA(r, n); DA(zz, n); DA(kp, n); DA(pt0, n + m); DA(pt1, n + m);
  DA(dxy, n + m); DA(dy, m); DA(cvec, n);
  DA(pdir, n); DA(ut, n + m); DA(g4, 2 * n);
  DA(vx, n + m); DA(vold, n + m);

  DA(D, n); DA(Dinv, n); DA(E, m); DA(Einv, m);
  const int np = std::max(std::max(c.gridM, c.gridA), 2048);   // also scratch for the scaling kernels
  DA(part_rz, np); DA(part_rr, np); DA(part_bb, np); DA(part_pkp, np);
  DA(part_s0, np); DA(part_s1, np); DA(part_s2, np); DA(part_gam, np); DA(part_del, np);
  // the residual scalars' lines and State lie back to back, so that a check reads both with one copy (hipeng_run_admm_check)
  DA(scal, SC_COUNT * 16 + (sizeof(State) + sizeof(double) - 1) / sizeof(double));
  c.st = reinterpret_cast<State *>(c.scal + SC_COUNT * 16);
  DA(part_h, (size_t)std::max(1, c.A.nblk - c.A.nwave) * c.gridA);
#ifdef OSQP_AMD_TIMELINE
  DA(tl, TL_CAP);
#endif
#undef DA
  {
    c.init_r = &c.g4[n].r; c.init_stride = 4; c.init_z = c.ut; c.fin_rr = c.part_rr; c.fin_cnt = c.gridM;
    HIPCHK(hipHostMalloc((void **)&e->h_state, sizeof(State), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&e->h_target, sizeof(long long), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&e->h_check, SC_COUNT * 16 * sizeof(double) + sizeof(State), hipHostMallocDefault));
  }
  if (dev_alloc(e, &e->d_prm, 1)) return HIPENG_ERR_HIP;
  c.prm = e->d_prm;
  e->prm.sigma = prm->sigma; e->prm.alpha = prm->alpha;
  e->prm.eps_rel = prm->pcg_eps_rel; e->prm.eps_abs = prm->pcg_eps_abs;
  e->prm.pcg_max_iter = (int)prm->pcg_max_iter; e->prm.cinv = 1.0;
  e->prm.use_cvec = 0; e->prm.has_scaling = 0; e->prm.pad0 = 0;
  e->prm.ex_theta = e->sw.extrap; e->prm.ex_h0 = e->sw.extrap_sched[0]; e->prm.ex_h1 = e->sw.extrap_sched[1]; e->prm.no_restart = 0;
  if (e->prm.ex_theta == 0.0) c.vx = c.va;   // plain warm start
  e->ex_theta0 = e->prm.ex_theta;
  if (prm->pcg_eps_rel < 0.5e-12) e->prm.ex_theta = 0.0;
  if (push_params(e)) return HIPENG_ERR_HIP;
  if (upload_vec(e, c.q, q, n) || upload_vec(e, c.l, l, m) || upload_vec(e, c.u, u, m) ||
      upload_vec(e, c.pdiag, e->pdiag.data(), n)) return HIPENG_ERR_HIP;
  e->stats.kernels_per_pcg_iter = 2;
  *out = e;
  if (int rc = build_blockdirect(e)) return rc;
  if (e->form == FORM_STEPS) if (int rc = build_blockres(e)) return rc;
  if (int rc = build_elim(e, P, A)) return rc;
  if (int rc = build_dense_direct(e, P, A, true)) return rc;          // small reduced systems: ahead of the resident PCG
  if (e->form == FORM_STEPS) if (int rc = build_resident(e)) return rc;
  if (int rc = build_dense_direct(e, P, A, false)) return rc;
  if (rho_vec) { int rc = hipeng_upload_rho(e, rho_vec); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" void hipeng_destroy(hipeng *e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (auto &g : e->graphs) (void)hipGraphExecDestroy(g.second);
  for (void *p : e->allocs) (void)hipFree(p);
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->h_state) (void)hipHostFree(e->h_state);
  if (e->h_target) (void)hipHostFree(e->h_target);
  if (e->h_check) (void)hipHostFree(e->h_check);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

extern "C" int hipeng_sync(hipeng *e) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" int hipeng_set_params(hipeng *e, const hipeng_params *prm) {
  if (!e || !prm) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const bool sigma_changed = prm->sigma != e->prm.sigma;
  e->prm.sigma = prm->sigma; e->prm.alpha = prm->alpha;
  e->prm.eps_rel = prm->pcg_eps_rel; e->prm.eps_abs = prm->pcg_eps_abs;
  e->prm.pcg_max_iter = (int)prm->pcg_max_iter; e->prm.no_restart = prm->no_restart ? 1 : 0;
  // Extrapolated start vectors pay while PCG does real work.  When the caller asks for more
  // than the default accuracy (tight eps_abs/eps_rel tighten pcg_eps_rel, see osqp_solve) every
  // digit of the solve counts and the residual-based stop from a closer start leaves a
  // slightly larger error: plain warm start below 1e-12 (the stop equality-row problems get by default).
  e->prm.ex_theta = prm->pcg_eps_rel >= 0.5e-12 ? e->ex_theta0 : 0.0;
  if (push_params(e)) return HIPENG_ERR_HIP;
  if (sigma_changed) {
    refresh_operator(e);
    // rho~ depends on sigma: the m-part of the start vector (rho~ A_X x~0, which k_pcg_init takes as it stands) is formed again by
    // hipeng_run_admm's k_refresh_m into va; vx must follow it, or the first residual is that of another operator
    if (e->c.nelim) start_history_void(e);
  }
  return 0;
}

extern "C" int hipeng_set_scaling(hipeng *e, const c_float *D, const c_float *E, c_float cc) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  if (D && (e->m == 0 || E)) {
    std::vector<double> Di(e->n), Ei(e->m);
    for (int j = 0; j < e->n; j++) Di[j] = 1.0 / D[j];
    for (int i = 0; i < e->m; i++) Ei[i] = 1.0 / E[i];
    if (upload_vec(e, e->c.D, D, e->n) || upload_vec(e, e->c.E, E, e->m) ||
        upload_vec(e, e->c.Dinv, Di.data(), e->n) || upload_vec(e, e->c.Einv, Ei.data(), e->m))
      return HIPENG_ERR_HIP;
    e->prm.has_scaling = 1; e->prm.cinv = 1.0 / cc;
    if (push_params(e)) return HIPENG_ERR_HIP;   // also fences the temporaries above
  } else {
    e->prm.has_scaling = 0; e->prm.cinv = 1.0;
    if (push_params(e)) return HIPENG_ERR_HIP;
  }
  return 0;
}

// Ruiz equilibration of the resident (raw) problem, `passes` sweeps, entirely on the
// device; afterwards the scaled q, l, u, the matrix values (triu(P) and A in the caller's
// CSC order) and D, E, c are copied back for the host mirrors of the workspace.
extern "C" int hipeng_ruiz_scale(hipeng *e, c_int passes, c_float *D, c_float *E, c_float *cost,
                                 c_float *q, c_float *l, c_float *u, c_float *Px, c_float *Ax) {
  if (!e || passes < 0) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const Ctx &c = e->c;
  const int n = e->n, m = e->m;
  double *dn = c.kp, *en = c.dy;                 // scratch vectors of length n and m
  const int gw = std::max(1, std::min(2048, (n + m + 3) / 4));
  const int gn = std::max(1, std::min(1024, (n + 3) / 4));
  HIPCHK(hipMemsetAsync(c.scal, 0, SC_COUNT * 16 * sizeof(double), e->stream));
  hipLaunchKernelGGL(k_fill, dim3(elem_grid(n)), dim3(TB), 0, e->stream, c.D, 1.0, n);
  hipLaunchKernelGGL(k_fill, dim3(elem_grid(std::max(m, 1))), dim3(TB), 0, e->stream, c.E, 1.0, m);
  hipLaunchKernelGGL(k_fill, dim3(1), dim3(TB), 0, e->stream, c.scal + SCI(SC_DYLHS), 1.0, 1);
  for (c_int p = 0; p < passes; p++) {
    hipLaunchKernelGGL(k_ruiz_norms, dim3(gw), dim3(TB), 0, e->stream, c, dn, en);
    hipLaunchKernelGGL(k_ruiz_apply, dim3(gw), dim3(TB), 0, e->stream, c, dn, en, e->M.d_val, e->A.d_val);
    hipLaunchKernelGGL(k_ruiz_cost_norms, dim3(gn), dim3(TB), 0, e->stream, c);
    hipLaunchKernelGGL(k_ruiz_cost_scalar, dim3(1), dim3(TB), 0, e->stream, c, gn);
    hipLaunchKernelGGL(k_ruiz_cost_apply, dim3(gn), dim3(TB), 0, e->stream, c, e->M.d_val);
  }
  hipLaunchKernelGGL(k_ruiz_finish, dim3(elem_grid(std::max(n, m))), dim3(TB), 0, e->stream, c);
  HIPCHK(hipGetLastError());
  if (repack_dense(e)) return HIPENG_ERR_HIP;
  // host mirrors
  double cc = 1.0;
  HIPCHK(hipMemcpyAsync(&cc, c.scal + SCI(SC_DYLHS), sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->M.val.data(), e->M.d_val, e->M.val.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (D) HIPCHK(hipMemcpyAsync(D, c.D, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (E && m) HIPCHK(hipMemcpyAsync(E, c.E, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (q) HIPCHK(hipMemcpyAsync(q, c.q, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (l && m) HIPCHK(hipMemcpyAsync(l, c.l, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (u && m) HIPCHK(hipMemcpyAsync(u, c.u, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (cost) *cost = cc;
  if (Px) for (size_t k = 0; k < e->P_toM_up.size(); k++) Px[k] = e->M.val[e->P_toM_up[k]];
  if (Ax) for (size_t k = 0; k < e->A_toM.size(); k++) Ax[k] = e->M.val[e->A_toM[k]];
  for (size_t k = 0; k < e->A_toM.size(); k++) e->A.val[e->A_csc2csr[k]] = e->M.val[e->A_toM[k]];
  for (int j = 0; j < n; j++) e->pdiag[j] = 0.0;
  for (size_t k = 0; k < e->P_toM_up.size(); k++) if (e->P_toM_lo[k] < 0) e->pdiag[e->M.col[e->P_toM_up[k]]] = e->M.val[e->P_toM_up[k]];
  if (upload_vec(e, c.pdiag, e->pdiag.data(), n)) return HIPENG_ERR_HIP;
  e->prm.has_scaling = passes > 0 ? 1 : 0; e->prm.cinv = 1.0 / cc;
  if (push_params(e)) return HIPENG_ERR_HIP;
  rhs_m_stale(e);
  return 0;
}

extern "C" int hipeng_upload_q(hipeng *e, const c_float *q) {
  if (!e || !q) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  if (upload_vec(e, e->c.q, q, e->n)) return HIPENG_ERR_HIP;
  HIPCHK(hipStreamSynchronize(e->stream));
  rhs_m_stale(e);
  return 0;
}

extern "C" int hipeng_upload_bounds(hipeng *e, const c_float *l, const c_float *u) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  if (upload_vec(e, e->c.l, l, e->m) || upload_vec(e, e->c.u, u, e->m)) return HIPENG_ERR_HIP;
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" int hipeng_upload_rho(hipeng *e, const c_float *rho_vec) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  if (e->m > 0) {
    if (!rho_vec) return HIPENG_ERR_ARG;
    if (upload_vec(e, e->c.rho, rho_vec, e->m)) return HIPENG_ERR_HIP;
    e->h_rho.assign(rho_vec, rho_vec + e->m);
    launch_elim_refresh(e);          // (refresh_operator below launches it once more: DESIGN 2, the oddities under the host-call table)
    launch_refresh_m(e, 0, START_HISTORY_VOID);
  }
  refresh_operator(e);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  pcg_count_will_jump(e);            // (usually, after a rho change)
  return 0;
}

// The operator's values changed under a set-up engine (new P, A from the host, or a device-side rescale in place): everything derived
// from them, then z~ = A x~ for the new A and the m-parts of the PCG input vectors, so that the PCG warm start stays consistent; error check, sync.
static int operator_values_changed(hipeng *e) {
  if (repack_dense(e)) return HIPENG_ERR_HIP;
  refresh_operator(e);
  if (e->m > 0) {
    launch_spmv(e, e->c.A, e->c.va, e->c.zt, 0);
    launch_refresh_m(e, 1, START_HISTORY_VOID);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" int hipeng_upload_matrices(hipeng *e, const csc *P, const csc *A) {
  if (!e || !P || !A) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const int n = e->n;
  if (P->p[n] != (long long)e->P_toM_up.size() || A->p[n] != (long long)e->A_toM.size())
    return HIPENG_ERR_ARG;
  for (long long k = 0; k < P->p[n]; k++) {
    e->M.val[e->P_toM_up[k]] = P->x[k];
    if (e->P_toM_lo[k] >= 0) e->M.val[e->P_toM_lo[k]] = P->x[k];
  }
  for (int j = 0; j < n; j++) {
    e->pdiag[j] = 0.0;
    for (long long k = P->p[j]; k < P->p[j + 1]; k++) if (P->i[k] == j) e->pdiag[j] = P->x[k];
  }
  for (long long k = 0; k < A->p[n]; k++) {
    e->M.val[e->A_toM[k]] = A->x[k];
    e->A.val[e->A_csc2csr[k]] = A->x[k];
  }
  if (upload_vec(e, e->M.d_val, e->M.val.data(), e->M.val.size()) ||
      upload_vec(e, e->A.d_val, e->A.val.data(), e->A.val.size()) ||
      upload_vec(e, e->c.pdiag, e->pdiag.data(), n)) return HIPENG_ERR_HIP;
  return operator_values_changed(e);
}

// The resident matrix values changed in place (device-side rescaling).
extern "C" int hipeng_matrices_changed(hipeng *e) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  return operator_values_changed(e);
}

extern "C" int hipeng_cold_start(hipeng *e) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const size_t nm = (size_t)(e->n + e->m) * sizeof(double);
  if (e->sw.fused_check) {
    const int cnm = std::max(1, e->n + e->m), cm = std::max(1, e->m);
    FillRanges f{{e->c.xy, e->c.va, e->c.vb, e->c.z, e->c.zt, e->c.nelim ? e->c.xte : nullptr}, {cnm, cnm, cnm, cm, cm, e->c.nelim ? e->m : 0}};
    hipLaunchKernelGGL(k_fill_ranges, dim3(elem_grid(cnm)), dim3(TB), 0, e->stream, f);
    HIPCHK(hipGetLastError());
  } else {
    HIPCHK(hipMemsetAsync(e->c.xy, 0, std::max<size_t>(nm, 8), e->stream));
    HIPCHK(hipMemsetAsync(e->c.va, 0, std::max<size_t>(nm, 8), e->stream));
    HIPCHK(hipMemsetAsync(e->c.vb, 0, std::max<size_t>(nm, 8), e->stream));
    HIPCHK(hipMemsetAsync(e->c.z, 0, std::max<size_t>(e->m, 1) * sizeof(double), e->stream));
    HIPCHK(hipMemsetAsync(e->c.zt, 0, std::max<size_t>(e->m, 1) * sizeof(double), e->stream));
    if (e->c.nelim) HIPCHK(hipMemsetAsync(e->c.xte, 0, (size_t)e->m * sizeof(double), e->stream));
  }
  pcg_count_will_jump(e); start_history_void(e);     // the first solve from zero needs far more PCG iterations than the steady state
  rhs_m_stale(e);                          // (vb = rho z - y = 0 is NOT the whole m-part when a row carries an eliminated variable: -rho a (-q_y) / D_y)
  return 0;
}

extern "C" int hipeng_set_iterates(hipeng *e, const c_float *x, const c_float *y) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const int n = e->n, m = e->m;
  if (y && upload_vec(e, e->c.xy + n, y, m)) return HIPENG_ERR_HIP;
  if (x) {
    if (upload_vec(e, e->c.xy, x, n)) return HIPENG_ERR_HIP;
    // PCG warm start x~ = x ; z = A x ; z~ = z   (osqp_warm_start, osqp.c:960-963)
    HIPCHK(hipMemcpyAsync(e->c.va, e->c.xy, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    if (e->c.nelim) hipLaunchKernelGGL(k_elim_split, dim3(elem_grid(n)), dim3(TB), 0, e->stream, e->c);
    if (m > 0) {
      launch_spmv(e, e->c.A, e->c.xy, e->c.z, 0);
      HIPCHK(hipMemcpyAsync(e->c.zt, e->c.z, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    }
  }
  if (m > 0) launch_refresh_m(e, 0, START_HISTORY_VOID);
  start_history_void(e);             // (without constraints too: x~ was rewritten)
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" int hipeng_set_z(hipeng *e, const c_float *z) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const int m = e->m;
  if (m > 0 && z) {
    if (upload_vec(e, e->c.z, z, m)) return HIPENG_ERR_HIP;
    // (z~ stays A x~: k_pcg_init takes the start vector's m-part for rho A x~0, whatever z is)
    launch_refresh_m(e, 0, START_HISTORY_VOID);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// ---- graphs ---------------------------------------------------------------
#define TR2(e, ...) do { if ((e)->sw.trace >= 2) { fprintf(stderr, "[osqp_amd:t2] " __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)
// for_resident: the launch that follows is k_pcg_resident and nothing else reads r0 and u0 before the next k_pcg_init (the K == 0
// graphs of a FORM_RESIDENT engine, and the timing hook of that pair).  Every other caller gets the default form: a launch-per-step
// graph that takes over after a launch gave up starts with its own k_pcg_init (k_admm_finalize leaves the iteration untouched then).
static bool init_resident_form(const hipeng *e) { return e->form == FORM_RESIDENT && e->rc.r0pos != nullptr; }
static void launch_init(hipeng *e, int bench = 0, bool for_resident = false) {
  if (e->c.vd) hipLaunchKernelGGL(k_vd, dim3(elem_grid(e->n + e->m)), dim3(TB), 0, e->stream, e->c);
  double *const none = nullptr;
  const dim3 g(e->c.gridM), b(TB);
  if (for_resident && init_resident_form(e)) {
    if (e->c.dP.nblk) hipLaunchKernelGGL((k_pcg_init<true, true>), g, b, 0, e->stream, e->c, bench, e->rc.r0pos);
    else hipLaunchKernelGGL((k_pcg_init<false, true>), g, b, 0, e->stream, e->c, bench, e->rc.r0pos);
  } else {
    if (e->c.dP.nblk) hipLaunchKernelGGL((k_pcg_init<true, false>), g, b, 0, e->stream, e->c, bench, none);
    else hipLaunchKernelGGL((k_pcg_init<false, false>), g, b, 0, e->stream, e->c, bench, none);
  }
}

static void launch_cg_A(hipeng *e, int it, int flags) {
  hipLaunchKernelGGL(k_cg_A, dim3(e->c.gridA), dim3(TB), 0, e->stream, e->c, it, flags);
  const int nhuge = e->c.nh ? 0 : e->c.A.nblk - e->c.A.nwave;   // folded into k_cg_B when c.nh > 0
  if (nhuge > 0 && !(flags & 16)) hipLaunchKernelGGL(k_huge_reduce, dim3(nhuge), dim3(TB), 0, e->stream, e->c, flags & 4);
}
static void launch_cg_B(hipeng *e, int it, int flags) {
  const bool d = e->c.dP.nblk > 0, f = e->c.nh > 0;
  if (d && f) hipLaunchKernelGGL((k_cg_B<true, true>), dim3(e->c.gridM), dim3(TB), 0, e->stream, e->c, it, flags);
  else if (d) hipLaunchKernelGGL((k_cg_B<true, false>), dim3(e->c.gridM), dim3(TB), 0, e->stream, e->c, it, flags);
  else if (f) hipLaunchKernelGGL((k_cg_B<false, true>), dim3(e->c.gridM), dim3(TB), 0, e->stream, e->c, it, flags);
  else hipLaunchKernelGGL((k_cg_B<false, false>), dim3(e->c.gridM), dim3(TB), 0, e->stream, e->c, it, flags);
}

static void launch_pcg_iter(hipeng *e, int it, int flags, int spec_lo = 0) {
  const int hi = spec_lo << 8;     // slots below spec_lo prefetch without looking at the flags first (k_cg_A)
  if (e->split) { launch_cg_A(e, it, (flags & 4) | 16 | hi); launch_cg_A(e, it, (flags & 4) | 32 | hi); }
  else launch_cg_A(e, it, (flags & 4) | hi);
  launch_cg_B(e, it, (flags & 4) | hi);
}

// One ADMM iteration as a graph: k_pcg_init, the operator on u0 ("pre" pass), K unrolled PCG
// iterations, k_admm_finalize.  If K was too small, k_admm_finalize raises `stalled` and the NEXT
// launch of the same graph continues the solve (its init and pre pass return at once).
// R such segments back to back form one graph (a graph launch has a fixed cost of its own on the GPU
// timeline); a segment whose predecessor stalled continues it, segments beyond admm_target return at once.
static int get_graph(hipeng *e, int K, int R, int spec_lo, hipGraphExec_t *out) {
  const int key = (K * 64 + R) * 1024 + spec_lo;
  auto f = e->graphs.find(key);
  if (f != e->graphs.end()) { *out = f->second; return 0; }
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  TR2(e, "get_graph K=%d R=%d: begin capture", K, R);
  HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
  for (int seg = 0; seg < R; seg++) {
    launch_init(e, 0, K == 0);
    if (K == 0) launch_resident(e);                   // the whole linear solve in one launch (K in registers)
    else { launch_cg_A(e, -1, 8); launch_cg_B(e, -1, 0); }   // operator apply on u0 (+ first convergence test), then w0 and the first dots
    for (int it = 0; it < K; it++) launch_pcg_iter(e, it, 0, spec_lo);
    if (e->c.A.nblk > e->c.A.nwave && !(K == 0 && e->form == FORM_BLOCK_DIRECT && e->bd.fin_dots))      // (block-direct: the kernel that wrote x~ left the partials)
      hipLaunchKernelGGL(k_huge_dot, dim3(e->c.gridA), dim3(TB), 0, e->stream, e->c, (const double *)nullptr, 0);
    {
      // dense-direct engines (one wavefront per long row in this kernel): enough workgroups that a wavefront has one or two rows --
      // a row is a chain of dependent round trips (the dot, then the row's own scalars), and at gridA <= 1024 each wavefront walked three
      int fg = e->c.gridA;
      if (e->c.fin_wave_rows) fg = std::max(fg, std::min(4096, (e->c.A.nwave - e->c.A.nstream + 3) / 4 + 1));
      if (e->sw.fin_grid != SW_UNSET) fg = e->sw.fin_grid;
      hipLaunchKernelGGL(k_admm_finalize, dim3(fg), dim3(TB), 0, e->stream, e->c);
    }
  }
  HIPCHK(hipStreamEndCapture(e->stream, &g));
  TR2(e, "get_graph: captured, instantiate");
  HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  TR2(e, "get_graph: instantiated");
  HIPCHK(hipGraphDestroy(g));
  e->graphs[key] = ge;
  *out = ge;
  return 0;
}

static int read_state(hipeng *e, State *s) {
  HIPCHK(hipMemcpyAsync(e->h_state, e->c.st, sizeof(State), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *s = *e->h_state;
  return 0;
}

static int next_K(int want, int cap) {
  // even unroll counts: step 2 up to 32, step 4 up to 96, then +25 %
  int K = 2;
  while (K < want) K = (K < 32) ? K + 2 : (K < 96 ? K + 4 : ((K + K / 4 + 1) & ~1));
  if (K > cap) K = std::max(2, (cap + 1) & ~1);
  return K;
}

// A resident launch gave up (State::res_fail): say what the workgroups left behind, clean up, count the strike.
// The record is meant to be decisive: for the workgroup whose wait timed out first it prints the word it last read from the
// workgroup it missed NEXT TO the word that is in memory now (read by the host), where the missed workgroup itself stood,
// when it published (its give-up clock minus the ticks it had waited) and both XCC ids -- "store landed but was never seen",
// "store never landed" and "the other one was late" read differently.
static int resident_gave_up(hipeng *e, const State &s, bool quiet) {
  const int nwg = e->one_launch_grid(); int *ddbg = e->one_launch_dbg();
  std::vector<int> d((size_t)nwg * RES_DBG, 0);
  bool have = ddbg && hipMemcpy(d.data(), ddbg, d.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  const bool injected = have && e->form == FORM_RESIDENT && e->rc.inject > 0 && d[(size_t)RES_DBG * (nwg - 1) + 3] == 4;
  if (!quiet || !injected) {
    fprintf(stderr, "osqp_amd: a resident PCG launch gave up waiting for its workgroups%s; %s with the launch-per-step kernels "
                    "[wait %d (1 flags, 2 granules) of exchange %d: workgroup %d missed workgroup %d]\n",
            injected ? " (injected by OSQP_AMD_RESIDENT_INJECT)" : " (GPU shared with another stream or process?)",
            e->res_fails >= 2 ? "continuing for good" : "finishing this call", s.res_dbg[0], s.res_dbg[1], s.res_dbg[2], s.res_dbg[3]);
    if (have) {
      std::map<long long, int> hist;
      for (int g = 0; g < nwg; g++) hist[((long long)d[(size_t)RES_DBG * g] << 16) | ((d[(size_t)RES_DBG * g + 1] & 255) << 8) | (d[(size_t)RES_DBG * g + 3] & 255)]++;
      fprintf(stderr, "osqp_amd:   workgroups by (exchange, mode, how they left: 1/2 own flag/granule wait timed out, 3 saw the give-up word, 4 injected, 0 never waited):");
      for (auto &h : hist) fprintf(stderr, " (%lld, %lld, %lld) x %d;", h.first >> 16, (h.first >> 8) & 255, h.first & 255, h.second);
      fprintf(stderr, " epoch base %u\n", s.res_epoch);
      const int wg = s.res_dbg[2], ow = s.res_dbg[3];
      if (wg >= 0 && wg < nwg) {
        const int *w = &d[(size_t)RES_DBG * wg];
        fprintf(stderr, "osqp_amd:   waiter %d (XCC %d): waited %.1f us, %d rounds, last read 0x%08x from workgroup %d (expected tag 0x%08x), gave up at clock 0x%08x\n",
                wg, w[7], w[6] * 0.01, w[9], (unsigned)w[5], w[4], s.res_epoch + (unsigned)w[0], (unsigned)w[8]);
        if (ow >= 0 && ow < nwg) {
          const int *o = &d[(size_t)RES_DBG * ow];
          unsigned long long memword = 0; bool got = false;
          if (s.res_dbg[0] == 1 && e->form == FORM_RESIDENT) { unsigned f = 0; got = hipMemcpy(&f, e->rc.flags + (size_t)ow * RES_FSTRIDE, 4, hipMemcpyDeviceToHost) == hipSuccess; memword = f; }
          else {
            const double *sb = e->one_launch_sbuf();
            const unsigned tag = s.res_epoch + (unsigned)w[0];
            int gi = 0; while (gi < 15 && !((w[10] >> gi) & 1)) gi++;
            got = hipMemcpy(&memword, reinterpret_cast<const unsigned long long *>(sb) + ((size_t)(tag & 1u) * nwg + ow) * RES_GSTRIDE + gi, 8, hipMemcpyDeviceToHost) == hipSuccess;
            memword >>= 32;
          }
          fprintf(stderr, "osqp_amd:   owner %d (XCC %d): stood in exchange %d (left: %d), published at clock 0x%08x (its give-up 0x%08x minus %.1f us of its own wait); "
                          "the word in memory now: %s0x%08llx\n", ow, o[7], o[0], o[3], (unsigned)(o[8] - o[6]), (unsigned)o[8], o[6] * 0.01, got ? "" : "(unreadable) ", memword);
        }
      }
    }
  }
  e->res_use = false;
  e->res_fails += 1;
  e->res_gave_up += 1;
  HIPCHK(hipMemsetAsync(&e->c.st->res_fail, 0, sizeof(int), e->stream));
  // the launch that gave up left flags and granules with tags beyond the epoch it started from (it never wrote the
  // epoch back): the next resident launch must not take them for its own -- start it far beyond (tags compare modulo 2^32)
  e->h_state->res_epoch = s.res_epoch + (1u << 20);
  HIPCHK(hipMemcpyAsync(&e->c.st->res_epoch, &e->h_state->res_epoch, sizeof(unsigned), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemsetAsync(e->c.st->res_dbg, 0, sizeof(int) * 4, e->stream));
  if (ddbg) HIPCHK(hipMemsetAsync(ddbg, 0, d.size() * sizeof(int), e->stream));
  return 0;
}

static void fill_scalars(const double *h, hipeng_scalars *o);
static int enqueue_residuals(hipeng *e);

// Whether the residual scalars taken directly behind a window's graphs belong to the iterate the call ends on: the window did all
// it was asked for (no stall continuation is left to run), no resident launch gave up, and no slow-wait record had to be cleared in
// between.  Anything else and the caller takes the residuals again, as hipeng_residuals does.
extern "C" int hipeng_early_scalars_usable(c_int remaining, int res_fail, int res_slow, int res_repub) {
  return remaining == 0 && !res_fail && !res_slow && !res_repub;
}

// hipeng_run_admm (early == null) and hipeng_run_admm_check
static int run_admm(hipeng *e, c_int count, hipeng_scalars *early, int *have) {
  if (have) *have = 0;
  if (!e || count < 0) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  State s;
  if (e->sw.trace >= 2) {
    if (const char *mp = e->sw.trace_maps[0] ? e->sw.trace_maps : nullptr) {     // address map, to read a crash stack
      static bool dumped = false;
      if (!dumped) {
        dumped = true;
        if (FILE *in = fopen("/proc/self/maps", "r")) {
          if (FILE *out = fopen(mp, "w")) { char buf[4096]; size_t k; while ((k = fread(buf, 1, sizeof buf, in)) > 0) fwrite(buf, 1, k, out); fclose(out); }
          fclose(in);
        }
      }
    }
  }
  // admm_done only moves inside this function: the host keeps its own copy, so a call starts
  // without a device round trip.  The device stops starting iterations at admm_target.
  if (count == 0) return 0;
  if (e->elim_rhs_dirty) {
    if (e->c.nelim && e->m > 0) launch_refresh_m(e, 0, START_HISTORY_KEPT);      // (a host call that needs the history void says so itself, as hipeng_set_params does)
    e->elim_rhs_dirty = false;
  }
  // A launch that gave up (a wait timed out) took the rest of that call to the launch-per-step kernels.  Apart from a GPU
  // that is shared for good, there is a rare transient (about one exchange in 1e5 on small, fast problems: a workgroup's
  // flag or granule stays invisible to some CUs): the next call tries resident launches again, three strikes end that.
  if (!e->res_use && e->resident_available()) e->res_use = true;
  bool had_fail = false;
  const long long start = e->admm_total, target = start + (long long)count;
  if (e->sw.fused_check) {
    hipLaunchKernelGGL(k_window_begin, dim3(1), dim3(64), 0, e->stream, e->c.st, target);      // (the three fields in one launch)
  } else {
    *e->h_target = target;
    HIPCHK(hipMemcpyAsync(&e->c.st->admm_target, e->h_target, sizeof(long long), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(&e->c.st->iters_max, 0, sizeof(int), e->stream));
    HIPCHK(hipMemsetAsync(&e->c.st->iters_min, 0x7f, sizeof(int), e->stream));
  }
  if (e->start_dirty) { if (reset_start(e)) return HIPENG_ERR_HIP; e->start_dirty = false; }
  long long remaining = count;
  const int cap = std::max(2, e->prm.pcg_max_iter);
  const int khead = e->sw.khead;   // unrolled iterations beyond the last window's maximum
  int guard = 0, call_max = 0;
  s.admm_done = start; s.iters_last = 0; s.iters_total = 0; s.forced = 0; s.neg_curv_seen = 0;
  const int segs = e->sw.graph_segs;
  while (remaining > 0) {
    // after a reset (cold start, new rho, new matrices) the PCG iteration count jumps: two
    // iterations to see where it lands, then whole windows
    const bool resident = e->res_use;
    // A resident launch needs every CU for itself (one workgroup per CU, all co-resident): resident windows of
    // different engines of this process on one device take turns.  (Across processes there is no such lock: a
    // launch that finds CUs taken times out and the engine falls back, see k_pcg_resident.)
    CuLease lease;
    if (resident && e->one_launch()) lease.take(e->device, e->res_cus, e->one_launch_grid());
    const long long burst = std::min<long long>(remaining, (e->calibrated || resident) ? 128 : 2);
    TR2(e, "launch burst=%lld K=%d", burst, e->K);
    // `burst` ADMM iterations = burst / segs graphs of `segs` segments + single-segment graphs for the rest
    // (graphs with many nodes only when the unroll is short: keeps instantiation cheap for long PCG runs)
    const int R = (resident || e->K <= 48) ? segs : 1;
    const int gK = resident ? 0 : e->K, gS = resident ? 0 : e->spec_lo;
    hipGraphExec_t gR = nullptr, g1 = nullptr;
    if (burst >= R && R > 1 && get_graph(e, gK, R, gS, &gR)) return HIPENG_ERR_HIP;
    if ((!gR || burst % R) && get_graph(e, gK, 1, gS, &g1)) return HIPENG_ERR_HIP;
    long long left = burst;
    for (; gR && left >= R; left -= R) { HIPCHK(hipGraphLaunch(gR, e->stream)); e->stats.graph_launches += 1; }
    for (; left > 0; left--) { HIPCHK(hipGraphLaunch(g1, e->stream)); e->stats.graph_launches += 1; }
    // A window that should be the call's last carries the residual pass behind its graphs: scalars and State come back in one
    // copy, after one wait.  Nothing the iterations read is written by that pass, so a window that turns out not to be the last
    // (a stall continuation, a launch that gave up) goes on as it would have, and the scalars are dropped.
    const bool fused = early && e->sw.fused_check && burst == remaining;
    if (fused) {
      if (enqueue_residuals(e)) return HIPENG_ERR_HIP;
      HIPCHK(hipMemcpyAsync(e->h_check, e->c.scal, SC_COUNT * 16 * sizeof(double) + sizeof(State), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      memcpy(&s, e->h_check + SC_COUNT * 16, sizeof(State));
    } else if (read_state(e, &s)) return HIPENG_ERR_HIP;
    lease.give();
    e->res_slow += s.res_slow; e->res_slow_max = std::max<long long>(e->res_slow_max, s.res_slow_max); e->res_repub += s.res_repub;
    if (s.res_slow || s.res_repub) {
      for (int k = 0; k < 4; k++) { e->res_slow_hist[k] += s.res_slow_hist[k]; e->res_slow_last[k] = s.res_slow_last[k]; }
      e->res_slow_xcc |= s.res_slow_xcc;
      if (e->sw.trace) fprintf(stderr, "[osqp_amd] resident waits of this window: %d took more than 50 us (50-200 us: %d, 200-500: %d, 0.5-2 ms: %d, longer: %d; longest %.1f us; XCC mask 0x%02x; "
                                    "latest: exchange %d, workgroup %d missed workgroup %d, wait %d), %d re-publications\n", s.res_slow, s.res_slow_hist[0], s.res_slow_hist[1], s.res_slow_hist[2],
                            s.res_slow_hist[3], s.res_slow_max * 0.01, s.res_slow_xcc, s.res_slow_last[0], s.res_slow_last[1], s.res_slow_last[2], s.res_slow_last[3], s.res_repub);
      HIPCHK(hipMemsetAsync(&e->c.st->res_slow, 0, 12 * sizeof(int), e->stream));
    }
    if (s.res_fail) { had_fail = true; if (resident_gave_up(e, s, !e->sw.trace)) return HIPENG_ERR_HIP; }
    const long long done_now = s.admm_done - start;
    const bool stalls = count - done_now > remaining - burst;       // some launches were continuations
    remaining = count - done_now;
    if (fused && hipeng_early_scalars_usable((c_int)remaining, s.res_fail, s.res_slow, s.res_repub)) { fill_scalars(e->h_check, early); *have = 1; }
    call_max = std::max(call_max, s.iters_max);
    const int in_flight = s.stalled ? std::max(s.iters[0], s.iters[1]) : 0;
    if (e->sw.trace) fprintf(stderr, "[osqp_amd] window: K=%d burst=%lld done=%lld iters_max=%d last=%d stalled=%d(%d) launches=%lld\n", e->K, burst, done_now, s.iters_max, s.iters_last, s.stalled, in_flight, (long long)e->stats.graph_launches);
    // next unroll count: the last window's maximum (the last solve's count right after a reset,
    // where the counts are still falling) plus a little head-room; a solve that needs more simply
    // takes a second graph launch
    int base = e->calibrated ? std::max(s.iters_max, in_flight) : std::max(s.iters_last, in_flight);
    if (stalls && base <= e->K) base = e->K + 2;
    e->K = next_K(std::max(2, base + khead), cap);
    // slots every solve of the last window needed (two below its smallest count, in steps of 4: few distinct graphs)
    e->spec_lo = (e->calibrated && s.iters_min < (1 << 20) && !stalls) ? std::min(1000, std::max(0, ((s.iters_min - 2) / 4) * 4)) : 0;
    e->calibrated = true;
    if (remaining > 0) {
      HIPCHK(hipMemsetAsync(&e->c.st->iters_max, 0, sizeof(int), e->stream));
      HIPCHK(hipMemsetAsync(&e->c.st->iters_min, 0x7f, sizeof(int), e->stream));
    }
    if (++guard > 1000000) { fprintf(stderr, "osqp_amd: the ADMM run loop did not terminate\n"); return HIPENG_ERR_HIP; }
  }
  if (!had_fail && e->res_use) e->res_fails = 0;     // strikes count in a row: a call of clean resident windows starts over
  e->admm_total = s.admm_done;
  e->stats.admm_done = (c_int)(s.admm_done - start);
  e->stats.pcg_iters_total = (c_int)s.iters_total;
  e->stats.pcg_iters_last = s.iters_last;
  e->stats.pcg_iters_max = call_max;
  e->stats.pcg_forced = s.forced;
  e->stats.neg_curvature = s.neg_curv_seen;
  return 0;
}

extern "C" int hipeng_run_admm(hipeng *e, c_int count) { return run_admm(e, count, nullptr, nullptr); }

// hipeng_run_admm followed by hipeng_residuals, with one wait between them where the window allows it: *have = 1 and *out holds the
// scalars of the iterate the call ended on; *have = 0 and the caller asks hipeng_residuals.
extern "C" int hipeng_run_admm_check(hipeng *e, c_int count, hipeng_scalars *out, int *have) {
  if (!out || !have) return HIPENG_ERR_ARG;
  return run_admm(e, count, out, have);
}

extern "C" int hipeng_reset_stats(hipeng *e) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  State s;
  if (read_state(e, &s)) return HIPENG_ERR_HIP;
  s.forced = 0; s.iters_total = 0; s.iters_max = 0; s.iters_last = 0; s.neg_curv_seen = 0; s.neg_curv = 0;
  HIPCHK(hipMemcpyAsync(e->c.st, &s, sizeof(State), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->stats = hipeng_stats{};
  e->stats.kernels_per_pcg_iter = 2;
  pcg_count_will_jump(e); e->K = 8;
  return 0;
}

extern "C" int hipeng_get_stats(hipeng *e, hipeng_stats *st) {
  if (!e || !st) return HIPENG_ERR_ARG;
  *st = e->stats;
  st->resident = e->resident_available() ? 1 : 0;
  return 0;
}

// ---- residual scalars -----------------------------------------------------
static void fill_scalars(const double *h, hipeng_scalars *o) {   // (every field of *o is written)
  o->pri_res_u = h[SCI(SC_PRI_U)]; o->pri_res_s = h[SCI(SC_PRI_S)];
  o->z_u = h[SCI(SC_Z_U)]; o->z_s = h[SCI(SC_Z_S)]; o->Ax_u = h[SCI(SC_AX_U)]; o->Ax_s = h[SCI(SC_AX_S)];
  o->dua_res_u = h[SCI(SC_DUA_U)]; o->dua_res_s = h[SCI(SC_DUA_S)];
  o->q_u = h[SCI(SC_Q_U)]; o->q_s = h[SCI(SC_Q_S)]; o->Aty_u = h[SCI(SC_ATY_U)]; o->Aty_s = h[SCI(SC_ATY_S)];
  o->Px_u = h[SCI(SC_PX_U)]; o->Px_s = h[SCI(SC_PX_S)];
  o->obj_scaled = h[SCI(SC_OBJ)];
  o->dy_norm_u = h[SCI(SC_DYN_U)]; o->dy_norm_s = h[SCI(SC_DYN_S)]; o->dy_lhs = h[SCI(SC_DYLHS)];
  o->dx_norm_u = h[SCI(SC_DXN_U)]; o->dx_norm_s = h[SCI(SC_DXN_S)]; o->q_dx = h[SCI(SC_QDX)];
  o->Atdy_u = h[SCI(SC_ATDY_U)]; o->Atdy_s = h[SCI(SC_ATDY_S)];
  o->Pdx_u = h[SCI(SC_PDX_U)]; o->Pdx_s = h[SCI(SC_PDX_S)];
  o->Adx_viol = h[SCI(SC_ADX_VIOL)];
}

// what one residual evaluation enqueues (hipeng_residuals, and hipeng_run_admm_check behind a window's graphs)
static int enqueue_residuals(hipeng *e) {
  HIPCHK(hipMemsetAsync(e->c.scal, 0, SC_COUNT * 16 * sizeof(double), e->stream));
  if (e->c.A.nblk > e->c.A.nwave) hipLaunchKernelGGL(k_huge_dot, dim3(e->c.gridA), dim3(TB), 0, e->stream, e->c, (const double *)e->c.xy, 1);
  hipLaunchKernelGGL(k_residuals, dim3(e->c.gridA + e->c.gridM), dim3(TB), 0, e->stream, e->c);
  hipLaunchKernelGGL(k_final_sums, dim3(1), dim3(TB), 0, e->stream, e->c);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int hipeng_residuals(hipeng *e, hipeng_scalars *out) {
  if (!e || !out) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  if (enqueue_residuals(e)) return HIPENG_ERR_HIP;
  double h[SCI(SC_COUNT)];
  HIPCHK(hipMemcpyAsync(h, e->c.scal, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  fill_scalars(h, out);
  return 0;
}

extern "C" int hipeng_certificates(hipeng *e, c_float eps_dx, int unscaled, hipeng_scalars *io) {
  if (!e || !io) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  // the five output slots (one 128-byte line each, SC_ATDY_U .. SC_ADX_VIOL) start from zero on every call:
  // the exact and the approximate check of one iteration both come here
  HIPCHK(hipMemsetAsync(e->c.scal + SCI(SC_ATDY_U), 0, (size_t)(SCI(SC_ADX_VIOL) - SCI(SC_ATDY_U) + 1) * sizeof(double), e->stream));
  hipLaunchKernelGGL(k_certificates, dim3(e->c.gridA + e->c.gridM), dim3(TB), 0, e->stream, e->c,
                     (double)eps_dx, unscaled);
  HIPCHK(hipGetLastError());
  double h[SCI(SC_COUNT)];
  HIPCHK(hipMemcpyAsync(h, e->c.scal, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  io->Atdy_u = h[SCI(SC_ATDY_U)]; io->Atdy_s = h[SCI(SC_ATDY_S)];
  io->Pdx_u = h[SCI(SC_PDX_U)]; io->Pdx_s = h[SCI(SC_PDX_S)]; io->Adx_viol = h[SCI(SC_ADX_VIOL)];
  return 0;
}

extern "C" int hipeng_download(hipeng *e, c_float *x, c_float *y, c_float *z, c_float *dx,
                               c_float *dy, int dy_projected) {
  if (!e) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const size_t n = e->n, m = e->m;
  if (x && n) HIPCHK(hipMemcpyAsync(x, e->c.xy, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (y && m) HIPCHK(hipMemcpyAsync(y, e->c.xy + n, m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (z && m) HIPCHK(hipMemcpyAsync(z, e->c.z, m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (dx && n) HIPCHK(hipMemcpyAsync(dx, e->c.dxy, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (dy && m) HIPCHK(hipMemcpyAsync(dy, dy_projected ? e->c.dxy + n : e->c.dy, m * sizeof(double),
                                     hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// ---- plugin-boundary solve --------------------------------------------------
extern "C" int hipeng_kkt_solve_unrefined(hipeng *e, c_float *b) {
  if (!e || !b) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const int n = e->n, m = e->m;
  // reduced right-hand side: cvec = b1, vb(m-part) = rho . b2 ; start from x~ = 0
  if (hipeng_cold_start(e)) return HIPENG_ERR_HIP;
  if (upload_vec(e, e->c.cvec, b, n)) return HIPENG_ERR_HIP;
  e->prm.use_cvec = 1;                       // (before the m-parts are formed: an eliminated variable's b_y comes from cvec then)
  if (push_params(e)) return HIPENG_ERR_HIP;
  if (m > 0) {
    // stage b2 in z, y = 0  =>  k_refresh_m writes vb = rho*z - y = rho.b2
    if (upload_vec(e, e->c.z, b + n, m)) return HIPENG_ERR_HIP;
    launch_refresh_m(e, 0, START_HISTORY_VOID);
  }
  int rc = hipeng_run_admm(e, 1);
  e->prm.use_cvec = 0;
  if (push_params(e)) return HIPENG_ERR_HIP;
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(b, e->c.va, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (m > 0) HIPCHK(hipMemcpyAsync(b + n, e->c.zt, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  std::vector<double> xte;
  if (e->c.nelim) {          // x~ of the eliminated variables comes from the back substitution (the PCG vector is zero there)
    xte.resize((size_t)m);
    HIPCHK(hipMemcpyAsync(xte.data(), e->c.xte, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  if (e->c.nelim) for (int j = 0; j < n; j++) if (e->erow[(size_t)j] >= 0) b[j] = xte[(size_t)e->erow[(size_t)j]];
  return 0;
}
extern "C" int hipeng_kkt_solve(hipeng *e, c_float *b) {
  if (!e || !b) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const int n = e->n, m = e->m;
  // The direct forms apply an explicit inverse: inside the ADMM loop to a residual (the warm start absorbs its error), here to the whole
  // right-hand side, where even an exact inverse leaves an error of cond(K) eps relative to |K^-1| |b| -- 15x that of an LU solve at
  // cond 500.  So one step of refinement: r = b1 + A'(rho . b2) - K x~ from the host copies of [P | A'] (long double sums), then
  // x~ += K^-1 r, z~ += A K^-1 r.
  const bool direct = e->res_use && e->explicit_inverse() && (m == 0 || e->h_rho.size() == (size_t)m);
  std::vector<double> b0;
  if (direct) b0.assign(b, b + n + m);
  if (int rc = hipeng_kkt_solve_unrefined(e, b)) return rc;
  if (!direct || !(e->res_use && e->explicit_inverse())) return 0;
  const HostMat &M = e->M;
  const long double sigma = e->prm.sigma;
  std::vector<long double> w((size_t)m, 0.0L);            // rho . (b2 - A x~)
  for (int j = 0; j < n; j++)
    for (int k = M.split[j]; k < M.rowptr[j + 1]; k++) w[(size_t)(M.col[k] - n)] -= (long double)M.val[k] * b[j];
  for (int i = 0; i < m; i++) w[(size_t)i] = (long double)e->h_rho[(size_t)i] * (w[(size_t)i] + b0[(size_t)n + i]);
  std::vector<double> r((size_t)n + m, 0.0);
  for (int j = 0; j < n; j++) {
    long double s = (long double)b0[(size_t)j] - sigma * b[j];
    for (int k = M.rowptr[j]; k < M.split[j]; k++) s -= (long double)M.val[k] * b[M.col[k]];
    for (int k = M.split[j]; k < M.rowptr[j + 1]; k++) s += (long double)M.val[k] * w[(size_t)(M.col[k] - n)];
    r[(size_t)j] = (double)s;
  }
  if (int rc = hipeng_kkt_solve_unrefined(e, r.data())) return rc;
  for (int q = 0; q < n + m; q++) b[q] += r[(size_t)q];
  return 0;
}
#include "engine_hooks.h"

// ---- ONE QP over several GPUs by rows, driven from C (include/osqp_amd_rowpart.h) ----
#include "kkt_sens.h"
#include "verify.h"
#include "rowpart_native.h"
