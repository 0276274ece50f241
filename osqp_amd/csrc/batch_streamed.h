// batch_streamed.h -- the streamed-inverse batch engine (OSQP_AMD_BATCH_STREAMED), included by batch.hip.
//
// For members of up to 1024 variables, where K^-1 no longer fits a CU's registers: each member's dense K^-1
// (NP x NP row-major, NP = n rounded up to 32, identity padding) lives in HBM and is streamed once per ADMM
// iteration (twice for refined members) as a GEMV with 16-byte loads.  Only the n- and m-vectors of one member
// live in LDS; the shared pattern is read from global memory (L2 resident) and the member's scaled P and A
// values from its slab io.Wv.  Four kernels, each one launch over the batch:
//   k_bs_setup   one workgroup per member: Ruiz scaling, row classes, workspace (batch_admm.h, as the tiled setup phase;
//                <true>: the re-equilibration of a matrix update, classes, rho and iterates kept);
//   k_bs_form    grid (NP rows, members): K = P + sigma I + A' diag(rho) A, dense, from a host-built list of
//                (A slot, A slot, row) triples per entry of triu(K): a fixed summation order, no atomics;
//   k_bs_invert  one workgroup per member: Gauss-Jordan in place in HBM without pivoting (K is SPD; gj_sweep,
//                the sweep polish and adjoint run too); a non-positive pivot flags the member (BF_NOT_PD);
//   k_bs_loop    one workgroup per member: admm_loop of batch_admm.h, the code k_batch_solve runs, with StreamedK
//                as its K solve.  A member whose rho moves saves its scaled x, z, y, iteration count and rho and
//                leaves with a rebuild request; the host re-forms and re-inverts those members and relaunches
//                the loop over them (osqp_amd_batch_solve).
// form and invert only touch members whose io.flag has BF_REBUILD, so a launch over the whole batch costs
// nothing for the others.

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

// The matrix side of a BL for a member whose scaled values stay in HBM: Pv / Av in its slab io.Wv, the pattern
// read from global memory.  (Polish and adjoint use nothing else of the BL.)
__device__ __forceinline__ void slab_view(BL &s, const BPattern &p, const BIO &io, long long qp) {
  s.Pv = io.Wv + qp * ((long long)p.nnzP + p.nnzA); s.Av = s.Pv + p.nnzP;
  s.Pp = p.Pp; s.Pi = p.Pi; s.Pc = p.Pc; s.Fp = p.Fp; s.Fi = p.Fi; s.Fk = p.Fk;
  s.Ap = p.Ap; s.Ai = p.Ai; s.Ac = p.Ac; s.Rp = p.Rp; s.Rj = p.Rj; s.Rk = p.Rk;
}

__device__ __forceinline__ BL bs_layout(double *lds, const BPattern &p, const BIO &io, long long qp, int NP) {
  BL s;
  double *w = lds;
  s.NP = NP; s.m = p.m;
  s.nv = w; w += 7 * NP; s.mv = w; w += 11 * p.m;
  s.red = w; w += 64; s.gp = w; w += 256;
  s.rowk = s.colk = nullptr;
  s.ctype = reinterpret_cast<int *>(w);
  slab_view(s, p, io, qp);
  return s;
}

// ---------------------------------------------------------------------------
// setup: the tiled engine's setup phase with the matrix values in the member's HBM slab (SLAB: the slab is
// written and re-read by different lanes of this workgroup, so its hand-offs are fenced).
// UPD: the same on the current raw data for a matrix update (osqp.c:1171-1279): row classes, rho and iterates stay.
// list (null: every member): one workgroup per listed member, qp = list[blockIdx.x].
// ---------------------------------------------------------------------------
template <bool UPD>
__global__ void __launch_bounds__(BS_NT) k_bs_setup(BPattern p, BSettings st, BIO io, int NP, const int *list) {
  const long long qp = list ? list[blockIdx.x] : blockIdx.x;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const BL s = bs_layout(lds, p, io, qp, NP);
  clear_vectors<BS_NT>(s);
  load_problem<BS_NT, true>(s, p, io, qp);
  const double cs = ruiz_scale<BS_NT, true, !UPD>(s, p, st);
  store_workspace<BS_NT, true, !UPD>(s, p, io, qp, cs, fmin(fmax(st.rho, 1e-6), 1e6), BF_REBUILD);   // K^-1 is due (k_bs_form, k_bs_invert)
}

// ---------------------------------------------------------------------------
// formation of K: block (i, k) writes row i of member list[k]'s K into its K^-1 slot (identity beyond n)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bs_form(BPattern p, BSPattern kp, BIO io, int NP, double sigma, const int *list) {
  __shared__ __attribute__((aligned(16))) double row[1024];
  const long long qp = list ? list[blockIdx.y] : (int)blockIdx.y;
  if (!(io.flag[qp] & BF_REBUILD)) return;
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
      for (int t = kp.Ep[e]; t < kp.Ep[e + 1]; ++t) acc += rho_of_class(ct[kp.Tr[t]], rho) * Av[kp.Ta[t]] * Av[kp.Tb[t]];
      row[j] = acc;
    }
  }
  __syncthreads();
  double *out = io.Wk + qp * (long long)NP * NP + (long long)i * NP;
  for (int j = threadIdx.x; j < NP; j += 256) out[j] = row[j];
}

// ---------------------------------------------------------------------------
// Gauss-Jordan inversion in place in HBM without pivoting (invert_tiles, one pivot per step) of the N x N block
// of a matrix of pitch NP.  Thread (tr, tc) of a 32 x 32 grid owns the entries (i, j) with i = tr mod 32,
// j = tc mod 32 for all pivots, so each entry is only ever read and written by its owner; the owners of row k and
// column k publish them to LDS (double buffered: row[0..N) and row[stride..stride + N), col likewise; one barrier
// per pivot).  Only the N x N block is touched: the padding stays the identity.  wrong(k, akk): pivot k has the
// wrong sign; returns (uniformly: every lane reads every pivot) whether any had.
// ---------------------------------------------------------------------------
template <class Wrong>
__device__ __forceinline__ bool gj_sweep(double *Ka, int N, int NP, double *row, double *col, int stride, Wrong wrong) {
  const int tr = threadIdx.x >> 5, tc = threadIdx.x & 31;
  bool bad = false;
#pragma unroll 1
  for (int k = 0; k < N; ++k) {
    double *rk = row + (k & 1) * stride, *ck = col + (k & 1) * stride;
    if (tr == (k & 31)) for (int j = tc; j < N; j += 32) rk[j] = Ka[(long long)k * NP + j];
    if (tc == (k & 31)) for (int i = tr; i < N; i += 32) ck[i] = Ka[(long long)i * NP + k];
    __syncthreads();
    const double akk = rk[k];
    bad |= wrong(k, akk);
    const double piv = 1.0 / akk;
    for (int i = tr; i < N; i += 32) {
      const double ci = ck[i];
      double *Ki = Ka + (long long)i * NP;
      if (i == k) {
        for (int j = tc; j < N; j += 32) Ki[j] = j == k ? piv : rk[j] * piv;
      } else {
        for (int j = tc; j < N; j += 32) Ki[j] = j == k ? 0.0 - ci * piv : __builtin_fma(-ci, rk[j] * piv, Ki[j]);
      }
    }
  }
  __syncthreads();
  return bad;
}

__global__ void __launch_bounds__(BS_NTI) k_bs_invert(int n, BIO io, int NP, const int *list) {
  __shared__ double rowk[2][1024], colk[2][1024];
  const long long qp = list ? list[blockIdx.x] : (int)blockIdx.x;
  const int fl = io.flag[qp];
  if (!(fl & BF_REBUILD)) return;
  const bool notpd = gj_sweep(io.Wk + qp * (long long)NP * NP, n, NP, rowk[0], colk[0], 1024,
                              [](int, double akk) { return !(akk > 0.0); });
  // the rebuild is done and the refinement verdict kept, to be taken again on the new K^-1
  if (threadIdx.x == 0) io.flag[qp] = (fl & BF_REFINE) | BF_OPEN | (notpd ? BF_NOT_PD : 0);
}

// ---------------------------------------------------------------------------
// the ADMM loop with K^-1 streamed from HBM
// ---------------------------------------------------------------------------
// A rho move cannot be followed inside the kernel (K is re-formed and re-inverted by kernels of their own): before
// the loop's last iteration the member saves its scaled iterates, counters and rho, sets io.flag = BF_REBUILD |
// (refinement verdict), appends itself to rb_list (rb_count) and leaves; in the last iteration (BA::end_iter: max_iter,
// or the clock of a solve with a time limit) no further solve with K follows, so it finishes and the rebuild is left
// to the host's last pass.
struct StreamedK {
  const double *Wk;
  int NP, n;
  int *rb_count, *rb_list;
  bool rebuild_due;
  __device__ __forceinline__ void solve(const BL &, const double *in, double *out) const { bs_gemv(Wk, NP, n, in, out); }
  __device__ __forceinline__ bool leave(const BL &s, const BPattern &p, const BSettings &st, const BIO &io, long long qp, const BA &a) const {
    if (a.iter >= a.end_iter) return false;
    const int m = p.m, tid = threadIdx.x;
    for (int j = tid; j < n; j += BS_NT) io.Xs[qp * n + j] = s_x[j];
    for (int i = tid; i < m; i += BS_NT) { io.Zs[qp * m + i] = s_z[i]; io.Ys[qp * m + i] = s_y[i]; }
    if (tid == 0) {
      io.info[qp * 8] = a.iter; io.info[qp * 8 + 5] = a.rho_updates; io.rho_io[qp] = a.rho;
      io.flag[qp] = BF_REBUILD | (a.need_refine ? BF_REFINE : 0);
      rb_list[atomicAdd(rb_count, 1)] = (int)qp;
    }
    return true;
  }
  __device__ __forceinline__ void rho_moved(const BL &, const BPattern &, const BSettings &, BA &) { rebuild_due = true; }
};

// list == nullptr: the first round, over the whole batch (in io.order when set), from the stored iterates
// when warm starting; otherwise a resumed round over list[0..gridDim.x): the members continue from the state
// they saved when their rho moved.  CLOCK: a solve with a time limit (admm_loop), clk the handle's clock words; the
// deadline persists across rounds, so a resumed member meets it at its next clock iteration.
template <bool CLOCK>
__global__ void __launch_bounds__(BS_NT) k_bs_loop(BPattern p, BSettings st, BIO io, int NP, const int *list,
                                                   int *rb_count, int *rb_list, unsigned long long *clk) {
  const bool resume = list != nullptr;
  const long long qp = resume ? list[blockIdx.x] : (io.order ? io.order[blockIdx.x] : (int)blockIdx.x);
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const BL s = bs_layout(lds, p, io, qp, NP);
  StreamedK eng{io.Wk + qp * (long long)NP * NP, NP, p.n, rb_count, rb_list, false};
  BDbg dbg;
  BA a;
  clear_vectors<BS_NT>(s);
  a.cs = load_workspace<BS_NT, true>(s, p, io, qp);
  a.rho = fmin(fmax(io.rho_io[qp], 1e-6), 1e6);
  init_iterates<BS_NT>(s, p, io, qp, a.rho, st.warm_start || resume);
  const int qflag = io.flag[qp];
  a.need_refine = (qflag & BF_REFINE) != 0;
  a.check_pending = (qflag & BF_OPEN) != 0;
  if (admm_loop<BS_NT, false, CLOCK>(s, p, st, io, qp, a, resume ? (int)io.info[qp * 8] : 0, eng, dbg, clk)) return;
  // a rebuild left for after the loop drops the refinement verdict, as the tiled engine's in-loop rebuild does
  store_solution<BS_NT>(s, p, st, io, qp, a, eng.rebuild_due ? BF_REBUILD : (a.check_pending ? BF_OPEN : (a.need_refine ? BF_REFINE : 0)));
  if (threadIdx.x == 0) io.rho_io[qp] = a.rho;
}
