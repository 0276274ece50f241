// batch_common_kkt.h -- polish, adjoint and tangent of the common-K engine on a shared Hessian inverse, included by
// batch.hip after batch_tangent.h.
//
// The other engines form and invert, per member, the whole regularised KKT matrix [P~ + delta I, Ar'; Ar, -delta I] of
// order n + mred.  In a common-K batch its (1,1) block is the same for every member and for the handle's life (the
// engine serves no update_matrices and keeps its scaling across update); only the active rows differ.  Block
// elimination on the shared block is the same regularised solve:
//   H  = (P~ + delta I)^-1              NP x NP, shared, once per handle (osqp_amd_batch_common_kkt)
//   Wt = A~ H                           m x NP row-major, shared, once per handle
//   S  = Ar H Ar' + delta I             mred x mred per member, SPD
//   [P~ + delta I, Ar'; Ar, -delta I] [x; nu] = [g1; g2]  <=>  t = H g1;  nu = S^-1 (Ar t - g2);  x = t - Wt[rows]' nu
// the exact Schur complement of the matrix the other engines invert, so the active sets, the formulas, the statuses,
// the refinement against the unregularised [P, Ar'; Ar, 0] and the acceptance rule are theirs unchanged.
//   k_bk_hform   grid (NP): row i of P~ + delta I, dense, identity beyond n; inverted by k_bc_pivot between two buffers
//                of its own, with a flag word of its own (io.flag[0] and io.Wk are not touched);
//   k_bk_wt      one workgroup per row i of A: Wt[i][:] = sum_k A~[i,k] H[k][:], in CSR order of the row;
//   k_bk_form    grid (NS rows, members of the chunk): row a of the member's S, identity beyond mred; NS = the largest
//                mred of the batch rounded up to 32, at least 32; the per-member buffer is NS x NS doubles;
//   k_bk_invert  one workgroup per member: gj_sweep over mred with the all-positive verdict;
//   BlockK       the solver k_bp_polish, k_ba_adjoint and k_bt_tangent are instantiated with (kkt_solve_block).
// No floating-point atomics: every value has one owner and a fixed summation order, so a member's bits depend neither
// on its position in the batch, nor on the chunking, nor on the other slices of a call.

struct BKkt {              // the shared pieces of a common-K handle (device pointers; null = not built)
  double *H = nullptr;     // [NP][NP] (P~ + delta I)^-1, identity padding
  double *Wt = nullptr;    // [m][NP] A~ H (null when m = 0)
};

// Row i of P~ + delta I (the handle's scaled values, slab 0) from the full symmetric pattern, identity beyond n.
__global__ void __launch_bounds__(256) k_bk_hform(BPattern p, BIO io, int NP, double delta, double *out) {
  __shared__ __attribute__((aligned(16))) double row[BS_MAX_N];
  const int i = blockIdx.x, n = p.n, tid = threadIdx.x;
  for (int j = tid; j < NP; j += 256) row[j] = 0.0;
  __syncthreads();
  if (i < n) {
    for (int k = p.Fp[i] + tid; k < p.Fp[i + 1]; k += 256) row[p.Fi[k]] = io.Wv[p.Fk[k]];
    __syncthreads();
    if (tid == 0) row[i] = row[i] + delta;
  } else if (tid == 0) row[i] = 1.0;
  __syncthreads();
  for (int j = tid; j < NP; j += 256) out[(size_t)i * NP + j] = row[j];
}

// Wt[i][j] = sum over the entries k of row i of A~, in CSR order: A~[i,k] H[k][j].  One workgroup per row, the threads
// over j (contiguous loads of H's rows); a row of any length is walked by the loop.
__global__ void __launch_bounds__(256) k_bk_wt(BPattern p, BIO io, int NP, const double *__restrict__ H, double *__restrict__ Wt) {
  const int i = blockIdx.x;
  const double *Av = io.Wv + p.nnzP;
  for (int j = threadIdx.x; j < NP; j += 256) {
    double acc = 0.0;
    for (int k = p.Rp[i]; k < p.Rp[i + 1]; ++k) acc = __builtin_fma(Av[p.Rk[k]], H[(size_t)p.Rj[k] * NP + j], acc);
    Wt[(size_t)i * NP + j] = acc;
  }
}

// Row a of S = Ar H Ar' + delta I of member list[blockIdx.y] into slot blockIdx.y of the buffer, identity beyond mred.
// Symmetry to the bit: both halves evaluate the same expression in the same order -- entry (a, b) and entry (b, a) are
// both, with lo = min(a, b) and hi = max(a, b), the sum over the entries k of row rows[hi] of A~ in CSR order of
// A~[rows[hi], k] * Wt[rows[lo]][col k], by fused multiply-adds from 0.0.  The workgroup keeps its own row of Wt in LDS
// (the lo operand of the half b >= a); for b < a the hi row is its own row of A~, the same for every thread.
__global__ void __launch_bounds__(256) k_bk_form(BPattern p, BIO io, BPol pl, BKkt kk, int NP, int NS, double delta, const int *list) {
  __shared__ __attribute__((aligned(16))) double wrow[BS_MAX_N];
  const long long qp = list[blockIdx.y];
  const int a = blockIdx.x, n = p.n, m = p.m, tid = threadIdx.x;
  const int mred = pl.mred[qp];
  double *out = pl.K + (long long)blockIdx.y * NS * NS + (long long)a * NS;
  if (a >= mred) {                               // identity padding
    for (int b = tid; b < NS; b += 256) out[b] = b == a ? 1.0 : 0.0;
    return;
  }
  const int *rows = pl.rows + qp * m;
  const int ra = rows[a];
  for (int j = tid; j < n; j += 256) wrow[j] = kk.Wt[(size_t)ra * NP + j];
  __syncthreads();
  const double *Av = io.Wv + p.nnzP;
  for (int b = tid; b < NS; b += 256) {
    double v = 0.0;
    if (b < mred) {
      const int rb = rows[b];
      if (b >= a) {
        for (int k = p.Rp[rb]; k < p.Rp[rb + 1]; ++k) v = __builtin_fma(Av[p.Rk[k]], wrow[p.Rj[k]], v);
      } else {
        const double *wb = kk.Wt + (size_t)rb * NP;
        for (int k = p.Rp[ra]; k < p.Rp[ra + 1]; ++k) v = __builtin_fma(Av[p.Rk[k]], wb[p.Rj[k]], v);
      }
      if (b == a) v = v + delta;
    }
    out[b] = v;
  }
}

// k_bp_invert's twin for S: gj_sweep over mred in the NS x NS slot blockIdx.x, exchange buffers of NS doubles (dynamic
// LDS: 4 * NS doubles).  S is positive definite: a pivot that is not positive rejects the member.
__global__ void __launch_bounds__(BS_NTI) k_bk_invert(BPol pl, int NS, const int *list) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const long long qp = list[blockIdx.x];
  const bool bad = gj_sweep(pl.K + (long long)blockIdx.x * NS * NS, pl.mred[qp], NS, lds, lds + 2 * NS, NS,
                            [](int, double akk) { return !(akk > 0.0); });
  if (threadIdx.x == 0 && bad) pl.stat[qp] = -1;
}

// kkt_solve_refined's sibling on the shared pieces: the same regularised solve by block elimination, then kkt_refine's
// steps against the unregularised matrix.  Sinv: the member's S^-1 (NS x NS); w: LDS scratch of max(NP, NS) doubles,
// 16-byte aligned.  out = K^-1 in, both in the [x; nu] layout:
//   w = [in_x; 0]            (bs_gemv reads whole padded rows)
//   t = H w                  into out[0, n)
//   w = [Ar t - in_nu; 0]    the sparse rows of A~ on t
//   nu = S^-1 w              into out[n, N)
//   x_j = t_j - sum_a nu_a Wt[rows[a]][j], a ascending; the threads over j, so a wavefront loads 512 contiguous bytes
template <class Rhs>
__device__ __forceinline__ void kkt_solve_block(const BL &s, const double *H, const double *Wt, const double *Sinv, int NP, int NS,
                                                int NPOL, int n, int N, const int *map, const int *rows, int refine_iter,
                                                Rhs rhs, double *sol, double *res, double *cor, double *w) {
  kkt_refine(s, NPOL, n, N, map, rows, refine_iter, rhs, sol, res, cor, [=](const double *in, double *out) {
    const int tid = threadIdx.x, mred = N - n;
    for (int j = tid; j < NP; j += BP_NT) w[j] = j < n ? in[j] : 0.0;
    __syncthreads();
    bs_gemv(H, NP, n, w, out);
    for (int a = tid; a < NS; a += BP_NT) w[a] = a < mred ? a_row_dot(s, out, rows[a]) - in[n + a] : 0.0;
    __syncthreads();
    bs_gemv(Sinv, NS, mred, w, out + n);
    for (int j = tid; j < n; j += BP_NT) {
      double acc = 0.0;
#pragma unroll 4
      for (int a = 0; a < mred; ++a) acc = __builtin_fma(out[n + a], Wt[(size_t)rows[a] * NP + j], acc);
      out[j] = out[j] - acc;
    }
    __syncthreads();
  });
}

// The common-K engine's solver: one slab of values (slab 0), S^-1 of the member in slot blockIdx.x of the chunk's buffer.
struct BlockK {
  const double *H, *Wt;
  int NP, NS;
  __device__ __forceinline__ long long slab(long long) const { return 0; }
  __device__ __forceinline__ const double *inverse(const double *K, int) const { return K + (long long)blockIdx.x * NS * NS; }
  template <class Rhs>
  __device__ __forceinline__ void solve(const BL &s, const double *Sinv, int NPOL, int n, int N, const int *map, const int *rows,
                                        int refine_iter, Rhs rhs, double *sol, double *res, double *cor, double *w) const {
    kkt_solve_block(s, H, Wt, Sinv, NP, NS, NPOL, n, N, map, rows, refine_iter, rhs, sol, res, cor, w);
  }
};
// the scratch BlockK::solve needs behind a kernel's own LDS
static size_t bk_scratch_bytes(int NP, int NS) { return sizeof(double) * (size_t)std::max(NP, NS); }
