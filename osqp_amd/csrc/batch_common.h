// batch_common.h -- the kernels of the common-K batch engine (OSQP_AMD_BATCH_COMMON), included by batch.hip.
//
// One model, many right-hand sides: every member shares P, A, one scaling (D, E, c), one set of row classes and one
// rho, so there is ONE K^-1 (NP x NP row-major, NP = n rounded up to 32, identity padding, io.Wk; formed by k_bs_form,
// inverted by k_bc_pivot with k_bs_invert's arithmetic), and the B linear solves of an ADMM iteration are one product
// X~ = K^-1 R on the matrix cores.  During a solve the vectors of the batch live index-major in HBM -- element j of
// member b at [j * Bp + b], Bp = B rounded up to 16 -- which is the layout the GEMM reads and writes, and in which a
// wavefront of the element-wise kernels walks 64 members of one row or column: the pattern and the matrix values are
// uniform over the wavefront, the vector loads and stores are contiguous.  Between solves the members are kept
// member-major in the workspace of the other engines (io.Wq, Wl, Wu, Xs, Zs, Ys; D, E, c and the classes replicated
// per member), so update, get and the device routes run the kernels they always ran.
//
// Per ADMM iteration, plain launches on the handle's stream:
//   k_bc_rhs    R = sigma x - q + A' w          (w = rho z - y, kept by the step)
//   k_bc_gemm   X~ = K^-1 R                     v_mfma_f64_16x16x4_f64, 64 x 64 tile per workgroup
//   [refinement, when the probe's verdict is on or still open:
//    k_bc_rows  T = rho .* (A X~);  k_bc_resid  Rr = R - (P X~ + sigma X~ + A' T);  k_bc_probe (open verdict only);
//    k_bc_gemm  X~ = K^-1 Rr + X~]
//   k_bc_step   z~ = A x~, then the x, z, y, w updates with relaxation and projection; finished members are skipped
// At check and adaptation points k_bc_check runs one workgroup per running member on the member's vectors in LDS:
// update_info / check_termination / store_solution of batch_admm.h, the code the other engines run.
// No floating-point atomics: every value has one owner and a fixed summation order, so a member's bits do not depend
// on its position in the batch or on B.  (The count of finished members is an integer atomicAdd.)

#define BC_TX 64           // members per workgroup of the element-wise kernels (one wavefront wide)
#define BC_TY 4            // rows or columns per workgroup
#define BC_TILE 64         // k_bc_gemm: output tile
#define BC_KC 16           // k_bc_gemm: k rows per LDS chunk
#define BC_LP 80           // k_bc_gemm: LDS row pitch in doubles (lanes lk, lk + 1 land 32 banks apart)

struct BCT {               // the index-major arrays of a solve (device), pitch Bp
  double *q, *x, *dx;      // [NP][Bp]
  double *l, *u, *z, *y, *w, *dy, *T;   // [m][Bp]; T = rho .* (A x~) of the refinement
  double *R, *Xt, *Rr;     // [NP][Bp] right-hand side, x~, residual of the refinement; rows [n, NP) stay zero
  int *done;               // [B] per column: 1 once its member has finished
  int *verdict;            // [B] per column: 1 when a probe found the member's relative residual above refine_tol
  double *est;             // [B] per column: rho estimate of a running member at an adaptation point, -1 once it has finished
  int *count;              // [1] finished members
  int *bad;                // [B + 1] class check: first disagreeing row per member (-1: none); [B]: a common class moved
  int *mem;                // [Bp] the member that owns a column (written by k_bc_load, moved by k_bc_pack)
  int *src;                // [B] host-written lists: the members of a subset solve, then the source columns of a pack
  int Bp;                  // the pitch of the allocation: B rounded up to 16
  int C;                   // the columns in use
};

typedef double bc_d4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// setup and updates
// ---------------------------------------------------------------------------
// D, E, c and the row classes of member 0 (the one-member image k_bs_setup scaled) for every other member
__global__ void __launch_bounds__(256) k_bc_spread(int n, int m, BIO io) {
  const long long qp = (long long)blockIdx.x + 1;
  for (int j = threadIdx.x; j < n; j += 256) io.Wd[qp * n + j] = io.Wd[j];
  for (int i = threadIdx.x; i < m; i += 256) { io.We[qp * m + i] = io.We[i]; io.Wt[qp * m + i] = io.Wt[i]; }
  if (threadIdx.x == 0) io.Wc[qp] = io.Wc[0];
}

// q^_j = max_b |Q[b][j]| of the raw [B][n] Q the handle holds (osqp_amd_batch_common_update_model): one thread per
// column walks the members, so a wavefront reads 64 contiguous doubles of each member.  A max is exact: q^ carries
// the bits of setup's host loop (bc_setup_launch), whatever the order.
__global__ void __launch_bounds__(256) k_bc_qhat(int n, long long B, const double *__restrict__ Q, double *__restrict__ qhat) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double v = 0.0;
#pragma unroll 8                                  // (eight members' loads in flight: the walk is latency-bound)
  for (long long b = 0; b < B; ++b) v = fmax(v, fabs(Q[b * n + j]));
  qhat[j] = v;
}

// Every member's scaled q, l, u from its stored raw Q, L, U with the D, E, c the model update has just spread:
// k_batch_update's expressions without its re-classification -- the row classes (io.Wt) and io.flag stay as they are,
// as in the reference's matrix update -- and reset_info's rho_updates = 0.  One workgroup per member.
__global__ void __launch_bounds__(256) k_bc_rescale(int n, int m, BIO io) {
  const long long qp = blockIdx.x;
  const double c = io.Wc[qp];
  for (int j = threadIdx.x; j < n; j += 256) io.Wq[qp * n + j] = (io.Q[qp * n + j] * io.Wd[qp * n + j]) * c;
  for (int i = threadIdx.x; i < m; i += 256) {
    const double e = io.We[qp * m + i];
    io.Wl[qp * m + i] = io.L[qp * m + i] * e;
    io.Wu[qp * m + i] = io.U[qp * m + i] * e;
  }
  if (threadIdx.x == 0) io.info[qp * 8 + 5] = 0.0;
}

// Would the bounds L, U (raw, [B][m]; null = the member's scaled bound as stored) leave every row with one class over
// the batch?  bad[qp] = the first row whose class differs from member 0's (-1: none); bad[B] = 1 when the class of
// some row of member 0 differs from the stored one (K is then due).  Writes nothing of the workspace.
// list (null: every member): one workgroup per listed member, L and U compact (row blockIdx.x); the class to agree
// with is the one the handle holds (io.Wt of member 0: the unlisted members keep it), bad[blockIdx.x] the verdict, and
// bad[B] is not written.
__global__ void __launch_bounds__(256) k_bc_classes(int m, long long B, BIO io, const double *L, const double *U,
                                                    int clamp, double rho_tol, int *bad, const int *list) {
  __shared__ int first;
  const long long qp = list ? list[blockIdx.x] : blockIdx.x, src = blockIdx.x;
  if (threadIdx.x == 0) first = m;
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += 256) {
    const double e = io.We[i];
    double lb, ub, l0, u0;
    if (L) { lb = L[src * m + i]; l0 = L[i]; if (clamp) { lb = lb < -OSQP_INFTY ? -OSQP_INFTY : lb; l0 = l0 < -OSQP_INFTY ? -OSQP_INFTY : l0; } lb *= e; l0 *= e; }
    else { lb = io.Wl[qp * m + i]; l0 = io.Wl[i]; }
    if (U) { ub = U[src * m + i]; u0 = U[i]; if (clamp) { ub = ub > OSQP_INFTY ? OSQP_INFTY : ub; u0 = u0 > OSQP_INFTY ? OSQP_INFTY : u0; } ub *= e; u0 *= e; }
    else { ub = io.Wu[qp * m + i]; u0 = io.Wu[i]; }
    const int t0 = list ? io.Wt[i] : row_class(l0, u0, rho_tol);
    if (row_class(lb, ub, rho_tol) != t0) atomicMin(&first, i);
    if (!list && qp == 0 && t0 != io.Wt[i]) bad[B] = 1;
  }
  __syncthreads();
  if (threadIdx.x == 0) bad[src] = first < m ? first : -1;
}

// the common K is due: k_bs_form reads member 0's flag and rho
__global__ void k_bc_mark(BIO io, double rho) {
  if (threadIdx.x == 0) { io.flag[0] = (io.flag[0] & BF_REFINE) | BF_REBUILD; io.rho_io[0] = rho; }
}

// One pivot of the Gauss-Jordan inversion of the one K, over the whole GPU: out = the matrix after pivot k of gj_sweep
// (batch_streamed.h) applied to in -- the same expression per entry, so the inverse has the bits k_bs_invert gives --
// with one owner per entry and two buffers instead of a workgroup's barrier.  k_bs_invert runs one workgroup per
// member, which suits a batch of matrices; for the single matrix of this engine it leaves all but one CU idle
// (measured at n = 600, B = 1024: a cold solve with two inversions took 140 ms with it and takes 51 ms this way;
// a pivot launch takes 3.8 us at n = 300 and 5.6 us at n = 1000).  Entries outside the n x n block (the identity padding) are
// copied.  Pivot 0 stores the flag word of a finished rebuild (BF_OPEN), a non-positive pivot adds BF_NOT_PD.
__global__ void __launch_bounds__(256) k_bc_pivot(const double *__restrict__ in, double *__restrict__ out, int n, int NP, int k, BIO io) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  const double akk = in[(size_t)k * NP + k];
  const double piv = 1.0 / akk;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
    int f = k == 0 ? BF_OPEN : io.flag[0];
    if (!(akk > 0.0)) f |= BF_NOT_PD;
    io.flag[0] = f;
  }
  if (j >= NP) return;
  const double rkj = j < n ? in[(size_t)k * NP + j] * piv : 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = blockIdx.y * 16 + threadIdx.y + 4 * r;
    if (i >= NP) continue;
    const double a = in[(size_t)i * NP + j];
    double v = a;
    if (i < n && j < n) {
      const double ci = in[(size_t)i * NP + k];
      if (i == k) v = j == k ? piv : rkj;
      else v = j == k ? 0.0 - ci * piv : __builtin_fma(-ci, rkj, a);
    }
    out[(size_t)i * NP + j] = v;
  }
}

// k_bc_pivot for two matrices in one launch: blockIdx.z chooses (in, out, flag word) of K or of H = (P~ + delta I)^-1, which
// a model update on a handle with the shared KKT pieces inverts side by side -- the 2n pivot launches are launch-bound and
// the two sequences independent.  The same expression per entry as k_bc_pivot, hence the same bits.
struct BCPair { const double *in[2]; double *out[2]; int *flag[2]; };
__global__ void __launch_bounds__(256) k_bc_pivot2(BCPair a, int n, int NP, int k) {
  const bool h = blockIdx.z != 0;                   // (selects, not an index: the argument stays in scalar registers)
  const double *__restrict__ in = h ? a.in[1] : a.in[0];
  double *__restrict__ out = h ? a.out[1] : a.out[0];
  const int j = blockIdx.x * 64 + threadIdx.x;
  const double akk = in[(size_t)k * NP + k];
  const double piv = 1.0 / akk;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
    int *flag = h ? a.flag[1] : a.flag[0];
    int f = k == 0 ? BF_OPEN : flag[0];
    if (!(akk > 0.0)) f |= BF_NOT_PD;
    flag[0] = f;
  }
  if (j >= NP) return;
  const double rkj = j < n ? in[(size_t)k * NP + j] * piv : 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = blockIdx.y * 16 + threadIdx.y + 4 * r;
    if (i >= NP) continue;
    const double v0 = in[(size_t)i * NP + j];
    double v = v0;
    if (i < n && j < n) {
      const double ci = in[(size_t)i * NP + k];
      if (i == k) v = j == k ? piv : rkj;
      else v = j == k ? 0.0 - ci * piv : __builtin_fma(-ci, rkj, v0);
    }
    out[(size_t)i * NP + j] = v;
  }
}

// k_batch_warm_start with the one slab of scaled values
__global__ void __launch_bounds__(256) k_bc_warm_start(BPattern p, BIO io, const double *X, const double *Y, const int *list) {
  __shared__ double xs[BW_MAX_N];
  const long long qp = list ? list[blockIdx.x] : blockIdx.x, src = blockIdx.x;
  const int n = p.n, m = p.m;
  if (X) {
    for (int j = threadIdx.x; j < n; j += 256) {
      const double v = (1.0 / io.Wd[qp * n + j]) * X[src * n + j];
      xs[j] = v; io.Xs[qp * n + j] = v;
    }
    __syncthreads();
    const double *Av = io.Wv + p.nnzP;
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
// the solve: element-wise kernels, thread (tx, ty) = column blockIdx.x * 64 + tx, index blockIdx.y * 4 + ty
// ---------------------------------------------------------------------------
#define BC_MEMBER_INDEX \
  const long long b = (long long)blockIdx.x * BC_TX + threadIdx.x; \
  const int idx = blockIdx.y * BC_TY + threadIdx.y;                \
  if (b >= t.C) return;

// the member-major workspace into the index-major arrays of the solve, member members[b] (null: member b) into column b;
// cold: zero iterates
__global__ void __launch_bounds__(BC_TX * BC_TY) k_bc_load(int n, int m, BIO io, BCT t, const int *__restrict__ members,
                                                           double rho, int warm) {
  BC_MEMBER_INDEX
  const long long Bp = t.Bp, qp = members ? members[b] : b;
  if (idx < n) {
    t.q[idx * Bp + b] = io.Wq[qp * n + idx];
    t.x[idx * Bp + b] = warm ? io.Xs[qp * n + idx] : 0.0;
    t.dx[idx * Bp + b] = 0.0;
  }
  if (idx < m) {
    const double z = warm ? io.Zs[qp * m + idx] : 0.0, y = warm ? io.Ys[qp * m + idx] : 0.0;
    t.l[idx * Bp + b] = io.Wl[qp * m + idx]; t.u[idx * Bp + b] = io.Wu[qp * m + idx];
    t.z[idx * Bp + b] = z; t.y[idx * Bp + b] = y; t.dy[idx * Bp + b] = 0.0;
    t.w[idx * Bp + b] = rho_of_class(io.Wt[idx], rho) * z - y;
  }
  if (idx == 0) { t.mem[b] = (int)qp; t.done[b] = 0; t.est[b] = 0.0; t.verdict[b] = 0; }
}

// R = sigma x - q + A' w
__global__ void __launch_bounds__(BC_TX * BC_TY) k_bc_rhs(BPattern p, BIO io, BCT t, double sigma) {
  BC_MEMBER_INDEX
  if (idx >= p.n) return;
  const long long Bp = t.Bp;
  const double *Av = io.Wv + p.nnzP;
  double acc = 0.0;
  for (int k = p.Ap[idx]; k < p.Ap[idx + 1]; ++k) acc += Av[k] * t.w[p.Ai[k] * Bp + b];
  t.R[idx * Bp + b] = (sigma * t.x[idx * Bp + b] - t.q[idx * Bp + b]) + acc;
}

// T = rho .* (A X~)
__global__ void __launch_bounds__(BC_TX * BC_TY) k_bc_rows(BPattern p, BIO io, BCT t, double rho) {
  BC_MEMBER_INDEX
  if (idx >= p.m) return;
  const long long Bp = t.Bp;
  const double *Av = io.Wv + p.nnzP;
  double acc = 0.0;
  for (int k = p.Rp[idx]; k < p.Rp[idx + 1]; ++k) acc += Av[p.Rk[k]] * t.Xt[p.Rj[k] * Bp + b];
  t.T[idx * Bp + b] = rho_of_class(io.Wt[idx], rho) * acc;
}

// Rr = R - K X~ through the sparse operator: K X~ = P X~ + sigma X~ + A' T
__global__ void __launch_bounds__(BC_TX * BC_TY) k_bc_resid(BPattern p, BIO io, BCT t, double sigma) {
  BC_MEMBER_INDEX
  if (idx >= p.n) return;
  const long long Bp = t.Bp;
  const double *Pv = io.Wv, *Av = io.Wv + p.nnzP;
  double px = 0.0, at = 0.0;
  for (int k = p.Fp[idx]; k < p.Fp[idx + 1]; ++k) px += Pv[p.Fk[k]] * t.Xt[p.Fi[k] * Bp + b];
  for (int k = p.Ap[idx]; k < p.Ap[idx + 1]; ++k) at += Av[k] * t.T[p.Ai[k] * Bp + b];
  t.Rr[idx * Bp + b] = t.R[idx * Bp + b] - (px + sigma * t.Xt[idx * Bp + b] + at);
}

// the probe of the explicit-inverse solve: one thread per running column, |Rr|_inf against refine_tol |R|_inf
__global__ void __launch_bounds__(256) k_bc_probe(int n, BCT t, double refine_tol) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= t.C || t.done[b]) return;
  const long long Bp = t.Bp;
  double rmax = 0.0, bmax = 0.0;
  for (int j = 0; j < n; ++j) { rmax = fmax(rmax, fabs(t.Rr[j * Bp + b])); bmax = fmax(bmax, fabs(t.R[j * Bp + b])); }
  if (rmax > refine_tol * bmax) t.verdict[b] = 1;
}

// z~ = A x~ and the x, z, y updates (auxil.c:185-225, proj.c:4-14), as admm_loop; rows first, then columns
__global__ void __launch_bounds__(BC_TX * BC_TY) k_bc_step(BPattern p, BIO io, BCT t, double rho, double alpha) {
  BC_MEMBER_INDEX
  if (t.done[b]) return;                     // a finished member is frozen
  const long long Bp = t.Bp;
  const double oma = 1.0 - alpha;
  if (idx < p.m) {
    const double *Av = io.Wv + p.nnzP;
    double zt = 0.0;
    for (int k = p.Rp[idx]; k < p.Rp[idx + 1]; ++k) zt += Av[p.Rk[k]] * t.Xt[p.Rj[k] * Bp + b];
    const long long e = idx * Bp + b;
    const double ri = rho_of_class(io.Wt[idx], rho), rinv = 1.0 / ri;
    const double zo = t.z[e], yo = t.y[e];
    double v = alpha * zt + oma * zo + rinv * yo;
    v = fmax(v, t.l[e]);
    const double zn = fmin(v, t.u[e]);
    const double dy = ri * (alpha * zt + oma * zo - zn);
    const double yn = yo + dy;
    t.z[e] = zn; t.dy[e] = dy; t.y[e] = yn;
    t.w[e] = ri * zn - yn;
  } else if (idx - p.m < p.n) {
    const long long e = (long long)(idx - p.m) * Bp + b;
    const double xo = t.x[e];
    const double xn = alpha * t.Xt[e] + oma * xo;
    t.dx[e] = xn - xo; t.x[e] = xn;
  }
}

// rho has moved: w = rho z - y of the running members with the new rho (refresh_w)
__global__ void __launch_bounds__(BC_TX * BC_TY) k_bc_load_w(int m, BIO io, BCT t, double rho) {
  BC_MEMBER_INDEX
  if (idx >= m || t.done[b]) return;
  const long long e = idx * (long long)t.Bp + b;
  t.w[e] = rho_of_class(io.Wt[idx], rho) * t.z[e] - t.y[e];
}

// rho has moved: every running member counts the update
__global__ void __launch_bounds__(256) k_bc_adopt(BIO io, BCT t) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b < t.C && !t.done[b]) io.info[(long long)t.mem[b] * 8 + 5] += 1.0;
}

// ---------------------------------------------------------------------------
// X~ = K^-1 R (+ add) on v_mfma_f64_16x16x4_f64.  K^-1 is symmetric, so the A operand (16 rows x 4 k) is read as 4 rows
// of K^-1 x 16 contiguous doubles; the B operand is 4 rows of R x 16 members.  A workgroup of four wavefronts owns a
// 64 x 64 tile (a wavefront: 32 x 32, 2 x 2 MFMA tiles); both operands go through LDS in chunks of BC_KC k rows, the
// next chunk's global loads in flight while the current one is multiplied.  Every output element accumulates k = 0,
// 4, 8, ... NP - 4 in this order whatever its tile, so a member's bits depend neither on its column nor on B.
// Bp is the pitch, C the columns in use: the grid and the guards cover Cp = C rounded up to 16 (the columns of [C, Cp)
// hold whatever earlier columns left there; nobody reads their product).  NP is a multiple of 32 and Cp of 16: the
// double2 loads are aligned and guarded by the even index alone.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bc_gemm(const double *__restrict__ Kinv, const double *__restrict__ Rin, double *out,
                                                 const double *add, int NP, int Bp, int C) {
  const int Cp = (C + 15) & ~15;
  __shared__ __attribute__((aligned(16))) double As[BC_KC * BC_LP], Bs[BC_KC * BC_LP];
  const int row0 = blockIdx.y * BC_TILE, col0 = blockIdx.x * BC_TILE;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, li = lane & 15, lk = lane >> 4;
  const int wr = (wv >> 1) * 32, wc = (wv & 1) * 32;
  bc_d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = bc_d4{0.0, 0.0, 0.0, 0.0};
  // thread t takes the double2 at (k row p / 32, column pair p % 32), p = t + 256 u, u < 2, of each operand
  double2 ga[2], gb[2];
  auto gload = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = t + 256 * u, kk = k0 + (p >> 5), c2 = (p & 31) * 2;
      ga[u] = row0 + c2 < NP ? *reinterpret_cast<const double2 *>(Kinv + (size_t)kk * NP + row0 + c2) : double2{0.0, 0.0};
      gb[u] = col0 + c2 < Cp ? *reinterpret_cast<const double2 *>(Rin + (size_t)kk * Bp + col0 + c2) : double2{0.0, 0.0};
    }
  };
  gload(0);
  for (int k0 = 0; k0 < NP; k0 += BC_KC) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = t + 256 * u, kr = p >> 5, c2 = (p & 31) * 2;
      *reinterpret_cast<double2 *>(As + kr * BC_LP + c2) = ga[u];
      *reinterpret_cast<double2 *>(Bs + kr * BC_LP + c2) = gb[u];
    }
    __syncthreads();
    if (k0 + BC_KC < NP) gload(k0 + BC_KC);
#pragma unroll
    for (int s = 0; s < BC_KC / 4; ++s) {
      double a[2], bv[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) { a[q] = As[(4 * s + lk) * BC_LP + wr + 16 * q + li]; bv[q] = Bs[(4 * s + lk) * BC_LP + wc + 16 * q + li]; }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bv[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // D[row = lk + 4 r][col = li]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + wr + 16 * i + lk + 4 * r, col = col0 + wc + 16 * j + li;
        if (row < NP && col < Cp) {
          const size_t e = (size_t)row * Bp + col;
          out[e] = add ? acc[i][j][r] + add[e] : acc[i][j][r];
        }
      }
}

// ---------------------------------------------------------------------------
// check and adaptation points: one workgroup per running column, its member's vectors in LDS, batch_admm.h's code.
// checked / adapt: what admm_loop does after iteration `iter` (check_termination, then the rho estimate of a member
// that goes on).  final: the solve ends here (iter >= max_iter; the host has dealt with rho): the stage machine's
// tail -- the exact test unless `checked` already made it, then the approximate one, then OSQP_MAX_ITER_REACHED;
// final = 2: the same where the host's clock ended the solve (bc_solve), with OSQP_TIME_LIMIT_REACHED.
// A member that finishes stores its solution (store_solution), sets done, est = -1 and counts itself.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BS_NT) k_bc_check(BPattern p, BSettings st, BIO io, BCT t, int NP, double rho, int iter,
                                                    int checked, int adapt, int final) {
  const long long col = blockIdx.x;
  if (t.done[col]) return;
  const long long qp = t.mem[col];                     // the member: the workspace and the results are addressed by it
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const BL s = bs_layout(lds, p, io, 0, NP);           // the one slab of scaled values
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const long long Bp = t.Bp;
  double *sc = s.red + 13;
  clear_vectors<BS_NT>(s);
  BA a;
  a.cs = load_workspace<BS_NT, true>(s, p, io, qp);
  a.rho = rho; a.iter = iter; a.rho_updates = (int)io.info[qp * 8 + 5];
  a.need_refine = a.check_pending = false;
  for (int j = tid; j < n; j += BS_NT) { s_x[j] = t.x[j * Bp + col]; s_dx[j] = t.dx[j * Bp + col]; }
  for (int i = tid; i < m; i += BS_NT) { s_z[i] = t.z[i * Bp + col]; s_y[i] = t.y[i * Bp + col]; s_dy[i] = t.dy[i * Bp + col]; }
  if (tid == 0) { for (int k = 0; k < S_COUNT_; ++k) sc[k] = 0.0; sc[S_STATUS] = OSQP_UNSOLVED; sc[S_RHO] = rho; }
  __syncthreads();
  update_info<BS_NT, false>(s, p, st, a.cs);
  bool fin = false;
  if (!final) {
    if (checked) fin = check_termination<BS_NT>(s, p, st, a.cs, false);
    if (!fin && adapt && tid == 0) t.est[col] = rho_estimate(sc, m, rho);
  } else {
    if (!checked) fin = check_termination<BS_NT>(s, p, st, a.cs, false);
    if (!fin && !check_termination<BS_NT>(s, p, st, a.cs, true)) {
      if (tid == 0) sc[S_STATUS] = final == 2 ? OSQP_TIME_LIMIT_REACHED : OSQP_MAX_ITER_REACHED;
      __syncthreads();
    }
    fin = true;
  }
  if (!fin) return;
  store_solution<BS_NT>(s, p, st, io, qp, a, 0);
  if (tid == 0) { t.done[col] = 1; t.est[col] = -1.0; atomicAdd(t.count, 1); }
}

// ---------------------------------------------------------------------------
// Stable compaction of the running columns: column c takes column t.src[c], c < Rn, with src increasing and
// src[c] >= c, in the nine state arrays (q, x, dx; l, u, z, y, w, dy) and in mem, est, verdict, done.  R, Xt, Rr and T
// are re-formed in every iteration before they are read and are not moved (rows [n, NP) of R are never written: they
// stay zero in every column).  In place: workgroup (row, array) owns one row of one array and walks it in ascending
// chunks of 256 columns, reading a chunk's sources, then -- after the barrier -- writing its destinations.  A chunk's
// sources lie at or beyond its first destination, hence beyond every destination of the chunks before it; its
// destinations are written only after the barrier every thread reaches once it has read the chunk, and a thread
// reaches the next barrier only after it has read the next chunk, so no source is overwritten before it is read.
// Array 9 is the four per-column words, moved by workgroup (0, 9) the same way.  Copies only: no arithmetic.
// ---------------------------------------------------------------------------
template <typename Tp>
__device__ __forceinline__ void bc_pack_row(Tp *row, const int *__restrict__ src, int Rn) {
  for (int c0 = 0; c0 < Rn; c0 += 256) {
    const int c = c0 + threadIdx.x;
    Tp v{};
    if (c < Rn) v = row[src[c]];
    __syncthreads();
    if (c < Rn) row[c] = v;
  }
}
__global__ void __launch_bounds__(256) k_bc_pack(int n, int m, BCT t, int Rn) {
  const int a = blockIdx.y;
  const long long r = blockIdx.x;
  if (a == 9) {
    if (r) return;
    bc_pack_row(t.mem, t.src, Rn); bc_pack_row(t.est, t.src, Rn);
    bc_pack_row(t.verdict, t.src, Rn); bc_pack_row(t.done, t.src, Rn);
    return;
  }
  if (r >= (a < 3 ? n : m)) return;
  double *const v = a == 0 ? t.q : a == 1 ? t.x : a == 2 ? t.dx : a == 3 ? t.l : a == 4 ? t.u : a == 5 ? t.z :
                    a == 6 ? t.y : a == 7 ? t.w : t.dy;
  bc_pack_row(v + r * t.Bp, t.src, Rn);
}
