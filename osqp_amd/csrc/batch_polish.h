// batch_polish.h -- polish (src/polish.c:19-350) for the solved members of a batch, included by batch.hip after
// both engines.  It serves either engine: it needs only the shared pattern, the member's scaled values (io.Wv),
// its scaled q, l, u, D, E, c and the scaled iterates the last solve left (io.Xs, io.Zs, io.Ys).
//
// Per member, in the member's scaled space like the reference (its w->data is scaled): guess the active rows,
// form the regularised KKT matrix [P + delta I, Ar'; Ar, -delta I] of order N = n + mred densely, invert it in
// place, solve for [-q; l_low; u_upp], take exactly polish_refine_iter refinement steps against the unregularised
// [P, Ar'; Ar, 0], project (z, y) on the normal cone, compute objective and residuals as update_info
// (batch_admm.h) does and apply the acceptance rule of polish.c:301-311.  The reference's delta and step count
// are kept on purpose: where active rows are linearly dependent x is unique but the multipliers are not, and
// the y the reference returns is a function of both.
//   k_bp_active  one workgroup per member: the two active tests, the index scan (lows first), mred and the
//                row <-> reduced-row maps;
//   k_bp_form    grid (NPOL rows, members of the chunk): row i of the member's NPOL x NPOL matrix, identity
//                beyond N; NPOL = n + largest mred of the batch, rounded up to 32;
//   k_bp_invert  one workgroup per member: the in-place Gauss-Jordan sweep of the streamed engine (gj_sweep,
//                batch_streamed.h) over N.  A quasi-definite matrix is strongly factorisable in this order: n
//                positive pivots, then mred negative ones; a pivot of the wrong sign (zero and NaN included)
//                rejects the member's polish;
//   k_bp_polish  one workgroup per member: everything after the inversion.
// The adjoint and the tangent (batch_adjoint.h, batch_tangent.h) run the same route with other right-hand sides and
// share its pieces: the three kernels above, load_row_maps and kkt_solve_refined.  What those two kernels have in
// common beyond that -- opening, close and LDS layout -- is bd_open, bd_close and bd_lds_bytes below; k_bp_polish's
// layout and tail differ and stay its own.
// The solve itself is a template parameter of the three kernels (FullK below: the inverse of the whole matrix, as
// described here; BlockK, batch_common_kkt.h: the common-K engine's block elimination on a shared Hessian inverse, which
// replaces k_bp_form and k_bp_invert by k_bk_form and k_bk_invert on the Schur complement of the active rows).
// An accepted member's X, Y, info8[2..4] and scaled iterates are overwritten; of a rejected or skipped
// member nothing is written but its status_polish.  rho, K^-1, io.flag, the row classes and rho_updates are
// never touched.

#define BP_MAX_N 2176      // largest order n + mred (n <= 1024, m <= 1129 in the streamed engine); k_bp_form's row buffer
#define BP_NT 512

struct BPol {              // polish workspace of a handle (device pointers)
  int *map;                // [B][m] reduced row of a row (lows first, then upps), -1 = not active
  int *rows;               // [B][m] row of a reduced row
  int *mred;               // [B] active rows; -1: the member's last solve did not end OSQP_SOLVED (skipped)
  int *nlow;               // [B] how many of them are active at the lower bound
  int *stat;               // [B] status_polish: 1 accepted, -1 tried and rejected, 0 not tried
  double *K;               // [members of a chunk][NPOL * NPOL] the KKT matrix, then its inverse (BlockK: [NS * NS], S and S^-1)
  const int *pos;          // [B] a member's row in the compact arrays of a _members call (null: its own index)
};

// Active rows from the stored scaled iterates and bounds (polish.c:19-100): low z - l < -y, upp u - z < y.
// (Both cannot hold for l <= u; a row that passed the low test is not tested again.)
// list (null: every member): one workgroup per listed member; of the others nothing is written.
__global__ void __launch_bounds__(256) k_bp_active(int m, BIO io, BPol pl, const int *list) {
  __shared__ int sc[256];
  __shared__ int base;
  const long long qp = list ? list[blockIdx.x] : blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) pl.stat[qp] = 0;
  if ((int)io.info[qp * 8 + 1] != OSQP_SOLVED) {
    if (tid == 0) pl.mred[qp] = -1;
    return;
  }
  const double *z = io.Zs + qp * m, *y = io.Ys + qp * m, *l = io.Wl + qp * m, *u = io.Wu + qp * m;
  int *map = pl.map + qp * m, *rows = pl.rows + qp * m;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int t0 = 0; t0 < m; t0 += 256) {
      const int i = t0 + tid;
      int f = 0;
      if (i < m) {
        const bool low = z[i] - l[i] < -y[i];
        f = pass == 0 ? low : (!low && u[i] - z[i] < y[i]);
      }
      sc[tid] = f;
      __syncthreads();
      for (int o = 1; o < 256; o <<= 1) {      // inclusive scan of the 256 flags
        const int v = tid >= o ? sc[tid - o] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
      }
      if (i < m) {
        if (f) { const int a = base + sc[tid] - 1; map[i] = a; rows[a] = i; }
        else if (pass == 0) map[i] = -1;
      }
      __syncthreads();
      if (tid == 255) base += sc[255];
      __syncthreads();
    }
    if (pass == 0 && tid == 0) pl.nlow[qp] = base;
  }
  if (tid == 0) pl.mred[qp] = base;
}

// Row i of [P + delta I, Ar'; Ar, -delta I] of member list[blockIdx.y] into slot blockIdx.y of the buffer.
// Both halves copy the same stored values, so the matrix is symmetric to the bit.
__global__ void __launch_bounds__(256) k_bp_form(BPattern p, BIO io, BPol pl, int NPOL, double delta, const int *list) {
  __shared__ __attribute__((aligned(16))) double row[BP_MAX_N];
  const long long qp = list[blockIdx.y];
  const int i = blockIdx.x, n = p.n, m = p.m, tid = threadIdx.x;
  const int N = n + pl.mred[qp];
  for (int j = tid; j < NPOL; j += 256) row[j] = 0.0;
  __syncthreads();
  const double *Pv = io.Wv + qp * ((long long)p.nnzP + p.nnzA), *Av = Pv + p.nnzP;
  if (i < n) {
    const int *map = pl.map + qp * m;
    for (int k = p.Fp[i] + tid; k < p.Fp[i + 1]; k += 256) row[p.Fi[k]] = Pv[p.Fk[k]];
    for (int k = p.Ap[i] + tid; k < p.Ap[i + 1]; k += 256) {
      const int a = map[p.Ai[k]];
      if (a >= 0) row[n + a] = Av[k];
    }
    __syncthreads();
    if (tid == 0) row[i] = row[i] + delta;
  } else if (i < N) {
    const int r = pl.rows[qp * m + (i - n)];
    for (int k = p.Rp[r] + tid; k < p.Rp[r + 1]; k += 256) row[p.Rj[k]] = Av[p.Rk[k]];
    if (tid == 0) row[i] = 0.0 - delta;
  } else if (tid == 0) row[i] = 1.0;             // identity padding
  __syncthreads();
  double *out = pl.K + (long long)blockIdx.y * NPOL * NPOL + (long long)i * NPOL;
  for (int j = tid; j < NPOL; j += 256) out[j] = row[j];
}

// gj_sweep over the order N = n + mred of the member in slot blockIdx.x, with exchange buffers of NPOL doubles
// (dynamic LDS: 4 * NPOL doubles) and the quasi-definite pivot verdict.
__global__ void __launch_bounds__(BS_NTI) k_bp_invert(int n, BPol pl, int NPOL, const int *list) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const long long qp = list[blockIdx.x];
  const bool bad = gj_sweep(pl.K + (long long)blockIdx.x * NPOL * NPOL, n + pl.mred[qp], NPOL, lds, lds + 2 * NPOL, NPOL,
                            [n](int k, double akk) { return k < n ? !(akk > 0.0) : !(akk < 0.0); });
  if (threadIdx.x == 0 && bad) pl.stat[qp] = -1;
}

// The member's row maps into LDS: map[0..m) and rows[0..mred) (visible after the next barrier).
__device__ __forceinline__ void load_row_maps(const BPol &pl, long long qp, int m, int mred, int *map, int *rows) {
  for (int i = threadIdx.x; i < m; i += BP_NT) {
    map[i] = pl.map[qp * m + i];
    if (i < mred) rows[i] = pl.rows[qp * m + i];
  }
}

// sol = K^-1 rhs, then exactly refine_iter steps of res = rhs - M sol, cor = K^-1 res, sol += cor against the
// unregularised M = [P, Ar'; Ar, 0] (polish.c:134-181), K^-1 being whatever apply(in, out) applies: out = K^-1 in on
// LDS vectors in the [x; nu] layout, ending on a barrier.  What kkt_solve_refined and kkt_solve_block
// (batch_common_kkt.h) share.  rhs(k): the right-hand side, k in [0, NPOL), zero in the padding [N, NPOL).  sol, res,
// cor: LDS, NPOL each; s: the member's slab_view; map, rows: LDS (load_row_maps).  Ends on a barrier.
template <class Apply, class Rhs>
__device__ __forceinline__ void kkt_refine(const BL &s, int NPOL, int n, int N, const int *map, const int *rows,
                                           int refine_iter, Rhs rhs, double *sol, double *res, double *cor, Apply apply) {
  const int tid = threadIdx.x;
  for (int k = tid; k < NPOL; k += BP_NT) res[k] = rhs(k);
  __syncthreads();
  apply(res, sol);
  for (int it = 0; it < refine_iter; ++it) {
    for (int k = tid; k < NPOL; k += BP_NT) {
      double v = 0.0;
      if (k < n) {
        double aty = 0.0;
        for (int kk = s.Ap[k]; kk < s.Ap[k + 1]; ++kk) {
          const int a = map[s.Ai[kk]];
          if (a >= 0) aty += s.Av[kk] * sol[n + a];
        }
        v = (rhs(k) - p_row_dot(s, sol, k)) - aty;
      } else if (k < N) v = rhs(k) - a_row_dot(s, sol, rows[k - n]);
      res[k] = v;
    }
    __syncthreads();
    apply(res, cor);
    for (int k = tid; k < N; k += BP_NT) sol[k] += cor[k];
    __syncthreads();
  }
}

// kkt_refine with the explicit inverse Kinv (NPOL x NPOL) of the whole regularised matrix
template <class Rhs>
__device__ __forceinline__ void kkt_solve_refined(const BL &s, const double *Kinv, int NPOL, int n, int N, const int *map,
                                                  const int *rows, int refine_iter, Rhs rhs, double *sol, double *res,
                                                  double *cor) {
  kkt_refine(s, NPOL, n, N, map, rows, refine_iter, rhs, sol, res, cor,
             [=](const double *in, double *out) { bs_gemv(Kinv, NPOL, N, in, out); });
}

// The KKT solver of k_bp_polish, k_ba_adjoint and k_bt_tangent, a template parameter of theirs as StreamedK is of the
// ADMM loop.  FullK: the tiled and the streamed engine -- every member has its own slab of values and the inverse of
// its whole regularised matrix, NPOL x NPOL, in slot blockIdx.x of the chunk's buffer.  (BlockK, the common-K engine's:
// batch_common_kkt.h.)  The last argument of solve is LDS scratch behind the kernel's own, which only BlockK uses.
struct FullK {
  __device__ __forceinline__ long long slab(long long qp) const { return qp; }
  __device__ __forceinline__ const double *inverse(const double *K, int NPOL) const { return K + (long long)blockIdx.x * NPOL * NPOL; }
  template <class Rhs>
  __device__ __forceinline__ void solve(const BL &s, const double *Kinv, int NPOL, int n, int N, const int *map, const int *rows,
                                        int refine_iter, Rhs rhs, double *sol, double *res, double *cor, double *) const {
    kkt_solve_refined(s, Kinv, NPOL, n, N, map, rows, refine_iter, rhs, sol, res, cor);
  }
};

// What k_ba_adjoint and k_bt_tangent hold of their workgroup's member once bd_open has run: its scalars and the
// carve-up of the LDS (bd_lds_bytes).  The member's slab_view stays a local of the kernel: held in here it cost the
// two kernels some 25 VGPRs.
struct BDView {
  long long qp, row, slot; // the member; its row of the call's arrays (pl.pos); its slice blockIdx.y of their [.][slices][.]
  int n, m, nlow, N;       // nlow of the N - n active rows sit at their lower bound
  double cs, cinv;         // the member's cost scaling c and 1 / c
  const double *Kinv;      // the solver's inverse of this member, slot blockIdx.x of the chunk (KS::inverse)
  double *sol, *res, *cor, *g;   // NPOL each: solution, residual, correction, right-hand side
  double *x, *D, *E, *y;   // n, n, m, m: the stored scaled iterates and the scaling
  int *map, *rows;         // m each (load_row_maps)
};

// LDS of k_ba_adjoint and k_bt_tangent: four vectors of NPOL (solution, residual, correction, right-hand side), x and
// D, E and y, and the two row maps.
__host__ __device__ __forceinline__ size_t bd_lds_bytes(int n, int m, int NPOL) {
  const size_t b = sizeof(double) * (4 * (size_t)NPOL + 2 * (size_t)n + 2 * (size_t)m) + sizeof(int) * 2 * (size_t)m;
  return (b + 15) & ~(size_t)15;
}

// The opening of a derivative kernel, grid (members of the chunk, slices).  pl.stat is the pivot verdict of the call's
// inversion (0, or -1 from k_bp_invert) and is only read; stat is the status the caller sees.  False (for the whole
// workgroup): the inversion met a pivot of the wrong sign, slice 0 has reported -1 and the outputs stay 0.  True: v is
// filled and x, D, E, y and the row maps are on their way into LDS (visible after the next barrier).
template <class KS>
__device__ __forceinline__ bool bd_open(const BPattern &p, const BIO &io, const BPol &pl, int *stat, int slices, int NPOL,
                                        const int *list, double *lds, const KS &ks, BDView &v) {
  const long long qp = list[blockIdx.x];
  const int tid = threadIdx.x;
  const long long row = pl.pos ? pl.pos[qp] : qp;
  if (pl.stat[qp] == -1) {
    if (blockIdx.y == 0 && tid == 0) stat[row] = -1;
    return false;
  }
  const int n = p.n, m = p.m;
  const int mred = pl.mred[qp];
  v.qp = qp; v.row = row; v.slot = row * slices + blockIdx.y;
  v.n = n; v.m = m; v.nlow = pl.nlow[qp]; v.N = n + mred;
  v.Kinv = ks.inverse(pl.K, NPOL);
  v.sol = lds; v.res = v.sol + NPOL; v.cor = v.res + NPOL; v.g = v.cor + NPOL;
  v.x = v.g + NPOL; v.D = v.x + n; v.E = v.D + n; v.y = v.E + m;
  v.map = reinterpret_cast<int *>(v.y + m); v.rows = v.map + m;
  v.cs = io.Wc[qp]; v.cinv = 1.0 / v.cs;
  for (int j = tid; j < n; j += BP_NT) { v.x[j] = io.Xs[qp * n + j]; v.D[j] = io.Wd[qp * n + j]; }
  for (int i = tid; i < m; i += BP_NT) { v.E[i] = io.We[qp * m + i]; v.y[i] = io.Ys[qp * m + i]; }
  load_row_maps(pl, qp, m, mred, v.map, v.rows);
  return true;
}

// The close of a derivative kernel: slice 0 of a member alone writes what is per member, `active` (-1 active at the
// lower bound, +1 at the upper, 0 inactive) and the status, so the slices of a member neither read what another
// writes nor write the same word.
__device__ __forceinline__ void bd_close(const BDView &v, int *active, int *stat) {
  if (blockIdx.y != 0) return;
  for (int i = threadIdx.x; i < v.m; i += BP_NT) {
    const int a = v.map[i];
    active[v.row * v.m + i] = a < 0 ? 0 : (a < v.nlow ? -1 : 1);
  }
  if (threadIdx.x == 0) stat[v.row] = 1;
}

// LDS of k_bp_polish: three vectors of NPOL (solution, residual, correction), q, D, five m-vectors (l, u, E, z, y),
// 32 reduction doubles and the two row maps.
__host__ __device__ __forceinline__ size_t bp_lds_bytes(int n, int m, int NPOL) {
  const size_t b = sizeof(double) * (3 * (size_t)NPOL + 2 * (size_t)n + 5 * (size_t)m + 32) + sizeof(int) * 2 * (size_t)m;
  return (b + 15) & ~(size_t)15;
}

template <class KS, class... KSArg>
__global__ void __launch_bounds__(BP_NT) k_bp_polish(BPattern p, BSettings st, BIO io, BPol pl, int NPOL, int refine_iter,
                                                     const int *list, KSArg... ksarg) {
  const KS ks{ksarg...};
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const long long qp = list[blockIdx.x];
  if (pl.stat[qp] == -1) return;                 // the inversion met a pivot of the wrong sign
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const int mred = pl.mred[qp], nlow = pl.nlow[qp], N = n + mred;
  const double *Kinv = ks.inverse(pl.K, NPOL);
  double *sol = lds, *res = sol + NPOL, *cor = res + NPOL;
  double *q = cor + NPOL, *D = q + n, *l = D + n, *u = l + m, *E = u + m, *z = E + m, *y = z + m, *gp = y + m;
  int *map = reinterpret_cast<int *>(gp + 32), *rows = map + m;
  BL s;
  slab_view(s, p, io, ks.slab(qp));
  for (int j = tid; j < n; j += BP_NT) { q[j] = io.Wq[qp * n + j]; D[j] = io.Wd[qp * n + j]; }
  for (int i = tid; i < m; i += BP_NT) { l[i] = io.Wl[qp * m + i]; u[i] = io.Wu[qp * m + i]; E[i] = io.We[qp * m + i]; }
  load_row_maps(pl, qp, m, mred, map, rows);
  const double cs = io.Wc[qp], pri0 = io.info[qp * 8 + 3], dua0 = io.info[qp * 8 + 4];
  __syncthreads();
  // rhs = [-q; l of the active lows; u of the active upps] (polish.c:226-233), zero in the padding
  auto rhs = [&](int k) -> double {
    if (k < n) return -q[k];
    if (k >= N) return 0.0;
    const int r = rows[k - n];
    return k - n < nlow ? l[r] : u[r];
  };
  ks.solve(s, Kinv, NPOL, n, N, map, rows, refine_iter, rhs, sol, res, cor, lds + bp_lds_bytes(n, m, NPOL) / sizeof(double));
  // z = A x, y from the multipliers of the active rows, (z, y) on the normal cone (polish.c:262-279, proj.c:16-29);
  // then objective and residuals of the polished point as update_info computes them (auxil.c:227-318)
  const bool unscaled = st.scaling && !st.scaled_termination;
  const double cinv = 1.0 / cs;
  double mx[2] = {0.0, 0.0}, sm[1] = {0.0};
  for (int i = tid; i < m; i += BP_NT) {
    const double ax = a_row_dot(s, sol, i);
    const int a = map[i];
    const double t = ax + (a >= 0 ? sol[n + a] : 0.0);
    const double zi = fmin(fmax(t, l[i]), u[i]);
    z[i] = zi; y[i] = t - zi;
    const double pr = ax + (-1.0) * zi;
    mx[0] = fmax(mx[0], fabs(unscaled ? (1.0 / E[i]) * pr : pr));
  }
  __syncthreads();
  for (int j = tid; j < n; j += BP_NT) {
    const double px = p_row_dot(s, sol, j), qj = q[j];
    double dr = qj + px;
    if (m > 0) dr = dr + a_col_dot(s, y, j);
    mx[1] = fmax(mx[1], fabs(unscaled ? (1.0 / D[j]) * dr : dr));
    sm[0] += sol[j] * (0.5 * px + qj);
  }
  b_reduce_many<BP_NT / 64, 2, 1>(mx, sm, gp);
  const double *g = gp + (BP_NT / 64) * 3;
  const double pri = m == 0 ? 0.0 : g[0];
  const double dua = unscaled ? g[1] * cinv : g[1];
  const double obj = g[2] * (st.scaling ? cinv : 1.0);
  // polish.c:301-311
  const bool ok = (pri < pri0 && dua < dua0) || (pri < pri0 && dua0 < 1e-10) || (dua < dua0 && pri0 < 1e-10);
  if (!ok) {
    if (tid == 0) pl.stat[qp] = -1;
    return;
  }
  for (int j = tid; j < n; j += BP_NT) {
    io.Xo[qp * n + j] = st.scaling ? sol[j] * D[j] : sol[j];
    io.Xs[qp * n + j] = sol[j];
  }
  for (int i = tid; i < m; i += BP_NT) {
    io.Yo[qp * m + i] = st.scaling ? (y[i] * E[i]) * cinv : y[i];
    io.Ys[qp * m + i] = y[i]; io.Zs[qp * m + i] = z[i];
  }
  if (tid == 0) {
    double *inf = io.info + qp * 8;
    inf[2] = obj; inf[3] = pri; inf[4] = dua;
    pl.stat[qp] = 1;
  }
}
