// verify.h -- the verdict on a point (x, y) and on certificates (dx, dy) against the RAW problem of one workspace (osqp_amd_verify in
// osqp_host.c), included by engine.hip.  The single-QP twin of batch_verify.h: the same record of 16 doubles, slot for slot
//    0 obj = x'Px / 2 + q'x      1 pri_res = |Ax - z|oo, z = clamp(Ax, l, u)      2 dua_res = |Px + q + A'y|oo
//    3 |Ax|oo   4 |z|oo   5 |Px|oo   6 |A'y|oo   7 |q|oo
//    8 eps_pri = eps_abs + eps_rel max(3, 4)          9 eps_dua = eps_abs + eps_rel max(5, 6, 7)
//   10 comp = max_i max(y+_i (u_i - z_i), y-_i (z_i - l_i))      11 dual_obj = -x'Px / 2 - sum_i (u_i y+_i - l_i y-_i)
//   12 gap = obj - dual_obj      13 optimal: pri_res < eps_pri and dua_res < eps_dua (strict, auxil.c:725,737)
//   14 prim_inf: is_primal_infeasible (auxil.c:361-424) on dy      15 dual_inf: is_dual_infeasible (auxil.c:426-512) on dx
// with y+ = max(y, 0), y- = max(-y, 0), D = E = I, c = 1, the same rule for infinite bounds (u > 1e26, l < -1e26: a term of 10 or 11
// whose multiplier part is 0 counts 0, a nonzero one makes 10 +OSQP_INFTY, 11 -OSQP_INFTY, 12 +OSQP_INFTY) and the same rule for
// "NaN" (an IEEE NaN or the number OSQP_NAN; one in x or y: 0-12 are OSQP_NAN and 13 is 0; one in dy / dx: 14 / 15 is 0).
// A hipver belongs to one workspace: it holds the patterns (A by rows with the CSC slot of each entry, A by columns, the full symmetric
// P with the triu slot of each entry: BPattern's Rp / Rj / Rk, Ap / Ai, Fp / Fi / Fk, built from the CSC pattern alone), device copies
// of the raw Px, Ax, q, l, u, and a buffer of per-workgroup partial results.  It knows nothing of the linear-solve form, the scaling or rho.
//   k_ver_point     one wavefront per row of A, then per column (row of the symmetric P and column of A): the lanes stride the entries,
//                   a fixed butterfly sums them (sens_wave_sum), and the finished entry goes into the wavefront's running maxima and
//                   sums, which are the same in all its lanes.  A row or column with more than VER_LONG entries is left out of the sweep
//                   and taken by a whole workgroup afterwards (threads stride, butterfly, the four wavefronts in order).  The workgroup
//                   adds its four wavefronts in order and stores one partial record.  It also projects dy, stores the projection, and
//                   takes |dy|oo, |dx|oo, u'dy+ + l'dy-, q'dx.
//   k_ver_combine   one wavefront; lane k walks slot k of the partial records in index order.  Stage 0 writes slots 0-13 and the scalars
//                   the certificates need; stage 1 writes slots 14 and 15.
//   k_ver_cert      A'dy, P dx, A dx by the same sweeps; the row test of A dx needs |dx|oo, hence the second launch.
// No atomics.  The grid is ver_grid(n, m): a record depends on the pattern, the values and the point, and on nothing else.

#define VER_NT 256               // threads per workgroup
#define VER_ROWS (VER_NT / 64)   // rows (or columns) a workgroup takes per sweep: one per wavefront
#define VER_GRID_CAP 1024        // workgroups at most
#define VER_LONG 512             // a row or column with more entries than this is taken by a workgroup, not by a wavefront
#define VER_SLOTS 16
#define VER_BINF INF_BOUND

enum { VP_PRI, VP_AX, VP_Z, VP_DUA, VP_PX, VP_ATY, VP_Q, VP_COMP, VP_INF, VP_NAN, VP_NDY, VP_NDX, VP_NANDY, VP_NANDX, VP_NMAX,
       VP_XPX = VP_NMAX, VP_QX, VP_SUP, VP_INEQ, VP_QDX, VP_N };   // k_ver_point: maxima, then sums
enum { VC_NATDY, VC_NPDX, VC_VIOL, VC_N };                          // k_ver_cert: maxima only
enum { VM_NDY, VM_NDX, VM_INEQ, VM_QDX, VM_NANDY, VM_NANDX, VM_N }; // what stage 0 leaves for the certificates

struct VerCtx {
  int n, m, nlongR, nlongC;
  const int *Rp, *Rj, *Rk;         // A by rows: pointers [m + 1], column, CSC slot
  const int *Ap, *Ai;              // A by columns
  const int *Fp, *Fi, *Fk;         // full symmetric P by columns: pointers [n + 1], row, triu slot
  const int *longR, *longC;        // the rows of A / the columns (either pattern) with more than VER_LONG entries, ascending
  const double *Px, *Ax, *q, *l, *u;
  const double *x, *y, *dx, *dy;   // the point and the certificates
  double *dyp;                     // [m] dy projected on the polar of the recession cone of [l, u]
  double *part;                    // [grid][VP_N] partial records
  double *mid;                     // [VM_N]
  double *V;                       // [VER_SLOTS]
  double eps_abs, eps_rel, eps_pinf, eps_dinf;
};

__host__ __device__ __forceinline__ int ver_grid(long long n, long long m) {
  const long long w = ((n > m ? n : m) + VER_ROWS - 1) / VER_ROWS;
  return (int)(w < 1 ? 1 : (w > VER_GRID_CAP ? VER_GRID_CAP : w));
}
static __device__ __forceinline__ bool ver_nan(double v) { return v != v || v == OSQP_NAN; }

// the sum of v over the workgroup, the same bits in every thread: the lanes by the butterfly, then the wavefronts in order
static __device__ __forceinline__ double ver_block_sum(double v, double *lds) {
  v = sens_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = lds[0];
#pragma unroll
  for (int w = 1; w < VER_ROWS; ++w) s += lds[w];
  return s;
}

// the wavefronts' records (the same in all lanes of each) into one, in order; NMAX maxima, then sums
template <int NMAX, int N>
static __device__ __forceinline__ void ver_emit(const double *acc, double *lds, double *out) {
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) lds[(threadIdx.x >> 6) * N + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    double v = lds[k];
    for (int w = 1; w < VER_ROWS; ++w) v = k < NMAX ? fmax(v, lds[w * N + k]) : v + lds[w * N + k];
    out[k] = v;
  }
}

// row i of A with a = (A x)_i; `store`: this lane writes the projected dy_i
static __device__ __forceinline__ void ver_row(const VerCtx &c, int i, double a, double *acc, bool store) {
  const double li = c.l[i], ui = c.u[i], yi = c.y[i], z = fmin(fmax(a, li), ui);
  if (ver_nan(yi)) acc[VP_NAN] = 1.0;
  acc[VP_PRI] = fmax(acc[VP_PRI], fabs(a - z)); acc[VP_AX] = fmax(acc[VP_AX], fabs(a)); acc[VP_Z] = fmax(acc[VP_Z], fabs(z));
  const double yp = fmax(yi, 0.0), ym = fmax(-yi, 0.0);
  if (yp != 0.0) {
    if (ui > VER_BINF) acc[VP_INF] = 1.0;
    else { acc[VP_COMP] = fmax(acc[VP_COMP], yp * (ui - z)); acc[VP_SUP] += ui * yp; }
  }
  if (ym != 0.0) {
    if (li < -VER_BINF) acc[VP_INF] = 1.0;
    else { acc[VP_COMP] = fmax(acc[VP_COMP], ym * (z - li)); acc[VP_SUP] -= li * ym; }
  }
  double d = c.dy[i];
  if (ver_nan(d)) acc[VP_NANDY] = 1.0;
  if (ui > VER_BINF) d = li < -VER_BINF ? 0.0 : fmin(d, 0.0);
  else if (li < -VER_BINF) d = fmax(d, 0.0);
  if (store) c.dyp[i] = d;
  acc[VP_NDY] = fmax(acc[VP_NDY], fabs(d));
  acc[VP_INEQ] += ui * fmax(d, 0.0) + li * fmin(d, 0.0);
}

// column j with px = (P x)_j and aty = (A'y)_j
static __device__ __forceinline__ void ver_col(const VerCtx &c, int j, double px, double aty, double *acc) {
  const double qj = c.q[j], xj = c.x[j], dj = c.dx[j];
  if (ver_nan(xj)) acc[VP_NAN] = 1.0;
  if (ver_nan(dj)) acc[VP_NANDX] = 1.0;
  acc[VP_DUA] = fmax(acc[VP_DUA], fabs((px + qj) + aty));
  acc[VP_PX] = fmax(acc[VP_PX], fabs(px)); acc[VP_ATY] = fmax(acc[VP_ATY], fabs(aty)); acc[VP_Q] = fmax(acc[VP_Q], fabs(qj));
  acc[VP_XPX] += xj * px; acc[VP_QX] += qj * xj;
  acc[VP_NDX] = fmax(acc[VP_NDX], fabs(dj));
  acc[VP_QDX] += qj * dj;
}

__global__ void __launch_bounds__(VER_NT) k_ver_point(VerCtx c) {
  __shared__ double lds[VER_ROWS * VP_N];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, tid = threadIdx.x;
  const long long nw = (long long)gridDim.x * VER_ROWS, w0 = (long long)blockIdx.x * VER_ROWS + wv;
  double acc[VP_N];
#pragma unroll
  for (int k = 0; k < VP_N; ++k) acc[k] = 0.0;
  for (long long r = w0; r < c.m; r += nw) {
    const int i = (int)r, b = c.Rp[i], e = c.Rp[i + 1];
    if (e - b > VER_LONG) continue;
    double a = 0.0;
    for (int k = b + lane; k < e; k += 64) a += c.Ax[c.Rk[k]] * c.x[c.Rj[k]];
    ver_row(c, i, sens_wave_sum(a), acc, lane == 0);
  }
  for (long long r = w0; r < c.n; r += nw) {
    const int j = (int)r, fb = c.Fp[j], fe = c.Fp[j + 1], ab = c.Ap[j], ae = c.Ap[j + 1];
    if (fe - fb > VER_LONG || ae - ab > VER_LONG) continue;
    double px = 0.0, aty = 0.0;
    for (int k = fb + lane; k < fe; k += 64) px += c.Px[c.Fk[k]] * c.x[c.Fi[k]];
    for (int k = ab + lane; k < ae; k += 64) aty += c.Ax[k] * c.y[c.Ai[k]];
    ver_col(c, j, sens_wave_sum(px), sens_wave_sum(aty), acc);
  }
  for (int t = blockIdx.x; t < c.nlongR; t += gridDim.x) {
    const int i = c.longR[t];
    double a = 0.0;
    for (int k = c.Rp[i] + tid; k < c.Rp[i + 1]; k += VER_NT) a += c.Ax[c.Rk[k]] * c.x[c.Rj[k]];
    a = ver_block_sum(a, lds);
    if (wv == 0) ver_row(c, i, a, acc, lane == 0);
  }
  for (int t = blockIdx.x; t < c.nlongC; t += gridDim.x) {
    const int j = c.longC[t];
    double px = 0.0, aty = 0.0;
    for (int k = c.Fp[j] + tid; k < c.Fp[j + 1]; k += VER_NT) px += c.Px[c.Fk[k]] * c.x[c.Fi[k]];
    for (int k = c.Ap[j] + tid; k < c.Ap[j + 1]; k += VER_NT) aty += c.Ax[k] * c.y[c.Ai[k]];
    px = ver_block_sum(px, lds); aty = ver_block_sum(aty, lds);
    if (wv == 0) ver_col(c, j, px, aty, acc);
  }
  ver_emit<VP_NMAX, VP_N>(acc, lds, c.part + (size_t)blockIdx.x * VP_N);
}

__global__ void __launch_bounds__(VER_NT) k_ver_cert(VerCtx c) {
  __shared__ double lds[VER_ROWS * VC_N];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, tid = threadIdx.x;
  const long long nw = (long long)gridDim.x * VER_ROWS, w0 = (long long)blockIdx.x * VER_ROWS + wv;
  const double thr = c.eps_dinf * c.mid[VM_NDX];
  double acc[VC_N] = {0.0, 0.0, 0.0};
  auto row = [&](int i, double adx) {
    if ((c.u[i] < VER_BINF && adx > thr) || (c.l[i] > -VER_BINF && adx < -thr)) acc[VC_VIOL] = 1.0;
  };
  auto col = [&](double atdy, double pdx) {
    acc[VC_NATDY] = fmax(acc[VC_NATDY], fabs(atdy)); acc[VC_NPDX] = fmax(acc[VC_NPDX], fabs(pdx));
  };
  for (long long r = w0; r < c.m; r += nw) {
    const int i = (int)r, b = c.Rp[i], e = c.Rp[i + 1];
    if (e - b > VER_LONG) continue;
    double a = 0.0;
    for (int k = b + lane; k < e; k += 64) a += c.Ax[c.Rk[k]] * c.dx[c.Rj[k]];
    row(i, sens_wave_sum(a));
  }
  for (long long r = w0; r < c.n; r += nw) {
    const int j = (int)r, fb = c.Fp[j], fe = c.Fp[j + 1], ab = c.Ap[j], ae = c.Ap[j + 1];
    if (fe - fb > VER_LONG || ae - ab > VER_LONG) continue;
    double pdx = 0.0, atdy = 0.0;
    for (int k = ab + lane; k < ae; k += 64) atdy += c.Ax[k] * c.dyp[c.Ai[k]];
    for (int k = fb + lane; k < fe; k += 64) pdx += c.Px[c.Fk[k]] * c.dx[c.Fi[k]];
    col(sens_wave_sum(atdy), sens_wave_sum(pdx));
  }
  for (int t = blockIdx.x; t < c.nlongR; t += gridDim.x) {
    const int i = c.longR[t];
    double a = 0.0;
    for (int k = c.Rp[i] + tid; k < c.Rp[i + 1]; k += VER_NT) a += c.Ax[c.Rk[k]] * c.dx[c.Rj[k]];
    a = ver_block_sum(a, lds);
    if (wv == 0) row(i, a);
  }
  for (int t = blockIdx.x; t < c.nlongC; t += gridDim.x) {
    const int j = c.longC[t];
    double pdx = 0.0, atdy = 0.0;
    for (int k = c.Ap[j] + tid; k < c.Ap[j + 1]; k += VER_NT) atdy += c.Ax[k] * c.dyp[c.Ai[k]];
    for (int k = c.Fp[j] + tid; k < c.Fp[j + 1]; k += VER_NT) pdx += c.Px[c.Fk[k]] * c.dx[c.Fi[k]];
    atdy = ver_block_sum(atdy, lds); pdx = ver_block_sum(pdx, lds);
    if (wv == 0) col(atdy, pdx);
  }
  ver_emit<VC_N, VC_N>(acc, lds, c.part + (size_t)blockIdx.x * VC_N);
}

// <<<1, 64>>>: lane k folds slot k of parts partial records, first to last
template <int STAGE>
__global__ void __launch_bounds__(64) k_ver_combine(VerCtx c, int parts) {
  constexpr int N = STAGE == 0 ? VP_N : VC_N, NMAX = STAGE == 0 ? VP_NMAX : VC_N;
  __shared__ double r[N];
  const int k = threadIdx.x;
  if (k < N) {
    double v = 0.0;
#pragma unroll 8
    for (int p = 0; p < parts; ++p) { const double t = c.part[(size_t)p * N + k]; v = k < NMAX ? fmax(v, t) : v + t; }
    r[k] = v;
  }
  __syncthreads();
  if (k != 0) return;
  if (STAGE == 0) {
    const bool inf = r[VP_INF] != 0.0, nan = r[VP_NAN] != 0.0;
    const double obj = 0.5 * r[VP_XPX] + r[VP_QX], dobj = inf ? -OSQP_INFTY : -0.5 * r[VP_XPX] - r[VP_SUP];
    const double eps_pri = c.eps_abs + c.eps_rel * fmax(r[VP_AX], r[VP_Z]);
    const double eps_dua = c.eps_abs + c.eps_rel * fmax(fmax(r[VP_PX], r[VP_ATY]), r[VP_Q]);
    const double rec[14] = {obj, r[VP_PRI], r[VP_DUA], r[VP_AX], r[VP_Z], r[VP_PX], r[VP_ATY], r[VP_Q], eps_pri, eps_dua,
                            inf ? OSQP_INFTY : r[VP_COMP], dobj, inf ? OSQP_INFTY : obj - dobj,
                            (r[VP_PRI] < eps_pri && r[VP_DUA] < eps_dua) ? 1.0 : 0.0};
    for (int s = 0; s < 13; ++s) c.V[s] = nan ? OSQP_NAN : rec[s];
    c.V[13] = nan ? 0.0 : rec[13];
    c.mid[VM_NDY] = r[VP_NDY]; c.mid[VM_NDX] = r[VP_NDX]; c.mid[VM_INEQ] = r[VP_INEQ]; c.mid[VM_QDX] = r[VP_QDX];
    c.mid[VM_NANDY] = r[VP_NANDY]; c.mid[VM_NANDX] = r[VP_NANDX];
  } else {
    const double ndy = c.mid[VM_NDY], ndx = c.mid[VM_NDX], ineq = c.mid[VM_INEQ], qdx = c.mid[VM_QDX];
    const bool nandy = c.mid[VM_NANDY] != 0.0, nandx = c.mid[VM_NANDX] != 0.0;
    c.V[14] = (!nandy && ndy > OSQP_DIVISION_TOL && ineq < c.eps_pinf * ndy && r[VC_NATDY] < c.eps_pinf * ndy) ? 1.0 : 0.0;
    c.V[15] = (!nandx && ndx > OSQP_DIVISION_TOL && qdx < c.eps_dinf * ndx && r[VC_NPDX] < c.eps_dinf * ndx &&
               r[VC_VIOL] == 0.0) ? 1.0 : 0.0;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct hipver {
  int device = 0, grid = 1;
  VerCtx c{};
  std::vector<void *> allocs;
  double *Px = nullptr, *Ax = nullptr, *q = nullptr, *l = nullptr, *u = nullptr, *pt = nullptr;
  size_t nnzP = 0, nnzA = 0;
  std::vector<double> stage;       // host side of pt: x, y, dx, dy in one copy
  c_int uploads[3] = {0, 0, 0};    // of P values, of A values, of q / l / u (each vector counts one)
};

// HIPENG_ERR_ALLOC when the device has no room, HIPENG_ERR_HIP for any other failure
template <typename T>
static int ver_alloc(hipver *v, T **p, size_t count) {
  void *q = nullptr;
  const hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return HIPENG_ERR_ALLOC;
    fprintf(stderr, "osqp_amd: HIP error %s at %s:%d (hipMalloc)\n", hipGetErrorString(e), __FILE__, __LINE__);
    return HIPENG_ERR_HIP;
  }
  v->allocs.push_back(q);
  *p = static_cast<T *>(q);
  return 0;
}
static int ver_put_new(hipver *v, const int **dst, const std::vector<int> &h) {
  int *p = nullptr;
  if (int rc = ver_alloc(v, &p, h.size())) return rc;
  if (!h.empty()) HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
  *dst = p;
  return 0;
}

static int ver_build(hipver *v, const csc *P, const csc *A) {
  const int n = v->c.n, m = v->c.m;
  const size_t nnzP = v->nnzP, nnzA = v->nnzA;
  // the CSC arrays are read as given: a pattern that is not one would send a kernel out of its arrays
  if (P->p[0] != 0 || A->p[0] != 0) return HIPENG_ERR_ARG;
  for (int j = 0; j < n; j++) {
    if (P->p[j + 1] < P->p[j] || A->p[j + 1] < A->p[j]) return HIPENG_ERR_ARG;
    for (c_int k = P->p[j]; k < P->p[j + 1]; k++) if (P->i[k] < 0 || P->i[k] > j) return HIPENG_ERR_ARG;
    for (c_int k = A->p[j]; k < A->p[j + 1]; k++) if (A->i[k] < 0 || A->i[k] >= m) return HIPENG_ERR_ARG;
  }
  // the three maps, as sens_build_maps makes them: full symmetric P by columns (the upper part of column j is triu's column j, the lower
  // part its row j), A by columns, A by rows with the CSC slot of every entry
  std::vector<int> Fp((size_t)n + 1, 0), Fi, Fk, Ap((size_t)n + 1), Ai(nnzA), Rp((size_t)m + 1, 0), Rj(nnzA), Rk(nnzA), longR, longC;
  for (int j = 0; j < n; j++)
    for (c_int k = P->p[j]; k < P->p[j + 1]; k++) { Fp[(size_t)j + 1]++; if (P->i[k] != j) Fp[(size_t)P->i[k] + 1]++; }
  for (int j = 0; j < n; j++) Fp[(size_t)j + 1] += Fp[(size_t)j];
  Fi.resize((size_t)Fp[(size_t)n]); Fk.resize((size_t)Fp[(size_t)n]);
  {
    std::vector<int> pos(Fp.begin(), Fp.end() - 1);
    for (int j = 0; j < n; j++)
      for (c_int k = P->p[j]; k < P->p[j + 1]; k++) { const int q = pos[(size_t)j]++; Fi[(size_t)q] = (int)P->i[k]; Fk[(size_t)q] = (int)k; }
    for (int j = 0; j < n; j++)
      for (c_int k = P->p[j]; k < P->p[j + 1]; k++)
        if (P->i[k] != j) { const int q = pos[(size_t)P->i[k]]++; Fi[(size_t)q] = j; Fk[(size_t)q] = (int)k; }
  }
  for (int j = 0; j <= n; j++) Ap[(size_t)j] = (int)A->p[j];
  for (size_t k = 0; k < nnzA; k++) { Ai[k] = (int)A->i[k]; Rp[(size_t)A->i[k] + 1]++; }
  for (int i = 0; i < m; i++) Rp[(size_t)i + 1] += Rp[(size_t)i];
  {
    std::vector<int> pos(Rp.begin(), Rp.end() - 1);
    for (int j = 0; j < n; j++)
      for (c_int k = A->p[j]; k < A->p[j + 1]; k++) { const int q = pos[(size_t)A->i[k]]++; Rj[(size_t)q] = j; Rk[(size_t)q] = (int)k; }
  }
  for (int i = 0; i < m; i++) if (Rp[(size_t)i + 1] - Rp[(size_t)i] > VER_LONG) longR.push_back(i);
  for (int j = 0; j < n; j++)
    if (Fp[(size_t)j + 1] - Fp[(size_t)j] > VER_LONG || Ap[(size_t)j + 1] - Ap[(size_t)j] > VER_LONG) longC.push_back(j);
  v->c.nlongR = (int)longR.size(); v->c.nlongC = (int)longC.size();
  int rc;
  if ((rc = ver_put_new(v, &v->c.Fp, Fp)) || (rc = ver_put_new(v, &v->c.Fi, Fi)) || (rc = ver_put_new(v, &v->c.Fk, Fk)) ||
      (rc = ver_put_new(v, &v->c.Ap, Ap)) || (rc = ver_put_new(v, &v->c.Ai, Ai)) || (rc = ver_put_new(v, &v->c.Rp, Rp)) ||
      (rc = ver_put_new(v, &v->c.Rj, Rj)) || (rc = ver_put_new(v, &v->c.Rk, Rk)) || (rc = ver_put_new(v, &v->c.longR, longR)) ||
      (rc = ver_put_new(v, &v->c.longC, longC))) return rc;
  const size_t N = (size_t)n, M = (size_t)m;
  if ((rc = ver_alloc(v, &v->Px, nnzP)) || (rc = ver_alloc(v, &v->Ax, nnzA)) || (rc = ver_alloc(v, &v->q, N)) ||
      (rc = ver_alloc(v, &v->l, M)) || (rc = ver_alloc(v, &v->u, M)) || (rc = ver_alloc(v, &v->pt, 2 * (N + M))) ||
      (rc = ver_alloc(v, &v->c.dyp, M)) || (rc = ver_alloc(v, &v->c.part, (size_t)v->grid * VP_N)) ||
      (rc = ver_alloc(v, &v->c.mid, (size_t)VM_N)) || (rc = ver_alloc(v, &v->c.V, (size_t)VER_SLOTS))) return rc;
  v->stage.resize(2 * (N + M));
  v->c.Px = v->Px; v->c.Ax = v->Ax; v->c.q = v->q; v->c.l = v->l; v->c.u = v->u;
  v->c.x = v->pt; v->c.y = v->pt + N; v->c.dx = v->pt + N + M; v->c.dy = v->pt + 2 * N + M;
  return 0;
}

// P (upper triangle), A: the patterns in the caller's CSC order; their values are not read
extern "C" int hipver_create(hipver **out, const csc *P, const csc *A, int device) {
  if (!out || !P || !A || P->n <= 0 || A->n != P->n || P->m != P->n || A->m < 0 || P->n > 0x7ffffff0LL || A->m > 0x7ffffff0LL ||
      2 * P->p[P->n] + A->p[A->n] > 0x7ffffff0LL) return HIPENG_ERR_ARG;
  *out = nullptr;
  hipver *v = new (std::nothrow) hipver();
  if (!v) return HIPENG_ERR_ALLOC;
  *out = v;                      // (a failed create is destroyed by the caller like a whole one)
  v->device = device;
  v->c.n = (int)P->n; v->c.m = (int)A->m; v->nnzP = (size_t)P->p[P->n]; v->nnzA = (size_t)A->p[A->n];
  v->grid = ver_grid(P->n, A->m);
  HIPCHK(hipSetDevice(device));
  try {
    return ver_build(v, P, A);
  } catch (const std::bad_alloc &) {
    return HIPENG_ERR_ALLOC;
  }
}

extern "C" void hipver_destroy(hipver *v) {
  if (!v) return;
  (void)hipSetDevice(v->device);   // (every call synchronises its stream before it returns: nothing is in flight)
  for (void *p : v->allocs) (void)hipFree(p);
  delete v;
}

// parts: bit 0 Px, 1 Ax, 2 q, 3 l, 4 u -- the raw values to copy to the device, on the stream of `e`
extern "C" int hipver_upload(hipver *v, hipeng *e, int parts, const c_float *Px, const c_float *Ax, const c_float *q, const c_float *l,
                             const c_float *u) {
  if (!v || !e) return HIPENG_ERR_ARG;
  const c_float *src[5] = {Px, Ax, q, l, u};
  double *dst[5] = {v->Px, v->Ax, v->q, v->l, v->u};
  const size_t len[5] = {v->nnzP, v->nnzA, (size_t)v->c.n, (size_t)v->c.m, (size_t)v->c.m};
  for (int k = 0; k < 5; k++) if ((parts >> k & 1) && !src[k] && len[k]) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(v->device));
  for (int k = 0; k < 5; k++) {
    if (!(parts >> k & 1)) continue;
    if (len[k]) HIPCHK(hipMemcpyAsync(dst[k], src[k], len[k] * sizeof(double), hipMemcpyHostToDevice, e->stream));
    v->uploads[k < 2 ? k : 2]++;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// the record of (x, y, dx, dy) -- host arrays, none NULL where its length is not 0 -- into V [16]; returns with the stream synchronised
extern "C" int hipver_run(hipver *v, hipeng *e, const c_float *x, const c_float *y, const c_float *dx, const c_float *dy, c_float eps_abs,
                          c_float eps_rel, c_float eps_pinf, c_float eps_dinf, c_float *V) {
  if (!v || !e || !V || !x || !dx || (v->c.m > 0 && (!y || !dy))) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(v->device));
  hipStream_t st = e->stream;
  const size_t n = (size_t)v->c.n, m = (size_t)v->c.m;
  double *h = v->stage.data();
  memcpy(h, x, n * sizeof(double)); memcpy(h + n + m, dx, n * sizeof(double));
  if (m) { memcpy(h + n, y, m * sizeof(double)); memcpy(h + 2 * n + m, dy, m * sizeof(double)); }
  HIPCHK(hipMemcpyAsync(v->pt, h, 2 * (n + m) * sizeof(double), hipMemcpyHostToDevice, st));
  VerCtx c = v->c;
  c.eps_abs = eps_abs; c.eps_rel = eps_rel; c.eps_pinf = eps_pinf; c.eps_dinf = eps_dinf;
  hipLaunchKernelGGL(k_ver_point, dim3(v->grid), dim3(VER_NT), 0, st, c);
  hipLaunchKernelGGL(k_ver_combine<0>, dim3(1), dim3(64), 0, st, c, v->grid);
  hipLaunchKernelGGL(k_ver_cert, dim3(v->grid), dim3(VER_NT), 0, st, c);
  hipLaunchKernelGGL(k_ver_combine<1>, dim3(1), dim3(64), 0, st, c, v->grid);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(V, v->c.V, VER_SLOTS * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// the kernels' constants: threads, rows per workgroup per sweep, grid cap, long-row threshold (needs no device)
extern "C" int hipver_info(int out[4]) {
  if (!out) return HIPENG_ERR_ARG;
  out[0] = VER_NT; out[1] = VER_ROWS; out[2] = VER_GRID_CAP; out[3] = VER_LONG;
  return 0;
}

// uploads since create: of P values, of A values, of q / l / u (each vector counts one)
extern "C" int hipver_uploads(const hipver *v, c_int out[3]) {
  if (!v || !out) return HIPENG_ERR_ARG;
  for (int k = 0; k < 3; k++) out[k] = v->uploads[k];
  return 0;
}
