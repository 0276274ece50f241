// kkt_sens.h -- the O(nnz) parts of the single-QP engine's solution derivatives (osqp_amd_adjoint / osqp_amd_tangent in
// osqp_host.c), included by engine.hip.  The KKT solves themselves are polish's (a polish-mode plugin instance and the
// refinement loop of osqp_host.c); what runs here, on that instance's stream, is the work on the patterns of P and A:
//   k_sens_grad      dPx[k], dAx[k] of the adjoint: one owner per CSC slot of triu(P) / A, coalesced stores, no atomics;
//   k_sens_tan_rhs   the tangent's right-hand side -(dq~ + dP~ x~ + dA~' y~_act) and db~_act - (dA~ x~)_act, ndir directions
//                    per launch: one wavefront per column (first n) or row of A (next m), lanes stride its entries, a
//                    fixed-order butterfly sums them.
// Formulas, scaling rules and sign conventions are batch_adjoint.h's and batch_tangent.h's for one member: the solve runs in the
// scaled space (P~ = c D P D, A~ = E A D, q~ = c D q, x = D x~, y = E y~ / c) with D, E, c as constants.
// A hipsens belongs to one workspace and lives until its cleanup: the point (x~, y~_act, act, D, E, c) is uploaded once per KKT
// instance, the int32 (row, col) arrays at the first call that asks for matrix gradients, the three maps of the tangent at the
// first tangent call.  The maps are BPattern's (batch.hip): the full symmetric P by columns with the triu slot of every entry,
// A by columns, A by rows with the CSC slot of every entry.

struct SensCtx {
  int n, m, nnzP, nnzA;
  const double *x, *yact, *D, *E;   // x~ [n], y~ on the active rows and 0 elsewhere [m], D [n], E [m]
  const int *act;                   // [m] -1 active at the lower bound, +1 at the upper, 0 inactive
  double cs;                        // cost scaling c
  const int *Prow, *Pcol, *Arow, *Acol;   // (row, col) of every CSC slot of triu(P) / A
  const int *Fp, *Fi, *Fk;          // full symmetric P by columns: pointers [n + 1], row, triu slot
  const int *Ap;                    // A by columns: pointers [n + 1] (rows are Arow, the slots are the positions)
  const int *Rp, *Rj, *Rk;          // A by rows: pointers [m + 1], column, CSC slot
};

// rx [n], rnu [m] (the multiplier part of the adjoint solve scattered to the rows, 0 on inactive ones)
__global__ void __launch_bounds__(TB) k_sens_grad(SensCtx s, const double *__restrict__ rx, const double *__restrict__ rnu,
                                                  double *__restrict__ dPx, double *__restrict__ dAx) {
  const long long t0 = (long long)blockIdx.x * TB + threadIdx.x, step = (long long)gridDim.x * TB;
  if (dAx)
    for (long long k = t0; k < s.nnzA; k += step) {
      const int i = s.Arow[k], j = s.Acol[k];
      dAx[k] = s.act[i] != 0 ? 0.0 - (s.E[i] * s.D[j]) * (s.yact[i] * rx[j] + rnu[i] * s.x[j]) : 0.0;
    }
  if (dPx)
    for (long long k = t0; k < s.nnzP; k += step) {
      const int i = s.Prow[k], j = s.Pcol[k];
      const double w = i == j ? rx[i] * s.x[i] : rx[i] * s.x[j] + rx[j] * s.x[i];
      dPx[k] = 0.0 - ((s.cs * s.D[i]) * s.D[j]) * w;
    }
}

// the sum of v over the 64 lanes, the same bits in every lane whatever the data: a fixed tree
static __device__ __forceinline__ double sens_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// g [ndir][n + m]; direction blockIdx.y.  A null tangent adds the 0.0 a tangent of zeros adds.
__global__ void __launch_bounds__(TB) k_sens_tan_rhs(SensCtx s, const double *__restrict__ dq, const double *__restrict__ dl,
                                                     const double *__restrict__ du, const double *__restrict__ dPx,
                                                     const double *__restrict__ dAx, double *__restrict__ g) {
  const int lane = threadIdx.x & 63, n = s.n, m = s.m;
  const long long d = blockIdx.y;
  const double *dP = dPx ? dPx + d * s.nnzP : nullptr, *dA = dAx ? dAx + d * s.nnzA : nullptr;
  const long long nw = (long long)gridDim.x * (TB / 64);
  for (long long w = (long long)blockIdx.x * (TB / 64) + (threadIdx.x >> 6); w < (long long)n + m; w += nw) {
    double v;
    if (w < n) {
      const int k = (int)w;
      const double dk = s.D[k];
      double px = 0.0, aty = 0.0;
      if (dP)
        for (int kk = s.Fp[k] + lane; kk < s.Fp[k + 1]; kk += 64) { const int i = s.Fi[kk]; px += (s.D[i] * dP[s.Fk[kk]]) * s.x[i]; }
      if (dA)
        for (int kk = s.Ap[k] + lane; kk < s.Ap[k + 1]; kk += 64) { const int i = s.Arow[kk]; aty += (s.E[i] * dA[kk]) * s.yact[i]; }
      px = sens_wave_sum(px); aty = sens_wave_sum(aty);
      const double qk = dq ? (s.cs * dk) * dq[d * n + k] : 0.0;
      v = 0.0 - ((qk + (s.cs * dk) * px) + dk * aty);
    } else {
      const int r = (int)(w - n), a = s.act[r];
      double ax = 0.0;
      if (dA && a != 0)
        for (int kk = s.Rp[r] + lane; kk < s.Rp[r + 1]; kk += 64) { const int j = s.Rj[kk]; ax += (s.D[j] * dA[s.Rk[kk]]) * s.x[j]; }
      ax = sens_wave_sum(ax);
      const double *db = a < 0 ? dl : du;
      v = a != 0 ? (db ? s.E[r] * db[d * m + r] : 0.0) - s.E[r] * ax : 0.0;
    }
    if (lane == 0) g[d * ((long long)n + m) + w] = v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct hipsens {
  int device = 0;
  SensCtx c{};
  std::vector<void *> allocs;
  double *x = nullptr, *yact = nullptr, *D = nullptr, *E = nullptr, *rx = nullptr, *rnu = nullptr, *oP = nullptr, *oA = nullptr;
  int *act = nullptr;
  bool have_rc = false, have_maps = false;
  double *tin = nullptr, *tout = nullptr;   // staging of a tangent call: the five inputs, then g
  size_t tin_cap = 0, tout_cap = 0;
};

template <typename T>
static int sens_alloc(hipsens *s, T **p, size_t count) {
  void *q = nullptr;
  HIPCHK(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
  s->allocs.push_back(q);
  *p = static_cast<T *>(q);
  return 0;
}
template <typename T>
static int sens_put(hipStream_t st, T *dst, const T *src, size_t count) {
  if (count) HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, st));
  return 0;
}
template <typename T>
static int sens_put_new(hipsens *s, hipStream_t st, const int **dst, const std::vector<T> &v) {
  int *p = nullptr;
  if (sens_alloc(s, &p, v.size()) || sens_put(st, p, v.data(), v.size())) return HIPENG_ERR_HIP;
  *dst = p;
  return 0;
}
static int sens_grid(long long work) { return (int)std::min<long long>(MAX_PARTS, std::max<long long>(1, (work + TB - 1) / TB)); }

extern "C" int hipsens_create(hipsens **out, c_int n, c_int m, c_int nnzP, c_int nnzA, int device) {
  if (!out || n <= 0 || m < 0 || nnzP < 0 || nnzA < 0 || n > 0x7ffffff0LL || m > 0x7ffffff0LL || nnzP + nnzA + nnzP > 0x7ffffff0LL)
    return HIPENG_ERR_ARG;
  *out = nullptr;
  hipsens *s = new (std::nothrow) hipsens();
  if (!s) return HIPENG_ERR_ALLOC;
  s->device = device;
  s->c.n = (int)n; s->c.m = (int)m; s->c.nnzP = (int)nnzP; s->c.nnzA = (int)nnzA; s->c.cs = 1.0;
  *out = s;                      // (a failed create is destroyed by the caller like a whole one)
  HIPCHK(hipSetDevice(device));
  if (sens_alloc(s, &s->x, n) || sens_alloc(s, &s->yact, m) || sens_alloc(s, &s->D, n) || sens_alloc(s, &s->E, m) ||
      sens_alloc(s, &s->act, m) || sens_alloc(s, &s->rx, n) || sens_alloc(s, &s->rnu, m)) return HIPENG_ERR_HIP;
  s->c.x = s->x; s->c.yact = s->yact; s->c.D = s->D; s->c.E = s->E; s->c.act = s->act;
  return 0;
}

extern "C" void hipsens_destroy(hipsens *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);   // (every call synchronises its stream before it returns: nothing is in flight)
  for (void *p : s->allocs) (void)hipFree(p);
  if (s->tin) (void)hipFree(s->tin);
  if (s->tout) (void)hipFree(s->tout);
  delete s;
}

// the point the derivatives are taken at; D, E NULL = ones
extern "C" int hipsens_set_point(hipsens *s, hipeng *pe, const c_float *x, const c_float *yact, const c_int *act,
                                 const c_float *D, const c_float *E, c_float cs) {
  if (!s || !pe || !x || (s->c.m > 0 && (!yact || !act))) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(s->device));
  const size_t n = (size_t)s->c.n, m = (size_t)s->c.m;
  std::vector<double> one(std::max(n, m), 1.0);
  std::vector<int> a32(m);
  for (size_t i = 0; i < m; i++) a32[i] = (int)act[i];
  if (sens_put(pe->stream, s->x, x, n) || sens_put(pe->stream, s->yact, yact, m) || sens_put(pe->stream, s->act, a32.data(), m) ||
      sens_put(pe->stream, s->D, D ? D : one.data(), n) || sens_put(pe->stream, s->E, E ? E : one.data(), m)) return HIPENG_ERR_HIP;
  s->c.cs = cs;
  HIPCHK(hipStreamSynchronize(pe->stream));   // the staging vectors die here
  return 0;
}

// dPx [nnzP] / dAx [nnzA] (either NULL = skip) from rx [n] and rnu [m]; P, A: the patterns, in the caller's CSC order
extern "C" int hipsens_grad(hipsens *s, hipeng *pe, const csc *P, const csc *A, const c_float *rx, const c_float *rnu,
                            c_float *dPx, c_float *dAx) {
  if (!s || !pe || !P || !A || !rx || (s->c.m > 0 && !rnu)) return HIPENG_ERR_ARG;
  if (P->p[P->n] != s->c.nnzP || A->p[A->n] != s->c.nnzA || P->n != s->c.n || A->m != s->c.m) return HIPENG_ERR_ARG;
  if (!dPx && !dAx) return 0;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = pe->stream;
  const int n = s->c.n, m = s->c.m, nnzP = s->c.nnzP, nnzA = s->c.nnzA;
  if (!s->have_rc) {
    std::vector<int> pr((size_t)nnzP), pc((size_t)nnzP), ar((size_t)nnzA), ac((size_t)nnzA);
    for (int j = 0; j < n; j++) {
      for (c_int k = P->p[j]; k < P->p[j + 1]; k++) { pr[(size_t)k] = (int)P->i[k]; pc[(size_t)k] = j; }
      for (c_int k = A->p[j]; k < A->p[j + 1]; k++) { ar[(size_t)k] = (int)A->i[k]; ac[(size_t)k] = j; }
    }
    if (sens_put_new(s, st, &s->c.Prow, pr) || sens_put_new(s, st, &s->c.Pcol, pc) || sens_put_new(s, st, &s->c.Acol, ac)) return HIPENG_ERR_HIP;
    if (!s->c.Arow && sens_put_new(s, st, &s->c.Arow, ar)) return HIPENG_ERR_HIP;
    if (sens_alloc(s, &s->oP, (size_t)nnzP) || sens_alloc(s, &s->oA, (size_t)nnzA)) return HIPENG_ERR_HIP;
    HIPCHK(hipStreamSynchronize(st));
    s->have_rc = true;
  }
  if (sens_put(st, s->rx, rx, (size_t)n) || sens_put(st, s->rnu, rnu, (size_t)m)) return HIPENG_ERR_HIP;
  hipLaunchKernelGGL(k_sens_grad, dim3(sens_grid(std::max(nnzP, nnzA))), dim3(TB), 0, st, s->c, (const double *)s->rx,
                     (const double *)s->rnu, dPx ? s->oP : nullptr, dAx ? s->oA : nullptr);
  HIPCHK(hipGetLastError());
  if (dPx && nnzP) HIPCHK(hipMemcpyAsync(dPx, s->oP, (size_t)nnzP * sizeof(double), hipMemcpyDeviceToHost, st));
  if (dAx && nnzA) HIPCHK(hipMemcpyAsync(dAx, s->oA, (size_t)nnzA * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

static int sens_build_maps(hipsens *s, hipStream_t st, const csc *P, const csc *A) {
  const int n = s->c.n, m = s->c.m, nnzA = s->c.nnzA;
  // full symmetric P by columns, entries of a column in ascending row order: the upper part of column j is triu's column j, the lower part
  // its row j (found in the columns behind j, which are visited in ascending order)
  std::vector<int> Fp((size_t)n + 1, 0), Fi, Fk, Ap((size_t)n + 1), Rp((size_t)m + 1, 0), Rj((size_t)nnzA), Rk((size_t)nnzA), ar((size_t)nnzA);
  for (int j = 0; j < n; j++)
    for (c_int k = P->p[j]; k < P->p[j + 1]; k++) { Fp[(size_t)j + 1]++; if (P->i[k] != j) Fp[(size_t)P->i[k] + 1]++; }
  for (int j = 0; j < n; j++) Fp[(size_t)j + 1] += Fp[(size_t)j];
  Fi.resize((size_t)Fp[(size_t)n]); Fk.resize((size_t)Fp[(size_t)n]);
  {
    std::vector<int> pos(Fp.begin(), Fp.end() - 1);
    for (int j = 0; j < n; j++)          // upper parts (rows <= j), in the order stored
      for (c_int k = P->p[j]; k < P->p[j + 1]; k++) { const int q = pos[(size_t)j]++; Fi[(size_t)q] = (int)P->i[k]; Fk[(size_t)q] = (int)k; }
    for (int j = 0; j < n; j++)          // lower parts: entry (i, j), i < j, is entry (j, i) of column i
      for (c_int k = P->p[j]; k < P->p[j + 1]; k++)
        if (P->i[k] != j) { const int q = pos[(size_t)P->i[k]]++; Fi[(size_t)q] = j; Fk[(size_t)q] = (int)k; }
  }
  for (int j = 0; j <= n; j++) Ap[(size_t)j] = (int)A->p[j];
  for (int k = 0; k < nnzA; k++) { ar[(size_t)k] = (int)A->i[k]; Rp[(size_t)A->i[k] + 1]++; }
  for (int i = 0; i < m; i++) Rp[(size_t)i + 1] += Rp[(size_t)i];
  {
    std::vector<int> pos(Rp.begin(), Rp.end() - 1);
    for (int j = 0; j < n; j++)
      for (c_int k = A->p[j]; k < A->p[j + 1]; k++) { const int q = pos[(size_t)A->i[k]]++; Rj[(size_t)q] = j; Rk[(size_t)q] = (int)k; }
  }
  if (sens_put_new(s, st, &s->c.Fp, Fp) || sens_put_new(s, st, &s->c.Fi, Fi) || sens_put_new(s, st, &s->c.Fk, Fk) ||
      sens_put_new(s, st, &s->c.Ap, Ap) || sens_put_new(s, st, &s->c.Rp, Rp) || sens_put_new(s, st, &s->c.Rj, Rj) ||
      sens_put_new(s, st, &s->c.Rk, Rk)) return HIPENG_ERR_HIP;
  if (!s->c.Arow && sens_put_new(s, st, &s->c.Arow, ar)) return HIPENG_ERR_HIP;
  HIPCHK(hipStreamSynchronize(st));
  s->have_maps = true;
  return 0;
}

// g [ndir][n + m]: the tangent's right-hand side on all rows (0 on the inactive ones); any NULL input = 0
extern "C" int hipsens_tan_rhs(hipsens *s, hipeng *pe, const csc *P, const csc *A, c_int ndir, const c_float *dq, const c_float *dl,
                               const c_float *du, const c_float *dPx, const c_float *dAx, c_float *g) {
  if (!s || !pe || !P || !A || !g || ndir < 1 || ndir > 65535) return HIPENG_ERR_ARG;
  if (P->p[P->n] != s->c.nnzP || A->p[A->n] != s->c.nnzA || P->n != s->c.n || A->m != s->c.m) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = pe->stream;
  if (!s->have_maps) if (int rc = sens_build_maps(s, st, P, A)) return rc;
  const size_t n = (size_t)s->c.n, m = (size_t)s->c.m, nd = (size_t)ndir;
  const size_t len[5] = {nd * n, nd * m, nd * m, nd * (size_t)s->c.nnzP, nd * (size_t)s->c.nnzA};
  const c_float *src[5] = {dq, dl, du, dPx, dAx};
  size_t need = 0;
  for (int k = 0; k < 5; k++) if (src[k]) need += len[k];
  if (need > s->tin_cap) {
    if (s->tin) HIPCHK(hipFree(s->tin));
    s->tin = nullptr; s->tin_cap = 0;
    HIPCHK(hipMalloc((void **)&s->tin, need * sizeof(double)));
    s->tin_cap = need;
  }
  if (nd * (n + m) > s->tout_cap) {
    if (s->tout) HIPCHK(hipFree(s->tout));
    s->tout = nullptr; s->tout_cap = 0;
    HIPCHK(hipMalloc((void **)&s->tout, nd * (n + m) * sizeof(double)));
    s->tout_cap = nd * (n + m);
  }
  const double *dev[5];
  size_t off = 0;
  for (int k = 0; k < 5; k++) {
    dev[k] = nullptr;
    if (!src[k]) continue;
    dev[k] = s->tin + off;
    if (sens_put(st, s->tin + off, src[k], len[k])) return HIPENG_ERR_HIP;
    off += len[k];
  }
  const long long waves = (long long)(n + m);
  const int grid = (int)std::min<long long>(MAX_PARTS, std::max<long long>(1, (waves + TB / 64 - 1) / (TB / 64)));
  hipLaunchKernelGGL(k_sens_tan_rhs, dim3(grid, (unsigned)ndir), dim3(TB), 0, st, s->c, dev[0], dev[1], dev[2], dev[3], dev[4], s->tout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(g, s->tout, nd * (n + m) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
