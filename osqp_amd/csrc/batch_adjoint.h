// batch_adjoint.h -- adjoint derivatives of the solution for the solved members of a batch, included by batch.hip
// after batch_polish.h.  Given gx = dl/dx and gy = dl/dy of a scalar l, it returns dl/dq, dl/dl, dl/du and, on
// request, dl/dPx and dl/dAx on the shared pattern.
//
// Per member, with the active rows (lows first, then upps, as k_bp_active orders them), Ar those rows of A, nu = y
// on them: locally M [x; nu] = [-q; b_active] with M = [P, Ar'; Ar, 0], so with M [rx; rnu] = [gx; gy_active]
//   dl/dq = -rx,   dl/dl_i (dl/du_i) = rnu_a at a row active at its lower (upper) bound, 0 elsewhere,
//   dl/dA_ij = -(nu_i rx_j + rnu_i x_j) on active rows, 0 elsewhere,
//   dl/dP_ii = -rx_i x_i,   dl/dP_ij = -(rx_i x_j + rx_j x_i) for a stored off-diagonal slot of triu(P).
// The handle holds the scaled problem (P~ = c D P D, A~ = E A D, q~ = c D q, x = D x~, y = E y~ / c), so the solve
// runs in that space like polish: right-hand side [D gx; E gy / c], then dq = -c D rx~, dl_i = E_i rnu~_a,
// dA_ij = E_i D_j (.), dP_ij = c D_i D_j (.), with D, E, c as constants (the unscaled solution does not depend on
// them).
//
// The route is polish's: k_bp_active, k_bp_form and k_bp_invert as they are (the delta-regularised matrix, inverted
// in place), on the polish buffers with a status array of its own, then
//   k_ba_adjoint  one workgroup per member: the right-hand side, polish's solve (kkt_solve_refined: the explicit
//                 inverse, then exactly polish_refine_iter refinement steps against the unregularised M), and the
//                 unscaled outputs.
//   k_ba_adjoint_multi  grid (members of the chunk, ncot): k_ba_adjoint for ncot cotangents per member that share
//                 the one inversion, one workgroup per member and cotangent, the shape of k_bt_tangent's launch.  The
//                 same expressions in the same order: cotangent d of a member carries the bits k_ba_adjoint gives for
//                 (dX[:, d], dY[:, d]), whatever ncot, the other cotangents and the chunking are.
// Nothing of the handle's solve state is written: X, Y, info, the stored
// iterates, rho, K^-1, flags and polish's status stay bit-equal.  Every output element has one owner: no atomics.

struct BAdj {              // staging of a handle's adjoint call (device pointers)
  const double *gx, *gy;   // [B][n] dl/dx, [B][m] dl/dy (null = 0)
  double *dQ, *dL, *dU;    // [B][n], [B][m], [B][m]
  double *dPx, *dAx;       // [B][nnzP], [B][nnzA]; null = not requested
  int *active;             // [B][m] -1 active at the lower bound, +1 at the upper, 0 inactive
};

// LDS of k_ba_adjoint: four vectors of NPOL (solution, residual, correction, right-hand side), x and D, E and y,
// and the two row maps.
__host__ __device__ __forceinline__ size_t ba_lds_bytes(int n, int m, int NPOL) {
  const size_t b = sizeof(double) * (4 * (size_t)NPOL + 2 * (size_t)n + 2 * (size_t)m) + sizeof(int) * 2 * (size_t)m;
  return (b + 15) & ~(size_t)15;
}

// pl.stat is the adjoint's status here (1 computed, -1 pivot of the wrong sign, 0 not tried), not polish's.
__global__ void __launch_bounds__(BP_NT) k_ba_adjoint(BPattern p, BIO io, BPol pl, BAdj ad, int NPOL, int refine_iter,
                                                      const int *list) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const long long qp = list[blockIdx.x];
  if (pl.stat[qp] == -1) return;                 // the inversion met a pivot of the wrong sign: the outputs stay 0
  const int n = p.n, m = p.m, tid = threadIdx.x;
  const int mred = pl.mred[qp], nlow = pl.nlow[qp], N = n + mred;
  const double *Kinv = pl.K + (long long)blockIdx.x * NPOL * NPOL;
  double *sol = lds, *res = sol + NPOL, *cor = res + NPOL, *g = cor + NPOL;
  double *x = g + NPOL, *D = x + n, *E = D + n, *y = E + m;
  int *map = reinterpret_cast<int *>(y + m), *rows = map + m;
  BL s;
  slab_view(s, p, io, qp);
  const double cs = io.Wc[qp], cinv = 1.0 / cs;
  for (int j = tid; j < n; j += BP_NT) { x[j] = io.Xs[qp * n + j]; D[j] = io.Wd[qp * n + j]; }
  for (int i = tid; i < m; i += BP_NT) { E[i] = io.We[qp * m + i]; y[i] = io.Ys[qp * m + i]; }
  load_row_maps(pl, qp, m, mred, map, rows);
  __syncthreads();
  // rhs = [D gx; E gy / c on the active rows], zero in the padding
  for (int k = tid; k < NPOL; k += BP_NT) {
    double v = 0.0;
    if (k < n) v = D[k] * ad.gx[qp * n + k];
    else if (k < N && ad.gy) { const int r = rows[k - n]; v = (E[r] * ad.gy[qp * m + r]) * cinv; }
    g[k] = v;
  }
  __syncthreads();
  kkt_solve_refined(s, Kinv, NPOL, n, N, map, rows, refine_iter, [g](int k) { return g[k]; }, sol, res, cor);
  // sol = [rx; rnu] of the scaled problem; the unscaled gradients
  for (int j = tid; j < n; j += BP_NT) ad.dQ[qp * n + j] = 0.0 - (cs * D[j]) * sol[j];
  for (int i = tid; i < m; i += BP_NT) {
    const int a = map[i];
    const double v = a >= 0 ? E[i] * sol[n + a] : 0.0;
    ad.dL[qp * m + i] = (a >= 0 && a < nlow) ? v : 0.0;
    ad.dU[qp * m + i] = a >= nlow ? v : 0.0;
    if (ad.active) ad.active[qp * m + i] = a < 0 ? 0 : (a < nlow ? -1 : 1);
  }
  if (ad.dAx)
    for (int k = tid; k < p.nnzA; k += BP_NT) {
      const int i = s.Ai[k], j = s.Ac[k], a = map[i];
      ad.dAx[qp * p.nnzA + k] = a >= 0 ? 0.0 - (E[i] * D[j]) * (y[i] * sol[j] + sol[n + a] * x[j]) : 0.0;
    }
  if (ad.dPx)
    for (int k = tid; k < p.nnzP; k += BP_NT) {
      const int i = s.Pi[k], j = s.Pc[k];
      const double w = i == j ? sol[i] * x[i] : sol[i] * x[j] + sol[j] * x[i];
      ad.dPx[qp * p.nnzP + k] = 0.0 - ((cs * D[i]) * D[j]) * w;
    }
  if (tid == 0) pl.stat[qp] = 1;
}

struct BAdjM {             // staging of a handle's adjoint_multi call (device pointers)
  const double *gx, *gy;   // [B][ncot][n] dl/dx, [B][ncot][m] dl/dy (null = 0)
  double *dQ, *dL, *dU;    // [B][ncot][n], [B][ncot][m], [B][ncot][m]
  double *dPx, *dAx;       // [B][ncot][nnzP], [B][ncot][nnzA]; null = not requested
  int *active;             // [B][m] -1 active at the lower bound, +1 at the upper, 0 inactive
  int *stat;               // [B] status_adjoint: 1 computed, -1 pivot of the wrong sign, 0 not tried
  int ncot;
};

// pl.stat is the pivot verdict of the inversion (0, or -1 from k_bp_invert) and is only read here, as in k_bt_tangent;
// the status the caller sees is ad.stat, which cotangent 0 of a member alone writes (with `active`): the cotangents
// of a member neither read what another writes nor write the same word.  LDS: ba_lds_bytes.
__global__ void __launch_bounds__(BP_NT) k_ba_adjoint_multi(BPattern p, BIO io, BPol pl, BAdjM ad, int NPOL, int refine_iter,
                                                            const int *list) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const long long qp = list[blockIdx.x];
  const int tid = threadIdx.x;
  if (pl.stat[qp] == -1) {                       // the inversion met a pivot of the wrong sign: the outputs stay 0
    if (blockIdx.y == 0 && tid == 0) ad.stat[qp] = -1;
    return;
  }
  const int n = p.n, m = p.m;
  const int mred = pl.mred[qp], nlow = pl.nlow[qp], N = n + mred;
  const long long slot = qp * ad.ncot + blockIdx.y;       // this workgroup's (member, cotangent)
  const double *Kinv = pl.K + (long long)blockIdx.x * NPOL * NPOL;
  double *sol = lds, *res = sol + NPOL, *cor = res + NPOL, *g = cor + NPOL;
  double *x = g + NPOL, *D = x + n, *E = D + n, *y = E + m;
  int *map = reinterpret_cast<int *>(y + m), *rows = map + m;
  BL s;
  slab_view(s, p, io, qp);
  const double cs = io.Wc[qp], cinv = 1.0 / cs;
  for (int j = tid; j < n; j += BP_NT) { x[j] = io.Xs[qp * n + j]; D[j] = io.Wd[qp * n + j]; }
  for (int i = tid; i < m; i += BP_NT) { E[i] = io.We[qp * m + i]; y[i] = io.Ys[qp * m + i]; }
  load_row_maps(pl, qp, m, mred, map, rows);
  __syncthreads();
  const double *gx = ad.gx + slot * n, *gy = ad.gy ? ad.gy + slot * m : nullptr;
  // rhs = [D gx; E gy / c on the active rows], zero in the padding
  for (int k = tid; k < NPOL; k += BP_NT) {
    double v = 0.0;
    if (k < n) v = D[k] * gx[k];
    else if (k < N && gy) { const int r = rows[k - n]; v = (E[r] * gy[r]) * cinv; }
    g[k] = v;
  }
  __syncthreads();
  kkt_solve_refined(s, Kinv, NPOL, n, N, map, rows, refine_iter, [g](int k) { return g[k]; }, sol, res, cor);
  // sol = [rx; rnu] of the scaled problem; the unscaled gradients into this cotangent's slices
  for (int j = tid; j < n; j += BP_NT) ad.dQ[slot * n + j] = 0.0 - (cs * D[j]) * sol[j];
  for (int i = tid; i < m; i += BP_NT) {
    const int a = map[i];
    const double v = a >= 0 ? E[i] * sol[n + a] : 0.0;
    ad.dL[slot * m + i] = (a >= 0 && a < nlow) ? v : 0.0;
    ad.dU[slot * m + i] = a >= nlow ? v : 0.0;
    if (blockIdx.y == 0) ad.active[qp * m + i] = a < 0 ? 0 : (a < nlow ? -1 : 1);
  }
  if (ad.dAx)
    for (int k = tid; k < p.nnzA; k += BP_NT) {
      const int i = s.Ai[k], j = s.Ac[k], a = map[i];
      ad.dAx[slot * p.nnzA + k] = a >= 0 ? 0.0 - (E[i] * D[j]) * (y[i] * sol[j] + sol[n + a] * x[j]) : 0.0;
    }
  if (ad.dPx)
    for (int k = tid; k < p.nnzP; k += BP_NT) {
      const int i = s.Pi[k], j = s.Pc[k];
      const double w = i == j ? sol[i] * x[i] : sol[i] * x[j] + sol[j] * x[i];
      ad.dPx[slot * p.nnzP + k] = 0.0 - ((cs * D[i]) * D[j]) * w;
    }
  if (blockIdx.y == 0 && tid == 0) ad.stat[qp] = 1;
}
