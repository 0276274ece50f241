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
//   k_ba_adjoint  grid (members of the chunk, ncot): one workgroup per member and cotangent, the shape of
//                 k_bt_tangent's launch, so the ncot cotangents of a member share the one inversion.  The right-hand
//                 side, polish's solve (kkt_solve_refined: the explicit inverse, then exactly polish_refine_iter
//                 refinement steps against the unregularised M), and the unscaled outputs.  Cotangent d of a member
//                 carries the same bits whatever ncot, the other cotangents and the chunking are; the single-cotangent
//                 entry points are the ncot = 1 call.
// Nothing of the handle's solve state is written: X, Y, info, the stored
// iterates, rho, K^-1, flags and polish's status stay bit-equal.  Every output element has one owner: no atomics.

struct BAdj {              // staging of a handle's adjoint call (device pointers)
  const double *gx, *gy;   // [B][ncot][n] dl/dx, [B][ncot][m] dl/dy (null = 0)
  double *dQ, *dL, *dU;    // [B][ncot][n], [B][ncot][m], [B][ncot][m]
  double *dPx, *dAx;       // [B][ncot][nnzP], [B][ncot][nnzA]; null = not requested
  int *active;             // [B][m] -1 active at the lower bound, +1 at the upper, 0 inactive
  int *stat;               // [B] status_adjoint: 1 computed, -1 pivot of the wrong sign, 0 not tried
  int ncot;
};

// Opening, close and LDS as k_bt_tangent (bd_open, bd_close, bd_lds_bytes in batch_polish.h): pl.stat is the pivot
// verdict of the inversion and is only read here; the status the caller sees is ad.stat.
template <class KS, class... KSArg>
__global__ void __launch_bounds__(BP_NT) k_ba_adjoint(BPattern p, BIO io, BPol pl, BAdj ad, int NPOL, int refine_iter,
                                                      const int *list, KSArg... ksarg) {
  const KS ks{ksarg...};
  extern __shared__ __attribute__((aligned(16))) double lds[];
  BDView mv;
  if (!bd_open(p, io, pl, ad.stat, ad.ncot, NPOL, list, lds, ks, mv)) return;
  const int n = mv.n, m = mv.m, N = mv.N, nlow = mv.nlow, tid = threadIdx.x;
  const long long slot = mv.slot;                          // this workgroup's (member, cotangent)
  const double cs = mv.cs, cinv = mv.cinv;
  const double *x = mv.x, *D = mv.D, *E = mv.E, *y = mv.y;
  const int *map = mv.map, *rows = mv.rows;
  double *sol = mv.sol, *g = mv.g;
  BL s;
  slab_view(s, p, io, ks.slab(mv.qp));
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
  ks.solve(s, mv.Kinv, NPOL, n, N, map, rows, refine_iter, [g](int k) { return g[k]; }, sol, mv.res, mv.cor,
           lds + bd_lds_bytes(n, m, NPOL) / sizeof(double));
  // sol = [rx; rnu] of the scaled problem; the unscaled gradients into this cotangent's slices
  for (int j = tid; j < n; j += BP_NT) ad.dQ[slot * n + j] = 0.0 - (cs * D[j]) * sol[j];
  for (int i = tid; i < m; i += BP_NT) {
    const int a = map[i];
    const double v = a >= 0 ? E[i] * sol[n + a] : 0.0;
    ad.dL[slot * m + i] = (a >= 0 && a < nlow) ? v : 0.0;
    ad.dU[slot * m + i] = a >= nlow ? v : 0.0;
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
  bd_close(mv, ad.active, ad.stat);
}
