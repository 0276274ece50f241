// batch_tangent.h -- forward sensitivities of the solution for the solved members of a batch, included by batch.hip
// after batch_adjoint.h.  Given tangents (dq, dl, du, dPx, dAx) of the data, ndir directions per member, it returns
// dx and dy of the solution: one column of the Jacobian per direction, where the adjoint gives one row per call.
//
// Per member, with the active rows (lows first, then upps, as k_bp_active orders them), Ar those rows of A, nu = y
// on them: locally P x + q + Ar' nu = 0 and Ar x = b_active (b = l on a row active at its lower bound, u at its
// upper), so
//   M [dx; dnu] = [-(dq + dP x + dA' y_act); db_act - (dA x)_act],   M = [P, Ar'; Ar, 0],
//   dy = dnu on the active rows, 0 elsewhere,
// with y_act = y on the active rows and 0 elsewhere, db = dl_i (du_i) on a row active at its lower (upper) bound,
// and an off-diagonal slot of triu(P) standing for both halves of dP.  The tangent of the other bound of a row, of
// an inactive row and of an infinite bound has no effect.
// The handle holds the scaled problem (P~ = c D P D, A~ = E A D, q~ = c D q, x = D x~, y = E y~ / c), so the solve
// runs in that space like polish and the adjoint: dq~ = c D dq, dP~ = c D dP D, dA~ = E dA D, db~ = E db, then
// dx = D dx~, dy = E dnu~ / c, with D, E, c as constants (the unscaled solution does not depend on them).
//
// The route is the adjoint's: k_bp_active, k_bp_form and k_bp_invert as they are, on the polish buffers with a
// pivot-verdict array of the call's own, then
//   k_bt_tangent  grid (members of the chunk, ndir): one workgroup per member and direction, so the directions of a
//                 member share the one inversion.  The right-hand side in LDS, polish's solve (kkt_solve_refined:
//                 the explicit inverse, then exactly polish_refine_iter refinement steps against the unregularised
//                 M), and the unscaled outputs.
// The three sparse products of the right-hand side have one owner per output element, which sums in storage order:
// dP~ x~ over a column of the full symmetric pattern, dA~' y~ over a CSC column, dA~ x~ over a CSR row.  A missing
// tangent adds the same 0.0 a tangent of zeros adds.  No atomics: the results are reproducible to the bit, and a
// direction's bits do not depend on which other directions the call carries.
// Nothing of the handle's solve state is written: X, Y, info, the stored iterates, rho, K^-1, flags and polish's
// status stay bit-equal.

struct BTan {              // staging of a handle's tangent call (device pointers)
  const double *dQ, *dL, *dU;   // [B][ndir][n], [B][ndir][m], [B][ndir][m] (null = 0)
  const double *dPx, *dAx;      // [B][ndir][nnzP], [B][ndir][nnzA] (null = 0)
  double *dX, *dY;              // [B][ndir][n], [B][ndir][m]
  int *active;                  // [B][m] -1 active at the lower bound, +1 at the upper, 0 inactive
  int *stat;                    // [B] status_tangent: 1 computed, -1 pivot of the wrong sign, 0 not tried
  int ndir;
};

// Opening, close and LDS as k_ba_adjoint (bd_open, bd_close, bd_lds_bytes in batch_polish.h): pl.stat is the pivot
// verdict of this call's inversion and is only read here; the status the caller sees is tg.stat.
template <class KS, class... KSArg>
__global__ void __launch_bounds__(BP_NT) k_bt_tangent(BPattern p, BIO io, BPol pl, BTan tg, int NPOL, int refine_iter,
                                                      const int *list, KSArg... ksarg) {
  const KS ks{ksarg...};
  extern __shared__ __attribute__((aligned(16))) double lds[];
  BDView mv;
  if (!bd_open(p, io, pl, tg.stat, tg.ndir, NPOL, list, lds, ks, mv)) return;
  const int n = mv.n, m = mv.m, N = mv.N, nlow = mv.nlow, tid = threadIdx.x;
  const long long slot = mv.slot;                         // this workgroup's (member, direction)
  const double cs = mv.cs, cinv = mv.cinv;
  const double *x = mv.x, *D = mv.D, *E = mv.E, *y = mv.y;
  const int *map = mv.map, *rows = mv.rows;
  double *sol = mv.sol, *g = mv.g;
  BL s;
  slab_view(s, p, io, ks.slab(mv.qp));
  __syncthreads();
  const double *dq = tg.dQ ? tg.dQ + slot * n : nullptr;
  const double *dl = tg.dL ? tg.dL + slot * m : nullptr, *du = tg.dU ? tg.dU + slot * m : nullptr;
  const double *dP = tg.dPx ? tg.dPx + slot * p.nnzP : nullptr, *dA = tg.dAx ? tg.dAx + slot * p.nnzA : nullptr;
  // rhs = [-(dq~ + dP~ x~ + dA~' y~_act); db~_act - (dA~ x~)_act], zero in the padding
  for (int k = tid; k < NPOL; k += BP_NT) {
    double v = 0.0;
    if (k < n) {
      const double dk = D[k];
      double px = 0.0, aty = 0.0;
      if (dP)
        for (int kk = s.Fp[k]; kk < s.Fp[k + 1]; ++kk) { const int i = s.Fi[kk]; px += (D[i] * dP[s.Fk[kk]]) * x[i]; }
      if (dA)
        for (int kk = s.Ap[k]; kk < s.Ap[k + 1]; ++kk) {
          const int i = s.Ai[kk];
          if (map[i] >= 0) aty += (E[i] * dA[kk]) * y[i];
        }
      const double qk = dq ? (cs * dk) * dq[k] : 0.0;
      v = 0.0 - ((qk + (cs * dk) * px) + dk * aty);
    } else if (k < N) {
      const int a = k - n, r = rows[a];
      const double *db = a < nlow ? dl : du;
      double ax = 0.0;
      if (dA)
        for (int kk = s.Rp[r]; kk < s.Rp[r + 1]; ++kk) { const int j = s.Rj[kk]; ax += (D[j] * dA[s.Rk[kk]]) * x[j]; }
      v = (db ? E[r] * db[r] : 0.0) - E[r] * ax;
    }
    g[k] = v;
  }
  __syncthreads();
  ks.solve(s, mv.Kinv, NPOL, n, N, map, rows, refine_iter, [g](int k) { return g[k]; }, sol, mv.res, mv.cor,
           lds + bd_lds_bytes(n, m, NPOL) / sizeof(double));
  // sol = [dx~; dnu~] of the scaled problem; the unscaled tangents
  for (int j = tid; j < n; j += BP_NT) tg.dX[slot * n + j] = D[j] * sol[j];
  for (int i = tid; i < m; i += BP_NT) {
    const int a = map[i];
    tg.dY[slot * m + i] = a >= 0 ? (E[i] * sol[n + a]) * cinv : 0.0;
  }
  bd_close(mv, tg.active, tg.stat);
}
