// engine_aux_kernels.h -- included by engine.hip after engine_block_check.h, the last of the forms' own kernels (it uses TB, Ctx,
// DevMat, LDS_DECL and the SpMV pieces of engine_device.h; k_refresh_m uses elim_vb of engine_pcg_steps.h).
// Kernels around the operator that belong to no single form: the slack elimination's k_elim_refresh and k_elim_split, the Jacobi
// preconditioner k_precond, k_refresh_m (the m-parts of the PCG input vectors) and the plain product k_spmv.

// ---------------------------------------------------------------------------
// Elimination of slack-like variables from the linear system (launch-per-step kernels and the resident PCG).
//
// A variable y that (1) appears in exactly ONE row i of A (coefficient a), (2) has no off-diagonal entry in P and
// (3) shares its row with no other such variable couples to the rest of K = P + sigma I + A' rho A only through that row:
//     K_yy = D_y = P_yy + sigma + rho_i a^2,     K_Xy = rho_i a A(i,X)'.
// Eliminating all such y exactly (a block elimination with a DIAGONAL block) leaves, for the other variables X,
//     S = P_XX + sigma I + A_X' diag(rho~) A_X,     rho~_i = rho_i (P_yy + sigma) / D_y   (rho~_i = rho_i on rows without a y),
// i.e. the same operator with another weight on those rows; right-hand side b~_X = b_X - K_Xy b_y / D_y, back substitution
// x~_y = (b_y - rho_i a (A_X x~_X)_i) / D_y.  Why it pays: on equality rows rho_i = 1e3 rho (include/constants.h:70), so K_yy
// is huge against the Schur complement it hides and K is badly conditioned (Lasso, docs/examples/lasso.rst:41-63: the
// residual variables y with y = Ad x - b; config 3 ran 98.6 PCG iterations per ADMM iteration); S has rho~ ~ P_yy + sigma
// there.  Inertia: K > 0 <=> S > 0 and D > 0, so the convexity probe may run on the reduced operator too.
// In the kernels: the PCG vectors are zero at the eliminated variables (k_pcg_init starts them so, k_cg_B keeps w_y = 0;
// k_form_K gives their rows and columns of the resident K nothing but a diagonal entry and weighs the rows with rho~),
// k_cg_A weighs rows with rho~ (Ctx::rhoe), k_admm_finalize back-substitutes and folds b_y into the m-part of the next
// right-hand side.  The ADMM iterates themselves (x, z, y, residuals) never see any of this.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) k_elim_refresh(Ctx c) {
  const double sigma = c.prm->sigma;
  for (int i = blockIdx.x * TB + threadIdx.x; i < c.m; i += gridDim.x * TB) {
    const int y = c.ecol[i];
    const double rho = c.rho[i];
    if (y < 0) { c.rhoe[i] = rho; c.ecoef[i] = 0.0; c.edinv[i] = 0.0; continue; }
    const double a = c.A.val[c.epos[i]], d0 = c.pdiag[y] + sigma, D = d0 + rho * a * a;
    c.ecoef[i] = a; c.edinv[i] = 1.0 / D; c.rhoe[i] = rho * d0 / D;
  }
}
// x~ of the eliminated variables lives in xte (per row), the PCG vectors are zero there: after the host wrote va's n-part
__global__ void __launch_bounds__(TB) k_elim_split(Ctx c) {
  for (int j = blockIdx.x * TB + threadIdx.x; j < c.n; j += gridDim.x * TB) {
    const int i = c.erow[j];
    if (i >= 0) { c.xte[i] = c.va[j]; c.va[j] = 0.0; }
  }
}

// ---------------------------------------------------------------------------
// auxiliary kernels
// ---------------------------------------------------------------------------
// Jacobi preconditioner: Minv_j = 1 / (P_jj + sigma + sum_i rho_i A_ij^2)
__global__ void __launch_bounds__(TB) k_precond(Ctx c) {
  const double sigma = c.prm->sigma;
  for (int j = blockIdx.x * TB + threadIdx.x; j < c.n; j += gridDim.x * TB) {
    double s = c.pdiag[j] + sigma;
    for (int k = c.M.split[j]; k < c.M.rowptr[j + 1]; ++k) {
      const double a = c.M.val[k];
      s += c.rhoe[c.M.col[k] - c.n] * a * a;
    }
    if (c.nelim && c.erow[j] >= 0) s = 1.0;       // (not part of the PCG system)
    c.minv[j] = 1.0 / s;
    c.g4[j].m = 1.0 / s; c.g4[c.n + j].m = 1.0 / s;
  }
}

// m-parts of the PCG input vectors from (z, z~, y, rho); rhoinv from rho.  zt_partial: zt holds A x~ WITHOUT the
// eliminated variables' terms (it was just recomputed from the PCG vector): complete it first.
__global__ void __launch_bounds__(TB) k_refresh_m(Ctx c, int zt_partial) {
  const double *y = c.xy + c.n;
  const Params prm = *c.prm;
  for (int i = blockIdx.x * TB + threadIdx.x; i < c.m; i += gridDim.x * TB) {
    const double rho = c.rho[i];
    c.rhoinv[i] = 1.0 / rho;
    const double vbn = rho * c.z[i] - y[i];
    if (c.nelim && c.ecol[i] >= 0) {
      const double a = c.ecoef[i], xt = c.xte[i];
      double ax = c.zt[i];
      if (zt_partial) c.zt[i] = ax + a * xt; else ax -= a * xt;
      c.va[c.n + i] = c.rhoe[i] * ax;
      c.vb[c.n + i] = elim_vb(c, prm, i, rho, vbn, c.xy[c.ecol[i]]);
    } else {
      c.va[c.n + i] = rho * c.zt[i];
      c.vb[c.n + i] = vbn;
    }
  }
}

// Generic SpMV used by set_iterates (z = A x) and by the kernel-level tests.
// sel: 0 = whole row, 1 = entries before split (P part), 2 = from split (A' part)
__global__ void __launch_bounds__(TB) k_spmv(DevMat Mx, const double *in, double *out, int sel) {
  LDS_DECL(1);
  for (int bi = blockIdx.x; bi < Mx.nblk; bi += gridDim.x) {
    const RowBlk b = Mx.blk[bi];
    if (IS_LONG(b)) {
      int ka = b.k0, kb = b.k1;
      if (sel == 1) kb = Mx.split[b.r0];
      if (sel == 2) ka = Mx.split[b.r0];
      const double s = long_row_dot(Mx, ka, kb, in, red);
      if (threadIdx.x == 0) out[b.r0] = s;
    } else {
      stage_products<1>(Mx, b, in, nullptr, lprod, nullptr);
      __syncthreads();
      for (int r = b.r0 + threadIdx.x; r < b.r1; r += TB) {
        int a0 = Mx.rowptr[r] - b.k0, a1 = Mx.rowptr[r + 1] - b.k0;
        if (sel == 1) a1 = Mx.split[r] - b.k0;
        if (sel == 2) a0 = Mx.split[r] - b.k0;
        out[r] = row_sum(lprod, a0, a1);
      }
    }
    __syncthreads();
  }
}
