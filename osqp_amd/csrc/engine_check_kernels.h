// engine_check_kernels.h -- included by engine.hip after engine_aux_kernels.h (it uses TB, Ctx, Params, the SC_* slots, the
// reductions, the SpMV pieces and LDS_DECL of engine_device.h; k_residuals uses huge_row_sum of engine_pcg_steps.h).
// What update_info and check_termination need: k_residuals (residuals, norms, objective and the cheap halves of both infeasibility
// tests in one launch), k_final_sums and k_certificates.

// Residuals, tolerances' norms, rho-estimate norms, objective and the cheap
// halves of both infeasibility tests in ONE launch:
//   workgroups [0, gridA)          : rows of A (A x, primal side, delta_y)
//   workgroups [gridA, gridA+gridM): rows of M (P x, A'y, dual side, delta_x)
__global__ void __launch_bounds__(TB) k_residuals(Ctx c) {
  LDS_DECL(1);
  const Params prm = *c.prm;
  const bool sc = prm.has_scaling;
  double *x = c.xy;
  if ((int)blockIdx.x < c.gridA) {
    double m_pu = 0, m_ps = 0, m_zu = 0, m_zs = 0, m_au = 0, m_as = 0, m_du = 0, m_ds = 0, lhs = 0;
    for (int bi = blockIdx.x; bi < c.A.nblk; bi += c.gridA) {
      const RowBlk b = c.A.blk[bi];
      const bool longrow = IS_LONG(b);
      if (!longrow) { stage_products<1>(c.A, b, x, nullptr, lprod, nullptr); __syncthreads(); }
      for (int i = b.r0 + (longrow ? 0 : threadIdx.x); i < b.r1; i += (longrow ? 1 : TB)) {
        double ax;
        if (longrow) ax = bi >= c.A.nwave ? huge_row_sum(c, bi, red) : long_row_dot(c.A, b.k0, b.k1, x, red);
        else ax = row_sum(lprod, c.A.rowptr[i] - b.k0, c.A.rowptr[i + 1] - b.k0);
        if (!longrow || threadIdx.x == 0) {
          const double zi = c.z[i], pr = ax + (-1.0) * zi;
          const double ei = sc ? c.Einv[i] : 1.0, e = sc ? c.E[i] : 1.0;
          m_pu = fmax(m_pu, fabs(ei * pr)); m_ps = fmax(m_ps, fabs(pr));
          m_zu = fmax(m_zu, fabs(ei * zi)); m_zs = fmax(m_zs, fabs(zi));
          m_au = fmax(m_au, fabs(ei * ax)); m_as = fmax(m_as, fabs(ax));
          // delta_y projected on the polar of the recession cone (auxil.c:375-388)
          double dy = c.dy[i];
          const double li = c.l[i], ui = c.u[i];
          if (ui > INF_BOUND) { if (li < -INF_BOUND) dy = 0.0; else dy = fmin(dy, 0.0); }
          else if (li < -INF_BOUND) dy = fmax(dy, 0.0);
          c.dxy[c.n + i] = dy;
          m_du = fmax(m_du, fabs(e * dy)); m_ds = fmax(m_ds, fabs(dy));
          lhs += ui * fmax(dy, 0.0) + li * fmin(dy, 0.0);
        }
      }
      __syncthreads();
    }
    block_max_to(m_pu, c.scal + SCI(SC_PRI_U), red); block_max_to(m_ps, c.scal + SCI(SC_PRI_S), red);
    block_max_to(m_zu, c.scal + SCI(SC_Z_U), red);   block_max_to(m_zs, c.scal + SCI(SC_Z_S), red);
    block_max_to(m_au, c.scal + SCI(SC_AX_U), red);  block_max_to(m_as, c.scal + SCI(SC_AX_S), red);
    block_max_to(m_du, c.scal + SCI(SC_DYN_U), red); block_max_to(m_ds, c.scal + SCI(SC_DYN_S), red);
    lhs = block_sum(lhs, red);
    if (threadIdx.x == 0) c.part_s0[blockIdx.x] = lhs;
    return;
  }
  const int bid = blockIdx.x - c.gridA;
  double m_du = 0, m_ds = 0, m_qu = 0, m_qs = 0, m_tu = 0, m_ts = 0, m_pu = 0, m_ps = 0;
  double m_xu = 0, m_xs = 0, obj = 0, qdx = 0;
  for (int bi = bid; bi < c.M.nblk; bi += c.gridM) {
    const RowBlk b = c.M.blk[bi];
    const bool longrow = IS_LONG(b);
    if (!longrow) { stage_products<1>(c.M, b, c.xy, nullptr, lprod, nullptr); __syncthreads(); }
    for (int j = b.r0 + (longrow ? 0 : threadIdx.x); j < b.r1; j += (longrow ? 1 : TB)) {
      double px, aty;
      if (longrow) {
        px  = long_row_dot(c.M, b.k0, c.M.split[j], c.xy, red);
        aty = long_row_dot(c.M, c.M.split[j], b.k1, c.xy, red);
      } else {
        const int a0 = c.M.rowptr[j] - b.k0, as = c.M.split[j] - b.k0, a1 = c.M.rowptr[j + 1] - b.k0;
        px = row_sum(lprod, a0, as);
        aty = row_sum(lprod, as, a1);
      }
      if (!longrow || threadIdx.x == 0) {
        const double qj = c.q[j], xj = x[j], dxj = c.dxy[j];
        double dr = qj + px;
        if (c.m > 0) dr = dr + aty;
        const double di = sc ? c.Dinv[j] : 1.0, d = sc ? c.D[j] : 1.0;
        m_du = fmax(m_du, fabs(di * dr));  m_ds = fmax(m_ds, fabs(dr));
        m_qu = fmax(m_qu, fabs(di * qj));  m_qs = fmax(m_qs, fabs(qj));
        m_tu = fmax(m_tu, fabs(di * aty)); m_ts = fmax(m_ts, fabs(aty));
        m_pu = fmax(m_pu, fabs(di * px));  m_ps = fmax(m_ps, fabs(px));
        m_xu = fmax(m_xu, fabs(d * dxj));  m_xs = fmax(m_xs, fabs(dxj));
        obj += xj * (0.5 * px + qj);
        qdx += qj * dxj;
      }
    }
    __syncthreads();
  }
  block_max_to(m_du, c.scal + SCI(SC_DUA_U), red); block_max_to(m_ds, c.scal + SCI(SC_DUA_S), red);
  block_max_to(m_qu, c.scal + SCI(SC_Q_U), red);   block_max_to(m_qs, c.scal + SCI(SC_Q_S), red);
  block_max_to(m_tu, c.scal + SCI(SC_ATY_U), red); block_max_to(m_ts, c.scal + SCI(SC_ATY_S), red);
  block_max_to(m_pu, c.scal + SCI(SC_PX_U), red);  block_max_to(m_ps, c.scal + SCI(SC_PX_S), red);
  block_max_to(m_xu, c.scal + SCI(SC_DXN_U), red); block_max_to(m_xs, c.scal + SCI(SC_DXN_S), red);
  obj = block_sum(obj, red); qdx = block_sum(qdx, red);
  if (threadIdx.x == 0) { c.part_s1[bid] = obj; c.part_s2[bid] = qdx; }
}

// Fixed-order final sums of the three partial arrays above (one workgroup).
__global__ void __launch_bounds__(TB) k_final_sums(Ctx c) {
  __shared__ double red[16];
  double s[1];
  reduce_parts<1>(c.part_s0, nullptr, nullptr, c.gridA, red, s);
  if (threadIdx.x == 0) c.scal[SCI(SC_DYLHS)] = s[0];
  reduce_parts<1>(c.part_s1, nullptr, nullptr, c.gridM, red, s);
  if (threadIdx.x == 0) c.scal[SCI(SC_OBJ)] = s[0];
  reduce_parts<1>(c.part_s2, nullptr, nullptr, c.gridM, red, s);
  if (threadIdx.x == 0) c.scal[SCI(SC_QDX)] = s[0];
}

// Second stage of the infeasibility tests (auxil.c:401-417, 456-497):
// A' dy_proj, P dx over M; A dx row test over A.
__global__ void __launch_bounds__(TB) k_certificates(Ctx c, double eps_dx, int unscaled) {
  LDS_DECL(1);
  const bool sc = c.prm->has_scaling && unscaled;
  if ((int)blockIdx.x < c.gridA) {
    double viol = 0;
    for (int bi = blockIdx.x; bi < c.A.nblk; bi += c.gridA) {
      const RowBlk b = c.A.blk[bi];
      const bool longrow = IS_LONG(b);
      if (!longrow) { stage_products<1>(c.A, b, c.dxy, nullptr, lprod, nullptr); __syncthreads(); }
      for (int i = b.r0 + (longrow ? 0 : threadIdx.x); i < b.r1; i += (longrow ? 1 : TB)) {
        double adx;
        if (longrow) adx = long_row_dot(c.A, b.k0, b.k1, c.dxy, red);
        else adx = row_sum(lprod, c.A.rowptr[i] - b.k0, c.A.rowptr[i + 1] - b.k0);
        if (!longrow || threadIdx.x == 0) {
          if (sc) adx = c.Einv[i] * adx;
          if ((c.u[i] < INF_BOUND && adx > eps_dx) || (c.l[i] > -INF_BOUND && adx < -eps_dx)) viol += 1.0;
        }
      }
      __syncthreads();
    }
    viol = block_sum(viol, red);
    if (threadIdx.x == 0 && viol > 0) atomic_max_pos(c.scal + SCI(SC_ADX_VIOL), viol);
    return;
  }
  const int bid = blockIdx.x - c.gridA;
  double m_tu = 0, m_ts = 0, m_pu = 0, m_ps = 0;
  for (int bi = bid; bi < c.M.nblk; bi += c.gridM) {
    const RowBlk b = c.M.blk[bi];
    const bool longrow = IS_LONG(b);
    if (!longrow) { stage_products<1>(c.M, b, c.dxy, nullptr, lprod, nullptr); __syncthreads(); }
    for (int j = b.r0 + (longrow ? 0 : threadIdx.x); j < b.r1; j += (longrow ? 1 : TB)) {
      double pdx, atdy;
      if (longrow) {
        pdx  = long_row_dot(c.M, b.k0, c.M.split[j], c.dxy, red);
        atdy = long_row_dot(c.M, c.M.split[j], b.k1, c.dxy, red);
      } else {
        const int a0 = c.M.rowptr[j] - b.k0, as = c.M.split[j] - b.k0, a1 = c.M.rowptr[j + 1] - b.k0;
        pdx = row_sum(lprod, a0, as);
        atdy = row_sum(lprod, as, a1);
      }
      if (!longrow || threadIdx.x == 0) {
        const double di = sc ? c.Dinv[j] : 1.0;
        m_tu = fmax(m_tu, fabs(di * atdy)); m_ts = fmax(m_ts, fabs(atdy));
        m_pu = fmax(m_pu, fabs(di * pdx));  m_ps = fmax(m_ps, fabs(pdx));
      }
    }
    __syncthreads();
  }
  block_max_to(m_tu, c.scal + SCI(SC_ATDY_U), red); block_max_to(m_ts, c.scal + SCI(SC_ATDY_S), red);
  block_max_to(m_pu, c.scal + SCI(SC_PDX_U), red);  block_max_to(m_ps, c.scal + SCI(SC_PDX_S), red);
}
