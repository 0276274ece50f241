// batch_members.h -- the member-list forms of the calls around the solve (osqp_amd_batch_*_members), included at the
// end of batch.hip.  Each one is its whole-batch twin for the listed members: `members [count]`, a host list, strictly
// ascending, every index in [0, B) (the checks of osqp_amd_batch_solve_members), in front of the twin's arguments, and
// every per-member array compact -- [count][.], row k belongs to member members[k].  Of a member that is not listed
// nothing changes: its raw and scaled q, l, u, classes, io.flag, results, certificates, stored iterates, solved flag
// and status_polish keep their bits.  count == B is the twin itself and takes the twin's own code path.
//
// The kernels are the twins', given the list (k_batch_update, k_batch_warm_start, k_bc_warm_start, k_bc_classes,
// k_bp_active: one workgroup per listed member, compact inputs read at blockIdx.x) or already taking one (k_bp_form,
// k_bk_form, the inversions, k_bp_polish, k_ba_adjoint, k_bt_tangent, whose compact outputs go through BPol::pos).
// The list is uploaded once per call (members_upload).  Refusals, in this order and with nothing written: a NULL handle
// (OSQP_WORKSPACE_NOT_INIT_ERROR), a bad list (OSQP_DATA_VALIDATION_ERROR), then the twin's own in the twin's order.

static c_int members_check(const osqp_amd_batch *b, const c_int *members, c_int count) {
  if (!members || count < 1 || count > b->B) return OSQP_DATA_VALIDATION_ERROR;
  for (c_int k = 0; k < count; k++)
    if (members[k] < 0 || members[k] >= b->B || (k && members[k] <= members[k - 1])) return OSQP_DATA_VALIDATION_ERROR;
  return 0;
}

// osqp_amd_batch_update / _update_dev for count < B listed members.  The compact rows go through the staging on the host
// route and are read in place on the device route; k_batch_update writes the raw rows of the listed members (clamped on
// the device route, as k_batch_stage_bounds clamps) and scales them.
static c_int update_members_call(osqp_amd_batch *b, bool dev, const c_int *members, c_int count, const c_float *Q,
                                 const c_float *L, const c_float *U) {
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {Q, L, U})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t R = (size_t)count, n = (size_t)b->n, m = (size_t)b->m, cnt = R * m;
  if (!m) L = U = nullptr;
  if (!dev && L && U)
    for (size_t k = 0; k < cnt; k++) if (L[k] > U[k]) return 1;   // osqp.c:815-822
  if (dev && L && U) {
    if (balloc_once(b, &b->d_bad, 1)) { (void)hipGetLastError(); return OSQP_MEM_ALLOC_ERROR; }
    int bad = 0;
    BCHK(hipMemsetAsync(b->d_bad, 0, sizeof(int), b->stream));
    hipLaunchKernelGGL(k_batch_check_bounds, dim3(bd_blocks((long long)cnt)), dim3(BD_NT), 0, b->stream, (long long)cnt, L, U, b->d_bad);
    BCHK(hipGetLastError());
    BCHK(hipMemcpyAsync(&bad, b->d_bad, sizeof(int), hipMemcpyDeviceToHost, b->stream));
    BCHK(hipStreamSynchronize(b->stream));
    if (bad) return 1;                             // nothing of the handle has been written
  }
  const std::vector<int> sel(members, members + count);
  if (members_upload(b, sel.data(), R, false)) return OSQP_MEM_ALLOC_ERROR;
  const double *sQ = Q, *sL = L, *sU = U;
  if (!dev) {
    if (stage_reserve(b, R * (n + 2 * m), 0)) return OSQP_MEM_ALLOC_ERROR;
    double *at = b->d_vals;
    for (const double **v : {&sQ, &sL, &sU}) {
      if (!*v) continue;
      const size_t len = R * (v == &sQ ? n : m);
      BCHK(hipMemcpyAsync(at, *v, len * sizeof(double), hipMemcpyHostToDevice, b->stream));
      *v = at; at += len;
    }
  }
  // common-K: the unlisted members keep the class the handle holds for every row, so the listed ones must too
  if (b->engine == OSQP_AMD_BATCH_COMMON && (sL || sU))
    if (const int rc = bc_check_classes(b, sL, sU, dev ? 1 : 0, nullptr, "update_members", members, R, b->d_mlist)) return rc;
  mark_members_unsolved(b, members, count);
  hipLaunchKernelGGL(k_batch_update, dim3((unsigned)R), dim3(256), 0, b->stream, b->n, b->m, b->io, sQ, sL, sU, (double)RHO_TOL,
                     (const int *)b->d_mlist, b->dQ, b->dL, b->dU, dev ? 1 : 0);
  BCHK(hipGetLastError());
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_update_members(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *Q,
                                               const c_float *L, const c_float *U) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (const c_int rc = members_check(b, members, count)) return rc;
  if (count == b->B) return osqp_amd_batch_update(b, Q, L, U);
  return update_members_call(b, false, members, count, Q, L, U);
}
extern "C" c_int osqp_amd_batch_update_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *Q,
                                                   const c_float *L, const c_float *U) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (const c_int rc = members_check(b, members, count)) return rc;
  if (count == b->B) return osqp_amd_batch_update_dev(b, Q, L, U);
  return update_members_call(b, true, members, count, Q, L, U);
}

// osqp_amd_batch_warm_start / _warm_start_dev for count < B listed members
static c_int warm_start_members_call(osqp_amd_batch *b, bool dev, const c_int *members, c_int count, const c_float *X,
                                     const c_float *Y) {
  if (dev && (X || Y)) {
    BCHK(hipSetDevice(b->device));
    if (dev_ptrs_check(b, {X, Y})) return OSQP_DATA_VALIDATION_ERROR;
  }
  b->st.warm_start = 1;                          // osqp.c:948
  if (!X && !Y) return 0;
  BCHK(hipSetDevice(b->device));
  const size_t R = (size_t)count, nx = X ? R * b->n : 0, ny = Y ? R * b->m : 0;
  const std::vector<int> sel(members, members + count);
  if (members_upload(b, sel.data(), R, false)) return OSQP_MEM_ALLOC_ERROR;
  const double *sX = X, *sY = Y;
  if (!dev) {
    if (stage_reserve(b, nx + ny, 0)) return OSQP_MEM_ALLOC_ERROR;
    if (nx) BCHK(hipMemcpyAsync(b->d_vals, X, nx * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (ny) BCHK(hipMemcpyAsync(b->d_vals + nx, Y, ny * sizeof(double), hipMemcpyHostToDevice, b->stream));
    sX = X ? b->d_vals : nullptr; sY = Y ? b->d_vals + nx : nullptr;
  }
  mark_members_unsolved(b, members, count);      // the stored iterates are the caller's now, not a solve's
  if (b->engine == OSQP_AMD_BATCH_COMMON)
    hipLaunchKernelGGL(k_bc_warm_start, dim3((unsigned)R), dim3(256), 0, b->stream, b->pat, b->io, sX, sY, (const int *)b->d_mlist);
  else
    hipLaunchKernelGGL(k_batch_warm_start, dim3((unsigned)R), dim3(256), 0, b->stream, b->pat, b->io, sX, sY, (const int *)b->d_mlist);
  BCHK(hipGetLastError());
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_warm_start_members(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *X,
                                                   const c_float *Y) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (const c_int rc = members_check(b, members, count)) return rc;
  if (count == b->B) return osqp_amd_batch_warm_start(b, X, Y);
  return warm_start_members_call(b, false, members, count, X, Y);
}
extern "C" c_int osqp_amd_batch_warm_start_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *X,
                                                       const c_float *Y) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (const c_int rc = members_check(b, members, count)) return rc;
  if (count == b->B) return osqp_amd_batch_warm_start_dev(b, X, Y);
  return warm_start_members_call(b, true, members, count, X, Y);
}

// polish for the listed members: the work is done for those on which polish has not run since their last solve
// (member_polished), in polish's chunks, with NPOL and NS of their largest mred; status_polish[k] is member members[k]'s.
extern "C" c_int osqp_amd_batch_polish_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int *status_polish) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (const c_int rc = members_check(b, members, count)) return rc;
  BC_UNSERVED(b, "osqp_amd_batch_polish_members");
  if (count == b->B) return osqp_amd_batch_polish(b, status_polish);
  if (!members_solved(b, members, count)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  BCHK(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  if (bp_reserve_maps(b)) return OSQP_MEM_ALLOC_ERROR;
  std::vector<int> todo;
  for (c_int k = 0; k < count; k++) if (!b->member_polished[(size_t)members[k]]) todo.push_back((int)members[k]);
  if (!todo.empty()) {
    if (members_upload(b, todo.data(), todo.size(), false)) return OSQP_MEM_ALLOC_ERROR;
    if (const c_int rc = bp_polish_run(b, &todo)) return rc;
    for (int q : todo) b->member_polished[(size_t)q] = 1;
  }
  if (status_polish) {
    std::vector<int> h(B);
    BCHK(hipMemcpyAsync(h.data(), b->pol.stat, B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    BCHK(hipStreamSynchronize(b->stream));
    for (c_int k = 0; k < count; k++) status_polish[k] = h[(size_t)members[k]];
  }
  return 0;
}

// The general adjoint (ncot >= 1 cotangents per member, arrays [count][ncot][.]) and the tangent of the listed members:
// adjoint_call and tangent_call of batch.hip with the list.
#define MEMBERS_OPEN(call)                                              \
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;                         \
  if (const c_int rc = members_check(b, members, count)) return rc;     \
  BC_UNSERVED(b, call);                                                 \
  const c_int *list = count == b->B ? nullptr : members;   /* all B members, ascending: the twin's own path */

extern "C" c_int osqp_amd_batch_adjoint_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int ncot,
                                                const c_float *dX, const c_float *dY, c_float *dQ, c_float *dL, c_float *dU,
                                                c_float *dPx, c_float *dAx, c_int *active, c_int *status_adjoint) {
  MEMBERS_OPEN("osqp_amd_batch_adjoint_members")
  return adjoint_call(b, false, "adjoint_members", ncot, dX, dY, dQ, dL, dU, dPx, dAx, active, status_adjoint, list, count);
}
extern "C" c_int osqp_amd_batch_adjoint_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_int ncot,
                                                    const c_float *dX, const c_float *dY, c_float *dQ, c_float *dL, c_float *dU,
                                                    c_float *dPx, c_float *dAx, int *active, int *status_adjoint) {
  MEMBERS_OPEN("osqp_amd_batch_adjoint_members_dev")
  return adjoint_call(b, true, "adjoint_members", ncot, dX, dY, dQ, dL, dU, dPx, dAx, active, status_adjoint, list, count);
}
extern "C" c_int osqp_amd_batch_tangent_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int ndir,
                                                const c_float *dQ, const c_float *dL, const c_float *dU, const c_float *dPx,
                                                const c_float *dAx, c_float *dX, c_float *dY, c_int *active, c_int *status_tangent) {
  MEMBERS_OPEN("osqp_amd_batch_tangent_members")
  return tangent_call(b, false, ndir, dQ, dL, dU, dPx, dAx, dX, dY, active, status_tangent, list, count);
}
extern "C" c_int osqp_amd_batch_tangent_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_int ndir,
                                                    const c_float *dQ, const c_float *dL, const c_float *dU, const c_float *dPx,
                                                    const c_float *dAx, c_float *dX, c_float *dY, int *active, int *status_tangent) {
  MEMBERS_OPEN("osqp_amd_batch_tangent_members_dev")
  return tangent_call(b, true, ndir, dQ, dL, dU, dPx, dAx, dX, dY, active, status_tangent, list, count);
}
#undef MEMBERS_OPEN

// The listed rows of the results: k_batch_gather into the staging and one copy per array to the host, or straight into
// the caller's device arrays, which receive exactly count rows.
static c_int get_members_call(osqp_amd_batch *b, bool dev, const c_int *members, c_int count, c_float *X, c_float *Y,
                              c_float *info8, c_float *DX, c_float *DY) {
  BCHK(hipSetDevice(b->device));
  if (dev && dev_ptrs_check(b, {X, Y, info8, DX, DY})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t R = (size_t)count, n = (size_t)b->n, m = (size_t)b->m;
  struct { c_float *dst; const double *src; size_t width; } rows[] = {
      {X, b->io.Xo, n}, {Y, b->io.Yo, m}, {info8, b->io.info, 8}, {DX, b->io.DXo, n}, {DY, b->io.DYo, m}};
  size_t total = 0;
  for (const auto &r : rows) if (r.dst) total += R * r.width;
  if (!total) return 0;
  const std::vector<int> sel(members, members + count);
  if (members_upload(b, sel.data(), R, false)) return OSQP_MEM_ALLOC_ERROR;
  if (!dev && stage_reserve(b, total, 0)) return OSQP_MEM_ALLOC_ERROR;
  double *at = b->d_vals;
  for (const auto &r : rows) {
    const size_t len = R * r.width;
    if (!r.dst || !len) continue;
    hipLaunchKernelGGL(k_batch_gather, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, b->stream, dev ? r.dst : at, r.src,
                       (long long)r.width, (const int *)b->d_mlist, (long long)R);
    BCHK(hipGetLastError());
    if (!dev) { BCHK(hipMemcpyAsync(r.dst, at, len * sizeof(double), hipMemcpyDeviceToHost, b->stream)); at += len; }
  }
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_get_members(osqp_amd_batch *b, const c_int *members, c_int count, c_float *X, c_float *Y,
                                            c_float *info8, c_float *DX, c_float *DY) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (const c_int rc = members_check(b, members, count)) return rc;
  if (count == b->B) return osqp_amd_batch_get(b, X, Y, info8, DX, DY);
  return get_members_call(b, false, members, count, X, Y, info8, DX, DY);
}
extern "C" c_int osqp_amd_batch_get_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_float *X, c_float *Y,
                                                c_float *info8, c_float *DX, c_float *DY) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (const c_int rc = members_check(b, members, count)) return rc;
  if (count == b->B) return osqp_amd_batch_get_dev(b, X, Y, info8, DX, DY);
  return get_members_call(b, true, members, count, X, Y, info8, DX, DY);
}

// out[q] = 1 where member q's results are those of a solve of the problem the handle holds now.  Touches no GPU memory.
extern "C" c_int osqp_amd_batch_solved_members(osqp_amd_batch *b, c_int *out) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!out) return OSQP_DATA_VALIDATION_ERROR;
  for (size_t q = 0; q < (size_t)b->B; q++) out[q] = b->member_solved[q] ? 1 : 0;
  return 0;
}
