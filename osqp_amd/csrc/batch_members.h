// batch_members.h -- the member-list forms of the calls around the solve (osqp_amd_batch_*_members), included at the
// end of batch.hip.  Each one is its whole-batch twin for the listed members: `members [count]`, a host list, strictly
// ascending, every index in [0, B) (members_check, the checks of osqp_amd_batch_solve_members), in front of the twin's
// arguments, and every per-member array compact -- [count][.], row k belongs to member members[k].  Of a member that is
// not listed nothing changes: its raw and scaled q, l, u, classes, io.flag, results, certificates, stored iterates,
// solved flag and status_polish keep their bits.
//
// A form shares the twin's body in batch.hip (update_call, update_matrices_call, update_rho_call, warm_start_call,
// get_call, adjoint_call, tangent_call, verify_call),
// which takes the list; an entry point here is MEMBERS_OPEN -- the NULL handle (OSQP_WORKSPACE_NOT_INIT_ERROR), the
// list (OSQP_DATA_VALIDATION_ERROR), the engine's refusal where the twin has one, in this order and with nothing
// written -- and that call, after which the twin's own refusals come in the twin's order.  A list of all B members
// goes on as no list, so count == B runs the twin's code and nothing else.
//
// The kernels are the twins', given the list (k_batch_update, k_batch_warm_start, k_bc_warm_start, k_bc_classes,
// k_bp_active, the matrix-update phase of k_batch_solve, k_bs_setup<true>: one workgroup per listed member, compact
// inputs read at blockIdx.x; k_batch_scatter, k_batch_update_rho: one thread per listed entry) or already taking one (k_bp_form,
// k_bk_form, the inversions, k_bp_polish, k_ba_adjoint, k_bt_tangent, whose compact outputs go through BPol::pos).
// The list is uploaded once per call (members_upload).

#define MEMBERS_OPEN(refusal)                                           \
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;                         \
  if (const c_int rc = members_check(b, members, count)) return rc;     \
  refusal;                                                              \
  const c_int *list = count == b->B ? nullptr : members;   /* all B members, ascending: the twin's own path */

extern "C" c_int osqp_amd_batch_update_members(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *Q,
                                               const c_float *L, const c_float *U) {
  MEMBERS_OPEN()
  return update_call(b, false, list, count, Q, L, U);
}
extern "C" c_int osqp_amd_batch_update_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *Q,
                                                   const c_float *L, const c_float *U) {
  MEMBERS_OPEN()
  return update_call(b, true, list, count, Q, L, U);
}

extern "C" c_int osqp_amd_batch_warm_start_members(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *X,
                                                   const c_float *Y) {
  MEMBERS_OPEN()
  return warm_start_call(b, false, list, count, X, Y);
}
extern "C" c_int osqp_amd_batch_warm_start_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *X,
                                                       const c_float *Y) {
  MEMBERS_OPEN()
  return warm_start_call(b, true, list, count, X, Y);
}

// New matrix values and rho for the listed members: update_matrices_call and update_rho_call of batch.hip with the list.
// The values are one [k] array written to every listed member (*_per_member = 0) or compact [count][k]; a handle with
// shared raw values switches to per-member storage (patch_values) and the unlisted rows hold what was shared.
extern "C" c_int osqp_amd_batch_update_matrices_members(osqp_amd_batch *b, const c_int *members, c_int count,
                                                        const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                                        const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member) {
  MEMBERS_OPEN(BC_NEVER(b, "osqp_amd_batch_update_matrices_members"))
  return update_matrices_call(b, false, list, count, Px, Px_idx, P_n, Px_per_member, Ax, Ax_idx, A_n, Ax_per_member);
}
extern "C" c_int osqp_amd_batch_update_matrices_members_dev(osqp_amd_batch *b, const c_int *members, c_int count,
                                                            const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                                            const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member) {
  MEMBERS_OPEN(BC_NEVER(b, "osqp_amd_batch_update_matrices_members_dev"))
  return update_matrices_call(b, true, list, count, Px, Px_idx, P_n, Px_per_member, Ax, Ax_idx, A_n, Ax_per_member);
}
extern "C" c_int osqp_amd_batch_update_rho_members(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *rho,
                                                   c_int per_member) {
  MEMBERS_OPEN()
  return update_rho_call(b, list, count, rho, per_member);
}

// polish for the listed members: the work is done for those on which polish has not run since their last solve
// (member_polished), in polish's chunks, with NPOL and NS of their largest mred; status_polish[k] is member members[k]'s.
extern "C" c_int osqp_amd_batch_polish_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int *status_polish) {
  MEMBERS_OPEN(BC_UNSERVED(b, "osqp_amd_batch_polish_members"))
  if (!list) return osqp_amd_batch_polish(b, status_polish);   // its own work rule: once per solve, on every member
  if (!members_solved(b, members, count)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  BCHK(hipSetDevice(b->device));
  if (bp_reserve_maps(b)) return OSQP_MEM_ALLOC_ERROR;
  std::vector<int> todo;
  for (c_int k = 0; k < count; k++) if (!b->member_polished[(size_t)members[k]]) todo.push_back((int)members[k]);
  if (!todo.empty()) {
    if (members_upload(b, todo.data(), todo.size(), false)) return OSQP_MEM_ALLOC_ERROR;
    if (const c_int rc = bp_polish_run(b, &todo)) return rc;
    for (int q : todo) b->member_polished[(size_t)q] = 1;
  }
  return polish_status_out(b, members, count, status_polish);
}

// The general adjoint (ncot >= 1 cotangents per member, arrays [count][ncot][.]) and the tangent of the listed members:
// adjoint_call and tangent_call of batch.hip with the list.
extern "C" c_int osqp_amd_batch_adjoint_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int ncot,
                                                const c_float *dX, const c_float *dY, c_float *dQ, c_float *dL, c_float *dU,
                                                c_float *dPx, c_float *dAx, c_int *active, c_int *status_adjoint) {
  MEMBERS_OPEN(BC_UNSERVED(b, "osqp_amd_batch_adjoint_members"))
  return adjoint_call(b, false, "adjoint_members", ncot, dX, dY, dQ, dL, dU, dPx, dAx, active, status_adjoint, list, count);
}
extern "C" c_int osqp_amd_batch_adjoint_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_int ncot,
                                                    const c_float *dX, const c_float *dY, c_float *dQ, c_float *dL, c_float *dU,
                                                    c_float *dPx, c_float *dAx, int *active, int *status_adjoint) {
  MEMBERS_OPEN(BC_UNSERVED(b, "osqp_amd_batch_adjoint_members_dev"))
  return adjoint_call(b, true, "adjoint_members", ncot, dX, dY, dQ, dL, dU, dPx, dAx, active, status_adjoint, list, count);
}
extern "C" c_int osqp_amd_batch_tangent_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int ndir,
                                                const c_float *dQ, const c_float *dL, const c_float *dU, const c_float *dPx,
                                                const c_float *dAx, c_float *dX, c_float *dY, c_int *active, c_int *status_tangent) {
  MEMBERS_OPEN(BC_UNSERVED(b, "osqp_amd_batch_tangent_members"))
  return tangent_call(b, false, ndir, dQ, dL, dU, dPx, dAx, dX, dY, active, status_tangent, list, count);
}
extern "C" c_int osqp_amd_batch_tangent_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_int ndir,
                                                    const c_float *dQ, const c_float *dL, const c_float *dU, const c_float *dPx,
                                                    const c_float *dAx, c_float *dX, c_float *dY, int *active, int *status_tangent) {
  MEMBERS_OPEN(BC_UNSERVED(b, "osqp_amd_batch_tangent_members_dev"))
  return tangent_call(b, true, ndir, dQ, dL, dU, dPx, dAx, dX, dY, active, status_tangent, list, count);
}
extern "C" c_int osqp_amd_batch_get_members(osqp_amd_batch *b, const c_int *members, c_int count, c_float *X, c_float *Y,
                                            c_float *info8, c_float *DX, c_float *DY) {
  MEMBERS_OPEN()
  return get_call(b, false, list, count, X, Y, info8, DX, DY);
}
extern "C" c_int osqp_amd_batch_get_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_float *X, c_float *Y,
                                                c_float *info8, c_float *DX, c_float *DY) {
  MEMBERS_OPEN()
  return get_call(b, true, list, count, X, Y, info8, DX, DY);
}
// the records of the listed members: X, DX [count][n], Y, DY [count][m] (NULL = the handle's own rows of them), V [count][16]
extern "C" c_int osqp_amd_batch_verify_members(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *X,
                                               const c_float *Y, const c_float *DX, const c_float *DY, c_float eps_abs,
                                               c_float eps_rel, c_float *V) {
  MEMBERS_OPEN()
  return verify_call(b, false, list, count, X, Y, DX, DY, eps_abs, eps_rel, V);
}
extern "C" c_int osqp_amd_batch_verify_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, const c_float *X,
                                                   const c_float *Y, const c_float *DX, const c_float *DY, c_float eps_abs,
                                                   c_float eps_rel, c_float *V) {
  MEMBERS_OPEN()
  return verify_call(b, true, list, count, X, Y, DX, DY, eps_abs, eps_rel, V);
}
#undef MEMBERS_OPEN

// out[q] = 1 where member q's results are those of a solve of the problem the handle holds now.  Touches no GPU memory.
extern "C" c_int osqp_amd_batch_solved_members(osqp_amd_batch *b, c_int *out) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!out) return OSQP_DATA_VALIDATION_ERROR;
  for (size_t q = 0; q < (size_t)b->B; q++) out[q] = b->member_solved[q] ? 1 : 0;
  return 0;
}
