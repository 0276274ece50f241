// batch_devio.h -- the entry points of a batch handle that take and return DEVICE arrays (osqp_amd_batch_*_dev),
// included at the end of batch.hip.  Each one is its host twin with the host copies taken out, and shares the twin's
// body in batch.hip, called with dev set (update_call, update_matrices_call, warm_start_call, get_call, adjoint_call,
// tangent_call, verify_call, bc_update_model): the same checks in the same order, the same kernels on the same workspace,
// the same b->solved / b->polished / noncvx bookkeeping.  An entry point here is the NULL-handle check, the engine's refusal
// where the twin has one, and that call.  What a twin does on the host before it copies happens on the device:
//   k_batch_check_bounds   counts the pairs l > u (after the clamp to +-OSQP_INFTY) of an update; one 4-byte read-back
//                          decides whether the update is refused, before anything of the handle is written;
//   k_batch_update         clamps the bounds on their way into the raw l, u of the handle (what setup read and matrix
//                          updates re-read).
// Everything else is a device-to-device copy or a kernel reading the caller's array in place.
//
// Every non-NULL device pointer of a call passes dev_ptr_check (batch.hip) before any copy or launch.  The calls run on
// the handle's stream and return with it synchronised; no stream or event of the caller's crosses the ABI, so the
// caller's inputs have to be complete when the call is made.

extern "C" c_int osqp_amd_batch_check_dev_ptr(osqp_amd_batch *b, const void *p) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!p) return OSQP_DATA_VALIDATION_ERROR;
  BCHK(hipSetDevice(b->device));
  return dev_ptr_check(b, p);
}

extern "C" c_int osqp_amd_batch_update_dev(osqp_amd_batch *b, const c_float *Q, const c_float *L, const c_float *U) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return update_call(b, true, nullptr, 0, Q, L, U);
}

extern "C" c_int osqp_amd_batch_update_matrices_dev(osqp_amd_batch *b,
                                                    const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                                    const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member) {
  BC_NEVER(b, "osqp_amd_batch_update_matrices_dev");
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return update_matrices_call(b, true, nullptr, 0, Px, Px_idx, P_n, Px_per_member, Ax, Ax_idx, A_n, Ax_per_member);
}

// (one body with its host twin, bc_update_model in batch.hip: the device pointers are checked after the host lists)
extern "C" c_int osqp_amd_batch_common_update_model_dev(osqp_amd_batch *b, const c_float *Px, const c_int *Px_idx, c_int P_n,
                                                        const c_float *Ax, const c_int *Ax_idx, c_int A_n) {
  return bc_update_model(b, true, "osqp_amd_batch_common_update_model_dev", Px, Px_idx, P_n, Ax, Ax_idx, A_n);
}

extern "C" c_int osqp_amd_batch_warm_start_dev(osqp_amd_batch *b, const c_float *X, const c_float *Y) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return warm_start_call(b, true, nullptr, 0, X, Y);
}

extern "C" c_int osqp_amd_batch_get_dev(osqp_amd_batch *b, c_float *X, c_float *Y, c_float *info8,
                                       c_float *DX, c_float *DY) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return get_call(b, true, nullptr, 0, X, Y, info8, DX, DY);
}

extern "C" c_int osqp_amd_batch_verify_dev(osqp_amd_batch *b, const c_float *X, const c_float *Y, const c_float *DX,
                                           const c_float *DY, c_float eps_abs, c_float eps_rel, c_float *V) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  return verify_call(b, true, nullptr, 0, X, Y, DX, DY, eps_abs, eps_rel, V);
}

// status_polish as osqp_amd_batch_polish reports it, without running polish: all 0 (not tried) when polish has not
// run since the last solve
extern "C" c_int osqp_amd_batch_polish_status_dev(osqp_amd_batch *b, int *status_polish) {
  BC_UNSERVED(b, "osqp_amd_batch_polish_status_dev");
  if (!b || !b->solved) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!status_polish) return 0;
  BCHK(hipSetDevice(b->device));
  if (dev_ptr_check(b, status_polish)) return OSQP_DATA_VALIDATION_ERROR;
  const size_t B = (size_t)b->B;
  if (b->polished) BCHK(hipMemcpyAsync(status_polish, b->pol.stat, B * sizeof(int), hipMemcpyDeviceToDevice, b->stream));
  else BCHK(hipMemsetAsync(status_polish, 0, B * sizeof(int), b->stream));
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}
