// batch_devio.h -- the entry points of a batch handle that take and return DEVICE arrays (osqp_amd_batch_*_dev),
// included at the end of batch.hip.  Each one is its host twin with the host copies taken out: the same checks in
// the same order, the same kernels on the same workspace, the same b->solved / b->polished / noncvx bookkeeping.
// What the twins do on the host before they copy happens here on the device:
//   k_batch_check_bounds   counts the pairs l > u (after the clamp to +-OSQP_INFTY) of an update; one 4-byte read-back
//                          decides whether the update is refused, before anything of the handle is written;
//   k_batch_stage_bounds   writes the clamped bounds into the raw l, u of the handle (what setup read and matrix
//                          updates re-read), where k_batch_update, unchanged, then finds them.
// Everything else is a device-to-device copy or an existing kernel reading the caller's array in place.
// The _dev twins of adjoint, adjoint_multi and tangent are not here: each shares one body with its host twin in
// batch.hip (adjoint_call, tangent_call), which asks dev_ptrs_check below.
//
// Every non-NULL device pointer of a call passes dev_ptr_check before any copy or launch.  The calls run on the
// handle's stream and return with it synchronised; no stream or event of the caller's crosses the ABI, so the
// caller's inputs have to be complete when the call is made.

// OSQP_DATA_VALIDATION_ERROR unless p is device memory of the handle's device as this process's HIP runtime knows it:
// a host pointer, managed or registered host memory, another device's memory and an address of another runtime's
// allocation (two HIP runtimes mapped side by side) are all refused.  Only asks the runtime; touches no GPU memory.
static c_int dev_ptr_check(const osqp_amd_batch *b, const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return OSQP_DATA_VALIDATION_ERROR;
  }
  return (at.type == hipMemoryTypeDevice && at.device == b->device) ? 0 : OSQP_DATA_VALIDATION_ERROR;
}
static c_int dev_ptrs_check(const osqp_amd_batch *b, std::initializer_list<const void *> ps) {
  for (const void *p : ps) if (p && dev_ptr_check(b, p)) return OSQP_DATA_VALIDATION_ERROR;
  return 0;
}

extern "C" c_int osqp_amd_batch_check_dev_ptr(osqp_amd_batch *b, const void *p) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!p) return OSQP_DATA_VALIDATION_ERROR;
  BCHK(hipSetDevice(b->device));
  return dev_ptr_check(b, p);
}

// the clamp of BatchOSQP.update (np.maximum(L, -OSQP_INFTY), np.minimum(U, OSQP_INFTY)); a NaN stays a NaN
__device__ __forceinline__ double clamp_lower(double v) { return v < -OSQP_INFTY ? -OSQP_INFTY : v; }
__device__ __forceinline__ double clamp_upper(double v) { return v > OSQP_INFTY ? OSQP_INFTY : v; }

#define BD_NT 256
#define BD_MAX_BLOCKS 1024
// *bad += the number of k in [0, cnt) with clamp(L[k]) > clamp(U[k]) (osqp.c:815-822 for every QP).  Grid-stride;
// the workgroup's count meets in LDS and at most one atomicAdd per workgroup leaves it.
__global__ void __launch_bounds__(BD_NT) k_batch_check_bounds(long long cnt, const double *L, const double *U, int *bad) {
  __shared__ int wsum[BD_NT / 64];
  int c = 0;
  for (long long k = (long long)blockIdx.x * BD_NT + threadIdx.x; k < cnt; k += (long long)gridDim.x * BD_NT)
    c += clamp_lower(L[k]) > clamp_upper(U[k]) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    if (t) atomicAdd(bad, t);
  }
}

// the clamped bounds into the raw l, u of the handle (null = keep); one owner per element
__global__ void __launch_bounds__(BD_NT) k_batch_stage_bounds(long long cnt, const double *L, const double *U,
                                                              double *rawL, double *rawU) {
  for (long long k = (long long)blockIdx.x * BD_NT + threadIdx.x; k < cnt; k += (long long)gridDim.x * BD_NT) {
    if (L) rawL[k] = clamp_lower(L[k]);
    if (U) rawU[k] = clamp_upper(U[k]);
  }
}
static unsigned bd_blocks(long long cnt) {
  return (unsigned)std::min<long long>((cnt + BD_NT - 1) / BD_NT, BD_MAX_BLOCKS);
}

extern "C" c_int osqp_amd_batch_update_dev(osqp_amd_batch *b, const c_float *Q, const c_float *L, const c_float *U) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  BCHK(hipSetDevice(b->device));
  if (dev_ptrs_check(b, {Q, L, U})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t B = (size_t)b->B;
  const long long cnt = (long long)B * b->m;
  if (L && U && cnt) {
    if (balloc_once(b, &b->d_bad, 1)) { (void)hipGetLastError(); return OSQP_MEM_ALLOC_ERROR; }
    int bad = 0;
    BCHK(hipMemsetAsync(b->d_bad, 0, sizeof(int), b->stream));
    hipLaunchKernelGGL(k_batch_check_bounds, dim3(bd_blocks(cnt)), dim3(BD_NT), 0, b->stream, cnt, L, U, b->d_bad);
    BCHK(hipGetLastError());
    BCHK(hipMemcpyAsync(&bad, b->d_bad, sizeof(int), hipMemcpyDeviceToHost, b->stream));
    BCHK(hipStreamSynchronize(b->stream));
    if (bad) return 1;                             // nothing of the handle has been written
  }
  if (b->engine == OSQP_AMD_BATCH_COMMON && (L || U) && cnt) {   // one class per row over the batch, before any write
    bool moved = false;
    if (const int rc = bc_check_classes(b, L, U, 1, &moved, "update")) return rc;
    if (moved) b->bc_rebuild = true;
  }
  mark_unsolved(b);
  if (Q) BCHK(hipMemcpyAsync(b->dQ, Q, B * b->n * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
  if ((L || U) && cnt)
    hipLaunchKernelGGL(k_batch_stage_bounds, dim3(bd_blocks(cnt)), dim3(BD_NT), 0, b->stream, cnt, L, U, b->dL, b->dU);
  hipLaunchKernelGGL(k_batch_update, dim3((unsigned)B), dim3(256), 0, b->stream, b->n, b->m, b->io,
                     Q ? b->dQ : nullptr, L ? b->dL : nullptr, U ? b->dU : nullptr, (double)RHO_TOL, (const int *)nullptr,
                     (double *)nullptr, (double *)nullptr, (double *)nullptr, 0);
  BCHK(hipGetLastError());
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" c_int osqp_amd_batch_update_matrices_dev(osqp_amd_batch *b,
                                                    const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                                    const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member) {
  BC_NEVER(b, "osqp_amd_batch_update_matrices_dev");
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  // the twin's refusals in the twin's order, on the host lists; then the device pointers; then the first write
  if (Px && Px_idx && P_n > b->nnzP) return 1;
  if (Ax && Ax_idx && A_n > b->nnzA) return 2;
  if ((Px && Px_idx && P_n < 0) || (Ax && Ax_idx && A_n < 0)) return OSQP_DATA_VALIDATION_ERROR;
  if (Px && Px_idx) for (c_int k = 0; k < P_n; k++) if (Px_idx[k] < 0 || Px_idx[k] >= b->nnzP) return OSQP_DATA_VALIDATION_ERROR;
  if (Ax && Ax_idx) for (c_int k = 0; k < A_n; k++) if (Ax_idx[k] < 0 || Ax_idx[k] >= b->nnzA) return OSQP_DATA_VALIDATION_ERROR;
  if (!Px && !Ax) return 0;
  BCHK(hipSetDevice(b->device));
  if (dev_ptrs_check(b, {Px, Ax})) return OSQP_DATA_VALIDATION_ERROR;
  mark_unsolved(b);
  const c_int pc = Px ? (Px_idx ? P_n : (c_int)b->nnzP) : 0, ac = Ax ? (Ax_idx ? A_n : (c_int)b->nnzA) : 0;
  if (stage_reserve(b, 0, (size_t)pc + ac)) return OSQP_MEM_ALLOC_ERROR;      // the index lists only
  if (Px && patch_values(b, &b->dPx, &b->io.Px, &b->io.strideP, b->nnzP, Px, Px_idx, pc, Px_per_member, 0, 0, true))
    return OSQP_MEM_ALLOC_ERROR;
  if (Ax && patch_values(b, &b->dAx, &b->io.Ax, &b->io.strideA, b->nnzA, Ax, Ax_idx, ac, Ax_per_member, 0, (size_t)pc, true))
    return OSQP_MEM_ALLOC_ERROR;
  if (b->engine == OSQP_AMD_BATCH_STREAMED) (void)bs_setup_launch(b, true);
  else batch_launch(b, 2);
  const long long bad = first_not_pd(b);
  if (bad < 0) return -102;
  b->noncvx = bad != b->B;
  if (b->noncvx) {
    fprintf(stderr, "osqp_amd batch: the new K of QP %zu of the batch is not positive definite (K = P + sigma I + "
                    "A' rho A with the updated values); solves are refused until a matrix update succeeds\n", (size_t)bad);
    return OSQP_NONCVX_ERROR;
  }
  return 0;
}

// (one body with its host twin, bc_update_model in batch.hip: the device pointers are checked after the host lists)
extern "C" c_int osqp_amd_batch_common_update_model_dev(osqp_amd_batch *b, const c_float *Px, const c_int *Px_idx, c_int P_n,
                                                        const c_float *Ax, const c_int *Ax_idx, c_int A_n) {
  return bc_update_model(b, true, "osqp_amd_batch_common_update_model_dev", Px, Px_idx, P_n, Ax, Ax_idx, A_n);
}

extern "C" c_int osqp_amd_batch_warm_start_dev(osqp_amd_batch *b, const c_float *X, const c_float *Y) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (X || Y) {
    BCHK(hipSetDevice(b->device));
    if (dev_ptrs_check(b, {X, Y})) return OSQP_DATA_VALIDATION_ERROR;
  }
  b->st.warm_start = 1;                          // osqp.c:948
  if (!X && !Y) return 0;
  mark_unsolved(b);
  if (b->engine == OSQP_AMD_BATCH_COMMON)
    hipLaunchKernelGGL(k_bc_warm_start, dim3((unsigned)b->B), dim3(256), 0, b->stream, b->pat, b->io, X, Y, (const int *)nullptr);
  else
    hipLaunchKernelGGL(k_batch_warm_start, dim3((unsigned)b->B), dim3(256), 0, b->stream, b->pat, b->io, X, Y, (const int *)nullptr);
  BCHK(hipGetLastError());
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// device-to-device copy of cnt elements into a caller's array (null or cnt = 0: skipped)
template <typename Tp>
static hipError_t give(osqp_amd_batch *b, Tp *dst, const Tp *src, size_t cnt) {
  return (dst && cnt) ? hipMemcpyAsync(dst, src, cnt * sizeof(Tp), hipMemcpyDeviceToDevice, b->stream) : hipSuccess;
}

extern "C" c_int osqp_amd_batch_get_dev(osqp_amd_batch *b, c_float *X, c_float *Y, c_float *info8,
                                       c_float *DX, c_float *DY) {
  if (!b) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  BCHK(hipSetDevice(b->device));
  if (dev_ptrs_check(b, {X, Y, info8, DX, DY})) return OSQP_DATA_VALIDATION_ERROR;
  const size_t B = (size_t)b->B, n = (size_t)b->n, m = (size_t)b->m;
  BCHK(give(b, X, b->io.Xo, B * n));
  BCHK(give(b, Y, b->io.Yo, B * m));
  BCHK(give(b, info8, b->io.info, B * 8));
  BCHK(give(b, DX, b->io.DXo, B * n));
  BCHK(give(b, DY, b->io.DYo, B * m));
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
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
  if (b->polished) BCHK(give(b, status_polish, (const int *)b->pol.stat, B));
  else BCHK(hipMemsetAsync(status_polish, 0, B * sizeof(int), b->stream));
  BCHK(hipStreamSynchronize(b->stream));
  return 0;
}
