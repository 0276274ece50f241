// engine_util_kernels.h -- included by engine.hip after engine_ruiz_kernels.h, right ahead of the host side (it uses
// TB, Ctx and State of engine_device.h).
// Small kernels the host calls use: k_fill, FillRanges / k_fill_ranges, k_start_reset, k_window_begin, k_repack.

__global__ void __launch_bounds__(TB) k_fill(double *p, double v, int cnt) {
  for (int i = blockIdx.x * TB + threadIdx.x; i < cnt; i += gridDim.x * TB) p[i] = v;
}

// Up to FILL_RANGES arrays set to zero in one launch (hipeng_cold_start: one launch instead of one memset per array).
#define FILL_RANGES 6
struct FillRanges { double *p[FILL_RANGES]; int cnt[FILL_RANGES]; };
__global__ void __launch_bounds__(TB) k_fill_ranges(FillRanges f) {
  for (int k = 0; k < FILL_RANGES; k++) {
    double *p = f.p[k];
    const int cnt = f.cnt[k];
    for (int i = blockIdx.x * TB + threadIdx.x; i < cnt; i += gridDim.x * TB) p[i] = 0.0;
  }
}

// reset_start in one launch: vx = vold = va over all n + m entries, and the history count back to zero.
__global__ void __launch_bounds__(TB) k_start_reset(Ctx c, int cnt) {
  for (int i = blockIdx.x * TB + threadIdx.x; i < cnt; i += gridDim.x * TB) {
    const double v = c.va[i];
    c.vx[i] = v; c.vold[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) c.st->hist_r = 0;
}

// What a window of hipeng_run_admm starts from: the target and the window's extremes of the PCG iteration count.
__global__ void k_window_begin(State *st, long long target) {
  if (threadIdx.x == 0) { st->admm_target = target; st->iters_max = 0; st->iters_min = 0x7f7f7f7f; }
}

// dst[k] = src_val[map[k]] (map < 0: structural zero inside a dense block)
__global__ void __launch_bounds__(TB) k_repack(const double *src, const int *map, double *dst, long long cnt) {
  for (long long k = (long long)blockIdx.x * TB + threadIdx.x; k < cnt; k += (long long)gridDim.x * TB) {
    const int q = map[k];
    dst[k] = q >= 0 ? src[q] : 0.0;
  }
}
