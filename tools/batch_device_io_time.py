"""Time of one MPC step and of the adjoint call with host arrays and with device arrays, for config 4 (1024 x n = 120,
m = 240, tiled engine) and for the streamed engine at n = 300, m = 600, B = 1024:
  step:     new Q, L, U -> update -> warm-started solve -> results (X, Y, info), from host arrays
            (BatchOSQP.update / results) and from device arrays that already hold the same numbers
            (BatchOSQP.update / results_into: the step data is assumed to be produced on the device);
  adjoint:  BatchOSQP.adjoint(dX, dY) against adjoint_into on the solved handle, without the matrix gradients.
Both routes run the same sequence of step data on a handle of their own, so the solves do the same work (the results
are compared bit for bit at the end).  Medians over --reps after --warmup untimed ones.  Device buffers are hipMalloc'd
through ctypes: no torch.
usage: python tools/batch_device_io_time.py [--reps 20] [--warmup 3] [--B 1024]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import osqp_amd  # noqa: E402
from osqp_amd.problems import mpc_batch  # noqa: E402
from tools.batch_streamed_time import problem  # noqa: E402

HIP = None


class Dev:
    """A hipMalloc'd [rows, cols] array with `__cuda_array_interface__` (kept for the life of the process)."""

    def __init__(self, shape, dtype=np.float64, init=None):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        p = C.c_void_p()
        if HIP.hipMalloc(C.byref(p), max(self.nbytes, 8)) != 0:
            raise MemoryError("hipMalloc")
        self.ptr = p.value
        self.__cuda_array_interface__ = dict(shape=self.shape, typestr="<f8" if self.dtype == np.float64 else "<i4",
                                             data=(self.ptr, False), version=2, strides=None)
        if init is not None:
            a = np.ascontiguousarray(init, dtype=self.dtype)
            assert a.shape == self.shape and HIP.hipMemcpy(self.ptr, a.ctypes.data, self.nbytes, 1) == 0

    def get(self):
        h = np.empty(self.shape, self.dtype)
        assert HIP.hipMemcpy(h.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return h


def main():
    global HIP
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=1024)
    a = ap.parse_args()
    s, Q, L, U = mpc_batch(batch=a.B)
    legs = [("tiled, config 4 (n=120, m=240)", "auto", s["P"], s["A"], Q, L, U),
            ("streamed (n=300, m=600)", "streamed") + tuple(problem(300, 600, a.B, seed=300))]
    for name, engine, P, A, Q, L, U in legs:
        hs = [osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine=engine) for _ in range(2)]
        if HIP is None:                      # after the library: the runtime the handles run on
            HIP = C.CDLL("libamdhip64.so")
            HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        B, n, m = hs[0].B, hs[0].n, hs[0].m
        rng = np.random.default_rng(0)
        for h in hs:
            h.solve(fetch=False)
        steps = a.warmup + a.reps
        # step data: q moves by a few per cent, the bounds widen and narrow a little (finite ones; the others stay)
        data = [(Q * (1 + 0.03 * rng.standard_normal(Q.shape)), L - 0.01 * rng.random(L.shape), U + 0.01 * rng.random(U.shape))
                for _ in range(steps)]
        ddata = [tuple(Dev(v.shape, init=v) for v in d) for d in data]
        X, Y, I = Dev((B, n)), Dev((B, m)), Dev((B, 8))
        t = {k: [] for k in ("step, host arrays", "step, device arrays", "adjoint, host arrays", "adjoint, device arrays")}
        for k in range(steps):
            t0 = time.perf_counter()
            assert hs[0].update(*data[k]) == 0
            r = hs[0].solve()
            t1 = time.perf_counter()
            assert hs[1].update(*ddata[k]) == 0
            hs[1].solve(fetch=False)
            hs[1].results_into(X=X, Y=Y, info=I)
            t2 = time.perf_counter()
            if k >= a.warmup:
                t["step, host arrays"].append(t1 - t0); t["step, device arrays"].append(t2 - t1)
        same = np.array_equal(r.x, X.get()) and np.array_equal(r.y, Y.get()) and np.array_equal(r.info_raw, I.get())
        dX, dY = rng.standard_normal((B, n)), rng.standard_normal((B, m))
        ddX, ddY = Dev((B, n), init=dX), Dev((B, m), init=dY)
        dq, dl, du = Dev((B, n)), Dev((B, m)), Dev((B, m))
        for k in range(steps):
            t0 = time.perf_counter()
            g = hs[0].adjoint(dX, dY)
            t1 = time.perf_counter()
            hs[1].adjoint_into(ddX, ddY, dq, dl, du)
            t2 = time.perf_counter()
            if k >= a.warmup:
                t["adjoint, host arrays"].append(t1 - t0); t["adjoint, device arrays"].append(t2 - t1)
        same = same and np.array_equal(g.dq, dq.get()) and np.array_equal(g.dl, dl.get()) and np.array_equal(g.du, du.get())
        med = {k: statistics.median(v) for k, v in t.items()}
        print("%s, B=%d, %d repetitions after %d warm-up:" % (name, B, a.reps, a.warmup))
        for k, v in t.items():
            print("    %-23s: median %9.3f ms (min %.3f, max %.3f)" % (k, 1e3 * med[k], 1e3 * min(v), 1e3 * max(v)))
        print("    steps per second x B: host %.3f M QPs/s, device %.3f M QPs/s; device / host time: step %.2f, adjoint %.2f"
              % (B / med["step, host arrays"] / 1e6, B / med["step, device arrays"] / 1e6,
                 med["step, device arrays"] / med["step, host arrays"], med["adjoint, device arrays"] / med["adjoint, host arrays"]))
        print("    solved %d of %d in the last step; the two routes' results and gradients are bit-equal: %s"
              % (int(np.sum(r.status_val == 1)), B, same))
        sys.stdout.flush()
        for h in hs:
            h.cleanup()


if __name__ == "__main__":
    main()
