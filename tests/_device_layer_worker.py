"""Worker of test_gpu_batch_device_io.test_layer_on_cuda_tensors: BatchQPLayer on CUDA tensors and on CPU tensors, in
a process of its own, because importing torch maps torch's own copy of the HIP runtime and the other GPU tests of the
suite must keep seeing the one the library was loaded with.  torch is imported before the library, so that both run
on one runtime and torch's allocations are device memory the library knows.
usage: _device_layer_worker.py <n> <m> <B> <seed> <out.npz>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import osqp_amd  # noqa: E402
from _batch_parity import shape_family  # noqa: E402


def run(device, P, A, calls, W):
    """Three forward / backward passes of one layer: the first sets the handle up, the others find it live.  The third
    one's loss is X.sum() + Y.sum(), whose incoming gradients are expanded (stride 0, not contiguous) tensors."""
    layer = osqp_amd.BatchQPLayer(P, A, engine="auto")
    out, routes, flags = {}, [], []
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=device, requires_grad=True)
    Wt = [torch.tensor(w, dtype=torch.float64, device=device) for w in W]
    for k, (Q, L, U, Ax, weighted) in enumerate(calls, 1):
        Qt, Lt, Ut, At = t(Q), t(L), t(U), t(Ax)
        X, Y = layer(Qt, Lt, Ut, Ax=At, return_y=True)
        routes.append(layer.last_route)
        ((X * Wt[0]).sum() + (Y * Wt[1]).sum() if weighted else X.sum() + Y.sum()).backward()
        r = layer.last_results
        flags.append(all(v.device == Qt.device for v in (X, Y, Qt.grad, Lt.grad, Ut.grad, At.grad)))
        if device != "cpu":
            flags.append(all(torch.is_tensor(v) and v.device == Qt.device
                             for v in (r.x, r.y, r.status_polish, layer.last_status_adjoint)))
        host = lambda v: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v)
        for name, v in (("X", X), ("Y", Y), ("dq", Qt.grad), ("dl", Lt.grad), ("du", Ut.grad), ("dAx", At.grad),
                        ("status_polish", r.status_polish), ("status_adjoint", layer.last_status_adjoint)):
            out["%s%d" % (name, k)] = host(v)
    layer.cleanup()
    return out, routes, flags


def main():
    n, m, B, seed = (int(v) for v in sys.argv[1:5])
    P, A, Q, L, U, _ = shape_family(n, m, B, seed)
    Ac = A.tocsc(); Ac.sort_indices()
    rng = np.random.default_rng(seed + 1)
    Ax = np.tile(Ac.data, (B, 1))
    calls = [(Q, L, U, Ax, True),
             (Q * rng.uniform(0.8, 1.2, Q.shape), np.roll(L, 1, axis=0) - 0.05, np.roll(U, 1, axis=0) + 0.07,
              Ax * rng.uniform(0.8, 1.25, Ax.shape), True),
             (Q * rng.uniform(0.8, 1.2, Q.shape), np.roll(L, 2, axis=0) - 0.03, np.roll(U, 2, axis=0) + 0.04,
              Ax * rng.uniform(0.8, 1.25, Ax.shape), False)]
    W = (rng.standard_normal((B, n)), rng.standard_normal((B, m)))
    res = {}
    routes, on_device = [], []
    for tag, device in (("dev", "cuda:0"), ("host", "cpu")):
        out, r, flags = run(device, P, A, calls, W)
        routes += r
        if tag == "dev":
            on_device = flags
        res.update({"%s_%s" % (tag, k): v for k, v in out.items()})
    res["routes"] = np.array(routes)
    res["outputs_on_device"] = np.array(all(on_device[0::2]))
    res["last_results_on_device"] = np.array(all(on_device[1::2]))
    np.savez(sys.argv[5], **res)


if __name__ == "__main__":
    main()
