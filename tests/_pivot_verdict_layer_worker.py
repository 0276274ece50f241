"""Worker of test_gpu_batch_pivot_verdict.test_layer: BatchQPLayer on the case "wrongpivot" of tests/_planted_qp.py, one
backward pass on CPU tensors per engine.  In a process of its own for the reason tests/_adjoint_layer_worker.py gives;
torch is imported before the library.
usage: _pivot_verdict_layer_worker.py <out.npz>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import osqp_amd  # noqa: E402
import _planted_qp as pq  # noqa: E402


def main():
    c = pq.case("wrongpivot")
    i = c.inc
    out = {}
    for engine in pq.ENGINES["wrongpivot"]:
        layer = osqp_amd.BatchQPLayer(c.P, c.A, engine=engine, **c.settings)
        t = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)
        Q, L, U, Px, Ax = t(c.Q), t(c.L), t(c.U), t(c.Px_all), t(c.Ax_all)
        X, Y = layer(Q, L, U, Px=Px, Ax=Ax, return_y=True)
        ((X * torch.tensor(i.gx)).sum() + (Y * torch.tensor(i.gy)).sum()).backward()
        assert layer.last_route == "host" and layer.h.shape()[0] == (1 if engine == "streamed" else 0)
        r = layer.last_results
        for k, v in dict(X=X.detach().numpy(), Y=Y.detach().numpy(), dq=Q.grad.numpy(), dl=L.grad.numpy(), du=U.grad.numpy(),
                         dPx=Px.grad.numpy(), dAx=Ax.grad.numpy(), status_val=r.status_val, status_polish=r.status_polish,
                         status_adjoint=layer.last_status_adjoint).items():
            out[engine + "_" + k] = np.asarray(v)
        layer.cleanup()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
