"""Worker of test_gpu_batch_adjoint.test_layer: the BatchQPLayer part runs in a process of its own, because importing
torch maps torch's own copy of the HIP runtime and the other GPU tests of the suite must keep seeing the one the
library was loaded with.  torch is imported before the library, as bench.py does.
usage: _adjoint_layer_worker.py <n> <m> <B> <seed> <incoming.npy> <out.npz>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import osqp_amd  # noqa: E402
from _batch_parity import shape_family  # noqa: E402


def main():
    n, m, B, seed = (int(v) for v in sys.argv[1:5])
    W = np.load(sys.argv[5])
    P, A, Q, L, U, _ = shape_family(n, m, B, seed)
    Ac = A.tocsc(); Ac.sort_indices()
    layer = osqp_amd.BatchQPLayer(P, A, engine="auto")
    t = lambda v, g=True: torch.tensor(v, dtype=torch.float64, requires_grad=g)
    Qt, Lt, Ut, At = t(Q), t(L), t(U), t(np.tile(Ac.data, (B, 1)))
    X = layer(Qt, Lt, Ut, Ax=At)
    assert X.shape == (B, n) and X.dtype == torch.float64
    (X * torch.tensor(W)).sum().backward()
    out = dict(X=X.detach().numpy(), dq=Qt.grad.numpy(), dl=Lt.grad.numpy(), du=Ut.grad.numpy(), dAx=At.grad.numpy(),
               status_polish=layer.last_results.status_polish, status_adjoint=layer.last_status_adjoint)
    # a second call on the live handle: the layer's own A again, only Q asks for a gradient, Y is returned too
    Q2, L2, U2 = t(Q), t(L, False), t(U, False)
    X2, Y2 = layer(Q2, L2, U2, return_y=True)
    (X2 * torch.tensor(W)).sum().backward()
    out.update(X2=X2.detach().numpy(), Y2=Y2.detach().numpy(), dq2=Q2.grad.numpy(),
               others_none=np.array(L2.grad is None and U2.grad is None))
    raised = []
    for exc, args in ((TypeError, (Q2.float(), L2, U2)), (ValueError, (Q2[:, :-1], L2, U2))):
        try:
            layer(*args)
            raised.append(False)
        except exc:
            raised.append(True)
    out["raised"] = np.array(raised)
    layer.cleanup()
    np.savez(sys.argv[6], **out)


if __name__ == "__main__":
    main()
