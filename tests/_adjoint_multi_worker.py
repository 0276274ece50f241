"""Worker of test_gpu_batch_adjoint_multi.test_device_route: the torch part runs in a process of its own, because
importing torch maps torch's own copy of the HIP runtime and the other GPU tests of the suite must keep seeing the one
the library was loaded with (tests/_adjoint_layer_worker.py).  torch is imported before the library, so that both run
on one runtime and torch's allocations are device memory the library knows.
usage: _adjoint_multi_worker.py <n> <m> <B> <seed> <in.npz> <out.npz>"""
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
    d = np.load(sys.argv[5])
    dX, dY = d["dX"], d["dY"]
    D = dX.shape[1]
    P, A, Q, L, U, _ = shape_family(n, m, B, seed)
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="auto")
    h.solve(fetch=False)
    h.polish(fetch=False)
    a = h.adjoint(dX, dY, matrices=True)
    cu = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda:0")
    new = lambda *s, **k: torch.empty(s, device="cuda:0", **{"dtype": torch.float64, **k})
    out = dict(dq=new(B, D, n), dl=new(B, D, m), du=new(B, D, m), dPx=new(B, D, h.Pu.nnz), dAx=new(B, D, h.Ah.nnz),
               active=new(B, m, dtype=torch.int32), status_adjoint=new(B, dtype=torch.int32))
    gX, gY = cu(dX), cu(dY)
    torch.cuda.synchronize()
    h.adjoint_into(gX, gY, **out)
    res = {}
    for k, g in out.items():
        res["host_" + k] = np.asarray(getattr(a, k))
        res["dev_" + k] = g.cpu().numpy().astype(res["host_" + k].dtype)
    # dY = None is dY = 0, and the optional outputs may be left out
    dq2, dl2, du2 = new(B, D, n), new(B, D, m), new(B, D, m)
    h.adjoint_into(gX, None, dq2, dl2, du2)
    a2 = h.adjoint(dX, None)
    res.update(host_dq_noY=a2.dq, dev_dq_noY=dq2.cpu().numpy(), host_dl_noY=a2.dl, dev_dl_noY=dl2.cpu().numpy())
    raised = []
    for kw in (dict(dX=dX), dict(dq=np.zeros((B, D, n)))):      # a host array among the device arrays
        args = dict(dX=gX, dY=gY, dq=out["dq"], dl=out["dl"], du=out["du"])
        args.update(kw)
        try:
            h.adjoint_into(**args)
            raised.append(False)
        except ValueError:
            raised.append(True)
    try:                                                        # the outputs must carry the cotangents' D
        h.adjoint_into(gX, gY, new(B, D + 1, n), out["dl"], out["du"])
        raised.append(False)
    except ValueError:
        raised.append(True)
    res["raised"] = np.array(raised)
    res["kkt_info"] = np.array(h.kkt_info())
    h.cleanup()
    np.savez(sys.argv[6], **res)


if __name__ == "__main__":
    main()
