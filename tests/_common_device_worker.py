"""Worker of test_gpu_batch_common.test_device_route_equals_host_route: two common-K handles set up from the same data,
one driven through host arrays, one through torch CUDA tensors.  In a process of its own, because importing torch maps
torch's own copy of the HIP runtime and the other GPU tests of the suite must keep seeing the one the library was loaded
with; torch is imported before the library, so that both run on one runtime.
usage: _common_device_worker.py <out.npz>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import osqp_amd  # noqa: E402
from _common_cases import FIXED, common_family  # noqa: E402


def main(out):
    n, m, B = 33, 66, 5
    P, A, Q, L, U, X0 = common_family(n, m, B, 1000 + n + m)
    rng = np.random.default_rng(5)
    Q2 = Q * 1.3 + 0.1 * rng.standard_normal(Q.shape)
    fin = np.isfinite(L) & np.isfinite(U) & (U > L)
    L2 = np.where(fin, L - 0.2, L); U2 = np.where(fin, U + 0.1, U)
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **FIXED)
    d = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", **FIXED)
    h.solve(); d.solve(fetch=False)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    Xw = X0 + 0.01; Yw = 0.1 * np.ones((B, m))
    tq, tl, tu, tx, ty = dev(Q2), dev(L2), dev(U2), dev(Xw), dev(Yw)
    torch.cuda.synchronize()
    assert h.update(Q=Q2, L=L2, U=U2) == 0 and d.update(Q=tq, L=tl, U=tu) == 0
    assert h.warm_start(X=Xw, Y=Yw) == 0 and d.warm_start(X=tx, Y=ty) == 0
    rh = h.solve(); d.solve(fetch=False)
    X = torch.empty((B, n), dtype=torch.float64, device="cuda"); Y = torch.empty((B, m), dtype=torch.float64, device="cuda")
    I = torch.empty((B, 8), dtype=torch.float64, device="cuda")
    d.results_into(X=X, Y=Y, info=I)
    res = dict(h_x=rh.x, h_y=rh.y, h_info=rh.info_raw, d_x=X.cpu().numpy(), d_y=Y.cpu().numpy(), d_info=I.cpu().numpy())
    # one member's row would change its class: the device update is refused and writes nothing
    ct = h.member_workspace(0)["ctype"]
    row = int(np.flatnonzero((ct == 0) & np.isfinite(L2[1]) & np.isfinite(U2[1]))[0])
    Lb, Ub = L2.copy(), U2.copy()
    Lb[1, row] = Ub[1, row] = 0.5 * (L2[1, row] + U2[1, row])
    tl2, tu2 = dev(Lb), dev(Ub)
    torch.cuda.synchronize()
    res["refused"] = d.update(L=tl2, U=tu2)
    d.solve(fetch=False); rh2 = h.solve()
    d.results_into(X=X, info=I)
    res.update(h_x2=rh2.x, h_info2=rh2.info_raw, d_x2=X.cpu().numpy(), d_info2=I.cpu().numpy())
    h.cleanup(); d.cleanup()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
