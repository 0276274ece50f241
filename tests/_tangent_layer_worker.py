"""Worker of test_gpu_batch_tangent.test_layer and test_device_route: the torch parts run in a process of their own,
because importing torch maps torch's own copy of the HIP runtime and the other GPU tests of the suite must keep
seeing the one the library was loaded with (tests/_adjoint_layer_worker.py).  torch is imported before the library, so
that both run on one runtime and torch's allocations are device memory the library knows.
usage: _tangent_layer_worker.py <host|device> <n> <m> <B> <seed> <in.npz> <out.npz>"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import osqp_amd  # noqa: E402
from _batch_parity import shape_family  # noqa: E402


def layer_tangents(layer, device, Q, L, U, Ax, d, names=("dq", "dl", "du", "dAx")):
    """One forward pass under forward_ad: the inputs named carry the draws' tangents, the others none.  Returns X, Y and
    their tangents as numpy arrays, and whether all four live on `device`."""
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=device)
    with fwAD.dual_level():
        dual = lambda v, k: fwAD.make_dual(t(v), t(d[k])) if k in names else t(v)
        X, Y = layer(dual(Q, "dq"), dual(L, "dl"), dual(U, "du"), Ax=dual(Ax, "dAx"), return_y=True)
        (X, tX), (Y, tY) = fwAD.unpack_dual(X), fwAD.unpack_dual(Y)
        assert tX is not None and tY is not None
        there = all(v.device == torch.device(device) for v in (X, Y, tX, tY))
        return [v.detach().cpu().numpy() for v in (X, Y, tX, tY)] + [there]


def host(P, A, Q, L, U, Ax, d, out):
    layer = osqp_amd.BatchQPLayer(P, A, engine="auto")
    X, Y, tX, tY, _ = layer_tangents(layer, "cpu", Q, L, U, Ax, d)
    out.update(X=X, Y=Y, tX=tX, tY=tY, status_polish=layer.last_results.status_polish,
               status_tangent=layer.last_status_tangent, route=np.array([layer.last_route]))
    out["tX_q"] = layer_tangents(layer, "cpu", Q, L, U, Ax, d, names=("dq",))[2]     # the others count as zero
    # backward mode in the same process, as tests/_adjoint_layer_worker.py runs it
    t = lambda v, g=True: torch.tensor(v, dtype=torch.float64, requires_grad=g)
    Qt = t(Q)
    X2 = layer(Qt, t(L), t(U), Ax=t(Ax))
    (X2 * torch.tensor(d["W"])).sum().backward()
    out["dq"] = Qt.grad.numpy()
    layer.cleanup()


def device(P, A, Q, L, U, Ax, d, out):
    B = Q.shape[0]
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="auto")
    h.solve(fetch=False)
    h.polish(fetch=False)
    kw = dict(dQ=d["dq"], dL=d["dl"], dU=d["du"], dPx=d["dPx"], dAx=d["dAx"])
    rng = np.random.default_rng(5)
    kw3 = {k: np.concatenate([v[:, None, :], rng.standard_normal((B, 2, v.shape[1]))], axis=1) for k, v in kw.items()}
    cu = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda:0")
    new = lambda *s, **k: torch.empty(s, device="cuda:0", **{"dtype": torch.float64, **k})
    t1, t3 = h.tangent(**kw), h.tangent(**kw3)
    dx, dy, act, st = new(B, h.n), new(B, h.m), new(B, h.m, dtype=torch.int32), new(B, dtype=torch.int32)
    dx3, dy3 = new(B, 3, h.n), new(B, 3, h.m)
    dev1, dev3 = {k: cu(v) for k, v in kw.items()}, {k: cu(v) for k, v in kw3.items()}
    torch.cuda.synchronize()
    h.tangent_into(dx, dy, active=act, status_tangent=st, **dev1)
    h.tangent_into(dx3, dy3, **dev3)
    for k, a, g in (("dx", t1.dx, dx), ("dy", t1.dy, dy), ("active", t1.active, act), ("status_tangent", t1.status_tangent, st),
                    ("dx3", t3.dx, dx3), ("dy3", t3.dy, dy3)):
        out["host_" + k] = np.asarray(a)
        out["dev_" + k] = g.cpu().numpy().astype(np.asarray(a).dtype)
    h.cleanup()
    routes = []
    for tag, where in (("dev", "cuda:0"), ("host", "cpu")):
        layer = osqp_amd.BatchQPLayer(P, A, engine="auto")
        _, _, tX, tY, there = layer_tangents(layer, where, Q, L, U, Ax, d)
        routes.append(layer.last_route)
        st = layer.last_status_tangent
        if tag == "dev":
            out["on_device"] = np.array(there and torch.is_tensor(st) and st.device == torch.device(where))
        out.update({"layer_%s_tX" % tag: tX, "layer_%s_tY" % tag: tY,
                    "layer_%s_status_tangent" % tag: np.asarray(st.cpu().numpy() if torch.is_tensor(st) else st).astype(np.int64)})
        layer.cleanup()
    out["routes"] = np.array(routes)


def main():
    mode = sys.argv[1]
    n, m, B, seed = (int(v) for v in sys.argv[2:6])
    d = dict(np.load(sys.argv[6]))
    P, A, Q, L, U, _ = shape_family(n, m, B, seed)
    Ac = A.tocsc(); Ac.sort_indices()
    out = {}
    (host if mode == "host" else device)(P, A, Q, L, U, np.tile(Ac.data, (B, 1)), d, out)
    np.savez(sys.argv[7], **out)


if __name__ == "__main__":
    main()
