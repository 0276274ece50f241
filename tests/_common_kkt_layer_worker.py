"""Worker of test_gpu_batch_common_kkt.test_layer and test_device_route: the torch parts run in a process of their own
(tests/_tangent_layer_worker.py says why), torch imported before the library.
usage: _common_kkt_layer_worker.py <host|dev> <in.npz> <out.npz>     (dev: also the device route of the calls)     in: W [B, n], dq [B, n], dl, du [B, m] (the tangents)"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import osqp_amd  # noqa: E402
from _common_kkt_reference import family  # noqa: E402

SHAPE = (17, 37, 4, 1054)
KW = dict(eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, polish=True)


def run(layer, where, Q, L, U, d, out, tag):
    t = lambda v, g=False: torch.tensor(v, dtype=torch.float64, device=where, requires_grad=g)
    Qt, Lt, Ut = t(Q, True), t(L, True), t(U, True)
    X = layer(Qt, Lt, Ut)
    (X * t(d["W"])).sum().backward()
    out.update({tag + "X": X.detach().cpu().numpy(), tag + "gQ": Qt.grad.cpu().numpy(), tag + "gL": Lt.grad.cpu().numpy(),
                tag + "gU": Ut.grad.cpu().numpy(), tag + "route": np.array([layer.last_route]),
                tag + "status_adjoint": np.asarray(torch.as_tensor(layer.last_status_adjoint).cpu().numpy()).astype(np.int64),
                tag + "status_polish": np.asarray(torch.as_tensor(layer.last_results.status_polish).cpu().numpy()).astype(np.int64)})
    with fwAD.dual_level():
        X2 = layer(fwAD.make_dual(t(Q), t(d["dq"])), fwAD.make_dual(t(L), t(d["dl"])), fwAD.make_dual(t(U), t(d["du"])))
        out[tag + "tX"] = fwAD.unpack_dual(X2).tangent.detach().cpu().numpy()


def main():
    mode = sys.argv[1]
    d = dict(np.load(sys.argv[2]))
    P, A, Q, L, U = family(SHAPE)
    out = {}
    for where, w in ((("cpu", "host_"),) if mode == "host" else (("cuda:0", "dev_"),)):
        for engine, e in (("common", "common_"), ("streamed", "streamed_")):
            layer = osqp_amd.BatchQPLayer(P, A, engine=engine, **(dict(KW, shared_kkt=True) if engine == "common" else KW))
            run(layer, where, Q, L, U, d, out, w + e)
            if engine == "common":
                # the two errors of the layer on this engine: matrix values; bounds whose row classes disagree
                t = lambda v: torch.tensor(v, dtype=torch.float64, device=where)
                try:
                    layer(t(Q), t(L), t(U), Ax=t(np.tile(A.tocsc().data, (Q.shape[0], 1))))
                    out[w + "px_error"] = np.array([""])
                except ValueError as e1:
                    out[w + "px_error"] = np.array([str(e1)])
                ct = layer.h.member_workspace(0)["ctype"]
                row = int(np.flatnonzero(ct == 0)[1])
                Lb, Ub = L.copy(), U.copy()
                Lb[2, row] = Ub[2, row] = 0.0
                try:
                    layer(t(Q), t(Lb), t(Ub))
                    out[w + "class_error"] = np.array([""])
                except RuntimeError as e2:
                    out[w + "class_error"] = np.array([str(e2)])
                out[w + "class_row"] = np.array([row])
            layer.cleanup()
    if mode == "host":
        np.savez(sys.argv[3], **out)
        return
    # host route against the device route of the calls themselves
    B = Q.shape[0]
    h = osqp_amd.BatchOSQP().setup(P, A, Q, L, U, engine="common", shared_kkt=True, **{k: v for k, v in KW.items() if k != "polish"})
    h.solve(fetch=False); h.polish(fetch=False)
    rng = np.random.default_rng(11)
    gx, gy = rng.standard_normal((B, 3, h.n)), rng.standard_normal((B, 3, h.m))
    a = h.adjoint(gx, gy, matrices=True)
    tn = h.tangent(dQ=d["dq"], dL=d["dl"], dU=d["du"])
    cu = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda:0")
    new = lambda *s, **k: torch.empty(s, device="cuda:0", **{"dtype": torch.float64, **k})
    g = dict(dq=new(B, 3, h.n), dl=new(B, 3, h.m), du=new(B, 3, h.m), dPx=new(B, 3, h.Pu.nnz), dAx=new(B, 3, h.Ah.nnz))
    act, st = new(B, h.m, dtype=torch.int32), new(B, dtype=torch.int32)
    dx, dy = new(B, h.n), new(B, h.m)
    ins = [cu(gx), cu(gy), cu(d["dq"]), cu(d["dl"]), cu(d["du"])]
    torch.cuda.synchronize()
    h.adjoint_into(ins[0], ins[1], active=act, status_adjoint=st, **g)
    h.tangent_into(dx, dy, dQ=ins[2], dL=ins[3], dU=ins[4])
    sp = new(B, dtype=torch.int32)
    h.results_into(status_polish=sp)
    same = all(np.array_equal(getattr(a, k), v.cpu().numpy()) for k, v in g.items())
    same = same and np.array_equal(a.active, act.cpu().numpy()) and np.array_equal(a.status_adjoint, st.cpu().numpy())
    same = same and np.array_equal(tn.dx, dx.cpu().numpy()) and np.array_equal(tn.dy, dy.cpu().numpy())
    out["routes_same"] = np.array(same)
    out["status_polish_dev"] = sp.cpu().numpy().astype(np.int64)
    out["status_polish_host"] = h.results().status_polish
    h.cleanup()
    np.savez(sys.argv[3], **out)


if __name__ == "__main__":
    main()
