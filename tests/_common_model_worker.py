"""Worker of tests/test_gpu_batch_common_model.py: the torch parts run in a process of their own (tests/_common_device_worker.py
says why), torch imported before the library.
usage: _common_model_worker.py dev <out.npz>                      update_model through host arrays and through CUDA tensors
       _common_model_worker.py <host|cuda> <in.npz> <out.npz>     the layer with the shared model's values as inputs
                                                                  in: W [B, n], tP [nnzP], tA [nnzA] (the tangents)"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import osqp_amd  # noqa: E402
from _common_cases import ADAPTIVE  # noqa: E402
from _common_kkt_reference import family  # noqa: E402
from _common_model_cases import LAYER_SHAPE as SHAPE, bits_case, moved_model  # noqa: E402

KW = dict(eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, polish=True)
DEV_SHAPE = (33, 66, 5)


def state(h, tag, out):
    """Everything the handle holds that a test can read, under tag."""
    for b in (0, h.B - 1):
        for k, v in h.member_workspace(b).items():
            out["%s_ws%d_%s" % (tag, b, k)] = np.asarray(v)
    pk = h.shared_kkt_peek()
    out[tag + "_H"], out[tag + "_Wt"] = pk["H"], pk["Wt"]


def dev_route(path):
    c = bits_case(DEV_SHAPE, "full")
    Pu, A, Px, Ax, Q, L, U, B = c["P0"], c["A0"], c["Px"], c["Ax"], c["Q"], c["L"], c["U"], DEV_SHAPE[2]
    h = osqp_amd.BatchOSQP().setup(Pu, A, Q, L, U, engine="common", shared_kkt=True, **ADAPTIVE)
    d = osqp_amd.BatchOSQP().setup(Pu, A, Q, L, U, engine="common", shared_kkt=True, **ADAPTIVE)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    out = {}
    # full arrays, then an index subset of each matrix with values of its own, then a solve
    iP, iA = np.arange(0, Pu.nnz, 2), np.arange(1, A.nnz, 3)
    sP, sA = 1.1 * Px[iP], 0.9 * Ax[iA]
    tP, tA, tsP, tsA = dev(Px), dev(Ax), dev(sP), dev(sA)
    torch.cuda.synchronize()
    out["rc"] = np.array([h.update_model(Px=Px, Ax=Ax), d.update_model(Px=tP, Ax=tA)])
    state(h, "h_full", out); state(d, "d_full", out)
    out["rc_idx"] = np.array([h.update_model(Px=sP, Px_idx=iP, Ax=sA, Ax_idx=iA), d.update_model(Px=tsP, Px_idx=iP, Ax=tsA, Ax_idx=iA)])
    state(h, "h_idx", out); state(d, "d_idx", out)
    rh, rd = h.solve(), d.solve()
    for k in ("x", "y", "info_raw"):
        out["h_" + k], out["d_" + k] = getattr(rh, k), getattr(rd, k)
    # a host pointer where a device pointer belongs, and a [B, k] tensor
    bad = d._lib.osqp_amd_batch_common_update_model_dev(d._h, Px.ctypes.data, None, 0, None, None, 0)
    out["bad_pointer"] = np.array([bad])
    try:
        d.update_model(Px=dev(np.tile(Px, (B, 1))))
        out["two_d"] = np.array([""])
    except ValueError as e:
        out["two_d"] = np.array([str(e)])
    state(d, "d_after", out)
    h.cleanup(); d.cleanup()
    np.savez(path, **out)


def layer_route(where, d, path):
    P, A, Q, L, U = family(SHAPE)
    Pu, A, _, _, Px2, _ = moved_model(P, A, 77)
    # A moves by columns, A' = A diag(s): the family's feasible points, divided by s, stay feasible, so every member still
    # solves and X can be compared between the engines
    Ax2 = A.data * np.repeat(np.random.default_rng(78).uniform(0.5, 1.8, A.shape[1]), np.diff(A.indptr))
    B = Q.shape[0]
    t = lambda v, g=False: torch.tensor(v, dtype=torch.float64, device=where, requires_grad=g)
    W = t(d["W"])
    out = {}
    common = osqp_amd.BatchQPLayer(Pu, A, engine="common", shared_kkt=True, **KW)
    # call 0 sets the handle up on moved values; call 1 brings the layer's own back through update_model, with gradients
    out["c_X_moved"] = common(t(Q), t(L), t(U), Px=t(Px2), Ax=t(Ax2)).detach().cpu().numpy()
    h0, builds0 = common.h, common.h.kkt_info().builds
    Pt, At = t(Pu.data, True), t(A.data, True)
    X = common(t(Q), t(L), t(U), Px=Pt, Ax=At)
    out["same_handle"] = np.array([common.h is h0])
    out["builds"] = np.array([builds0, common.h.kkt_info().builds])
    (X * W).sum().backward()
    out.update(c_X=X.detach().cpu().numpy(), c_gP=Pt.grad.cpu().numpy(), c_gA=At.grad.cpu().numpy(), c_route=np.array([common.last_route]),
               c_status_adjoint=np.asarray(torch.as_tensor(common.last_status_adjoint).cpu().numpy()).astype(np.int64))
    with fwAD.dual_level():
        X2 = common(t(Q), t(L), t(U), Px=fwAD.make_dual(t(Pu.data), t(d["tP"])), Ax=fwAD.make_dual(t(A.data), t(d["tA"])))
        out["c_tX"] = fwAD.unpack_dual(X2).tangent.detach().cpu().numpy()
    # A alone moved, then nothing given: the values go back to the layer's own
    out["c_X_A"] = common(t(Q), t(L), t(U), Ax=t(Ax2)).detach().cpu().numpy()
    out["c_X_own"] = common(t(Q), t(L), t(U)).detach().cpu().numpy()
    out["same_handle_end"] = np.array([common.h is h0])
    # the errors that stay
    for key, kw, exc in (("per_member", dict(Ax=t(np.tile(A.data, (B, 1)))), ValueError), ("short", dict(Ax=t(A.data[:-1])), ValueError)):
        try:
            common(t(Q), t(L), t(U), **kw)
            out["err_" + key] = np.array([""])
        except exc as e:
            out["err_" + key] = np.array([str(e)])
    common.cleanup()
    streamed = osqp_amd.BatchQPLayer(Pu, A, engine="streamed", **KW)
    try:
        streamed(t(Q), t(L), t(U), Ax=t(A.data))
        out["err_streamed"] = np.array([""])
    except ValueError as e:
        out["err_streamed"] = np.array([str(e)])
    rows = lambda v: np.tile(v, (B, 1))
    out["s_X_moved"] = streamed(t(Q), t(L), t(U), Px=t(rows(Px2)), Ax=t(rows(Ax2))).detach().cpu().numpy()
    Pb, Ab = t(rows(Pu.data), True), t(rows(A.data), True)
    X = streamed(t(Q), t(L), t(U), Px=Pb, Ax=Ab)
    (X * W).sum().backward()
    out.update(s_X=X.detach().cpu().numpy(), s_gP=Pb.grad.cpu().numpy(), s_gA=Ab.grad.cpu().numpy())
    with fwAD.dual_level():
        X2 = streamed(t(Q), t(L), t(U), Px=fwAD.make_dual(t(rows(Pu.data)), t(rows(d["tP"]))),
                      Ax=fwAD.make_dual(t(rows(A.data)), t(rows(d["tA"]))))
        out["s_tX"] = fwAD.unpack_dual(X2).tangent.detach().cpu().numpy()
    out["s_X_A"] = streamed(t(Q), t(L), t(U), Ax=t(rows(Ax2))).detach().cpu().numpy()
    streamed.cleanup()
    np.savez(path, **out)


if __name__ == "__main__":
    if sys.argv[1] == "dev":
        dev_route(sys.argv[2])
    else:
        layer_route("cpu" if sys.argv[1] == "host" else "cuda:0", dict(np.load(sys.argv[2])), sys.argv[3])
