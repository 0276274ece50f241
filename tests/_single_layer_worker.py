"""Worker of test_gpu_single_sens.test_layer: osqp_amd.QPLayer runs in a process of its own, because importing torch
maps torch's own copy of the HIP runtime and the other GPU tests of the suite must keep seeing the one the library was
loaded with (tests/_adjoint_layer_worker.py).  torch is imported before the library, as bench.py does.
For each device (cpu, cuda): a backward pass through a fresh layer and forward_ad tangents through another fresh layer
(a second call on one layer would warm-start, and its polished point would differ in the last bits), beside
adjoint() / tangent() of a plain handle on the same member of the planted case.
usage: _single_layer_worker.py <case> <member> <out.npz>"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import osqp_amd  # noqa: E402
import _planted_qp as pq  # noqa: E402
from _single_sens_reference import member_qp  # noqa: E402


def main():
    c, b = pq.case(sys.argv[1]), int(sys.argv[2])
    pb, inc = member_qp(c, b), pq.member_inc(c, b)
    h = osqp_amd.OSQP().setup(**pb, polish=1)
    r = h.solve()
    a = h.adjoint(inc.gx, inc.gy, matrices=True)
    t = h.tangent(inc.dQ[0], inc.dL[0], inc.dU[0], inc.dPx[0], inc.dAx[0])
    out = dict(x=r.x, y=r.y, dq=a.dq, dl=a.dl, du=a.du, dPx=a.dPx, dAx=a.dAx, dx=t.dx, dy=t.dy,
               status=np.array([r.info.status_val, r.info.status_polish, a.status_adjoint, t.status_tangent]))
    h.cleanup()
    data = (pb["q"], pb["l"], pb["u"], pb["P"].data, pb["A"].data)
    for dev in ("cpu", "cuda"):
        T = lambda v, g=False: torch.tensor(np.asarray(v), dtype=torch.float64, device=dev, requires_grad=g)
        layer = osqp_amd.QPLayer(pb["P"], pb["A"])
        ins = [T(v, True) for v in data]
        x, y = layer(ins[0], ins[1], ins[2], Px=ins[3], Ax=ins[4], return_y=True)
        assert x.device.type == dev and y.device.type == dev and x.dtype == torch.float64
        ((x * T(inc.gx)).sum() + (y * T(inc.gy)).sum()).backward()
        for k, v in zip(("dq", "dl", "du", "dPx", "dAx"), ins):
            assert v.grad.device.type == dev
            out["%s_%s" % (dev, k)] = v.grad.cpu().numpy()
        out["%s_x" % dev] = x.detach().cpu().numpy(); out["%s_y" % dev] = y.detach().cpu().numpy()
        out["%s_status" % dev] = np.array([layer.last_results.info.status_polish, layer.last_status_adjoint])
        # only q asks for a gradient: the others get none, and the matrix gradients are not computed
        q2 = T(data[0], True)
        x2 = layer(q2, T(data[1]), T(data[2]))
        (x2 * T(inc.gx)).sum().backward()
        out["%s_q_only" % dev] = np.array(q2.grad is not None and tuple(q2.grad.shape) == (c.n,))
        layer.cleanup()
        layer = osqp_amd.QPLayer(pb["P"], pb["A"])
        with fwAD.dual_level():
            duals = [fwAD.make_dual(T(v), T(tv)) for v, tv in zip(data, (inc.dQ[0], inc.dL[0], inc.dU[0], inc.dPx[0], inc.dAx[0]))]
            xd, yd = layer(duals[0], duals[1], duals[2], Px=duals[3], Ax=duals[4], return_y=True)
            tx, ty = fwAD.unpack_dual(xd).tangent, fwAD.unpack_dual(yd).tangent
            assert tx.device.type == dev and ty.device.type == dev
            out["%s_dx" % dev] = tx.cpu().numpy(); out["%s_dy" % dev] = ty.cpu().numpy()
        out["%s_status_tangent" % dev] = np.array(layer.last_status_tangent)
        layer.cleanup()
    np.savez(sys.argv[3], **out)


if __name__ == "__main__":
    main()
