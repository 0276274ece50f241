"""Time of the calls around the batch solve whose host, device and member forms share one body (update, warm_start,
get, adjoint, tangent, and the layers over them), this tree against a built checkout of the parent commit, by the rule of tools/batch_limits_time.py: the two trees
alternate repetition by repetition on one device, one process per repetition, and this tree's median of each figure
has to lie inside the parent's own min-max range.  The figures, each the median over --steps timed steps of a
repetition after two untimed ones:
  batch leg of bench.py        warm_start.ms_update and warm_start.ms_solve as the tree's own bench.py --full reports
                               them (config 4, 1024 x n = 120, m = 240, tiled engine: update(Q, L, U) from the host and
                               the warm-started solve that follows; means over its 5 steps), one run per repetition;
  tools/batch_device_io_time   one MPC step, update -> solve -> results, from host arrays and from device arrays, on
                               config 4 and on the streamed engine at n = 300, m = 600;
  tools/batch_members_time     on the common-K engine at n = 300, m = 600 with its shared KKT pieces: update(Q) of the
                               whole batch and update(Q, members=S), |S| = 16;
  the derivative calls         on config 4 after a solve: adjoint from host arrays and adjoint_into on device arrays,
                               tangent and tangent_into (one cotangent, one direction per member);
  the layers                   (a process of their own, which imports torch first) one BatchQPLayer step on config 4
                               -- forward, then backward of X.sum() -- on CPU tensors and on CUDA tensors, and one
                               QPLayer step on the `pad` member tests/_single_layer_worker.py uses, on CPU tensors.
usage: python tools/batch_call_forms_time.py --parent-tree DIR [--reps 9] [--steps 10] [--B 1024] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(call):
    t0 = time.perf_counter()
    call()                                # returns with the handle's stream synchronised
    return time.perf_counter() - t0


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    from osqp_amd.problems import mpc_batch
    sys.path.insert(0, ROOT)
    from tools.batch_common_time import problem as common_problem
    from tools.batch_device_io_time import Dev
    from tools.batch_members_time import subset
    from tools.batch_streamed_time import problem as streamed_problem
    import tools.batch_device_io_time as dio
    out, B, steps = {}, a.B, a.steps + 2
    med = lambda v: statistics.median(v[2:])
    rng = np.random.default_rng(0)
    s, Q, L, U = mpc_batch(batch=B)
    osqp_amd.lib()
    dio.HIP = C.CDLL("libamdhip64.so")    # after the library: the runtime the handles run on
    dio.HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    dio.HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    # one MPC step from host arrays and from device arrays
    for name, engine, pb in (("tiled, config 4", "auto", (s["P"], s["A"], Q, L, U)),
                             ("streamed, n=300", "streamed", tuple(streamed_problem(300, 600, B, seed=300))[:5])):
        P, A, Q1, L1, U1 = pb
        hs = [osqp_amd.BatchOSQP().setup(P, A, Q1, L1, U1, engine=engine) for _ in range(2)]
        for h in hs:
            h.solve(fetch=False)
        data = [(Q1 * (1 + 0.03 * rng.standard_normal(Q1.shape)), L1 - 0.01 * rng.random(L1.shape), U1 + 0.01 * rng.random(U1.shape))
                for _ in range(steps)]
        ddata = [tuple(Dev(v.shape, init=v) for v in d) for d in data]
        X, Y, I = Dev((B, hs[0].n)), Dev((B, hs[0].m)), Dev((B, 8))

        def host_step(k):
            assert hs[0].update(*data[k]) == 0
            hs[0].solve()

        def device_step(k):
            assert hs[1].update(*ddata[k]) == 0
            hs[1].solve(fetch=False)
            hs[1].results_into(X=X, Y=Y, info=I)
        th, td = [], []
        for k in range(steps):
            th.append(timed(lambda: host_step(k)))
            td.append(timed(lambda: device_step(k)))
        out["step, host arrays (%s)" % name], out["step, device arrays (%s)" % name] = med(th), med(td)
        if engine == "auto":                  # the derivative calls on the point the last step left
            n, m = hs[0].n, hs[0].m
            gX, gY, tQ = rng.standard_normal((B, n)), rng.standard_normal((B, m)), rng.standard_normal((B, n))
            d = {k: Dev((B, c)) for k, c in dict(dq=n, dl=m, du=m, dx=n, dy=m).items()}
            dgX, dgY, dtQ, st = Dev(gX.shape, init=gX), Dev(gY.shape, init=gY), Dev(tQ.shape, init=tQ), Dev((B,), np.int32)
            for label, call in (
                    ("adjoint, host arrays", lambda: hs[0].adjoint(gX, gY)),
                    ("adjoint_into, device arrays", lambda: hs[1].adjoint_into(dgX, dgY, d["dq"], d["dl"], d["du"], status_adjoint=st)),
                    ("tangent, host arrays", lambda: hs[0].tangent(dQ=tQ)),
                    ("tangent_into, device arrays", lambda: hs[1].tangent_into(d["dx"], d["dy"], dQ=dtQ, status_tangent=st))):
                out["%s (%s)" % (label, name)] = med([timed(call) for _ in range(steps)])
        for h in hs:
            h.cleanup()
    # the common-K engine: update of everybody and of 16 members
    P, A, Q2, L2, U2 = tuple(common_problem(300, 600, B, seed=300))[:5]
    h = osqp_amd.BatchOSQP().setup(P, A, Q2, L2, U2, engine="common", shared_kkt=True)
    h.solve(fetch=False)
    S = subset(16) if B == 1024 else np.arange(0, B, max(B // 16, 1))[:16]
    tw, tm = [], []
    for r in range(steps):
        Qr = Q2 * (1.0 + 0.01 * (r + 1))
        tw.append(timed(lambda: h.update(Q=Qr)))
        rows = Q2[S] * (1.0 + 0.02 * (r + 1) * (-1) ** r)
        tm.append(timed(lambda: h.update(Q=rows, members=S)))
    out["update (whole), common-K"], out["update_members, |S| = 16, common-K"] = med(tw), med(tm)
    h.cleanup()
    print("JSON " + json.dumps(out))


def layers_leg(a):
    import torch                          # before the library is first loaded (osqp_amd/layer.py says why)
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import osqp_amd
    from osqp_amd.problems import mpc_batch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _planted_qp as pq
    from _single_sens_reference import member_qp
    out, B, steps = {}, a.B, a.steps + 2
    med = lambda v: statistics.median(v[2:])
    rng = np.random.default_rng(0)
    s, Q, L, U = mpc_batch(batch=B)
    data = [(Q * (1 + 0.03 * rng.standard_normal(Q.shape)), L - 0.01 * rng.random(L.shape), U + 0.01 * rng.random(U.shape))
            for _ in range(steps)]
    for route, device in (("host", "cpu"), ("device", "cuda")):
        layer = osqp_amd.BatchQPLayer(s["P"], s["A"])
        tensors = [tuple(torch.tensor(v, dtype=torch.float64, device=device, requires_grad=k == 0) for k, v in enumerate(d))
                   for d in data]

        def step(k):
            layer(*tensors[k]).sum().backward()
            if device == "cuda":
                torch.cuda.synchronize()
        out["BatchQPLayer step, %s route (tiled, config 4)" % route] = med([timed(lambda: step(k)) for k in range(steps)])
        assert layer.last_route == route and tensors[-1][0].grad is not None
        layer.cleanup()
    pb = member_qp(pq.case("pad"), 1)
    layer = osqp_amd.QPLayer(pb["P"], pb["A"])
    tensors = [tuple(torch.tensor(v * (1 + 0.01 * k) if j == 0 else v, dtype=torch.float64, requires_grad=j == 0)
                     for j, v in enumerate((pb["q"], pb["l"], pb["u"]))) for k in range(steps)]
    out["QPLayer step, CPU tensors (pad member)"] = med([timed(lambda: layer(*tensors[k]).sum().backward()) for k in range(steps)])
    layer.cleanup()
    print("JSON " + json.dumps(out))


def bench_leg(tree):
    """warm_start.ms_update / ms_solve of the batch leg of the tree's bench.py, in seconds."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1", "--full", "--no-cpu", "--no-configs",
           "--no-inexact"]
    p = subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, cwd=tree)
    ws = json.loads(p.stdout.strip().splitlines()[-1])["batch"]["warm_start"]
    return {"bench.py batch leg: warm_start.ms_update": 1e-3 * ws["ms_update"],
            "bench.py batch leg: warm_start.ms_solve": 1e-3 * ws["ms_solve"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--out", help="write the table here too")
    ap.add_argument("--leg", choices=("calls", "layers"), help="run one repetition in this process (what the tool starts itself)")
    ap.add_argument("--tree", help="with --leg: the tree to import osqp_amd from (default: this one)")
    a = ap.parse_args()
    if a.leg:
        return leg(a) if a.leg == "calls" else layers_leg(a)
    if not a.parent_tree:
        sys.exit("--parent-tree DIR is needed: the figures are judged against the parent's own range")
    base = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--B", str(a.B)]
    got = {"parent": [], "this": []}
    for rep in range(a.reps):
        for title, args in (("parent", ["--tree", a.parent_tree]), ("this", [])):
            figures = bench_leg(os.path.abspath(a.parent_tree) if title == "parent" else ROOT)
            for which in ("calls", "layers"):
                p = subprocess.run(base + ["--leg", which] + args, check=True, timeout=600, stdout=subprocess.PIPE, text=True)
                figures.update(json.loads([l for l in p.stdout.splitlines() if l.startswith("JSON ")][-1][5:]))
            got[title].append(figures)
            print("repetition %d, %s: done" % (rep + 1, title), file=sys.stderr, flush=True)
    ms = lambda v: "median %9.3f ms (min %.3f, max %.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
    lines = ["B = %d; %d repetitions per tree, alternating, one process each; per repetition the median of %d steps after two "
             "warm-up steps" % (a.B, a.reps, a.steps)]
    for name in got["this"][0]:
        pv, tv = [r[name] for r in got["parent"]], [r[name] for r in got["this"]]
        lines.append(name + ":")
        lines.append("  parent %s" % ms(pv))
        lines.append("  this   %s  -> median %s the parent's range"
                     % (ms(tv), "inside" if min(pv) <= statistics.median(tv) <= max(pv) else "OUTSIDE"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
