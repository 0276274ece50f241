"""One rank of the row-partitioned solve (started by tests/test_rowpart.py through osqp_amd.launch.spawn_ranks).
usage: _rowpart_worker.py <cpu|gpu|native> <problem> <out.npz>   (native: the loop driven from C, osqp_amd_rp_solve; the gloo group as its collective)
<problem> = list:<name>,<name>,...: the named edge problems of tests/_rowpart_reference.py, all solved in this one process group (torch's
start-up is the cost, not the solves); <out.npz> then holds <name>/<field> entries, among them `ranks_equal`: every rank's x and info
record compared with rank 0's bit for bit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.distributed as dist

mode, which, out = sys.argv[1], sys.argv[2], sys.argv[3]
dist.init_process_group("gloo")
from osqp_amd.problems import portfolio_qp, random_sparse_qp
from osqp_amd import rowpart

STATUS_CODE = {"solved": 1, "solved inaccurate": 2, "maximum iterations reached": -2}


def solve_one(pb, kw):
    if mode == "cpu":     # CPU rehearsal of the collective logic: scipy SpMVs, scaling taken from the oracle's workspace (test infrastructure)
        import oracle.oracle as orc
        so = orc.OracleOSQP().setup(**pb)
        scaled = rowpart.scaled_problem_from_handle(so)
        ops = rowpart.ScipyOps
    else:
        scaled = rowpart.scaled_problem_from_engine(**pb)
        ops = rowpart.HipOps
    if mode == "native":
        s = rowpart.NativeRowPartitionedOSQP(collective="group").setup(scaled, device=0, **kw)
        r = s.solve()
        s.cleanup()
    else:
        s = rowpart.RowPartitionedOSQP().setup(scaled, ops, device=0, **kw)
        r = s.solve()
    return r, s.rows


def fields(r):
    return dict(x=r.x, y=r.y, iter=r.info.iter, status=r.info.status, obj=r.info.obj_val, rho_updates=r.info.rho_updates,
                pcg_iters=r.info.pcg_iters, collectives=r.info.collectives, world=dist.get_world_size())


def ranks_equal(r):
    """Every rank's x and info record against rank 0's, bit for bit (the bits travel as int64)."""
    i = r.info
    rec = np.concatenate([np.array([i.iter, i.rho_updates, STATUS_CODE[i.status], i.pcg_iters, i.obj_val, i.pri_res, i.dua_res, i.rho_estimate],
                                   dtype=np.float64), np.asarray(r.x, dtype=np.float64), np.asarray(r.y, dtype=np.float64)])
    mine = torch.from_numpy(rec.view(np.int64).copy())
    every = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(every, mine)
    return all(bool(torch.equal(t, every[0])) for t in every)


if which.startswith("list:"):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _rowpart_reference as R
    res = {}
    for name in which[5:].split(","):
        r, rows = solve_one(R.edge_problem(name), R.EDGE_SETTINGS)
        same = ranks_equal(r)
        for k, v in fields(r).items():
            res[name + "/" + k] = v
        res[name + "/ranks_equal"] = same
        res[name + "/rows"] = np.array(rows)
    if dist.get_rank() == 0:
        np.savez(out, **res)
else:
    if which == "portfolio_small":
        pb, kw = portfolio_qp(8, 25, sector_rows=5, seed=3), dict(eps_abs=1e-5, eps_rel=1e-5)
    elif which == "random":
        pb, kw = random_sparse_qp(300, 600, seed=5), {}
    else:
        pb, kw = portfolio_qp(), dict(eps_abs=1e-4, eps_rel=1e-4, adaptive_rho_interval=100)
    r, _ = solve_one(pb, kw)
    if dist.get_rank() == 0:
        np.savez(out, **fields(r))
dist.barrier()
dist.destroy_process_group()
