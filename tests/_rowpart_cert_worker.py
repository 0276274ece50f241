"""One rank of the infeasibility and live-handle tests of the row-partitioned solve (started by tests/test_rowpart_infeasible.py through
osqp_amd.launch.spawn_ranks; world = 1 runs without a spawn through run()).  usage: _rowpart_cert_worker.py <out.npz>
Every problem of tests/_rowpart_cert_reference.py and its update sequence are solved in this one process group by RowPartitionedOSQP with
scipy SpMVs; <out.npz> holds <name>/<field> entries, among them `ranks_equal`: every rank's status, iteration count, solution and
certificates compared with rank 0's bit for bit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

STATUS = ("solved", "solved inaccurate", "maximum iterations reached", "primal infeasible", "primal infeasible inaccurate",
          "dual infeasible", "dual infeasible inaccurate")


def record(r):
    i = r.info
    return np.concatenate([np.array([i.iter, i.rho_updates, STATUS.index(i.status), i.obj_val, i.pri_res, i.dua_res], dtype=np.float64),
                           *(np.asarray(v, dtype=np.float64) for v in (r.x, r.y, r.prim_inf_cert, r.dual_inf_cert))])


def ranks_equal(rec):
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
        return True
    mine = torch.from_numpy(np.ascontiguousarray(rec, dtype=np.float64).view(np.int64).copy())
    every = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(every, mine)
    return all(bool(torch.equal(t, every[0])) for t in every)


def fields(r, pre):
    i = r.info
    return {pre + k: v for k, v in dict(x=r.x, y=r.y, prim_inf_cert=r.prim_inf_cert, dual_inf_cert=r.dual_inf_cert, status=i.status, iter=i.iter,
                                        obj=i.obj_val, rho_updates=i.rho_updates, ranks_equal=ranks_equal(record(r))).items()}


def run(make):
    """make(scaled, **settings) -> a set-up solver of this rank.  Returns the dict of results."""
    import oracle.oracle as orc
    import _rowpart_cert_reference as CR
    from osqp_amd import rowpart
    res = {}
    scaled_of = lambda pb: rowpart.scaled_problem_from_handle(orc.OracleOSQP().setup(**pb))
    for name in CR.SOLVE_NAMES:
        pb, kw = CR.solve_problem(name)
        scaled = scaled_of(pb)
        s = make(scaled, **kw)
        c0 = s.collectives
        r = s.solve()
        res.update(fields(r, name + "/"))
        res[name + "/collectives"] = r.info.collectives - c0
        res[name + "/rows"] = np.array(s.rows)
        res[name + "/iterates_zero"] = not any(bool(v.any()) for v in (s.x, s.xt, s.z, s.y))
        # the same iterations with the tests off
        s = make(scaled, **dict(CR.off(kw), max_iter=r.info.iter))
        c0 = s.collectives
        ro = s.solve()
        res[name + "/collectives_off"] = ro.info.collectives - c0
        res[name + "/iter_off"] = ro.info.iter
        if name == "feasible":
            res[name + "/same_bits_off"] = bool(np.array_equal(ro.x, r.x) and np.array_equal(ro.y, r.y))
    # the update sequence; then the same without the refused bounds: the next solve must be bit-equal
    pb, kw, steps = CR.sequence()
    for label, skip_bad in (("seq", False), ("seq_clean", True)):
        s = make(scaled_of(pb), **kw)
        k = 0
        for j, (call, args) in enumerate(steps):
            if skip_bad and j == 1:
                continue
            out = getattr(s, call)(**args)
            if call == "solve":
                res.update(fields(out, "%s/%d/" % (label, k)))
                k += 1
            else:
                res["%s/rc%d" % (label, j)] = int(out)
        res[label + "/solves"] = k
    return res


if __name__ == "__main__":
    import torch.distributed as dist
    from osqp_amd import rowpart
    dist.init_process_group("gloo")
    res = run(lambda scaled, **kw: rowpart.RowPartitionedOSQP().setup(scaled, rowpart.ScipyOps, **kw))
    res["world"] = dist.get_world_size()
    if dist.get_rank() == 0:
        np.savez(sys.argv[1], **res)
    dist.barrier()
    dist.destroy_process_group()
