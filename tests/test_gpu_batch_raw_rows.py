"""GPU test of what osqp_amd_batch_update leaves in the handle's raw q, l, u, in each of its four forms -- whole batch
or members=, host arrays or device arrays -- on the tiled, the streamed and the common-K engine.

Four handles of one problem, none of them solved, take the same new data by one form each, then one shared matrix
update (update_matrices; update_model on the common-K engine) and one solve.  The matrix update recomputes the scaling
and every member's scaled q, l, u from the raw rows, so a wrong raw row shows in the solve, and which call wrote a
member's scaled row before does not matter.  The four results are equal to the bit, and every member meets the oracle
set up on the new data and the new values at the bars of tests/_batch_parity.py (tests/test_batch_raw_rows_host.py: the
oracle ends `solved` on all of them).

Defect check, on a build made aside: k_batch_update without the raw write of l in the whole-batch forms.  The three
cases here fail (the whole-batch results part from the member ones); test_gpu_batch_device_io.py, _members.py,
_updates.py, _common_members.py and _common_model.py stay green, so nothing else sees that row."""
import pytest

from _batch_parity import assert_parity
from _members_cases import B, ENGINES, Device, handle, same
from _raw_rows_cases import S, case, oracle_runs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("engine", ENGINES)
def test_raw_rows_of_every_form(gpu_lib, oracle_mod, engine):
    c = case(engine)
    dev = Device()
    forms = {"whole, host": lambda h: h.update(**c.full),
             "whole, device": lambda h: h.update(**{k: dev.put(v) for k, v in c.full.items()}),
             "members, host": lambda h: h.update(members=S, **c.rows),
             "members, device": lambda h: h.update(members=S, **{k: dev.put(v) for k, v in c.rows.items()})}
    res = {}
    try:
        for name, update in forms.items():
            h = handle(engine, c.pb)
            assert update(h) == 0, name
            assert (h.update_model(Ax=c.Ax2) if engine == "common" else h.update_matrices(Ax=c.Ax2)) == 0, name
            res[name] = h.solve()
            h.cleanup()
    finally:
        dev.close()
    first = res["whole, host"]
    for name, r in res.items():
        same(r, first, what="%s: %s against whole, host" % (engine, name))
    for b, ro in enumerate(oracle_runs(oracle_mod, engine)):
        assert ro.info.status_val == 1, (engine, b)
        assert_parity(first, b, ro, "%s raw rows" % engine)
    assert B == len(first.x)
