"""Host companion of tests/test_gpu_batch_raw_rows.py: on the CPU, the oracle ends `solved` on all nine members of each
engine's case, so the parity check of the GPU test leaves no member out."""
import pytest

from _members_cases import B, ENGINES
from _raw_rows_cases import oracle_runs


@pytest.mark.parametrize("engine", ENGINES)
def test_oracle_solves_every_member(oracle_mod, engine):
    runs = oracle_runs(oracle_mod, engine)
    assert len(runs) == B
    assert [ro.info.status_val for ro in runs] == [1] * B, [(ro.info.status_val, ro.info.iter) for ro in runs]
