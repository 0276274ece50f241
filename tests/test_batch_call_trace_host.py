"""The batch Python API reaches the library as it did before batch.py and layer.py got one body per call pair: the
scripted session of tests/_call_trace.py -- every public call of BatchOSQP in every form it has, the
one-engine-per-member route and the layers, over recording stand-ins -- gives the trace tests/golden/batch_call_trace.json
holds, entry names, scalar arguments, array slots, returned shapes and raised texts alike.  No GPU, no library call."""
import json

import pytest

import _call_trace as ct


@pytest.fixture(scope="module")
def recorded():
    with open(ct.FIXTURE) as f:
        return ct.expand(json.load(f))


@pytest.fixture(scope="module")
def replayed():
    return ct.trace()


def test_the_session_is_the_recorded_one(recorded, replayed):
    assert sorted(replayed) == sorted(recorded)


def test_every_step_gives_the_recorded_trace(recorded, replayed):
    differ = [label for label in recorded if replayed.get(label) != recorded[label]]
    for label in differ[:5]:
        print("%s:\n  recorded %s\n  replayed %s" % (label, json.dumps(recorded[label]), json.dumps(replayed.get(label))))
    assert not differ, "%d steps differ from the recorded trace, the first: %s" % (len(differ), differ[:5])


def test_the_session_covers_the_forms(recorded):
    """The fixture is the session the issue describes, not a trimmed one: every entry of the batch ABI that a public call
    reaches appears in it, and so do the three return codes and the refusals."""
    calls = {c.split("(")[0] for records in recorded.values() for (made, _), _ in records for c in made}
    from osqp_amd.batch import MEMBER_CALLS
    for name in list(MEMBER_CALLS) + ["update", "update_dev", "warm_start", "warm_start_dev", "update_matrices", "update_matrices_dev",
                                      "common_update_model", "common_update_model_dev", "update_rho", "solve", "solve_members",
                                      "solve_limited", "polish", "polish_status_dev", "adjoint", "adjoint_dev", "adjoint_multi",
                                      "adjoint_multi_dev", "tangent", "tangent_dev", "get", "get_dev", "setup", "setup_engine",
                                      "setup_common", "common_kkt", "cleanup"]:
        assert name in calls, name
    assert any(c.startswith("OSQP[2].update_rho") for c in calls) and any(c.startswith("BatchOSQP.update_model") for c in calls)
    raised = [out for records in recorded.values() for (_, out), _ in records if isinstance(out, str) and out.startswith("raises ")]
    for words in ("failed (1)", "failed (5)", "failed (7)", "host and device arrays", "one single-QP engine per member",
                  "is not served by the one-engine-per-member route", "(QP 2 of the batch)", "without its shared KKT pieces"):
        assert any(words in text for text in raised), words
