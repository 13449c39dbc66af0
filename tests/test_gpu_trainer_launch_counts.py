"""GPU box: which launches a trainer.HipTrainer iteration issues, per arrangement, against a table recorded BEFORE the runner
interface and `plan_schedule` were written (tests/golden/trainer_launch_counts.json, tests/golden/make_trainer_launch_counts.py).

Every other GPU test of the trainer asserts bits, and nearly every capability a runner may lack (runner_interface.TrainStepRunner)
selects a slower path with the same bits — the ray terms leave the Adam branch, batch selection is a launch of its own, the
gates are cleared level by level, the loss values come from a dozen reductions. This is the test that notices a fast path
switched off: the launches per `nsamd_*` entry point of one proposal-update and one other iteration (and of each variant's
capture pass where the arrangement captures graphs) must equal the record, and the trainer's flags must equal both the record
and `plan_schedule`'s row. smoke()'s sizes: 16 rays, (256, 96, 48) samples, tables of 2^12 and 2^10 rows."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import trainer_arrangements as A  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "trainer_launch_counts.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(A.ARRANGEMENTS))
def test_trainer_issues_the_recorded_launches_and_carries_the_plans_flags(recorded, monkeypatch, name):
    from nerfstudio_amd.trainer import plan_schedule

    assert set(recorded) == set(A.ARRANGEMENTS)
    want = recorded[name]
    assert ("capture" in want) == A.ARRANGEMENTS[name][4]
    assert sum(want["update"].values()) + sum(sum(c.values()) for c in want.get("capture", {}).values()) > 10  # (a record, not a blank)
    counts = A.count_launches(monkeypatch.setattr)
    tr, got = A.record(name, counts, monkeypatch.setenv, monkeypatch.setattr)
    plan = plan_schedule(runner=tr.runner, **A.plan_inputs(name))._asdict()
    flags = {k: getattr(tr.runner if k in ("cameras_outside", "gates_precleared") else tr, k) for k in want["flags"]}
    print(name, flags, got)
    for k, v in flags.items():
        assert v is want["flags"][k], (name, k, v)
        if k in plan:  # (`pipelined` is the trainer's property; `capture` has cleared nothing here: dp_fork is the eager value)
            assert v is plan[k], (name, k, v, plan[k])
    assert set(plan) <= set(flags)
    assert tr.pipelined == (plan["dp"] and tr.runner is not None)
    for part in ("update", "other"):
        assert got[part] == want[part], (name, part, got[part], want[part])
    assert got.get("capture") == want.get("capture"), (name, got.get("capture"), want.get("capture"))
