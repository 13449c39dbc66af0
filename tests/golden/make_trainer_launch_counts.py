#!/usr/bin/env python3
"""Writes tests/golden/trainer_launch_counts.json: per arrangement of tests/trainer_arrangements.py, the trainer's schedule flags and
the number of launches per `nsamd_*` entry point of one proposal-update iteration, one other iteration and — where the arrangement
captures graphs — each variant's capture pass.

The committed table was recorded on an MI355X from the commit BEFORE trainer.plan_schedule and runner_interface.TrainStepRunner
existed; tests/test_gpu_trainer_launch_counts.py holds later code to it. Run this again only for a deliberate change of the
schedule, from the commit before that change — never to make the test pass.

    python tests/golden/make_trainer_launch_counts.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import trainer_arrangements as A  # noqa: E402

FLAGS = ("dp", "dp_sharded", "dp_fork", "use_graph", "defer", "cam_inside", "prologue", "prologue_ring", "source_inside", "pipelined")
RUNNER_FLAGS = ("cameras_outside", "gates_precleared")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "trainer_launch_counts.json")
    counts = A.count_launches(setattr)
    table = {}
    for name in A.ARRANGEMENTS:
        tr, rec = A.record(name, counts, os.environ.__setitem__, setattr)
        rec["flags"] = {**{k: bool(getattr(tr, k)) for k in FLAGS}, **{k: bool(getattr(tr.runner, k)) for k in RUNNER_FLAGS}}
        table[name] = rec
        del tr
    os.environ.pop("NSAMD_CAMERAS_OUTSIDE", None)
    with open(out_path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(table, sort_keys=True))


if __name__ == "__main__":
    main()
