"""trainer.plan_schedule — the one place that decides which arrangement a HipTrainer construction gets — against its rules
written out as formulas, over every combination of its inputs; and the runner interface the trainer insists on
(runner_interface.TrainStepRunner). CPU tier: the function needs no device, no tensors and no environment."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nerfstudio_amd.runner_interface import PackedStepRunner, TrainStepRunner  # noqa: E402
from nerfstudio_amd.trainer import HipTrainer, SchedulePlan, plan_schedule  # noqa: E402

BOOLS = ("force_dp", "use_graph", "on_gpu", "own_runner", "cam_group", "has_source", "cameras_outside_switch")
CAPS = ("cam_opt", "single_jitter", "jitter", "side_stream", "prop_gates")  # what the plan reads of a runner


def _runner(cam_opt=False, single_jitter=False, jitter=False, side_stream=False, prop_gates=False):
    """A runner with these capabilities and nothing else (no tensors, no device)."""
    r = TrainStepRunner()
    r.single_jitter = single_jitter
    for name, have in (("cam_opt", cam_opt), ("jitter", jitter), ("side_stream", side_stream), ("prop_gates", prop_gates)):
        if have:
            setattr(r, name, object())
    return r


def _all_inputs():
    runners = [None] + [_runner(*caps) for caps in itertools.product((False, True), repeat=len(CAPS))]
    for bits in itertools.product((False, True), repeat=len(BOOLS)):
        for runner, world, dp_mode, defer_switch in itertools.product(runners, (1, 2), ("allreduce", "sharded"), (None, False, True)):
            yield dict(zip(BOOLS, bits), runner=runner, world=world, dp_mode=dp_mode, defer_switch=defer_switch)


def test_plan_follows_the_rules_for_every_combination_of_its_inputs():
    count = 0
    for kw in _all_inputs():
        p = plan_schedule(**kw)
        count += 1
        assert all(type(v) is bool for v in p), (kw, p)
        runner = kw["runner"]
        dp = kw["world"] > 1 or kw["force_dp"]
        use_graph = kw["use_graph"] and kw["on_gpu"]
        assert p.dp == dp and p.dp_sharded == (dp and kw["dp_mode"] == "sharded") and p.use_graph == use_graph, kw
        if runner is None:  # the module path: every other flag is false
            assert p == SchedulePlan(dp, p.dp_sharded, False, use_graph, False, False, False, False, False, False, False), kw
            continue
        cam_on = runner.cam_opt is not None
        cam_inside = cam_on and kw["cam_group"] and not dp and not kw["cameras_outside_switch"]
        cameras_outside = cam_on and not cam_inside
        switch = use_graph if kw["defer_switch"] is None else kw["defer_switch"]  # NSAMD_DEFER_MAIN_ADAM, default: use_graph
        defer = not dp and kw["on_gpu"] and switch
        prologue = kw["on_gpu"] and kw["own_runner"] and runner.single_jitter and runner.jitter is not None
        prologue_ring = prologue and not cameras_outside and not dp
        assert p.cam_inside == cam_inside and p.cameras_outside == cameras_outside and p.defer == defer, kw
        assert p.prologue == prologue and p.prologue_ring == prologue_ring, kw
        assert p.source_inside == (kw["has_source"] and prologue_ring), kw
        assert p.dp_fork == (dp and runner.side_stream is not None) and p.gates_precleared == (runner.prop_gates is not None), kw
        # invariants
        assert not p.cam_inside or not p.dp
        assert not p.prologue_ring or p.prologue
        assert not p.source_inside or p.prologue_ring
        assert not p.defer or (kw["on_gpu"] and not p.dp)
        assert p.cameras_outside == (cam_on and not p.cam_inside)
    assert count == 2 ** len(BOOLS) * (1 + 2 ** len(CAPS)) * 12


# train_step.NerfactoTrainStep as the plan sees it (camera optimiser off / on), and tests/cpu_runner.CpuRunner
KERNELS = dict(single_jitter=True, jitter=True, side_stream=True, prop_gates=True)
GPU = dict(runner=_runner(**KERNELS), own_runner=True, world=1, force_dp=False, dp_mode="allreduce", use_graph=True, on_gpu=True,
           cam_group=False, has_source=False, cameras_outside_switch=False, defer_switch=None)  # bench.py's default: graphs, pool, N = 1
CAMERA = dict(runner=_runner(cam_opt=True, **KERNELS), cam_group=True)
CPU = dict(runner=_runner(jitter=True), own_runner=False, on_gpu=False)


def _plan(*groups, **over):
    kw = dict(GPU)
    for g in groups:
        kw.update(g)
    return plan_schedule(**{**kw, **over})


def _row(**true):
    fields = dict.fromkeys(SchedulePlan._fields, False)
    assert set(true) <= set(fields)
    return SchedulePlan(**{**fields, **true})


def test_named_rows():
    inside = dict(use_graph=True, defer=True, prologue=True, prologue_ring=True, gates_precleared=True)
    assert _plan() == _row(**inside)  # bench.py's default
    assert _plan(use_graph=False) == _row(prologue=True, prologue_ring=True, gates_precleared=True)  # --no-graph
    assert _plan(use_graph=False, defer_switch=True) == _row(defer=True, prologue=True, prologue_ring=True, gates_precleared=True)
    assert _plan(defer_switch=False) == _row(use_graph=True, prologue=True, prologue_ring=True, gates_precleared=True)
    assert _plan(CAMERA) == _row(cam_inside=True, **inside)  # camera optimiser on
    assert _plan(CAMERA, cameras_outside_switch=True) == _row(  # ... with NSAMD_CAMERAS_OUTSIDE=1
        use_graph=True, defer=True, cameras_outside=True, prologue=True, gates_precleared=True)
    assert _plan(CAMERA, cam_group=False).cameras_outside  # (an arena without the group cannot step it inside)
    dp = dict(dp=True, dp_fork=True, use_graph=True, prologue=True, gates_precleared=True)
    assert _plan(force_dp=True) == _row(**dp)  # --force-dp
    assert _plan(force_dp=True, dp_mode="sharded") == _row(dp_sharded=True, **dp)  # --force-dp --dp-mode sharded
    assert _plan(CAMERA, world=2) == _row(cameras_outside=True, **dp)
    assert _plan(has_source=True) == _row(source_inside=True, **inside)  # the pipeline seam with a device batch source
    assert _plan(CAMERA, has_source=True, cameras_outside_switch=True).source_inside is False
    # a CPU stand-in runner handed in by TrainEngine.runner_factory: nothing, whatever was asked for
    assert _plan(CPU) == _row() and _plan(CPU, has_source=True) == _row() and _plan(CPU, world=2) == _row(dp=True)
    assert _plan(runner=None, own_runner=False) == _row(use_graph=True)  # the module path (bench.py --autograd)


def test_gpu_arrangements_are_rows_of_the_plan():
    """tests/trainer_arrangements.py (the GPU launch-count test) describes its constructions in the plan's own terms."""
    import trainer_arrangements as A

    plans = {name: plan_schedule(runner=_runner(cam_opt=A.ARRANGEMENTS[name][0] != "off", **KERNELS), **A.plan_inputs(name))
             for name in A.ARRANGEMENTS}
    assert plans["eager"] == _plan(use_graph=False) and plans["captured"] == _plan()
    assert plans["camera_inside"] == _plan(CAMERA) and plans["camera_outside"] == _plan(CAMERA, cameras_outside_switch=True)
    assert plans["force_dp"] == _plan(force_dp=True) and plans["source"] == _plan(has_source=True)


# ---- the interface is loud ----------------------------------------------------------------------------------------------------
INTERFACE = {"side_stream": None, "cam_opt": None, "cameras_outside": False, "single_jitter": False, "jitter": None, "bg_rays": None,
             "prop_gates": None, "gates_precleared": False, "ray_terms_on": False, "fuse_select": False, "pending_select": None,
             "want_loss_vals": False, "_loss_vals_fresh": False, "grad_lookup": None}


def test_interface_states_every_optional_capability_with_its_default():
    stated = {k: v for k, v in vars(TrainStepRunner).items() if not k.startswith("__")}
    assert stated == INTERFACE
    assert PackedStepRunner.writes_arena_grads is False and PackedStepRunner.grad_lookup is None


def test_stand_ins_and_kernel_schedules_derive_from_the_interface():
    import cpu_runner
    import test_device_batches_cpu

    from nerfstudio_amd.ngp_step import NgpTrainStep
    from nerfstudio_amd.train_step import NerfactoTrainStep

    for cls in (NerfactoTrainStep, cpu_runner.CpuRunner, test_device_batches_cpu._ToyRunner):
        assert issubclass(cls, TrainStepRunner)
        assert not set(INTERFACE) & set(vars(cls)), "a stand-in restates no default; the schedule sets its own in __init__"
    assert issubclass(NgpTrainStep, PackedStepRunner) and NgpTrainStep.writes_arena_grads is True
    assert issubclass(cpu_runner.CpuNgpRunner, PackedStepRunner) and cpu_runner.CpuNgpRunner.writes_arena_grads is False


def test_trainer_refuses_a_runner_outside_the_interface():
    import torch

    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.cameras.rays import RayBundle
    from test_device_batches_cpu import _ToyModel, _ToyRunner

    model = _ToyModel()
    arena = ParamArena(model.get_param_groups(), lr=1e-2, eps=1e-15)
    rb = RayBundle(origins=torch.zeros(16, 3), directions=torch.ones(16, 3), pixel_area=torch.ones(16, 1),
                   camera_indices=torch.zeros(16, 1, dtype=torch.int64))
    batch = {"image": torch.zeros(16, 3)}
    duck = type("Duck", (), dict(vars(_ToyRunner)))  # the same methods, not the interface
    with pytest.raises(TypeError, match="TrainStepRunner"):
        HipTrainer(model, arena, rb, batch, use_graph=False, runner=duck(model, 16, "cpu"))
    tr = HipTrainer(model, arena, rb, batch, use_graph=False, runner=_ToyRunner(model, 16, "cpu"))
    assert tr.runner.grad_lookup is not None and tr.runner.gates_precleared is False and tr.runner.cameras_outside is False
    assert not (tr.defer or tr.prologue or tr.prologue_ring or tr.dp or tr.use_graph or tr.cam_inside or tr.source_inside)
