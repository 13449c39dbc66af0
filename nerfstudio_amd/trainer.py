"""The nerfacto training iteration as the product runs it fastest: the explicit kernel schedule (train_step.py) captured in
hipGraphs, the main-field Adam deferred beside the next proposal forward, all step-dependent scalars in device memory, and
— for more than one rank — the pipelined gradient exchange of dp_schedule.py.

Reference seam: `Trainer.train_iteration` (engine/trainer.py:487-531) -> `VanillaPipeline.get_train_loss_dict`
(pipelines/base_pipeline.py:290-303) -> `Optimizers` (engine/optimizers.py:74-193) behind `DistributedDataParallel`
(base_pipeline.py:279-282). Two callers drive this class:
  * `pipeline.HipPipeline` — the `nerfacto-hip` method's pipeline: the reference's own trainer calls
    `get_train_loss_dict(step)`, which hands the datamanager's batch to `set_batch` and runs `train_iteration`;
  * `bench.py` — the same object over a pool of synthetic ray batches resident in HBM.

Eager mode runs the Python body every step. Graph mode captures that same body ONCE per schedule variant (proposal networks
updated this step / not, ray_samplers.py:590) into a hipGraph and replays it: ~60 kernel launches become one graph launch,
which is what a sub-millisecond step needs (MI355X_MICROARCH.md price list: eager goes host-bound below ~3 us per kernel).
Everything that changes from step to step lives in device memory: the ray batch, the jitter draws (counter-based Philox),
the anneal exponent and Adam's bias-corrected step sizes (`hyper`). The first node of the body (nsamd_step_prologue) draws
the step's uniforms and reads the step's scalars out of a ring of rows in pinned host memory that the host writes before
each launch. Where the body does not select the batch itself (the data-parallel segments, the camera parts outside the
body) or there is no prologue (the module path), the scalars arrive by a 32-byte async copy instead.

N = 1: one body (`_body`) serves every schedule, eager or captured. With graphs (default) the main-field Adam of iteration k
runs at the head of iteration k+1's graph, on a branch beside select-batch / jitter / the proposal forward (four captured
variants: proposal update x pending Adam). Same dependencies as Adam at the end of the iteration, hence the same bits;
`finish()` runs the last pending update (a caller that reads the parameters — evaluation, checkpoint — calls it first).
Without graphs the iteration runs in order, Adam at its end.

N > 1 (data parallel): the iteration runs as segments (eager launches by default, captured hipGraphs on request) and the
main-field gradient exchange (RCCL, its own stream) is PIPELINED across steps (dp_schedule.PipelinedExchange). The proposal
forward of step k+1 reads only proposal-network parameters, so
    step k:   [proposal fwd k] -> (wait X_main k-1) [Adam main k-1] -> [main fwd + losses + main bwd k]
              -> X_main k (async) -> [proposal bwd k] -> X_props k -> [Adam props k]      (last two: update steps)
hides the exchange behind the proposal backward of step k AND the proposal forward of step k+1, with exactly the sequential
semantics (every parameter is updated before its next use).

Camera optimiser on (models/nerfacto.py:131, the reference's nerfacto default): the [num_cameras, 6] exponential map and its
autograd backward are ~100 tiny torch kernels. N = 1: they are captured with everything else (a whole-iteration capture holds
forward, autograd backward and optimiser alike) — launched eagerly around the replay they made the step host-bound (1.80 ms
against 0.76, profiles/r04_camera_optimizer.txt). N > 1 (eager segments) or NSAMD_CAMERAS_OUTSIDE=1: batch selection and pose
corrections before the segments, the rays' share of `pose_adjustment.grad`, the group's exchange and Adam after them; the
kernels read the corrected rays and leave dL/d(origins, directions) per ray either way.

Which of these arrangements a construction gets is decided in one place, `plan_schedule` (a pure function of the arguments, the
runner's capabilities and two switches); what the drivers ask of a runner is stated in runner_interface.TrainStepRunner.
"""
from __future__ import annotations

import os
import sys
from typing import Callable, Dict, NamedTuple, Optional

import torch

from . import _native as N
from .runner_interface import TrainStepRunner

BATCH_SLOTS = 8  # default number of pre-generated ray batches of a pool (bench.py)

_HYPER = {"fields": 0, "proposal_networks": 2, "camera_opt": 6}  # offsets of (step size, 1/sqrt(bc2)) per optimiser group
_HYPER_ANNEAL, _HYPER_SLOT, _HYPER_FLOATS = 4, 5, 8


class SchedulePlan(NamedTuple):
    dp: bool                # the data-parallel segments (N > 1, or force_dp: the same over a one-rank communicator)
    dp_sharded: bool        # reduce-scatter -> Adam on the rank's 1/N arena shard -> all-gather; else the reference's DDP semantics
    dp_fork: bool           # the proposal backward chains beside the main chain (eager data-parallel segments: `capture` clears it)
    use_graph: bool
    defer: bool             # the main-field Adam of iteration k at the head of iteration k+1
    cam_inside: bool        # the camera optimiser's torch ops and Adam are part of the (captured) iteration body
    cameras_outside: bool   # ... or run around it (the runner's attribute)
    prologue: bool          # nsamd_step_prologue is the body's first launch (the step's draws)
    prologue_ring: bool     # ... and fetches the step's scalars from the ring in host memory (else: the upload)
    source_inside: bool     # the batch source's launch is part of the (captured) iteration body
    gates_precleared: bool  # `_zero` clears the proposal levels' gradient flags with the gradients (the runner's attribute)


def plan_schedule(*, runner: Optional[TrainStepRunner], own_runner: bool, world: int, force_dp: bool, dp_mode: str, use_graph: bool,
                  on_gpu: bool, cam_group: bool, has_source: bool, cameras_outside_switch: bool,
                  defer_switch: Optional[bool]) -> SchedulePlan:
    """The schedule of one HipTrainer construction: a function of its arguments alone (no device, no tensor, no environment).
    runner: None (the module path: nothing beyond dp / dp_sharded / use_graph) or the runner, of which only the capabilities of
    runner_interface.TrainStepRunner are read; own_runner: the trainer built it (none was injected); cam_group: the arena has
    a "camera_opt" group; cameras_outside_switch: NSAMD_CAMERAS_OUTSIDE=1; defer_switch: NSAMD_DEFER_MAIN_ADAM (None: unset)."""
    dp = world > 1 or force_dp
    use_graph = use_graph and on_gpu
    if runner is None:
        return SchedulePlan(dp, dp and dp_mode == "sharded", False, use_graph, *[False] * 7)
    cam_on = runner.cam_opt is not None
    cam_inside = cam_on and cam_group and not dp and not cameras_outside_switch
    cameras_outside = cam_on and not cam_inside  # see the module docstring
    # N = 1: the main-field Adam of iteration k (470 MB of HBM streaming) runs BESIDE the proposal forward of iteration k+1
    # (L2-resident gathers and per-ray scans that read only proposal-network parameters) — the single-GPU form of the
    # pipelined schedule; same dependencies, same bits. Measured on three MI355X boxes (profiles/r02_schedule_ab.txt): 1.3 / 3
    # / 4.5 % faster than Adam at the end of the iteration when replayed from hipGraphs, neutral with eager launches — so it
    # is the default with graphs. NSAMD_DEFER_MAIN_ADAM=0/1: A/B.
    defer = not dp and on_gpu and (use_graph if defer_switch is None else defer_switch)
    prologue = on_gpu and own_runner and bool(runner.single_jitter) and runner.jitter is not None
    # The batch slot must be read INSIDE the iteration body: with the camera parts outside the graph the batch is selected
    # eagerly ahead of the replay, i.e. before the prologue would have written the slot (then: the upload for the scalars, the
    # prologue for the draws only). The data-parallel segments keep the upload as well — their Adam launches are segments of
    # their own, ordered by the exchange — and take the DRAWS from the prologue: one generator for every schedule, so that a
    # one-rank data-parallel run trains through the bits of the single-GPU one.
    prologue_ring = prologue and not cameras_outside and not dp
    return SchedulePlan(dp=dp, dp_sharded=dp and dp_mode == "sharded", dp_fork=dp and runner.side_stream is not None,
                        use_graph=use_graph, defer=defer, cam_inside=cam_inside, cameras_outside=cameras_outside, prologue=prologue,
                        prologue_ring=prologue_ring, source_inside=has_source and prologue_ring,
                        gates_precleared=runner.prop_gates is not None)


class HipTrainer:
    """model: nerfacto.NerfactoModel or the plugin's HipNerfactoModel; arena: arena.ParamArena over its optimiser groups
    ("fields", "proposal_networks"[, "camera_opt"]).

    pool: {"origins" [slots,n,3], "directions", "cameras" [slots,n], "target" [slots,n,3]} resident in HBM — iteration i
    trains on slot i % slots, selected on the device (replayable); None: the caller fills the runner's static buffers
    (`set_batch`) before every iteration.
    source: a device_batches.DeviceBatchSource (instead of a pool): every iteration SAMPLES its batch from the source's image
    store. With the device prologue supplying the step's scalars (`prologue_ring`: N = 1, the camera parts inside the body) the
    source's launch is a node of the body where `nsamd_select_batch` is for a pool — its draw number is the prologue's own
    counter — and is captured with the rest: a replay needs nothing from the host for its batch. Otherwise (no prologue, the
    camera parts outside the body, the data-parallel segments) the trainer calls `source.next_batch()` EAGERLY ahead of the
    iteration and copies it into the static buffers as `set_batch` does: still no CPU work per pixel, but not the captured path.
    lr_source(group, iteration) -> learning rate of that iteration (default: the nerfacto recipe's schedulers over arena.lr).
    drive_callbacks: call the model's BEFORE/AFTER_TRAIN_ITERATION callbacks here (False when a trainer does: HipPipeline).
    runner: a runner_interface.TrainStepRunner standing in for train_step.NerfactoTrainStep (CPU tests of the host logic)."""

    def __init__(self, model, arena, ray_bundle, batch, world: int = 1, use_graph: bool = True, use_runner: bool = True,
                 pool=None, source=None, force_dp: bool = False, dp_mode: str = "allreduce",
                 lr_source: Optional[Callable[[str, int], float]] = None, drive_callbacks: bool = True, runner=None) -> None:
        if hasattr(getattr(model, "config", None), "depth_loss_type"):
            # its iteration (and the graphs captured from it) carries no depth target, sigma decay or depth batch
            raise NotImplementedError("HipTrainer: depth supervision (depth-nerfacto) is only on the module path")
        if source is not None and pool is not None:
            raise ValueError("HipTrainer: `pool` and `source` are mutually exclusive (one owner of the step's batch)")
        if source is not None and not (use_runner or runner is not None):
            raise ValueError("HipTrainer: a batch source needs the explicit kernel schedule (use_runner)")
        if runner is not None and not isinstance(runner, TrainStepRunner):
            raise TypeError(f"HipTrainer: the runner must be a runner_interface.TrainStepRunner, got {type(runner).__name__}")
        self.model, self.arena, self.rb, self.batch, self.world = model, arena, ray_bundle, batch, world
        self.pool, self.source = pool, source
        self.slots = int(pool["origins"].shape[0]) if pool is not None else 1
        self.step = self.opt_step = 0
        self.drive_callbacks = drive_callbacks
        self._true_steps = dict(arena.step_counts)
        dev = ray_bundle.origins.device
        self.on_gpu = dev.type == "cuda"
        # device-resident step-dependent scalars: Adam (step size, 1/sqrt(bc2)) per optimiser group, the anneal exponent,
        # the batch slot of this step
        self.hyper = torch.zeros(_HYPER_FLOATS, device=dev)
        # The host runs ahead of the GPU, so the pinned source of an async copy must not be rewritten before the copy
        # has executed: a ring of slots, each guarded by the event recorded after its last copy.
        self.hyper_ring = [torch.zeros(_HYPER_FLOATS).pin_memory() if self.on_gpu else torch.zeros(_HYPER_FLOATS) for _ in range(64)]
        # (numpy views of the pinned slots: a scalar store into a tensor costs ~5 us of dispatch, eight of them per iteration
        #  were a tenth of the host's share of a step through the pipeline seam)
        self.hyper_ring_np = [h.numpy() for h in self.hyper_ring]
        self.hyper_events = [None] * 64
        self.hyper_slot = 0
        if lr_source is None:
            from .schedulers import ExponentialDecayScheduler, ExponentialDecaySchedulerConfig, nerfacto_schedulers

            sched = nerfacto_schedulers()
            # method_configs.py:117-120: camera_opt = Adam(lr 1e-3, eps 1e-15) + ExponentialDecay(lr_final 1e-4, 5000 steps)
            sched["camera_opt"] = ExponentialDecayScheduler(ExponentialDecaySchedulerConfig(lr_final=1e-4, max_steps=5000))
            base = {"fields": arena.lr, "proposal_networks": arena.lr, "camera_opt": 1e-3}
            lr_source = lambda group, it: sched[group].get_lr(max(it, 0), base[group])  # noqa: E731
        self.lr_source = lr_source
        self.exchange = None  # dp_schedule.PipelinedExchange (N > 1 with the runner)
        self.ring_rows = 256
        self.hyper_views = {g: self.hyper[o:o + 2] for g, o in _HYPER.items()}
        self.loss_buf = torch.zeros((), device=dev)
        model.proposal_sampler.anneal_dev = self.hyper[_HYPER_ANNEAL:_HYPER_ANNEAL + 1]
        self.graphs = None
        self._capture_tried = False  # pipeline.TrainEngine: one capture attempt per trainer
        self.defer_scatter = False  # read by bench.py: the main table scatter is never deferred to the next iteration
        self.opt_parallel = True  # False: the deferred Adam runs on the main stream (per-kernel timing)
        # the ray terms on the Adam branch read a batch the fused selection is still to copy out of the pool's own rows
        # (nsamd_field_mlp.batch_slot): no edge from the bins launch to that branch; False: behind the bins, by an event
        self.terms_from_pool = True
        # False: the jitter buffer of the runner is filled by the caller before every iteration (parity tests inject the
        # draws the CPU oracle uses; the default draws them on the device inside the iteration, graph-safe Philox)
        self.draw_jitter = True
        self._pending_main = False  # deferred schedule: the main-field Adam of the previous iteration is still to run
        self.cam_group = "camera_opt" if "camera_opt" in arena.groups else None
        own_runner = runner is None
        if use_runner and own_runner:  # explicit kernel schedule over static buffers (train_step.py); default
            from .train_step import NerfactoTrainStep

            runner = NerfactoTrainStep(model, ray_bundle.origins.shape[0], dev)
        self.runner = r = runner
        defer_env = os.environ.get("NSAMD_DEFER_MAIN_ADAM")
        plan = plan_schedule(runner=r, own_runner=own_runner, world=world, force_dp=force_dp, dp_mode=dp_mode, use_graph=use_graph,
                             on_gpu=self.on_gpu, cam_group=self.cam_group is not None, has_source=source is not None,
                             cameras_outside_switch=os.environ.get("NSAMD_CAMERAS_OUTSIDE", "0") == "1",
                             defer_switch=None if defer_env is None else defer_env == "1")
        # (plain attributes: tests, bench.py and utils/roofline.py read and assign them; `capture` clears dp_fork)
        (self.dp, self.dp_sharded, self.dp_fork, self.use_graph, self.defer, self.cam_inside, cameras_outside, self.prologue,
         self.prologue_ring, self.source_inside, gates_precleared) = plan
        if r is None:
            return
        r.grad_lookup = arena.grad_lookup()
        r.gates_precleared, r.cameras_outside = gates_precleared, cameras_outside
        r.set_batch(ray_bundle.origins, ray_bundle.directions, ray_bundle.camera_indices, batch["image"])
        r.anneal_dev = self.hyper[_HYPER_ANNEAL:_HYPER_ANNEAL + 1]
        if self.defer:
            self.opt_stream = torch.cuda.Stream(device=dev)
            self._opt_fork, self._opt_join, self._batch_ready = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        # ---- device-side head of the iteration (nsamd_step_prologue), on the GPU with the trainer's own runner ----
        # A replayed graph had two host-issued operations in front of it every iteration — the 32-byte upload of `hyper` and the
        # offset fill of torch's graph-safe generator (for the jitter's uniform_) — and each eager -> graph hand-over leaves the
        # stream idle for ~8 us (profiles/r05_s9_seam_trace_gaps.txt). With the prologue the first node of the graph draws the
        # step's uniforms with a counter-based generator and fetches the step's scalars itself, from a ring of rows in pinned
        # HOST memory the device reads directly: the host writes row i % rows for iteration i (exact host arithmetic, at the
        # time it would have issued the upload) and launches; the device's own row counter picks it up. Nothing is predicted, so
        # it serves a trainer whose learning rates come from outside (pipeline.TrainEngine) as well. An event every 64 rows
        # keeps the host from lapping the device. (A table of rows predicted ahead in device memory measured the same, the
        # per-iteration upload 3 % slower: profiles/r05_s11_ab_step_prologue.txt.)
        if self.prologue:
            self.step_counter = torch.zeros(2, device=dev, dtype=torch.int64)  # [row, draw]
            # The draws are keyed by (seed, draw counter). The counter starts at the model's training step, so that a trainer
            # built in the middle of a run (a resumed checkpoint, an engine rebuilt for another batch size) does not replay
            # the jitter and background draws of steps 0, 1, ...; the rank is mixed into the seed, so that data-parallel
            # ranks that share torch's seed still draw different numbers (the reference: one generator per process).
            self.step_counter[1] = int(getattr(model, "step", 0) or 0)
            rank = 0
            if world > 1 and os.environ.get("NSAMD_BENCH_SAME_RAYS") != "1":  # (the functional check: every rank the same rays AND draws)
                import torch.distributed as dist

                rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            self.rng_seed = ((int(torch.initial_seed()) + 0x632BE59BD9B4E019 * rank) * 0x9E3779B97F4A7C15
                             + 0x5851F42D4C957F2D) & 0xFFFFFFFFFFFFFFFF
        if self.prologue_ring:
            self.ring_host = torch.zeros(self.ring_rows, _HYPER_FLOATS).pin_memory()  # (device-visible: hipHostMalloc)
            self.ring_np = self.ring_host.numpy()
            self._ring_pos = 0                 # rows written so far == the device's row counter at the next launch
            self._ring_events = [None] * 4     # recorded every 64 rows
        if source is not None:
            assert source.num_rays == r.n, "the source and the static buffers must agree on the rays per batch"
            # as the jitter's counter: a trainer built in the middle of a run does not replay the pixels of steps 0, 1, ...
            source.set_draw(int(getattr(model, "step", 0) or 0))
        if self.dp:
            from .dp_schedule import PipelinedExchange

            self.exchange = PipelinedExchange(arena, self._run, before_main_update=self._push_hyper, sharded=self.dp_sharded)
            # the coarse levels of the main table can only ever touch 288 k of their 2.6 M rows: exchange those
            # compactly (2.3 MB instead of 21 MB of the 67 MB main-field all-reduce)
            enc = model.field.mlp_base.encoding
            if hasattr(enc, "spec"):
                rows, index = enc.spec.reachable_prefix()
                if index.numel() and index.numel() < rows // 2 and not self.dp_sharded:
                    arena.register_compact(enc.hash_table, rows, index)  # (the reduce-scatter takes the slice as it lies)

    # -- the batch ---------------------------------------------------------------------------------------------------
    def set_batch(self, ray_bundle, batch) -> None:
        """The next iteration's rays and targets (a trainer's `datamanager.next_train`, base_datamanager.py:506-515), copied
        into the static buffers the captured graphs read. Stream-ordered: no host synchronisation."""
        assert self.pool is None, "this trainer rotates its own pool of batches"
        assert self.source is None, "this trainer samples its own batches"
        o = ray_bundle.origins.reshape(-1, 3)
        if self.runner is not None:
            assert o.shape[0] == self.runner.n, "the captured schedule is built for a fixed number of rays per batch"
            self.runner.set_batch(o, ray_bundle.directions.reshape(-1, 3), ray_bundle.camera_indices.reshape(-1), batch["image"])
        else:
            self.rb, self.batch = ray_bundle, batch

    # -- pieces of one iteration ---------------------------------------------------------------------------------------
    def _hyper_row(self, out, step, counts, have_pending):
        """The step-dependent scalars of iteration `step` into `out` (8 floats, numpy): Adam step sizes of the NEXT update of
        each group (`counts`: the groups' step counters before the iteration) + the anneal exponent + the batch slot."""
        from . import functional as F

        a = self.arena
        # iteration i runs with lr(i); a pending (pipelined) main-field update belongs to the previous iteration
        it_fields = step - 1 if have_pending else step
        out[:] = 0.0
        for group, off in _HYPER.items():
            if group not in a.groups:
                continue
            lr = self.lr_source(group, max(it_fields, 0) if group == "fields" else step)
            out[off], out[off + 1] = F.adam_hyper(counts[group] + 1, lr, a.betas)
        out[_HYPER_ANNEAL] = self.model.proposal_sampler._anneal
        out[_HYPER_SLOT] = float(step % self.slots)

    def _push_hyper(self, direct: bool = False):
        """Adam step sizes of the NEXT update of each group + the anneal exponent -> device (async, race-free). `direct`: into
        `hyper` itself whatever the mode (a caller that launches an update outside an iteration body: `finish`)."""
        a = self.arena
        if self.prologue_ring and not direct:
            # the graph's first node reads row `counter % rows` out of pinned host memory: write it, launch, done
            i = self._ring_pos
            if i % 64 == 0:
                k = (i // 64) % 4
                ago = self._ring_events[(k + 2) % 4]  # recorded 128 rows ago: the rows about to be rewritten were read long before
                if ago is not None:
                    ago.synchronize()
                ev = torch.cuda.Event()
                ev.record(N.current_stream())
                self._ring_events[k] = ev
            self._hyper_row(self.ring_np[i % self.ring_rows], self.step, a.step_counts, self._have_pending)
            self._ring_pos = i + 1
            return
        slot = self.hyper_slot
        self.hyper_slot = (slot + 1) % len(self.hyper_ring)
        if self.hyper_events[slot] is not None:
            self.hyper_events[slot].synchronize()  # the copy that last read this slot (64 pushes ago) is done
        h, hn = self.hyper_ring[slot], self.hyper_ring_np[slot]
        self._hyper_row(hn, self.step, a.step_counts, self._have_pending)
        self.hyper.copy_(h, non_blocking=True)
        if self.on_gpu:
            ev = torch.cuda.Event()
            ev.record(N.current_stream())
            self.hyper_events[slot] = ev

    def _step_prologue(self):
        """First launch of an iteration body (captured with it): the step's draws and, with the ring, the step's scalars."""
        if not self.prologue:
            return
        r = self.runner
        draw = self.draw_jitter
        j = r.jitter if draw else None
        bg = r.bg_rays if (draw and r.bg_rays is not None) else None
        rows_ptr, rows = (self.ring_host.data_ptr(), self.ring_rows) if self.prologue_ring else (None, 0)
        N.check(N.load().nsamd_step_prologue(
            N.ptr(self.step_counter), rows_ptr, rows, N.ptr(self.hyper), N.ptr(j), j.numel() if j is not None else 0,
            N.ptr(bg), bg.numel() if bg is not None else 0, self.rng_seed, N.stream()), "step_prologue")

    def _zero(self, updated, groups=None):
        """Zero-fills ahead of an iteration's forward; `groups`: only these gradient slices (a later segment of the same
        iteration: the proposal levels' gradient flags are raised by then and stay as they are)."""
        whole = groups is None
        if groups is None:
            groups = ["fields", "proposal_networks"] if updated else ["fields"]
            if self.cam_inside:
                groups = groups + [self.cam_group]
        self.arena.zero_grad(groups, skip=self.runner.written_params())
        if whole and updated:
            self._clear_gates()

    def _clear_gates(self):
        # (instead of one 4-byte memset node per level ahead of its weights backward; BEFORE the losses launch, which raises
        # the flags when it also runs the levels' weights backward)
        if self.runner.gates_precleared:
            self.runner.prop_gates.zero_()

    def _stepped(self, updated, pending):
        """The optimiser groups whose Adam launches one iteration issues — the reference steps a group only when it received
        gradients (engine/optimizers.py:160-172): the main field's (deferred schedule: the previous iteration's, when one is
        pending), the proposal networks' on update steps, the camera optimiser's when it is part of the body."""
        return ((["fields"] if pending or not self.defer else []) + (["proposal_networks"] if updated else [])
                + ([self.cam_group] if self.cam_inside else []))

    def _body(self, updated, pending):
        """One N = 1 iteration over the runner, eager or captured as the graph ("all", updated, pending):
            in order:  select batch -> zero-fills -> proposal forward -> main forward, losses, backward chains -> Adam
            deferred:  [Adam main k-1, zero-fills, ray terms k  ||  select batch, proposal forward k] -> main forward, losses,
                       backward chains k -> [Adam proposals k]                                          (update steps)
        Inside a captured hipGraph the two halves of the deferred first line are parallel branches. With the camera parts
        outside, batch selection and the pose corrections have already run (eagerly, `_cameras_before`)."""
        r, a = self.runner, self.arena
        assert self.defer or not pending
        beside = pending and self.opt_parallel
        main = N.current_stream() if beside else None  # (the stream the Adam branch forks from and joins)
        # The ray terms of this iteration's main-field forward (train_step.ray_terms_launch) need the updated head weights and
        # the selected batch, nothing else: beside a pending Adam they go on its branch, behind an event the main branch
        # records once the batch is in place — off the critical path instead of a launch (and a dependent-launch gap) in
        # front of the hash forward.
        terms_beside = beside and r.ray_terms_on
        # ... and where `forward_proposals` will select the batch out of the pool (`_select_batch` hands it over), they read
        # the pool's rows themselves: behind the Adam and the zero-fills on that branch, no event, and the bins launch keeps
        # the first proposal field as its only child — which a replayed graph leaves on the bins' hardware queue
        # (profiles/critical_chain_hops_ab.txt)
        select = self._pool_select() if (terms_beside and self.terms_from_pool and not r.cameras_outside) else None
        terms_after_bins = terms_beside and select is None

        def terms_behind_batch():  # (runs inside forward_proposals, right behind the launch that selects the batch)
            self._batch_ready.record(main)
            self.opt_stream.wait_event(self._batch_ready)
            with N.on_stream(self.opt_stream):
                r.ray_terms_launch()
                self._opt_join.record(self.opt_stream)

        self._step_prologue()  # the step's scalars and draws: first node, every branch below depends on it
        if beside:
            self._opt_fork.record(main)
            self.opt_stream.wait_event(self._opt_fork)
            with N.on_stream(self.opt_stream):
                a.step(grad_scale=1.0, groups=["fields"], hyper_dev=self.hyper_views)  # what iteration k-1 left behind
                # ... and, off the critical path, this iteration's zero-fills: the Adam above was the last reader of the field
                # gradients, the proposal / camera groups were consumed at the end of their last update iteration, and
                # nothing before the join below writes a gradient
                self._zero(updated)
                if select is not None:
                    r.ray_terms_launch(select=select)
                if not terms_after_bins:
                    self._opt_join.record(self.opt_stream)
        elif pending:
            a.step(grad_scale=1.0, groups=["fields"], hyper_dev=self.hyper_views)
        if not r.cameras_outside:
            self._select_batch()
            r.apply_camera_corrections()
        if not self.defer:
            # the main table's gradient is written, not accumulated; the proposal group's gradients are neither produced nor
            # consumed on a step that does not update it (ray_samplers.py:590-599), so its 10 MB need no zero-fill then
            self._zero(updated)
        r.forward_proposals(self.draw_jitter and not self.prologue, need_enc=updated, after_bins=terms_behind_batch if terms_after_bins else None)
        if beside:
            main.wait_event(self._opt_join)
        elif self.defer:
            self._zero(updated)
        r.forward_main_and_losses(updated, terms_ready=terms_beside)
        r.backward_all(updated)  # the backward chains run as parallel branches
        late = self._stepped(updated, pending=False)  # (a pending main-field update has run at the head)
        if late:
            a.step(grad_scale=1.0, groups=late, hyper_dev=self.hyper_views)

    def _module_body(self, updated):
        """use_runner=False: forward, losses and backward through the nn.Modules and autograd, then — N > 1 — one blocking
        all-reduce of the whole arena (not pipelined), then Adam."""
        from .cameras.rays import RayBundle

        self._select_batch()
        self.arena.zero_grad()
        m = self.model
        m.proposal_sampler.force_updated = updated
        rb = RayBundle(origins=self.rb.origins, directions=self.rb.directions, pixel_area=self.rb.pixel_area,
                       camera_indices=self.rb.camera_indices)
        out = m(rb)
        metrics = m.get_metrics_dict(out, self.batch)
        loss_dict = m.get_loss_dict(out, self.batch, metrics)
        loss = sum(loss_dict.values())
        loss.backward()
        self.loss_buf.copy_(loss.detach())
        if self.dp:
            self.arena.all_reduce()
        self.arena.step(grad_scale=1.0 / self.world, groups=self._stepped(updated, pending=False), hyper_dev=self.hyper_views)

    def _pool_select(self):
        """(slot pointer, slots, pool) of the step's batch where the runner's `forward_proposals` selects it out of the pool
        itself (no source, no camera optimiser: the kernels read what the selection copies), else None."""
        r = self.runner
        if self.source is not None or self.pool is None or r is None or r.cam_opt is not None or not r.fuse_select:
            return None
        return (N.ptr(self.hyper[_HYPER_SLOT:_HYPER_SLOT + 1]), self.slots, self.pool)

    def _select_batch(self):
        """This step's rays out of the HBM-resident pool (slot index in device memory: replayable) — the hand-over the
        reference's datamanager does each iteration (base_datamanager.py:506-515)."""
        if self.source is not None:
            if self.source_inside:
                # sampled here, inside the body: the prologue (first node) has already advanced the draw counter, hence -1
                r = self.runner
                co = r.cam_opt is not None  # the kernels read the pose-corrected copies
                o, d = (r.raw_origins, r.raw_directions) if co else (r.origins, r.directions)
                self.source.launch(o, d, r.camera_indices, r.target, self.step_counter[1:], -1)
            return  # (else: `_source_batch` has filled the buffers ahead of the iteration)
        if self.pool is None:
            return
        from . import functional as F

        p = self.pool
        if self.runner is not None:
            r = self.runner
            co = r.cam_opt is not None  # the kernels read the pose-corrected copies
            select = self._pool_select()
            if select is not None:
                # the runner's next `forward_proposals` selects the batch in the launch that writes the initial bins
                r.pending_select = select
                return
            o, d = (r.raw_origins, r.raw_directions) if co else (r.origins, r.directions)
            c, t = r.camera_indices, r.target
        else:
            o, d, c, t = self.rb.origins, self.rb.directions, self.rb.camera_indices, self.batch["image"]
        F.select_batch_launch(self.hyper[_HYPER_SLOT:_HYPER_SLOT + 1], self.slots, p["origins"], p["directions"], p["cameras"],
                              p["target"], o, d, c, t)

    def _source_batch(self):
        """The eager form of a source (class docstring): `next_batch()` into the static buffers, ahead of the iteration."""
        rb, batch = self.source.next_batch()
        self.runner.set_batch(rb.origins, rb.directions, rb.camera_indices.reshape(-1), batch["image"])

    # -- camera optimiser: the host-side halves around the captured part ---------------------------------------------------
    @property
    def _cams_outside(self):
        return self.runner is not None and self.runner.cameras_outside

    def _cameras_before(self):
        """Batch selection + pose corrections (cameras/camera_optimizers.py:148-153), eagerly, ahead of the replay."""
        self._select_batch()
        self.runner.apply_camera_corrections()

    def _cameras_after(self, updated):
        """dL/d(origins, directions) per ray -> pose_adjustment.grad (+ the L2 regulariser), the group's exchange and Adam."""
        a, g = self.arena, self.cam_group
        if g is None:
            return
        a.zero_grad([g])
        self.runner.backward_cameras(updated, force=True)
        if self.dp:
            h = a.all_reduce_group(g)
            if h is not None:
                h.wait()
        a.step(grad_scale=1.0 / self.world, groups=[g], hyper_dev=self.hyper_views)

    # -- data-parallel segments (N > 1, runner) --------------------------------------------------------------------------
    @property
    def pipelined(self):
        return self.dp and self.runner is not None

    def _seg(self, name):
        """The body of one captured segment (also what the eager path runs)."""
        r, a = self.runner, self.arena
        if name == "pfwd":
            self._step_prologue()  # (the step's draws; the scalars were uploaded by `_push_hyper`)
            if not self._cams_outside:
                self._select_batch()
                r.apply_camera_corrections()
            r.forward_proposals(self.draw_jitter and not self.prologue)
        elif name in (("main", True), ("main", False)):
            if name[1] and self.dp_fork:
                # update step, eager launches: the proposal chains start on their side streams here, beside the main chain
                # (as in the N = 1 schedule) — and, since the exchange starts the main-field collective right after this
                # segment, beside that too; "pbwd" only joins them
                self._zero(True)
                r.forward_main_and_losses(True)
                r.backward_fork(True)
            else:
                self._zero(False)
                if name[1]:
                    self._clear_gates()
                r.forward_main_and_losses(name[1])
                r.backward_main()
        elif name == "pbwd":
            if self.dp_fork:
                r.backward_join(True)
            else:
                self._zero(True, groups=["proposal_networks"])
                r.backward_proposals()
        elif name in ("mopt", "popt"):
            grp = "fields" if name == "mopt" else "proposal_networks"
            if self.dp_sharded:  # this rank's 1/N of the group; the exchange all-gathers the updated parameters
                a.step_shard(grp, grad_scale=1.0 / self.world, hyper_dev=self.hyper_views)
            else:
                a.step(grad_scale=1.0 / self.world, groups=[grp], hyper_dev=self.hyper_views)
        else:
            raise KeyError(name)

    def _run(self, name):
        if self.graphs is not None:
            self.graphs[name].replay()
            if name == "mopt":
                self.arena.step_counts["fields"] += 1  # the replayed Adam launch did step the group
            elif name == "popt":
                self.arena.step_counts["proposal_networks"] += 1
        else:
            self._seg(name)

    def finish(self):
        """Apply every pending update: afterwards the parameters reflect every iteration taken (callers: the end of a timed
        region, evaluation, checkpointing)."""
        if self.exchange is not None:
            self.exchange.finish()
        if self._pending_main:  # deferred schedule: the last iteration's main-field update
            self._push_hyper(direct=True)
            self.arena.step(grad_scale=1.0, groups=["fields"], hyper_dev=self.hyper_views)
            self._pending_main = False
            self._true_steps = dict(self.arena.step_counts)

    @property
    def _have_pending(self):
        return self._pending_main or (self.exchange is not None and self.exchange.pending)

    # -- graph capture ---------------------------------------------------------------------------------------------
    def warm_variants(self):
        """One eager iteration of each schedule variant (proposal networks updated / not) on a side stream — allocator and
        lazy-attribute warm-up ahead of a capture. They are real training iterations (parameters and Adam state move) that
        do not advance the step counter; an eager run that is to train through the same states as a captured one calls
        this at the same point (tests/test_gpu_bench_parity.py)."""
        torch.cuda.synchronize()
        assert not self._have_pending
        side = torch.cuda.Stream()
        side.wait_stream(N.current_stream())
        with N.on_stream(side):
            defer, self.defer = self.defer, False  # (in order, so that every schedule trains through the same states)
            for upd in (True, False):
                self._iteration(upd, replay=False)
            self.finish()
            self.defer = defer
        N.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def capture(self, warm: bool = True):
        """warm=False: the caller has already run eager iterations of this schedule (kernel attributes, lazily built
        workspaces and the allocator are warm) and must not train twice on one batch (pipeline.HipPipeline)."""
        if warm:
            self.warm_variants()
        else:
            self.finish()
            torch.cuda.synchronize()
        graphs = {}
        if self.pipelined:
            from .dp_schedule import SEGMENTS

            self.dp_fork = False  # captured segments keep the proposal backward in its own segment
            for name in SEGMENTS:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._seg(name)
                graphs[name] = g
        else:
            for upd in (True, False):
                for pend in ((True, False) if self.defer else (False,)):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):  # the whole iteration is one graph
                        if self.runner is not None:
                            self._body(upd, pend)
                        else:
                            self._module_body(upd)
                    graphs[("all", upd, pend)] = g
        for name in self.arena.step_counts:  # captures executed nothing; undo the host-side counters they bumped
            self.arena.step_counts[name] = self._true_steps[name]
        self.graphs = graphs

    def try_capture(self, warm: bool = True):
        if not self.use_graph or (self.dp and not self.pipelined):
            return False
        try:
            self.capture(warm)
            return True
        except Exception as e:  # noqa: BLE001 - any capture problem degrades to the eager path, never to no result
            print(f"[nerfstudio_amd.trainer] hipGraph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr)
            self.graphs = None
            try:
                torch.cuda.synchronize()
            except Exception:  # noqa: BLE001
                pass
            return False

    # -- one training iteration ------------------------------------------------------------------------------------
    def _iteration(self, updated, replay):
        """The host's share around an iteration's body: the model's step callback, the step's scalars, the camera parts
        outside the captured body; the body itself runs as eager launches, as the replay of its captured variant, or as the
        data-parallel segments (which replay their own graphs once captured)."""
        pending = self._pending_main
        if self.drive_callbacks:
            self.model.set_step(self.step)  # BEFORE_TRAIN_ITERATION callback: proposal weight anneal
        self._push_hyper()
        if self.source is not None and not self.source_inside:
            self._source_batch()
        if self._cams_outside:
            self._cameras_before()
        if self.pipelined:
            self.exchange.iteration(updated)
        elif replay:
            self.graphs[("all", updated, pending)].replay()
            for name in self._stepped(updated, pending):
                self.arena.step_counts[name] += 1  # the replayed Adam launches did step these groups
        elif self.runner is not None:
            self._body(updated, pending)
        else:
            self._module_body(updated)
        if self.defer:
            self._pending_main = True
        if self._cams_outside:
            self._cameras_after(updated)
        self._true_steps = dict(self.arena.step_counts)

    def train_iteration(self):
        ps = self.model.proposal_sampler
        updated = ps.updated_this_step()
        self._iteration(updated, replay=self.graphs is not None)
        self.opt_step += 1
        if updated:
            ps.mark_updated()
        if self.drive_callbacks:
            self.model.after_step(self.step)  # AFTER_TRAIN_ITERATION callback
        self.step += 1
        return self.loss_buf

    def last_loss(self):
        if self.runner is not None:
            return sum(self.runner.loss_dict().values())
        return self.loss_buf

    def loss_dict(self) -> Dict[str, torch.Tensor]:
        return self.runner.loss_dict()
