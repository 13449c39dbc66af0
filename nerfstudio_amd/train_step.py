"""One nerfacto training iteration as an explicit kernel schedule (no autograd graph, no torch arithmetic).

What the reference does per step (engine/trainer.py:487-531 -> pipelines/base_pipeline.py:290-303 ->
models/nerfacto.py:298-392): collider, ProposalNetworkSampler (3 levels), NerfactoField, weights, renderers, MSE +
interlevel + distortion losses, `backward()`, optimiser. `NerfactoModel` (nerfacto.py) reproduces that through the
module API with autograd; `NerfactoTrainStep` issues THE SAME kernels in a fixed order over buffers allocated once:

  forward : forward_step.NerfactoForward, its base (the schedule an eval render runs on its own) -> weights_fwd -> composite_fwd
  backward: mse_loss, distortion_loss, interlevel_loss x 2 (value + gradient in one pass each)
            -> composite_bwd -> weights_bwd -> field_mlp_bwd -> hash_bwd(main)
            -> (only on proposal-update steps, ray_samplers.py:590) weights_bwd -> density_mlp_bwd -> hash_bwd x 2

The base owns the rays, the sampler state and the fields' outputs; this class adds the target, the levels' kept features, every
gradient and loss buffer, workspaces, gates, streams and events, the camera optimiser, the normals stage, depth supervision.

~25 launches, every one a libnsamd kernel (round 5: batch selection + initial bins are one launch, the main field's
weight-gradient reduce rides the table scatter's apply pass; the fully merged forms of the per-ray stages were bit-identical and
measured slower — csrc/experiments/rounds2to5_opt_in_variants.patch); parameter gradients
accumulate directly into `param.grad` (the views of arena.ParamArena). Nothing here depends on host-side values that change from step to step (the jitter is drawn on the
device, the anneal exponent lives in device memory), so the whole iteration can be captured in a hipGraph once per
schedule variant and replayed. Numerically identical to the autograd path (tests/test_gpu_kernels.py compares them).

The launches this schedule shares with the module path (or with trainer / eval_render) go through the helpers of functional.py
— depth_loss_launch, field_normals_launch, nerf_encode_launch, linear_launch, normals_losses_launch, normals_composite_launch,
distance_gradient_scale_launch, weights_backward_launch, camera_apply_launch, camera_backward_launch, select_batch_launch
and the field helpers — with this runner's static buffers; the entry points only this schedule launches are called here.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _native as N
from . import functional as F
from .forward_step import NerfactoForward
from .nerfacto import NerfactoModel
from .runner_interface import TrainStepRunner
from .utils import profiler


class NerfactoTrainStep(NerfactoForward, TrainStepRunner):
    def __init__(self, model: NerfactoModel, num_rays: int, device, compute_depths: bool = True) -> None:
        super().__init__(model, num_rays, device, compute_depths)
        cfg, n, mm = self.cfg, self.n, self.m_main
        self.gradient_scaling = bool(getattr(cfg, "use_gradient_scaling", False))
        # the normals stage of a `predict_normals` model whose field carries the modules (the eval render has its own,
        # eval_render.EvalRenderer)
        want_normals = bool(getattr(cfg, "predict_normals", False)) and bool(getattr(model.field, "use_pred_normals", False))
        if want_normals and self.gradient_scaling:
            # the reference scales the predicted normals' gradient as well (models/nerfacto.py:321-322)
            raise NotImplementedError("explicit schedule: predict_normals together with use_gradient_scaling is only on the "
                                      "module path")
        f32 = dict(device=device, dtype=torch.float32)
        e = lambda *shape: torch.empty(shape, **f32)  # noqa: E731
        if cfg.background_color == "random":
            # the rendered colour carries no background; the loss blends `rand_like(pred) * (1 - accumulation)` into the
            # prediction (renderers.py:112-115, 194-196; models/nerfacto.py:377-381) — a per-ray colour the kernels read
            # (zero-initialised: callers that inject the jitter — `draw_jitter=False` — and no background of their own
            # composite against black, never against uninitialised memory)
            self.bg_rays = torch.zeros((n, 3), **f32)
        self.target = e(n, 3)
        for lvl, m in enumerate(x.numel() for x in self.p_dens):  # what forward_proposals(need_enc=True) keeps of the levels
            self.p_enc[lvl], self.p_sel[lvl], self.p_pre[lvl] = e(self.props[lvl].encoding.get_out_dim(), m), e(m), e(m)
        # ---- losses / gradients ----
        self.sq_err = e(n)  # per-ray sum of squared rgb errors
        self.dist_per_ray = e(n)
        self.inter_per_ray = [e(n) for _ in range(self.n_prop)]
        self.d_rgb_out = e(n, 3)
        self.dw_dist = e(n, self.counts[-1])
        self.dw_prop = [e(n, self.counts[lvl]) for lvl in range(self.n_prop)]
        self.d_rgb_s, self.d_dens_main = e(mm, 3), e(mm)
        # host arrays of device pointers for nsamd_proposal_losses (the buffers are static, so built once)
        self._pl_s_bins = N.ptr_array(self.s_bins[: self.n_prop])
        self._pl_weights = N.ptr_array(self.weights[: self.n_prop])
        self._pl_per_ray = N.ptr_array(self.inter_per_ray)
        self._pl_dw = N.ptr_array(self.dw_prop)
        self._pl_S = (C.c_int32 * self.n_prop)(*self.counts[: self.n_prop])
        if self.ray_terms_on:  # their inputs, kept for the backward: weight gradient of the 48 per-ray columns
            self.ray_inputs = e(n, 16 + (32 if model.field.embedding_appearance is not None else 0))
        # Saved tile (include/nsamd.h, nsamd_field_mlp.saved_hb): the forward leaves head layer 1's output, as its wavefronts hold
        # it, for the backward of the same step, which reads it and `f_rgb` instead of recomputing head layers 1 and 2. Whole
        # 16-sample tiles, zeroed once: a partial last tile's absent samples are never written. A static address, so a captured
        # iteration stays valid. `_saved_fresh`: the tile is that of the last `forward_main`.
        self.saved_hb = torch.zeros(((mm + 15) // 16, 4, 64, 4), **f32)
        self._saved_fresh = False
        self.f_denc = e(*self.f_enc.shape)
        self.p_ddens = [e(*x.shape) for x in self.p_dens]
        self.p_denc = [e(*x.shape) for x in self.p_enc]
        self.field_ws = F.field_bwd_workspace(device)[0]
        # one scratch per proposal level: their backward chains may run concurrently on different streams
        self.density_ws = [F.density_bwd_workspace(device, slot=lvl) for lvl in range(self.n_prop)]
        # Zero-gradient gating of the proposal chains (include/nsamd.h): one device flag per level, raised by the level's
        # weights backward when any ray carries interlevel-loss gradient; while it is clear the rest of the chain
        # (density MLP backward, table scatter, ray gradients) returns at once — the zero-filled gradients are the result.
        # False: the ungated entry points.
        self.gate_proposals = True
        self.prop_gates = torch.zeros(max(self.n_prop, 1) * 4, device=device, dtype=torch.int32)  # 16 B apart
        self.gates_precleared = False  # True: the caller zeroes `prop_gates` before every proposal backward (trainer.HipTrainer)
        # ... and its per-ray form (1 = the ray carries gradient): levels that are only partly without gradient
        self.prop_ray_masks = [torch.zeros(n, device=device, dtype=torch.uint8) for _ in range(self.n_prop)]
        # The main field's backward emits the table scatter's pass-1 records itself (nsamd_field_mlp_bwd_scatter: no `denc`
        # round trip, no route launch); NSAMD_FUSE_ROUTE=0: the two entry points (A/B).
        self.fuse_route = os.environ.get("NSAMD_FUSE_ROUTE", "1") == "1"
        self.keep_denc = False  # True: the fused launch also stores the encoded-feature gradient in `f_denc` (tests read it)
        # the same stage of the proposal levels' backward chains as one launch across the levels (False: level by level)
        self.merge_prop_levels = True
        # the iteration's loss values and training metrics, written by the losses launch's finishing pass (nsamd.h):
        # rgb_loss, interlevel_loss, distortion_loss, psnr, distortion, sum of the three losses
        self.loss_vals = torch.zeros(32, **f32)  # (8 results + the finishing pass's scratch: partial sums, ticket)
        self._loss_vals_fresh = False
        self.want_loss_vals = False  # the separate-launch path: also launch nsamd_train_loss_values (set by pipeline.TrainEngine)
        # (slot pointer, slots, pool) of a batch selection the caller leaves to `forward_proposals` (one launch with the initial
        # bins, nsamd_select_bins); NSAMD_FUSE_SELECT=0: the caller launches nsamd_select_batch itself (A/B)
        self.pending_select = None
        # depth supervision (set_depth_target): None = today's launches, nothing else
        self.depth = self._depth_buffers = None
        self._slot0 = None  # a device zero: `set_batch` as a one-slot batch selection
        self._outputs = None
        self.fuse_select = os.environ.get("NSAMD_FUSE_SELECT", "1") == "1"
        # update steps: the main backward chain is issued (and its graph nodes created) before the proposal chains' fork, so
        # that a replayed graph keeps composite_bwd on the losses' hardware queue (backward_fork)
        self.main_chain_first = True
        # Second stream for the proposal-network backward: the two backward chains are independent, and since the
        # scatter kernels were reworked (latency-bound phases, small workgroups) they overlap: 3.87 -> 4.02 M rays/s on
        # MI355X (profiles/). `side_stream = None` runs them back to back (the data-parallel path does: its proposal
        # chain is the cover for the main-field all-reduce).
        # Every level's chain on this ONE side stream (round 6, profiles/r06_s19_*: three alternating repeats, window
        # 0.6265 / 0.6304 / 0.6275 against 0.6494 / 0.6512 / 0.6278 ms with a stream per level, long run 0.689 against 0.695; the
        # chains in line on the main stream 0.674 / 0.736 — same bits in all three).
        self.side_stream = torch.cuda.Stream(device=device)
        self._fork, self._join = torch.cuda.Event(), torch.cuda.Event()
        self._open_branches = []  # the proposal_branches() `backward_fork` has started and `backward_join` has yet to wait for
        # camera optimiser: the rays' gradient through the main grid on its own stream, beside the table scatter's apply pass
        # (see backward_field_and_table)
        self.reduce_stream = torch.cuda.Stream(device=device)
        self._red_fork, self._red_join = torch.cuda.Event(), torch.cuda.Event()
        # ---- camera optimiser (nerfstudio's nerfacto default is SO3xR3, the benchmark recipe is "off") ----
        # Host-side torch computes the corrected rays from `pose_adjustment` (a [num_cameras, 6] parameter); the kernels
        # return dL/d(origins, directions) per ray (nsamd_hashgrid_encode_bwd_rays, one buffer per sampling level so that
        # the levels' backward chains stay independent), and autograd carries it back to the parameter.
        co = getattr(model, "camera_optimizer", None)
        self.cam_opt = co if (co is not None and co.config.mode != "off") else None
        # The exponential map, the pose-to-ray arithmetic and their backward as two launches (nsamd_camera_apply /
        # nsamd_camera_backward) instead of ~100 eager torch kernels + autograd nodes: any optimiser with the reference's
        # parameterisation (a [num_cameras, 6] `pose_adjustment`, mode SO3xR3 / SE3, every camera trainable) — this
        # package's or the reference's own. NSAMD_CAMERA_KERNELS=0: the torch route (A/B).
        self.cam_kernels = False
        if self.cam_opt is not None:
            pose = getattr(co, "pose_adjustment", None)
            self.cam_kernels = (os.environ.get("NSAMD_CAMERA_KERNELS", "1") == "1" and pose is not None and pose.is_cuda
                                and pose.dtype == torch.float32 and pose.dim() == 2 and pose.shape[1] == 6
                                and co.config.mode in ("SO3xR3", "SE3")
                                # nsamd_ray_grads has four slots: the levels' and the normals chain's
                                and len(self.counts) + int(want_normals) <= 4
                                and getattr(co, "non_trainable_camera_indices", None) is None)
            self.cam_mode = F.CAMERA_MODES.get(co.config.mode, 0)
            self.raw_origins, self.raw_directions = e(n, 3), e(n, 3)
            self.d_origins = [e(n, 3) for _ in self.counts]
            self.d_directions = [e(n, 3) for _ in self.counts]
            self._corrected = None
            self.camera_reg = torch.zeros((), **f32)
        self.normals = self._normals_buffers(device) if want_normals else None
        self._normals_fresh = False  # the stage's results belong to the last forward_main
        self.reg_in_backward = True  # backward_cameras also differentiates the pose regulariser
        # True: `backward_join` leaves the camera optimiser's share to the caller (`backward_cameras(updated, force=True)`
        # after a replayed graph: the exponential map's autograd graph is host-side torch and stays out of the capture)
        self.cameras_outside = False
        self.grad_lookup = None  # {id(parameter): gradient buffer} of an arena that does not bind `param.grad`
        self.main_table_write_only = True  # the main table's gradient is written, not accumulated (written_params)

    # -------------------------------------------------------------------------------------------------------------
    def set_batch(self, origins: Tensor, directions: Tensor, camera_indices: Tensor,
                  target_rgb: Optional[Tensor] = None) -> None:
        cams = camera_indices.reshape(-1)
        if (target_rgb is not None and origins.is_cuda and all(
                x.dtype == torch.float32 and x.is_contiguous() and x.shape == (self.n, 3) and x.device == self.origins.device
                for x in (origins, directions, target_rgb)) and cams.dtype == torch.int64 and cams.is_contiguous()
                and cams.shape[0] == self.n and cams.device == self.origins.device):
            # a datamanager's device-resident batch: ONE launch (a pool of one slot) instead of four copy kernels
            if self._slot0 is None:
                self._slot0 = torch.zeros(1, device=self.origins.device)
            o, d = (self.raw_origins, self.raw_directions) if self.cam_opt is not None else (self.origins, self.directions)
            F.select_batch_launch(self._slot0, 1, origins, directions, cams, target_rgb, o, d, self.camera_indices, self.target)
            return
        if self.cam_opt is not None:  # the kernels see the pose-corrected rays (apply_camera_corrections)
            self.raw_origins.copy_(origins)
            self.raw_directions.copy_(directions)
        else:
            self.origins.copy_(origins)
            self.directions.copy_(directions)
        self.camera_indices.copy_(camera_indices.reshape(-1))
        if target_rgb is not None:
            self.target.copy_(target_rgb)

    def set_depth_target(self, termination_depth: Optional[Tensor], directions_norm: Optional[Tensor] = None,
                         sigma: float = 0.01, mult: float = 1e-3, is_euclidean: bool = False, loss_type: int = 1) -> None:
        """Depth supervision of depth-nerfacto (models/depth_nerfacto.py:90-104, :124-125) on the explicit schedule, DS_NERF only:
        with a target set, `losses()` issues one nsamd_depth_loss launch behind nsamd_proposal_losses that ADDS mult * d(depth
        loss) to `dw_dist` and — on proposal-update steps, where the reference's proposal weights carry gradient — to
        `dw_prop`; `loss_dict()` reports `depth_loss`. termination_depth `[n]` / `[n,1]` (None: no depth supervision again),
        directions_norm likewise (required unless the depth is Euclidean). The buffers are static: a new target of the same
        batch size is copied into them. Eager launches only: trainer.HipTrainer and captured graphs decline."""
        if termination_depth is None:
            self.depth = None  # (the static buffers stay in `_depth_buffers` for the next target)
            return
        loss_type = int(getattr(loss_type, "value", loss_type))
        if loss_type != F.DEPTH_DS_NERF:
            raise NotImplementedError("explicit schedule: only the DS_NERF depth loss; URF and the depth ranking loss are "
                                      "on the module path")
        if not is_euclidean and directions_norm is None:
            raise ValueError("a depth that is not Euclidean needs directions_norm")
        d = self._depth_buffers
        if d is None:
            f32 = dict(device=self.origins.device, dtype=torch.float32)
            d = self._depth_buffers = {"target": torch.empty(self.n, **f32), "norm": torch.empty(self.n, **f32),
                                       "per_ray": torch.empty(len(self.counts), self.n, **f32), "value": torch.zeros((), **f32)}
        d["target"].copy_(termination_depth.reshape(-1))
        if not is_euclidean:
            d["norm"].copy_(directions_norm.reshape(-1))
        d["euclidean"], d["sigma"], d["mult"] = bool(is_euclidean), float(sigma), float(mult)
        self.depth = d

    def _normals_buffers(self, device) -> Dict[str, object]:
        """Static buffers of the normals stage, allocated once: per-sample analytic normals, the predicted-normals MLP's 27-wide
        input rows (12 encoded columns | 15 geometry features), the KEPT activations of its three layers and the head's
        pre-activation, the per-ray terms and rendered channels; for the backward the pre-activation's gradient, two ping-pong
        `[M, 64]` gradient blocks (the base MLP's recomputed hidden activations reuse one), the input rows' gradient, the base
        output's 16-wide gradient (column 0, the density pre-activation, stays zero), the row-major hash features and their
        gradient; with a camera optimiser the loss's view-direction gradient and one more (d_origins, d_directions) pair. The
        accumulating table scatter's cached workspace for this sample count is taken here as well."""
        f32 = dict(device=device, dtype=torch.float32)
        e = lambda *shape: torch.empty(shape, **f32)  # noqa: E731
        n, mm = self.n, self.m_main
        fld = self.model.field
        pe = fld.position_encoding
        cam = self.cam_opt is not None
        F._scatter_workspace(fld.mlp_base.encoding.spec, device, mm)  # the accumulating table scatter's workspace: here, not lazily
        return {"freqs": (2 ** torch.linspace(pe.min_freq, pe.max_freq, pe.num_frequencies)).to(device),
                "n_smp": e(mm, 3), "enc": e(mm, 12), "in": e(mm, 27), "act": [e(mm, 64) for _ in range(3)], "pre": e(mm, 3),
                "orientation": e(n), "pred": e(n), "normals_img": e(n, 3), "pred_img": e(n, 3),
                "d_pre": e(mm, 3), "d_a": e(mm, 64), "d_b": e(mm, 64), "d_in": e(mm, 27), "dy16": torch.zeros((mm, 16), **f32),
                "enc_rows": e(mm, 32), "d_enc": e(mm, 32), "d_dir_loss": e(n, 3) if cam else None,
                "d_origins": e(n, 3) if cam else None, "d_directions": e(n, 3) if cam else None}

    def _normals_rows(self):
        """The predicted-normals branch's row buffers: each layer's input and, one further, its output."""
        nb = self.normals
        return (nb["in"], *nb["act"], nb["pre"])

    @profiler.time_function
    def normals_forward(self) -> None:
        """The normals stage of `losses` (models/nerfacto.py:325-344), behind the weights: analytic normals and the geometry
        features from the hash features forward_main left, the predicted-normals branch with its activations kept, the two
        loss terms with their gradients (to the head's pre-activation; to the view directions for a camera optimiser) and the
        two rendered channels. It depends on nothing `losses` takes from the target, so a second `losses` of the same forward
        (FusedTrainStep: once for the outputs, once with the real target) does not repeat it."""
        from .eval_render import pred_normals_layers

        if self._normals_fresh:
            return
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("explicit schedule: predict_normals inside a captured graph; normals in captured "
                                      "iterations are only on the module path")
        nb, fld, cfg, n = self.normals, self.model.field, self.cfg, self.n
        L, M = self.n_prop, self.m_main
        pts = self._points(L)
        enc = fld.mlp_base.encoding
        F.field_normals_launch(pts, M, fld._transform, fld._box, enc.hash_table, enc.spec, self.f_enc,
                               fld.mlp_base.mlp.param_tensors(), nb["n_smp"], None, nb["in"], 27, 12)
        F.nerf_encode_launch(pts, M, nb["freqs"], False, nb["enc"])
        nb["in"][:, :12].copy_(nb["enc"])  # (the encoder writes dense 12-wide rows)
        rows = self._normals_rows()
        for i, (W, b, act) in enumerate(pred_normals_layers(fld)):
            F.linear_launch(rows[i], W, b, M, act, rows[i + 1])
        F.normals_losses_launch(self.weights[L], nb["n_smp"], nb["pre"], self.directions,
                                float(cfg.orientation_loss_mult) / n, float(cfg.pred_normal_loss_mult) / n, nb["orientation"],
                                nb["pred"], nb["d_pre"], nb["d_dir_loss"])
        F.normals_composite_launch(self.weights[L], nb["n_smp"], nb["pre"], nb["normals_img"], nb["pred_img"])
        self._normals_fresh = True

    @profiler.time_function
    def normals_backward(self) -> None:
        """The predicted-normal loss's gradient chain, on the current stream behind backward_main (whose table scatter writes;
        everything here ACCUMULATES): head and the three layers of the predicted-normals MLP down to its input rows; their
        geometry-feature columns through the base MLP (hidden activations recomputed from a row-major copy of the hash
        features) and the table scatter; with a camera optimiser the rays' share — through the hash grid, through the
        frequency encoding of the raw positions, and the orientation loss's view-direction gradient — into one more
        (d_origins, d_directions) pair for backward_cameras."""
        from .eval_render import pred_normals_layers

        nb, fld = self.normals, self.model.field
        L, M = self.n_prop, self.m_main
        pts = self._points(L)
        layers, rows = pred_normals_layers(fld), self._normals_rows()
        d_rows = (nb["d_in"], nb["d_a"], nb["d_b"], nb["d_a"], nb["d_pre"])
        for i in range(len(layers) - 1, -1, -1):
            W, b, act = layers[i]
            F.linear_backward_launch(rows[i], W, rows[i + 1], d_rows[i + 1], M, act, d_rows[i], self._grad(W), self._grad(b))
        # base MLP: layer 1 (64 -> 16, no activation) from dy = [0 | d geometry features], layer 0 (32 -> 64, ReLU)
        W0, b0, W1, b1 = fld.mlp_base.mlp.param_tensors()
        hidden, d_hidden = nb["d_b"], nb["d_a"]
        nb["enc_rows"].copy_(self.f_enc.t())  # (the hash forward leaves the features feature-major)
        F.linear_launch(nb["enc_rows"], W0, b0, M, 1, hidden)
        nb["dy16"][:, 1:].copy_(nb["d_in"][:, 12:])
        F.linear_backward_launch(hidden, W1, None, nb["dy16"], M, 0, d_hidden, self._grad(W1), self._grad(b1))
        F.linear_backward_launch(nb["enc_rows"], W0, hidden, d_hidden, M, 1, nb["d_enc"], self._grad(W0), self._grad(b0))
        tbl = fld.mlp_base.encoding
        F.table_scatter(pts, M, fld._transform, fld._box, tbl.hash_table, tbl.spec, nb["d_enc"], 32, 1,
                        self._grad(tbl.hash_table))
        if self.cam_opt is not None:
            nb["d_origins"].zero_()
            nb["d_directions"].copy_(nb["d_dir_loss"])
            N.check(N.load().nsamd_hashgrid_encode_bwd_rays(pts, M, fld._transform, fld._box, N.ptr(tbl.hash_table),
                                                            tbl.spec.native(), N.ptr(nb["d_enc"]), 32, 1, N.ptr(nb["d_origins"]),
                                                            N.ptr(nb["d_directions"]), 1, N.stream()), "hashgrid_encode_bwd_rays")
            F.nerf_encode_bwd_rays_launch(pts, M, nb["freqs"], False, nb["d_in"], 27, nb["d_origins"], nb["d_directions"],
                                          accumulate=True)

    def prepare_grads(self, updated: bool) -> None:
        """For callers without a gradient arena (a trainer that runs `zero_grad(set_to_none=True)`, engine/optimizers.py:
        160-172): give every parameter this iteration produces a gradient for a buffer. Fresh buffers are zero-filled,
        except the main table's, which the scatter writes; a gradient that already exists is accumulated into
        (gradient accumulation), the main table's included."""
        fld = self.model.field
        table = fld.mlp_base.encoding.hash_table
        self.main_table_write_only = table.grad is None
        owners = [fld] + (list(self.model.proposal_networks) if updated else [])
        for mod in owners:
            for prm in mod.parameters():
                if prm.requires_grad and prm.grad is None:
                    prm.grad = torch.empty_like(prm) if prm is table else torch.zeros_like(prm)

    def _grad(self, p: Tensor) -> Tensor:
        if self.grad_lookup is not None:  # an arena that keeps `param.grad` unset (arena.ParamArena(bind_grads=False))
            g = self.grad_lookup.get(id(p))
            if g is not None:
                return g
        assert p.grad is not None and p.grad.is_contiguous(), "parameters need preallocated .grad (use arena.ParamArena)"
        return p.grad

    # -------------------------------------------------------------------------------------------------------------
    def forward_backward(self, updated: bool, draw_jitter: bool = True) -> None:
        """One iteration up to (not including) the optimiser. `updated`: proposal networks receive gradient this step
        (ProposalNetworkSampler.updated_this_step()). Gradients ACCUMULATE into param.grad (zero them first)."""
        self.forward_and_losses(updated, draw_jitter)
        self.backward_all(updated)

    def proposal_branches(self):
        """[(stream, join event, proposal levels)]: how the proposal backward splits over streams — every level on the one
        side stream, or [] without a side stream."""
        return [] if self.side_stream is None else [(self.side_stream, self._join, None)]

    def backward_all(self, updated: bool) -> None:
        """Everything after the losses: the main backward chain, the proposal chains on the steps that update them
        (parallel streams where they share nothing; parallel branches inside a captured hipGraph), and the camera
        optimiser's share."""
        self.backward_fork(updated)
        self.backward_join(updated)

    def backward_fork(self, updated: bool) -> None:
        """First half of backward_all: the proposal chains go onto their side streams (not yet joined), the main chain runs
        on the current stream. A data-parallel caller starts the main-field gradient exchange between this and
        backward_join — the proposal chains then run beside the main chain AND beside the collective."""
        branches = self.proposal_branches() if updated else []
        self._open_branches = branches
        if branches:
            # The backward chains are independent (disjoint gradients, separate scratch): fork the proposal chains onto
            # their own streams so that these latency-bound kernels overlap with the main chain.
            # The main chain is issued FIRST: inside a captured graph the fork's first-created child stays on its parent's
            # hardware queue and every further child starts on another one, 8-11 us late. The main chain's 6 us compositing
            # backward is the critical one; created second it hopped, and the field backward behind it started 19 instead
            # of 11 us after the losses, into the proposal chains' first kernel (profiles/critical_chain_hops_ab.txt:
            # -15 us per step on the long run). The dependencies are the same either way.
            main = N.current_stream()
            self._fork.record(main)
            if self.main_chain_first:
                self.backward_main()
                if self.normals is not None:
                    self.normals_backward()
            for stream, join, levels in branches:
                stream.wait_event(self._fork)
                with N.on_stream(stream):
                    self.backward_proposals(levels=levels)
                    join.record(stream)
            if not self.main_chain_first:
                self.backward_main()
                if self.normals is not None:
                    self.normals_backward()
        else:
            self.backward_main()
            if self.normals is not None:
                self.normals_backward()
            if updated:
                self.backward_proposals()

    def backward_join(self, updated: bool) -> None:
        """Second half of backward_all: wait for the proposal chains, then the camera optimiser's share."""
        main = N.current_stream()
        for _, join, _ in self._open_branches:
            main.wait_event(join)
        self._open_branches = []
        self.backward_cameras(updated)

    def written_params(self):
        """Parameters whose gradient this runner WRITES (hash tables, nsamd_hashgrid_encode_bwd_set): callers need not
        zero them (ParamArena.zero_grad(skip=...)). All other gradients accumulate and must be zeroed first."""
        # Only the 67 MB main table: for the 5 MB proposal tables the zero-fill is nothing and the accumulating call needs
        # no worst-case spill list.
        return [self.model.field.mlp_base.encoding.hash_table] if self.main_table_write_only else []

    def forward_and_losses(self, updated: bool, draw_jitter: bool = True) -> None:
        self.apply_camera_corrections()
        self.forward_proposals(draw_jitter, need_enc=updated)
        self.forward_main_and_losses(updated)

    # ---- camera optimiser -----------------------------------------------------------------------------------------
    def apply_camera_corrections(self) -> None:
        """origins + t, R @ directions with the current pose corrections (camera_optimizers.py:148-153) into the ray
        buffers the kernels read; the autograd graph of the tiny exponential map is kept for backward_cameras."""
        if self.cam_opt is None:
            return
        if self.cam_kernels:
            F.camera_apply_launch(self.cam_opt.pose_adjustment, self.cam_mode, self.raw_origins, self.raw_directions,
                                  self.camera_indices, self.origins, self.directions)
            return
        if hasattr(self.cam_opt, "corrected_rays"):
            o, d = self.cam_opt.corrected_rays(self.raw_origins, self.raw_directions, self.camera_indices)
        else:  # the reference's own CameraOptimizer: forward(indices) -> [n,3,4] corrections (camera_optimizers.py:107-153)
            c = self.cam_opt(self.camera_indices)
            o = self.raw_origins + c[:, :3, 3]
            d = torch.bmm(c[:, :3, :3], self.raw_directions[..., None]).squeeze(-1)
        self._corrected = (o, d)
        self.origins.copy_(o.detach())
        self.directions.copy_(d.detach())

    def _gate(self, lvl: int):
        """Device address of proposal level `lvl`'s gradient flag (None: gating off)."""
        return self.prop_gates.data_ptr() + 16 * lvl if self.gate_proposals else None

    def _rays_backward(self, lvl: int, net, denc: Tensor, gate=None, ray_mask=None) -> None:
        """dL/d(origins, directions) of sampling level `lvl` from its encoded-feature gradient (on the current stream)."""
        lib, m = N.load(), self.n * self.counts[lvl]
        enc = net.mlp_base.encoding if hasattr(net.mlp_base, "encoding") else net.encoding
        N.check(lib.nsamd_hashgrid_encode_bwd_rays_gated(
            self._points(lvl), m, net._transform, net._box, N.ptr(enc.hash_table), enc.spec.native(), N.ptr(denc), 1, m,
            N.ptr(self.d_origins[lvl]), N.ptr(self.d_directions[lvl]), 0, gate, ray_mask, N.stream()),
            "hashgrid_encode_bwd_rays")

    @profiler.time_function
    def backward_cameras(self, updated: bool, force: bool = False) -> None:
        """Per-ray gradients of every level that received one -> `pose_adjustment.grad` (plus the L2 regulariser of
        camera_optimizers.py:179-185, whose value is kept in `camera_reg`). Call after the backward chains have joined."""
        if self.cam_opt is None or (self.cameras_outside and not force):
            return
        L = self.n_prop
        if self.cam_kernels:
            pose = self.cam_opt.pose_adjustment
            if self.grad_lookup is not None and id(pose) in self.grad_lookup:
                g = self.grad_lookup[id(pose)]
            else:
                if pose.grad is None:
                    pose.grad = torch.zeros_like(pose)
                g = pose.grad
            levels = (list(range(L)) if updated else []) + [L]  # the proposal networks saw the rays too (interlevel loss)
            d_os, d_ds = [self.d_origins[lvl] for lvl in levels], [self.d_directions[lvl] for lvl in levels]
            if self.normals is not None:  # the normals chain's share of the rays' gradient (normals_backward)
                d_os.append(self.normals["d_origins"])
                d_ds.append(self.normals["d_directions"])
            cfg = self.cam_opt.config
            reg = self.reg_in_backward  # (else the caller differentiates the regulariser itself — fused_step.FusedTrainStep)
            F.camera_backward_launch(pose, self.cam_mode, self.raw_directions, self.camera_indices, d_os, d_ds,
                                     float(cfg.trans_l2_penalty) if reg else 0.0, float(cfg.rot_l2_penalty) if reg else 0.0, g,
                                     self.camera_reg if reg else None)
            return
        d_o, d_d = self.d_origins[L], self.d_directions[L]
        if updated:  # the proposal networks saw the rays too (interlevel loss)
            d_o = d_o + sum(self.d_origins[:L])
            d_d = d_d + sum(self.d_directions[:L])
        if self.normals is not None:
            d_o, d_d = d_o + self.normals["d_origins"], d_d + self.normals["d_directions"]
        o, d = self._corrected
        outs, ups = [o, d], [d_o, d_d]
        if self.reg_in_backward:
            reg = {}
            self.cam_opt.get_loss_dict(reg)
            # a STATIC buffer: every captured schedule variant must leave the value where `loss_dict` reads it
            self.camera_reg.copy_(reg["camera_opt_regularizer"].detach())
            outs.append(reg["camera_opt_regularizer"])
            ups.append(torch.ones_like(self.camera_reg))
        # (else: the caller differentiates the regulariser itself — fused_step.FusedTrainStep)
        pose = [p for p in self.cam_opt.parameters() if p.requires_grad]
        if self.grad_lookup is not None and all(id(p) in self.grad_lookup for p in pose):
            for p, g in zip(pose, torch.autograd.grad(outs, pose, ups, allow_unused=True)):
                if g is not None:
                    self.grad_lookup[id(p)].add_(g)
        else:
            torch.autograd.backward(outs, ups)
        self._corrected = None

    @profiler.time_function
    def forward_proposals(self, draw_jitter: bool = True, need_enc: bool = True, after_bins=None,
                          stratified: bool = True) -> None:
        """NerfactoForward.forward_proposals for training: reads only the proposal networks' parameters, so with data parallelism
        it can run while the main-field gradients of the previous step are still being all-reduced (bench.py). need_enc: keep
        the levels' encoded features / selector / pre-activation for backward_proposals (False on the steps where the proposal
        networks get no gradient, ray_samplers.py:590). after_bins: called right behind the launch that writes the initial
        bins (and selects the batch), before the proposal levels."""
        self._proposals(draw_jitter, need_enc, after_bins, stratified)

    def _initial_bins(self, jit0: Optional[Tensor], per_edge: bool) -> None:
        sel, self.pending_select = self.pending_select, None
        if sel is None:
            return super()._initial_bins(jit0, per_edge)
        # the step's batch out of the caller's pool of batches AND the initial bins in one launch (trainer.HipTrainer hands
        # the selection over instead of launching it: the bins need nears / fars / the draw, not the rays)
        slot, slots, pool = sel
        N.check(N.load().nsamd_select_bins(
            slot, slots, self.n, N.ptr(pool["origins"]), N.ptr(pool["directions"]), N.ptr(pool["cameras"]),
            N.ptr(pool["target"]), N.ptr(self.origins), N.ptr(self.directions), N.ptr(self.camera_indices), N.ptr(self.target),
            N.ptr(self.nears), N.ptr(self.fars), N.ptr(self.edges), N.ptr(jit0), int(per_edge), self.counts[0], self.spacing,
            N.ptr(self.s_bins[0]), N.ptr(self.t_bins[0]), N.stream()), "select_bins")

    def forward_main_and_losses(self, updated: bool, terms_ready: bool = False) -> None:
        """Main field on the final samples, compositing, and the three losses with their gradients."""
        self.forward_main(terms_ready)
        self.losses(updated)

    @profiler.time_function
    def forward_main(self, terms_ready: bool = False, app_const: Optional[Tensor] = None) -> None:
        super().forward_main(terms_ready, app_const)
        self._saved_fresh, self._normals_fresh = app_const is None, False  # (an eval-mode forward stores no tile)

    @profiler.time_function
    def losses(self, updated: bool) -> None:
        """Weights, compositing (rgb / accumulation / depths: the model outputs) and the three losses with their gradients
        against `self.target`. Reads only what forward_main left behind, so it can be repeated with another target."""
        lib, st, n, cfg = N.load(), N.stream(), self.n, self.cfg
        ck = N.check
        L = self.n_prop
        S = self.counts[L]
        self._loss_vals_fresh = False
        # weights + compositing + MSE value/gradient in one launch (+ the global depth clip)
        ck(lib.nsamd_render_train(N.ptr(self.f_rgb), N.ptr(self.f_dens), N.ptr(self.t_bins[L]), n, S, self.bg_mode,
                                  self.bg_vals, N.ptr(self.target), 1.0 / (3 * n), N.ptr(self.weights[L]), N.ptr(self.rgb),
                                  N.ptr(self.acc), N.ptr(self.depth_exp),
                                  N.ptr(self.depth_med[L]) if self.compute_depths else None, N.ptr(self.minmax_ws),
                                  N.ptr(self.sq_err), N.ptr(self.d_rgb_out), N.ptr(self.bg_rays), st), "render_train")
        # ---- proposal losses: value + gradient, all levels in one launch (models/nerfacto.py:363-375) ----
        ck(lib.nsamd_proposal_losses(N.ptr(self.s_bins[L]), N.ptr(self.weights[L]), S, self.n_prop, self._pl_s_bins,
                                     self._pl_weights, self._pl_S, n, float(cfg.interlevel_loss_mult) / (n * S),
                                     float(cfg.distortion_loss_mult) / n, self._pl_per_ray,
                                     self._pl_dw if updated else None, N.ptr(self.dist_per_ray), N.ptr(self.dw_dist), st),
           "proposal_losses")
        d = self.depth
        if d is not None:
            # ---- depth supervision: one more launch that adds its gradients to the ones just written ----
            if torch.cuda.is_current_stream_capturing():
                raise NotImplementedError("explicit schedule: a depth target inside a captured graph; depth supervision in "
                                          "captured iterations is only on the module path")
            scale = d["mult"] / (n * len(self.counts))
            # the final level always; the proposal levels on update steps only
            dws = (self.dw_prop if updated else [None] * self.n_prop) + [self.dw_dist]
            F.depth_loss_launch(self.weights, self.t_bins, d["target"], None if d["euclidean"] else d["norm"], None, d["sigma"],
                                F.DEPTH_DS_NERF, scale, d["per_ray"], dws, None, accumulate=True)
            torch.sum(d["per_ray"], dim=(0, 1), out=d["value"])
            d["value"].mul_(scale)
        if self.normals is not None:
            self.normals_forward()
        if self.want_loss_vals:
            # a caller that reads the loss dictionary every iteration (pipeline.TrainEngine): the values and the training metrics
            # as five floats from one small launch instead of a dozen reductions issued by the host
            ck(lib.nsamd_train_loss_values(N.ptr(self.sq_err), N.ptr(self.dist_per_ray), self.n_prop, self._pl_per_ray, n, S,
                                           float(cfg.interlevel_loss_mult), float(cfg.distortion_loss_mult),
                                           N.ptr(self.loss_vals), st), "train_loss_values")
            self._loss_vals_fresh = True

    @profiler.time_function
    def backward_main(self, field: bool = True) -> None:
        """composite -> weights -> field MLPs -> main hash table (MSE + distortion gradients). `field=False`: stop before
        the field's MLPs (the caller runs `backward_field_and_table`)."""
        lib, st, n = N.load(), N.stream(), self.n
        ck = N.check
        L = self.n_prop
        S = self.counts[L]
        ck(lib.nsamd_render_train_bwd(N.ptr(self.f_rgb), N.ptr(self.weights[L]), N.ptr(self.f_dens), N.ptr(self.t_bins[L]),
                                      n, S, self.bg_mode, self.bg_vals, N.ptr(self.d_rgb_out), N.ptr(self.dw_dist),
                                      N.ptr(self.d_rgb_s), N.ptr(self.d_dens_main), N.ptr(self.bg_rays), st),
           "render_train_bwd")
        if self.gradient_scaling:  # scale_gradients_by_distance_squared on the field's outputs (models/nerfacto.py:321-322)
            F.distance_gradient_scale_launch(self.t_bins[L], self.d_dens_main, self.d_rgb_s)
        if field:
            self.backward_field_and_table()

    def backward_field_and_table(self) -> None:
        """Second half of backward_main: the main field's MLPs (from `d_dens_main`, `d_rgb_s`) and the table scatter. Separate
        so that tests can drive the field backward with upstream gradients of their own. The table's gradient is written, or
        accumulated into an existing one (prepare_grads)."""
        fld = self.model.field
        L = self.n_prop
        params, emb = F.field_params(fld)
        # (the ray terms are what forward_main computed for this batch and these parameters)
        fm = F.field_mlp(params, emb, fld.average_init_density, self.ray_terms, self.ray_inputs)
        if self._saved_fresh:  # (and head layer 1's output, with the rgb it wrote)
            fm.saved_hb, fm.saved_rgb = N.ptr(self.saved_hb), N.ptr(self.f_rgb)
        cam = self.cam_opt is not None  # the camera optimiser's share needs the encoded-feature gradient as well
        tbl = fld.mlp_base.encoding
        F.field_backward(tbl.hash_table, tbl.spec, fld._transform, fld._box, self._points(L), self.m_main, self.f_enc, self.f_sel,
                         self.directions, self._cams(None), None, self.counts[L], fm, self.d_dens_main, self.d_rgb_s, self.f_denc,
                         F.field_mlp_grads(params, emb, self._grad), self.field_ws, self._grad(tbl.hash_table),
                         self.main_table_write_only, fuse=self.fuse_route, keep_denc=cam or self.keep_denc,
                         on_denc=(lambda: self._rays_backward(L, fld, self.f_denc)) if cam else None,
                         fused_launch=self._field_bwd_phases if (cam or N.PROFILE is not None) else None)

    def _field_bwd_phases(self, args) -> None:
        """The fused main-field backward (nsamd_field_mlp_bwd_scatter) as separate phases: under N.PROFILE one launch group at
        a time (the per-kernel table, utils/roofline.py; same bits), else for the camera optimiser's share."""
        lib, st = N.load(), N.stream()
        L, fld = self.n_prop, self.model.field

        def launch(phase: int) -> None:
            N.check(lib.nsamd_field_mlp_bwd_scatter_phase(*args, phase, st), "field_mlp_bwd_scatter_phase")

        if N.PROFILE is not None:
            for phase in (1, 2, 4):
                launch(phase)
            if self.cam_opt is not None:
                self._rays_backward(L, fld, self.f_denc)
            return
        # camera optimiser: the rays' gradient through the main grid (a gather pass over the table, 96 us) needs the
        # encoded-feature gradient the kernel has just written and nothing of the table scatter's apply pass (LDS
        # atomics, latency-bound): beside it on the second stream instead of behind it
        launch(1)
        main = N.current_stream()
        self._red_fork.record(main)
        self.reduce_stream.wait_event(self._red_fork)
        with N.on_stream(self.reduce_stream):
            self._rays_backward(L, fld, self.f_denc)
            self._red_join.record(self.reduce_stream)
        launch(6)  # (the reduce rides the apply pass)
        main.wait_event(self._red_join)

    @profiler.time_function
    def backward_proposals(self, levels=None) -> None:
        """Backward of the proposal networks (interlevel loss only; main-level weights are detached, losses.py:119-120).
        Needs the dw_prop written by losses(updated=True). `levels`: subset of proposal levels (their
        chains share nothing, so they may run on different streams)."""
        lib, st, n = N.load(), N.stream(), self.n
        ck = N.check
        lvls = list(range(self.n_prop) if levels is None else levels)
        if (self.merge_prop_levels and len(lvls) >= 2 and self.gate_proposals and self.cam_opt is None
                and N.PROFILE is None):
            # every stage of the levels' chains as ONE launch across the levels (nsamd_proposal_levels_bwd; same bits)
            arr = self._proposal_level_structs(lvls)
            if arr is not None:
                ck(lib.nsamd_proposal_levels_bwd(arr, len(lvls), int(self.gates_precleared), st), "proposal_levels_bwd")
                return
        for lvl in lvls:
            net = self.props[lvl]
            S, m = self.counts[lvl], n * self.counts[lvl]
            W0, b0, W1, b1 = net.mlp_base[1].param_tensors()
            dm = F.density_mlp(W0, b0, W1, b1, net.average_init_density)
            gate = self._gate(lvl)
            dws = self.density_ws[lvl]
            spec = net.encoding.spec
            ws, ws_n = F._scatter_workspace(spec, self.f_enc.device, m)
            grads = [self._grad(p) for p in (W0, b0, W1, b1)]
            if gate is None or ws is None:  # ungated chain (`gate_proposals` off, or no binned-scatter workspace for this shape)
                F.weights_backward_launch(self.t_bins[lvl], self.p_dens[lvl], self.dw_prop[lvl], self.p_ddens[lvl])
                F.density_backward(self.p_enc[lvl], self.p_sel[lvl], self.p_pre[lvl], self.p_ddens[lvl], m, dm, self.p_denc[lvl],
                                   grads, dws)
                if self.cam_opt is not None:
                    self._rays_backward(lvl, net, self.p_denc[lvl])
                F.table_scatter(self._points(lvl), m, net._transform, net._box, net.encoding.hash_table, spec, self.p_denc[lvl],
                                1, m, self._grad(net.encoding.hash_table))
                continue
            # the weights backward raises the level's flag when any ray carries interlevel gradient; the rest of the
            # chain returns at once while it is clear (the zero-filled gradients are then already the result)
            mask = N.ptr(self.prop_ray_masks[lvl])
            ck(lib.nsamd_weights_bwd_gate(N.ptr(self.t_bins[lvl]), N.ptr(self.p_dens[lvl]), N.ptr(self.dw_prop[lvl]),
                                          n, S, N.ptr(self.p_ddens[lvl]), gate, mask, int(self.gates_precleared), st),
               "weights_bwd_gate")
            ck(lib.nsamd_density_mlp_bwd_gated(N.ptr(self.p_enc[lvl]), N.ptr(self.p_sel[lvl]), N.ptr(self.p_pre[lvl]),
                                               N.ptr(self.p_ddens[lvl]), m, dm, N.ptr(self.p_denc[lvl]), *map(N.ptr, grads),
                                               N.ptr(dws), dws.numel(), gate, mask, S, st), "density_mlp_bwd_gated")
            if self.cam_opt is not None:
                self._rays_backward(lvl, net, self.p_denc[lvl], gate, mask)
            ck(lib.nsamd_hashgrid_encode_bwd_gated(self._points(lvl), m, net._transform, net._box,
                                                   N.ptr(net.encoding.hash_table), spec.native(),
                                                   N.ptr(self.p_denc[lvl]), 1, m,
                                                   N.ptr(self._grad(net.encoding.hash_table)), N.ptr(ws), ws_n, gate,
                                                   mask, st), "hashgrid_encode_bwd_gated")

    def _proposal_level_structs(self, lvls):
        """ctypes array of nsamd_proposal_level_bwd for `lvls` (None: a level without a binned-scatter workspace). The structs
        hold raw addresses of this runner's static buffers and of the parameters / gradients, which do not move."""
        arr = (N.ProposalLevelBwd * len(lvls))()
        n = self.n
        for i, lvl in enumerate(lvls):
            net = self.props[lvl]
            S, m = self.counts[lvl], n * self.counts[lvl]
            W0, b0, W1, b1 = net.mlp_base[1].param_tensors()
            spec = net.encoding.spec
            ws, ws_n = F._scatter_workspace(spec, self.f_enc.device, m)
            if ws is None:
                return None
            dws = self.density_ws[lvl]
            e = arr[i]
            e.num_rays, e.samples_per_ray = n, S
            e.t_bins, e.density, e.dweights = N.ptr(self.t_bins[lvl]), N.ptr(self.p_dens[lvl]), N.ptr(self.dw_prop[lvl])
            e.ddensity, e.gate, e.ray_mask = N.ptr(self.p_ddens[lvl]), self._gate(lvl), N.ptr(self.prop_ray_masks[lvl])
            e.enc, e.selector, e.pre = N.ptr(self.p_enc[lvl]), N.ptr(self.p_sel[lvl]), N.ptr(self.p_pre[lvl])
            e.mlp = F.density_mlp(W0, b0, W1, b1, net.average_init_density)
            e.denc = N.ptr(self.p_denc[lvl])
            e.dW0, e.db0, e.dW1, e.db1 = (N.ptr(self._grad(t)) for t in (W0, b0, W1, b1))
            e.mlp_workspace, e.mlp_workspace_floats = N.ptr(dws), dws.numel()
            e.origins, e.directions = N.ptr(self.origins), N.ptr(self.directions)
            e.transform, e.aabb = net._transform, net._box
            e.table, e.grid = N.ptr(net.encoding.hash_table), spec.native()
            e.dtable = N.ptr(self._grad(net.encoding.hash_table))
            e.scatter_workspace, e.scatter_workspace_floats = N.ptr(ws), ws_n
        return arr

    # -------------------------------------------------------------------------------------------------------------
    def loss_dict(self) -> Dict[str, Tensor]:
        """Loss values of the last iteration (models/nerfacto.py:363-375); a few tiny torch reductions, call on demand."""
        n, S = self.n, self.counts[-1]
        if self._loss_vals_fresh:  # what the losses launch left behind: no reduction launches
            # ONE clone: the buffer is overwritten by every iteration, and a caller that keeps the dictionaries of several
            # iterations (a trainer's logging history) must not see them all change to the latest values
            v = self.loss_vals[:3].clone()
            out = {"rgb_loss": v[0], "distortion_loss": v[2], "interlevel_loss": v[1]}
        else:
            out = {"rgb_loss": self.sq_err.sum() / (3 * n),
                   "distortion_loss": self.cfg.distortion_loss_mult * self.dist_per_ray.sum() / n}
            inter = sum(p.sum() for p in self.inter_per_ray) / (n * S)
            out["interlevel_loss"] = self.cfg.interlevel_loss_mult * inter
        if self.cam_opt is not None:
            out["camera_opt_regularizer"] = self.camera_reg
        if self.depth is not None:
            out["depth_loss"] = self.depth["value"].clone()
        if self.normals is not None:  # models/nerfacto.py:379-388: mult * mean of the rendered per-ray terms
            out["orientation_loss"] = self.cfg.orientation_loss_mult * self.normals["orientation"].sum() / n
            out["pred_normal_loss"] = self.cfg.pred_normal_loss_mult * self.normals["pred"].sum() / n
        return out

    def outputs(self) -> Dict[str, Tensor]:
        """The tensors NerfactoModel.get_outputs returns, as views of the static buffers (built once: the buffers never move, and a
        trainer asks for them every iteration — a dozen view constructions were a measurable share of the host's work per step)."""
        if self._outputs is None:
            out = {"rgb": self.rgb, "accumulation": self.acc[:, None], "expected_depth": self.depth_exp[:, None],
                   "weights_list": [w[..., None] for w in self.weights]}
            if self.compute_depths:
                out["depth"] = self.depth_med[-1][:, None]
                for i in range(self.n_prop):
                    out[f"prop_depth_{i}"] = self.depth_med[i][:, None]
            if self.normals is not None:
                nb = self.normals
                out.update(normals=nb["normals_img"], pred_normals=nb["pred_img"], rendered_orientation_loss=nb["orientation"],
                           rendered_pred_normal_loss=nb["pred"])
            self._outputs = out
        return dict(self._outputs)
