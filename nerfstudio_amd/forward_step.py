"""The nerfacto forward as an explicit kernel schedule over static buffers, allocated once, capturable in a hipGraph:

  piecewise_bins -> [density_field_fwd -> proposal_resample] x proposal levels -> (ray terms) -> hash_fwd(main) + field_mlp_fwd

`NerfactoForward` is all eval_render.EvalRenderer builds — rays in, per-sample density and rgb out; the renderer issues weights
and compositing itself — and the base of train_step.NerfactoTrainStep, which adds the target, the kept activations, every
gradient and loss buffer, the streams and the backward. A buffer only the training schedule has is None here, never a
placeholder: nothing on this class hands a kernel an address it has no memory behind. Constructing one needs neither a GPU nor
the native library (tests/test_forward_step_cpu.py walks its buffers on the CPU).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _native as N
from . import functional as F
from .nerfacto import NerfactoModel
from .utils import profiler


class NerfactoForward:
    # train_step.NerfactoTrainStep alone allocates: the random background's colours, the ray terms' inputs, the backward's tile
    bg_rays = ray_inputs = saved_hb = None

    def __init__(self, model: NerfactoModel, num_rays: int, device, compute_depths: bool = True) -> None:
        self.model = model
        cfg = self.cfg = model.config
        self.n = n = int(num_rays)
        self.counts = (*cfg.num_proposal_samples_per_ray, cfg.num_nerf_samples_per_ray)
        self.n_prop = len(cfg.num_proposal_samples_per_ray)
        self.compute_depths = compute_depths
        if cfg.background_color not in ("last_sample", "black", "white", "random"):
            raise ValueError(cfg.background_color)
        # use_single_jitter=False (ray_samplers.py:104-107, 318-322): one draw per bin EDGE instead of one per ray — the
        # per-level jitter buffers become [n, S+1] and the resampling goes through the unfused kernels
        self.single_jitter = bool(getattr(cfg, "use_single_jitter", True))
        f32 = dict(device=device, dtype=torch.float32)
        e = lambda *shape: torch.empty(shape, **f32)  # noqa: E731
        # "random": the rendered colour carries no background (mode 3: the training losses blend a per-ray colour, `bg_rays`)
        self.bg_mode, self.bg_vals = (3, None) if cfg.background_color == "random" else F._bg_args(cfg.background_color, device)
        # ---- per-step inputs (static addresses; the caller fills them) ----
        self.origins, self.directions = e(n, 3), e(n, 3)
        self.camera_indices = torch.zeros((n,), device=device, dtype=torch.int64)
        self.nears = torch.full((n,), float(cfg.near_plane), **f32)  # NearFarCollider, training mode
        self.fars = torch.full((n,), float(cfg.far_plane), **f32)
        self.jitter = e(self.n_prop + 1, n)  # single jitter: one draw per level and ray
        self.jitter_edges = None if self.single_jitter else [e(n, s + 1) for s in self.counts]  # per edge: [n, S+1] per level
        self.anneal_dev = torch.ones((1,), **f32)
        # ---- sampler state ----
        self.s_bins = [e(n, s + 1) for s in self.counts]
        self.t_bins = [e(n, s + 1) for s in self.counts]
        self.weights = [e(n, s) for s in self.counts]
        # ---- fields ----
        self.props = list(model.proposal_networks) if not cfg.use_same_proposal_network else \
            [model.proposal_networks[0]] * self.n_prop
        # the levels' encoded features / selector / pre-activation: kept for a backward only (see `ensure_proposal_features`)
        self.p_enc, self.p_sel, self.p_pre = ([None] * self.n_prop for _ in range(3))
        self.p_dens = [e(n * s) for s in self.counts[:-1]]
        self.m_main = mm = n * self.counts[-1]
        fld = model.field
        self.f_enc, self.f_sel, self.f_dens, self.f_rgb = e(fld.mlp_base.encoding.get_out_dim(), mm), e(mm), e(mm), e(mm, 3)
        # ---- outputs ----
        self.rgb, self.acc, self.depth_exp = e(n, 3), e(n), e(n)
        self.minmax_ws = e(2 + 2 * ((n + 3) // 4))
        self.depth_med = [e(n) for _ in self.counts]
        # Ray terms (include/nsamd.h, nsamd_field_mlp.ray_terms): head layer 0's share of the 48 per-ray inputs (SH of the view
        # direction, appearance row) once per ray instead of once per sample (a 16-point tile must lie inside one ray).
        self.ray_terms_on = F.ray_terms_apply(self.counts[-1], mm)
        self.ray_terms = e(n, 64) if self.ray_terms_on else None
        self.spacing = int(getattr(model.proposal_sampler.initial_sampler, "spacing", 0))
        # host-evaluated tables (bit-identical to the reference's CPU linspace)
        self.edges = F._linspace("edges", self.counts[0], device)
        self.u_base = [None] + [F._linspace("u", s, device) for s in self.counts[1:]]

    def ensure_proposal_features(self, lvl: int) -> None:
        """A proposal network the fused density kernel does not take (the two-kernel pair needs the level's encoded features and
        selector): allocate them on first use, where the schedule has not (eval_render.EvalRenderer: in its warm-up launch)."""
        if self.p_sel[lvl] is None:
            m, dev = self.n * self.counts[lvl], self.p_dens[lvl].device
            self.p_enc[lvl] = torch.empty((self.props[lvl].encoding.get_out_dim(), m), device=dev)
            self.p_sel[lvl] = torch.empty((m,), device=dev)

    def _points(self, lvl: int) -> N.Points:
        return N.make_points(None, self.origins, self.directions, self.t_bins[lvl], self.counts[lvl])

    @profiler.time_function
    def forward_proposals(self, draw_jitter: bool = True, stratified: bool = True) -> None:
        """Initial bins and the proposal levels (density fields + resampling); the fused forward writes nothing but the
        densities. stratified=False: eval sampling (ray_samplers.py:104-111, 323-327) — bin centres in the initial sampler, the
        fixed offset in the PDF resampling, nothing drawn."""
        self._proposals(draw_jitter, False, None, stratified)

    def _initial_bins(self, jit0: Optional[Tensor], per_edge: bool) -> None:
        F.piecewise_bins_launch(self.nears, self.fars, self.edges, jit0, int(per_edge), self.spacing, self.s_bins[0],
                                self.t_bins[0])

    def _proposals(self, draw_jitter: bool, keep: bool, after_bins, stratified: bool) -> None:
        """The body of `forward_proposals`. keep: the levels' encoded features / selector / pre-activation stay in `p_enc` /
        `p_sel` / `p_pre` for a backward — a schedule without those buffers refuses before it launches anything."""
        if keep and any(x is None for x in (*self.p_enc, *self.p_sel, *self.p_pre)):
            raise RuntimeError(f"{type(self).__name__} has no buffers to keep the proposal levels' features in")
        lib, st, n = N.load(), N.stream(), self.n
        ck = N.check
        per_edge = stratified and not self.single_jitter
        if draw_jitter and stratified:
            if per_edge:
                for j in self.jitter_edges:
                    j.uniform_()
            else:
                self.jitter.uniform_()  # torch.rand per level and ray (ray_samplers.py:105, :322), drawn on the device
            if self.bg_rays is not None:
                self.bg_rays.uniform_()  # rand_like(pred) of the loss blend (renderers.py:195)
        self._initial_bins((self.jitter_edges[0] if per_edge else self.jitter[0]) if stratified else None, per_edge)
        if after_bins is not None:  # (trainer.HipTrainer: the ray terms, behind the batch selection)
            after_bins()
        # ---- proposal levels ----
        for lvl in range(self.n_prop):
            net = self.props[lvl]
            S, m = self.counts[lvl], n * self.counts[lvl]
            dm = F.density_mlp(*net.mlp_base[1].param_tensors(), net.average_init_density)
            # hash grid + MLP + trunc_exp in one launch, features in registers (nsamd_density_field_fwd); networks the
            # fused kernel is not built for go through the two-kernel pair
            fused = lib.nsamd_density_field_fwd(
                self._points(lvl), m, net._transform, net._box, N.ptr(net.encoding.hash_table), net.encoding.spec.native(), dm,
                N.ptr(self.p_enc[lvl]) if keep else None, N.ptr(self.p_sel[lvl]) if keep else None,
                N.ptr(self.p_dens[lvl]), N.ptr(self.p_pre[lvl]) if keep else None, st)
            if fused == N.ERR_UNSUPPORTED:
                self.ensure_proposal_features(lvl)
                F.hash_forward(self._points(lvl), m, net._transform, net._box, net.encoding.hash_table, net.encoding.spec,
                               self.p_enc[lvl], 1, m, self.p_sel[lvl])
                F.density_forward(self.p_enc[lvl], self.p_sel[lvl], m, dm, self.p_dens[lvl], self.p_pre[lvl])
            else:
                ck(fused, "density_field_fwd")
            S2 = self.counts[lvl + 1]
            if per_edge:
                # one draw per new bin edge: the fused launch below draws per ray, so this (non-default) configuration takes
                # its three constituents — same numbers (nsamd.h)
                F.weights_launch(self.t_bins[lvl], self.p_dens[lvl], self.weights[lvl])
                if self.compute_depths:
                    F.composite_launch(None, self.weights[lvl], self.t_bins[lvl], N.BG_NONE, None, False, None, None, None,
                                       self.depth_med[lvl], None, None)
                F.pdf_resample_launch(self.s_bins[lvl], self.weights[lvl], self.u_base[lvl + 1], self.jitter_edges[lvl + 1],
                                      self.nears, self.fars, 1.0, self.anneal_dev, 0.01, 1e-5, self.spacing, 1, False, S2,
                                      self.s_bins[lvl + 1], self.t_bins[lvl + 1], None)
                continue
            # weights of this level, its median depth (prop_depth_i, models/nerfacto.py:346-347) and the PDF resampling
            ck(lib.nsamd_proposal_resample(N.ptr(self.t_bins[lvl]), N.ptr(self.s_bins[lvl]), N.ptr(self.p_dens[lvl]), S,
                                           N.ptr(self.u_base[lvl + 1]), N.ptr(self.jitter[lvl + 1]) if stratified else None,
                                           N.ptr(self.nears), N.ptr(self.fars), 1.0, N.ptr(self.anneal_dev), 0.01, 1e-5,
                                           1.0 / (2 * (S2 + 1)), self.spacing, n, S2, N.ptr(self.weights[lvl]),
                                           N.ptr(self.depth_med[lvl]) if self.compute_depths else None,
                                           N.ptr(self.s_bins[lvl + 1]), N.ptr(self.t_bins[lvl + 1]), st),
               "proposal_resample")

    def _field_mlp(self) -> N.FieldMlp:
        fld = self.model.field
        return F.field_mlp(*F.field_params(fld), fld.average_init_density)

    def _cams(self, app_const: Optional[Tensor]) -> Optional[Tensor]:
        """The camera indices the main field reads its appearance rows by (None: no appearance table, or `app_const`)."""
        return self.camera_indices if (self.model.field.embedding_appearance is not None and app_const is None) else None

    def ray_terms_launch(self, fm: Optional[N.FieldMlp] = None, app_const: Optional[Tensor] = None, select=None) -> None:
        """nsamd_field_ray_terms for the batch in the static buffers: head layer 0's share of the 48 per-ray inputs. Needs the
        batch's (pose-corrected) directions and camera indices and the CURRENT head_W0 / head_b0 / appearance table — i.e. it
        runs after batch selection and after the main-field Adam of the previous iteration. On torch's current stream.
        app_const: see forward_main (the per-ray inputs are then not kept: no backward reads them). select: the `pending_select`
        (slot pointer, slots, pool) the same iteration's `forward_proposals` fills the static buffers from — the terms are then
        read out of the pool itself (the same rows, the same bits) and need not wait for that launch; only without a camera
        optimiser, whose corrected directions exist nowhere but in the static buffers (trainer.HipTrainer._pool_select)."""
        fm = fm if fm is not None else self._field_mlp()
        inputs = self.ray_inputs if app_const is None else None
        if select is not None:
            slot, slots, pool = select
            F.ray_terms_launch(pool["directions"], None if self._cams(app_const) is None else pool["cameras"], app_const, self.n,
                               fm, self.ray_terms, inputs, slot=slot, slots=slots)
            return
        F.ray_terms_launch(self.directions, self._cams(app_const), app_const, self.n, fm, self.ray_terms, inputs)

    @profiler.time_function
    def forward_main(self, terms_ready: bool = False, app_const: Optional[Tensor] = None) -> None:
        """Hash grid + MLPs of the main field on the final samples -> per-sample density and rgb. terms_ready: the caller has
        launched `ray_terms_launch` for this batch and these parameters itself (trainer.HipTrainer: off the critical path).
        app_const: one appearance row for every sample instead of the rays' cameras' (eval mode, eval_render.EvalRenderer)."""
        L = self.n_prop
        fm = self._field_mlp()
        if self.ray_terms_on:
            if not terms_ready:
                self.ray_terms_launch(fm, app_const)
            fm.ray_terms = N.ptr(self.ray_terms)
            fm.ray_inputs = N.ptr(self.ray_inputs if app_const is None else None)
        # (an eval-mode forward has no backward: no tile is stored, and that of an earlier forward no longer matches f_rgb)
        if self.saved_hb is not None and app_const is None:
            fm.saved_hb = N.ptr(self.saved_hb)
        fld = self.model.field
        tbl = fld.mlp_base.encoding
        F.field_forward(tbl.hash_table, tbl.spec, fld._transform, fld._box, self._points(L), self.m_main, self.f_enc, self.f_sel,
                        self.directions, self._cams(app_const), app_const, self.counts[L], fm, self.f_dens, self.f_rgb)
