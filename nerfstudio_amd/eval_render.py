"""Full-image eval render of the nerfacto path as a device-side chunk loop.

Reference: `Model.get_outputs_for_camera_ray_bundle` (models/base_model.py:178-205) slices the camera's ray bundle into
chunks of `eval_num_rays_per_chunk` rays in Python, runs `forward` on each — ~60 module calls and as many tensor
allocations per chunk — and `torch.cat`s every output. Here one chunk is ONE explicit kernel schedule over static buffers
(forward_step.NerfactoForward, the base of the training runner, in eval mode), captured once per chunk size in a hipGraph; a frame is

    for each chunk:  copy the chunk's rays into the static input buffers -> replay -> copy the outputs into their
                     rows of the preallocated image buffers

i.e. no per-chunk Python graph of modules, no allocation, no `torch.cat`. Eval semantics as the reference's
(models/nerfacto.py:298-348 with `self.training == False`): near plane reset to 0 (scene_colliders.py:186-191), no jitter —
bin centres in the initial sampler, the fixed 1/(2 nb) offset in the PDF resampling (ray_samplers.py:104-111, 323-327) —,
the mean (or zero) appearance embedding for every sample (fields/nerfacto_field.py:253-261), nan_to_num on the samples and
a clamp of the composited colour (renderers.py:225-231), expected depth clipped to the CHUNK's min / max sample midpoint
(the reference clips per forward call, i.e. per chunk, renderers.py:380-383). A last, shorter chunk is padded with copies
of its last ray (which leaves that min / max untouched) and only its valid rows are copied out.
Same kernels, same order as the module path, launched through the same helpers (functional.weights_launch, composite_launch,
field_normals_launch, nerf_encode_launch, linear_launch, normals_composite_launch): the outputs are equal bit for bit
(tests/test_gpu_kernels.py).
A bundle that carries its own nears AND fars keeps them, as the collider leaves such a bundle alone (scene_colliders.py:40-44),
and `render_texels` generates the texel rays of a textured mesh export — bounds included — inside the loop
(tests/test_gpu_texture.py); either way the schedule's bounds are back at 0 / far_plane when the call returns.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from . import _native as N
from . import eval_frame
from . import functional as F
from .eval_frame import in_loop_camera_args, lens_camera_args, pinhole_camera_args  # noqa: F401  (imported from here too)
from .utils import profiler


_PN_BLOCK = 1 << 18  # samples per pass of the predicted-normals MLP (its two [block, 64] activation buffers: 64 MiB each)


def pred_normals_layers(fld):
    """The dense layers of a NerfactoField's predicted-normals branch (nerfacto_field.py:181-191) as (W, b, activation) in order:
    the MLP's three layers (ReLU, ReLU, none) and the 64 -> 3 head without its activation — 27 -> 64 -> 64 -> 64 -> 3. The one
    list both the eval form below and the training stage (train_step.NerfactoTrainStep) launch."""
    W0, b0, W1, b1, W2, b2 = fld.mlp_pred_normals.param_tensors()
    head = fld.field_head_pred_normals.net
    return ((W0, b0, 1), (W1, b1, 1), (W2, b2, 0), (head.weight, head.bias, 0))


def pred_normals_mlp_launch(fld, pts: N.Points, M: int, freqs: Tensor, pn_enc: Tensor, pn_in: Tensor, pn_a: Tensor, pn_b: Tensor,
                            pn_pre: Tensor) -> None:
    """The predicted-normals branch of a NerfactoField in eval (nerfacto_field.py:287-295) on M points whose geometry features
    already sit in columns 12..26 of `pn_in` [M, 27], over caller-owned buffers on the current stream: nsamd_nerf_encode of the
    raw positions (`pn_enc` [M, 12], copied into columns 0..11), then the MLP's three layers (ReLU, ReLU, none) and the 64 -> 3
    head with no activation — nsamd_normals_composite applies tanh and the normalisation — into `pn_pre` [M, 3], in blocks of
    the rows `pn_a` / `pn_b` [block, 64] hold."""
    F.nerf_encode_launch(pts, M, freqs, False, pn_enc)
    pn_in[:, :12].copy_(pn_enc)  # (the encoder writes dense 12-wide rows)
    layers = pred_normals_layers(fld)
    block = pn_a.shape[0]
    for a in range(0, M, block):
        k = min(a + block, M) - a
        rows = (pn_in[a:a + k], pn_a, pn_b, pn_a, pn_pre[a:a + k])  # each layer's input and, one further, its output
        for i, (W, b, act) in enumerate(layers):
            F.linear_launch(rows[i], W, b, k, act, rows[i + 1])


class EvalRenderer:
    def __init__(self, model, chunk: Optional[int] = None, use_graph: bool = True, normals: bool = False) -> None:
        """normals: also render `normals` and `pred_normals` (a `predict_normals` model; `supported(model, normals=True)`): three
        more stages behind the chunk's weights — see `_launch_normals`."""
        from .forward_step import NerfactoForward

        self.model = model
        self.normals = bool(normals)
        if self.normals and supported(model, normals=True) is not None:
            raise ValueError(f"EvalRenderer(normals=True): {supported(model, normals=True)}")
        self.chunk = int(chunk or model.config.eval_num_rays_per_chunk)
        dev = next(model.parameters()).device
        N.require_cuda(next(model.parameters()))
        self.step = NerfactoForward(model, self.chunk, dev, compute_depths=True)
        self.step.nears.zero_()  # NearFarCollider at inference (reset_near_plane)
        fld = model.field
        emb = fld.embedding_appearance.embedding.weight if fld.embedding_appearance is not None else None
        self.app_const = torch.zeros(emb.shape[1], device=dev) if emb is not None else None
        self.use_graph = use_graph
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._captured_addresses = ()
        if self.step.bg_mode == 3:  # "random": eval composites without a background (renderers.py:112-115 adds none)
            self.bg_mode, self.bg_vals = N.BG_NONE, None
        else:
            self.bg_mode, self.bg_vals = self.step.bg_mode, self.step.bg_vals
        if self.normals:
            # static buffers of the normals stages, allocated once: per-sample analytic normals, the predicted-normals MLP's
            # 27-wide input rows (12 encoded columns | 15 geometry features), its head's pre-activation, two ping-pong activation
            # blocks, and the chunk's two rendered channels
            e = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
            mm = self.step.m_main
            pe = model.field.position_encoding
            self.pn_freqs = (2 ** torch.linspace(pe.min_freq, pe.max_freq, pe.num_frequencies)).to(dev)
            self.n_smp, self.pn_enc, self.pn_in, self.pn_pre = e(mm, 3), e(mm, 12), e(mm, 27), e(mm, 3)
            blk = min(mm, _PN_BLOCK)
            self.pn_a, self.pn_b = e(blk, 64), e(blk, 64)
            self.normals_img, self.pred_normals_img = e(self.chunk, 3), e(self.chunk, 3)

    # ---- one chunk ------------------------------------------------------------------------------------------------------
    def _refresh_constants(self) -> None:
        """Per-frame values that live in device memory (so that a captured graph sees the current ones): the anneal exponent
        and the appearance row of eval mode."""
        m, s = self.model, self.step
        s.anneal_dev.fill_(float(m.proposal_sampler._anneal))
        eval_frame.eval_appearance_row(m.field, self.app_const)

    def _launch_chunk(self) -> None:
        """The kernel schedule of one chunk (all arguments are static buffers: capturable): the forward schedule in
        eval mode, then weights + compositing with the clamp."""
        s = self.step
        s.forward_proposals(stratified=False)
        s.forward_main(app_const=self.app_const)
        L = s.n_prop
        F.weights_launch(s.t_bins[L], s.f_dens, s.weights[L])
        F.composite_launch(s.f_rgb, s.weights[L], s.t_bins[L], self.bg_mode, self.bg_vals, True, s.rgb, s.acc, s.depth_exp,
                           s.depth_med[L], None, s.minmax_ws)
        if self.normals:
            self._launch_normals()

    def _launch_normals(self) -> None:
        """The normals stages of one chunk, behind forward_main (which left the hash features in `f_enc`) and the weights:
        1. nsamd_field_normals: per-sample analytic normals + the geometry features into columns 12..26 of `pn_in`;
        2. the predicted-normals MLP as the module path runs it (nerfacto_field.py:287-295): nsamd_nerf_encode of the raw
           positions into columns 0..11, three nsamd_linear_fwd layers (ReLU, ReLU, none) and the 64 -> 3 head, block by block
           over the two ping-pong buffers;
        3. nsamd_normals_composite: head activation, both weighted sums, renormalisation and shading per ray."""
        s, fld = self.step, self.model.field
        L = s.n_prop
        M, pts = s.m_main, s._points(L)
        enc = fld.mlp_base.encoding
        F.field_normals_launch(pts, M, fld._transform, fld._box, enc.hash_table, enc.spec, s.f_enc,
                               fld.mlp_base.mlp.param_tensors(), self.n_smp, None, self.pn_in, 27, 12)
        pred_normals_mlp_launch(fld, pts, M, self.pn_freqs, self.pn_enc, self.pn_in, self.pn_a, self.pn_b, self.pn_pre)
        F.normals_composite_launch(s.weights[L], self.n_smp, self.pn_pre, self.normals_img, self.pred_normals_img)

    def _addresses(self):
        """Everything the captured launches read through raw pointers that this object does not own: the model's parameters
        and buffers (a ParamArena built later re-homes them, `.to()` moves them, an embedding may be swapped)."""
        m = self.model
        return tuple(t.data_ptr() for t in list(m.parameters()) + list(m.buffers()))

    def _run_chunk(self) -> None:
        if not self.use_graph:
            self._launch_chunk()
            return
        if self.graph is not None and self._addresses() != self._captured_addresses:
            self.graph = None  # the graph holds stale pointers: capture again
        if self.graph is None:
            # the warm-up launch below may allocate (a proposal network the fused density kernel does not take): outside the capture
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # lazy kernel attributes / first-use work outside the capture
                self._launch_chunk()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch_chunk()
            self.graph = g
            self._captured_addresses = self._addresses()
        self.graph.replay()

    # ---- a frame ----------------------------------------------------------------------------------------------------------
    def _render_rays(self, total: int, dev, load_chunk) -> Dict[str, Tensor]:
        """The frame's chunk loop over `total` rays: `load_chunk(a, k)` puts rays a .. a + k - 1 into the schedule's input
        buffers, the chunk runs, and its k valid rows are copied into the preallocated `[total, C]` outputs."""
        s, n = self.step, self.chunk
        one, three = (1, None), (3, None)  # (channels, the default dtype)
        out = eval_frame.frame_outputs(total, dev, {
            "rgb": three, "accumulation": one, "depth": one, "expected_depth": one, **{f"prop_depth_{i}": one for i in range(s.n_prop)},
            **({"normals": three, "pred_normals": three} if self.normals else {})})
        self._refresh_constants()
        for a in range(0, total, n):
            k = min(a + n, total) - a
            b = a + k
            load_chunk(a, k)
            self._run_chunk()
            out["rgb"][a:b].copy_(s.rgb[:k])
            out["accumulation"][a:b, 0].copy_(s.acc[:k])
            out["expected_depth"][a:b, 0].copy_(s.depth_exp[:k])
            out["depth"][a:b, 0].copy_(s.depth_med[-1][:k])
            for i in range(s.n_prop):
                out[f"prop_depth_{i}"][a:b, 0].copy_(s.depth_med[i][:k])
            if self.normals:
                out["normals"][a:b].copy_(self.normals_img[:k])
                out["pred_normals"][a:b].copy_(self.pred_normals_img[:k])
        return out

    @profiler.time_function
    @torch.no_grad()
    def render(self, camera_ray_bundle) -> Dict[str, Tensor]:
        """-> the reference's output dict for a camera (`rgb`, `accumulation`, `depth`, `expected_depth`, `prop_depth_i`; a
        normals runner: also `normals`, `pred_normals`), each `[*image_shape, C]`."""
        s, n = self.step, self.chunk
        image_shape = camera_ray_bundle.origins.shape[:-1]
        o = camera_ray_bundle.origins.reshape(-1, 3)
        d = camera_ray_bundle.directions.reshape(-1, 3)
        nears, fars = getattr(camera_ray_bundle, "nears", None), getattr(camera_ray_bundle, "fars", None)
        if nears is None or fars is None:  # the collider's planes (scene_colliders.py:40-44 sets them when either is missing)
            load_chunk = eval_frame.padded_loader((s.origins, s.directions), (o, d), n)
            return eval_frame.as_image(self._render_rays(o.shape[0], o.device, load_chunk), image_shape)
        # A bundle that carries its own bounds (the texel rays of exporter/texture_utils.py:386-400) keeps them, as the collider
        # leaves it alone: they ride into the schedule with the rays, and the runner — cached on the model — gets its planes back.
        nr, fr = nears.reshape(-1).to(torch.float32), fars.reshape(-1).to(torch.float32)
        load_chunk = eval_frame.padded_loader((s.origins, s.directions, s.nears, s.fars), (o, d, nr, fr), n)
        try:
            return eval_frame.as_image(self._render_rays(o.shape[0], o.device, load_chunk), image_shape)
        finally:
            self._restore_bounds()

    def _restore_bounds(self) -> None:
        """The schedule's per-ray bounds back to what every camera frame renders with: near 0, far `far_plane`."""
        self.step.nears.zero_()
        self.step.fars.fill_(float(self.model.config.far_plane))

    @profiler.time_function
    @torch.no_grad()
    def render_texels(self, atlas, mesh, raylen_dev: Tensor, out_u8: Tensor, out_f32: Optional[Tensor] = None) -> None:
        """The texture of `mesh` (vertices, normals `[V,3]` fp32, faces `[F,3]` int32 on the device) over `atlas`
        (texture.TexelAtlas): one ray per texel, from half of raylen_dev[0] outside the surface along the negated normal, near 0,
        far raylen (exporter/texture_utils.py:374-400). Per chunk ONE nsamd_texel_rays launch writes the rays and their bounds
        straight into the schedule's static input buffers, the chunk runs as for any frame, and nsamd_texture_store writes its
        rgb rows as 8-bit levels into out_u8 `[H W, 3]` (or `[H, W, 3]`) uint8: no `[H, W]` bundle, no `[total, C]` output —
        only rgb leaves a chunk. out_f32 `[H W, 3]` fp32 receives the unquantised rgb as well (tests)."""
        s, n = self.step, self.chunk
        total = int(atlas.width) * int(atlas.height)
        pod = atlas.native()
        self._refresh_constants()
        try:
            for a in range(0, total, n):
                k = min(a + n, total) - a
                F.texel_rays_launch(pod, mesh.vertices, mesh.normals, mesh.faces, raylen_dev, a, k, n, s.origins, s.directions,
                                    s.nears, s.fars)
                self._run_chunk()
                F.texture_store_launch(s.rgb, k, a, out_u8)
                if out_f32 is not None:
                    out_f32[a:a + k].copy_(s.rgb[:k])
        finally:
            self._restore_bounds()

    @profiler.time_function
    @torch.no_grad()
    def render_camera(self, c2w: Tensor, fx: float, fy: float, cx: float, cy: float, height: int, width: int,
                      lens=None) -> Dict[str, Tensor]:
        """`render` for ONE pinhole camera WITHOUT a ray bundle: each chunk's rays are generated straight into the schedule's
        static input buffers (nsamd_raygen_pinhole_grid: pixel first + i of the implicit row-major grid, the arithmetic of
        Cameras.generate_rays(camera_indices=0, keep_shape=True), cameras/cameras.py:321-503 perspective branch) — what
        Model.get_outputs_for_camera (models/base_model.py:166-175) builds as an [H, W] bundle with ~40 torch launches over
        full-image tensors and then slices. Same bits as `render` on that bundle. c2w: [3, 4] on the model's device.
        lens = (camera_type, distortion): the camera is of CameraType 1 - 3 (perspective, fisheye, equirectangular) with six
        distortion parameters or None, and its chunks come from nsamd_raygen_lens_grid (the bits of functional.raygen_lens)."""
        s, n = self.step, self.chunk
        dev = s.origins.device
        c2w, lens = eval_frame.prepare_view(c2w, lens, dev)

        def load_chunk(a, k):
            F.raygen_grid_launch(c2w, fx, fy, cx, cy, lens, width, a, k, n, s.origins, s.directions)

        return eval_frame.as_image(self._render_rays(int(height) * int(width), dev, load_chunk), (int(height), int(width)))


def supported(model, normals: bool = False) -> Optional[str]:
    """None, or why this model's eval render has to stay on the module path. normals=False: the plain runner (it has no normals
    outputs, so it refuses a `predict_normals` model); normals=True: the runner with the normals stages."""
    cfg = model.config
    if not normals and getattr(cfg, "predict_normals", False):
        return "predict_normals"
    if not all(hasattr(model, a) for a in ("proposal_networks", "field", "proposal_sampler")):
        return "not a nerfacto model"
    if normals:
        fld = model.field
        if not (getattr(cfg, "predict_normals", False) and getattr(fld, "use_pred_normals", False)):
            return "not a predict_normals model"
        if fld.mlp_base.encoding.spec.num_levels != 16:
            return "normals need a 16-level main grid"
    return None


def runner_for(model, device) -> Optional[EvalRenderer]:
    """The model's cached EvalRenderer (rebuilt when the chunk size changed) for an eval render of rays on `device`, or None:
    the module path (training mode, not a GPU, NSAMD_EVAL_RUNNER=0, or a configuration `supported` refuses)."""
    if not eval_frame.runner_enabled(model, device):
        return None
    normals = eval_frame.predicts_normals(model)
    if supported(model, normals=normals) is not None:
        return None
    runner = getattr(model, "_eval_runner", None)
    if runner is None or runner.chunk != model.config.eval_num_rays_per_chunk or runner.normals != normals:
        runner = model._eval_runner = EvalRenderer(model, normals=normals)
    return runner
