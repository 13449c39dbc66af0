"""Full-image eval render of the instant-ngp path as a device-side chunk loop — what eval_render.EvalRenderer is to nerfacto.

Reference: `Model.get_outputs_for_camera_ray_bundle` (models/base_model.py:178-205) slices the frame in Python and runs
`forward` per chunk: through this package's modules ~40 torch glue launches, an allocation per intermediate, a bincount, a
`torch.cat` per output and a host read of the sample count during which the GPU idles. In eval mode the sampler has no
sigma_fn (ray_samplers.py:404-431: `get_sigma_fn` returns None when not training) and does not jitter: no visibility
thinning, no alpha threshold, no compaction — every occupied lattice step gets the full field and is composited. So a chunk is

    march (count) -> prefix -> [host read of the total] -> march (write) -> positions + direction rows -> field
    -> weights + compositing + per-ray midpoint range in one launch -> depth clip

over static, capacity-sized buffers, launched eagerly through the helpers of `functional` (the candidate count is data-dependent
and the kernels take it by value: nothing is captured). The per-ray tail is nsamd_packed_render_fwd, bit for bit
nsamd_packed_weights_fwd + nsamd_packed_composite_fwd, written straight into the chunk's rows of the preallocated frame outputs;
the clip of renderers.py:381-383 (per forward call, i.e. per chunk) is an amin / amax over the chunk's per-ray midpoint ranges.

The host read does not drain the GPU: the per-ray arrays exist twice, and chunk c + 1's count pass, prefix and total copy are
issued BEFORE chunk c's write / points / field / render launches, with an event behind the copy. The host waits for that event
only — chunk c's field runs meanwhile. `prefetch=False` reads and launches strictly in turn; the bits are the same.

A chunk without any candidate takes the reference's fake sample (ray 0, [1, 1]; ray_samplers.py:494-500) through the same
launches. What differs from the module path is the rounding of the positions only (nsamd_packed_ray_points against the torch
expression), as for ngp_step.NgpTrainStep.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from . import _native as N
from . import eval_frame
from . import functional as F
from .ngp_step import STASH_CAP
from .utils import profiler


class DeviceLaunches:
    """The runner's launches and its one host read, on the current stream. A CPU test stands in an object with these methods
    built from the oracle's restatements (as tests/cpu_runner.py does for the training runners)."""

    def host_word(self) -> Tensor:
        return torch.zeros(1, dtype=torch.int64).pin_memory()

    def event(self):
        return torch.cuda.Event()

    def raygen(self, c2w: Tensor, fx: float, fy: float, cx: float, cy: float, lens, width: int, first: int, count: int,
               origins: Tensor, directions: Tensor) -> None:
        """Rays of pixels first .. first + count - 1 of one camera's row-major grid (lens None: pinhole; else (type, distortion))."""
        F.raygen_grid_launch(c2w, fx, fy, cx, cy, lens, width, first, count, count, origins, directions)

    @staticmethod
    def _grid(grid) -> N.OccGrid:
        return F._occgrid_native(grid.binaries, grid._roi, grid._coarse)

    def march_count(self, origins, directions, t_min, t_max, n, near, far, grid, step, cone, counts, stash) -> None:
        F.occgrid_march_count_launch(origins, directions, t_min, t_max, n, near, far, self._grid(grid), step, cone, None, counts,
                                     stash, STASH_CAP)

    def packed_info(self, counts, n, info, total) -> None:
        F.packed_info_launch(counts, n, info, total)

    def total_copy(self, total: Tensor, host: Tensor, event) -> None:
        """The total on its way to the pinned word, an event behind the copy."""
        host.copy_(total, non_blocking=True)
        event.record()

    def total_read(self, host: Tensor, event) -> int:
        """THE host read of a chunk: waits for that chunk's copy only, not for what was launched behind it."""
        event.synchronize()
        return int(host[0])

    def march_write(self, origins, directions, t_min, t_max, n, near, far, grid, step, cone, info, stash, ray_indices, t_starts,
                    t_ends) -> None:
        F.occgrid_march_write_launch(origins, directions, t_min, t_max, n, near, far, self._grid(grid), step, cone, None, info,
                                     stash, STASH_CAP, ray_indices, t_starts, t_ends)

    def ray_points(self, origins, directions, ray_indices, t_starts, t_ends, count, positions, sample_directions) -> None:
        F.packed_ray_points_launch(origins, directions, ray_indices, t_starts, t_ends, count, positions, sample_directions)

    def field(self, fld, positions, count, enc, sel, sample_directions, app_const, density, rgb) -> None:
        """NerfactoField on `count` points, one direction row per point, the eval appearance row for all of them."""
        tbl = fld.mlp_base.encoding
        fm = F.field_mlp(*F.field_params(fld), fld.average_init_density)
        F.field_forward(tbl.hash_table, tbl.spec, fld._transform, fld._box, N.make_points(positions=positions), count, enc, sel,
                        sample_directions, None, app_const, 1, fm, density, rgb)

    def render(self, t_starts, t_ends, sigmas, rgb, info, n, bg_mode, bg_vals, out_rgb, acc, depth, mid_lo, mid_hi) -> None:
        F.packed_render_launch(t_starts, t_ends, sigmas, rgb, info, n, bg_mode, bg_vals, True, out_rgb, acc, depth, mid_lo, mid_hi)


class _Slot:
    """One of the two sets of per-ray arrays: chunk c + 1 is counted into one while chunk c's launches read the other."""

    def __init__(self, chunk: int, dev, launches) -> None:
        f = lambda *shape, dtype=torch.float32: torch.zeros(shape, device=dev, dtype=dtype)  # noqa: E731
        self.origins, self.directions = f(chunk, 3), f(chunk, 3)
        self.t_min, self.t_max = f(chunk), f(chunk)
        self.counts = f(chunk, dtype=torch.int32)
        self.stash = f(chunk, STASH_CAP, 2)
        self.info = f(chunk, 2, dtype=torch.int64)
        self.total = f(1, dtype=torch.int64)
        self.host, self.event = launches.host_word(), launches.event()
        self.first = self.k = 0


class NgpEvalRenderer:
    def __init__(self, model, chunk: Optional[int] = None, prefetch: bool = True, cap_candidates: int = 0, launches=None) -> None:
        """prefetch: issue the next chunk's count pass before this chunk's field (False: read, then launch, strictly in turn —
        same bits). cap_candidates: the candidate buffers' first capacity (grown 1.5 x on demand). launches: see DeviceLaunches."""
        reason = supported(model)
        if reason is not None:
            raise ValueError(f"NgpEvalRenderer: {reason}")
        self.model = model
        self.chunk = int(chunk or model.config.eval_num_rays_per_chunk)
        self.prefetch = bool(prefetch)
        dev = next(model.parameters()).device
        if launches is None:
            N.require_cuda(next(model.parameters()))
            launches = DeviceLaunches()
        self.dev, self.launches = dev, launches
        self.slots = (_Slot(self.chunk, dev, launches), _Slot(self.chunk, dev, launches))
        self.mid_lo, self.mid_hi = torch.empty(self.chunk, device=dev), torch.empty(self.chunk, device=dev)
        fld = model.field
        self.L2 = fld.mlp_base.encoding.spec.out_dim
        # (sic) the embedding exists, 32 wide, when use_appearance_embedding is FALSE (models/instant_ngp.py:104)
        emb = fld.embedding_appearance.embedding.weight if fld.embedding_appearance is not None else None
        self.app_const = torch.zeros(emb.shape[1], device=dev) if emb is not None else None
        self.cap_c, self.grown = 0, 0
        self._grow_candidates(int(cap_candidates) if cap_candidates > 0 else 64 * self.chunk)
        self.bg_mode, self.bg_vals = 0, None

    def _grow_candidates(self, cap: int) -> None:
        if cap <= self.cap_c:
            return
        b = lambda *shape, dtype=torch.float32: torch.empty(shape, device=self.dev, dtype=dtype)  # noqa: E731
        self.grown += self.cap_c > 0
        self.cap_c = cap
        self.c_ri = b(cap, dtype=torch.int64)
        self.c_ts, self.c_te = b(cap), b(cap)
        self.c_pos, self.c_dirs = b(cap, 3), b(cap, 3)
        self.c_enc = b(self.L2 * cap)  # the 32-row feature block, feature-major over the chunk's candidates
        self.c_sel, self.c_sigma = b(cap), b(cap)
        self.c_rgb = b(cap, 3)

    # ---- a frame ----------------------------------------------------------------------------------------------------------
    def _refresh_constants(self) -> None:
        """Once per frame: the eval appearance row (fields/nerfacto_field.py:253-261: the embedding's mean, or zeros) into its
        static buffer, the background of the eval compositing, the grid's derived state."""
        m = self.model
        eval_frame.eval_appearance_row(m.field, self.app_const)
        self.bg_mode, self.bg_vals = F._packed_bg(m.renderer_rgb.background_color)
        m.occupancy_grid.ensure_derived()

    def _render_rays(self, total: int, load_chunk, has_bounds: bool) -> Dict[str, Tensor]:
        """The frame's chunk loop over `total` rays; `load_chunk(slot, first, k)` puts rays first .. first + k - 1 into the
        slot's origins / directions (and t_min / t_max with `has_bounds`)."""
        dev, n, L = self.dev, self.chunk, self.launches
        cfg = self.model.config
        out = eval_frame.frame_outputs(total, dev, {"rgb": (3, None), "accumulation": (1, None), "depth": (1, None),
                                                    "num_samples_per_ray": (1, torch.int64)})
        self._refresh_constants()
        grid = self.model.occupancy_grid
        march = (float(cfg.near_plane), min(float(cfg.far_plane), 3.0e38), grid, float(cfg.render_step_size), float(cfg.cone_angle))
        firsts = list(range(0, total, n))

        def rays(s: _Slot):
            k = s.k
            bounds = (s.t_min[:k], s.t_max[:k]) if has_bounds else (None, None)
            return (s.origins[:k], s.directions[:k], *bounds, k)

        def issue(c: int) -> None:  # chunk c's rays, count pass, prefix and total copy, into slot c & 1
            s = self.slots[c & 1]
            s.first, s.k = firsts[c], min(n, total - firsts[c])
            load_chunk(s, s.first, s.k)
            L.march_count(*rays(s), *march, s.counts[:s.k], s.stash[:s.k])
            L.packed_info(s.counts, s.k, s.info, s.total)
            L.total_copy(s.total, s.host, s.event)

        if firsts and self.prefetch:
            issue(0)
        for c in range(len(firsts)):
            s = self.slots[c & 1]
            if not self.prefetch:
                issue(c)
            mc = L.total_read(s.host, s.event)
            if self.prefetch and c + 1 < len(firsts):
                issue(c + 1)  # in front of this chunk's field: the next read finds its total ready
            self._launch_tail(s, mc, rays(s), march, out)
        return out

    def _launch_tail(self, s: _Slot, mc: int, rays, march, out: Dict[str, Tensor]) -> None:
        """Chunk `s` behind its host read: write pass, positions + direction rows, field, the per-ray tail into the chunk's rows
        of the frame outputs, depth clip."""
        L, k = self.launches, s.k
        a, b = s.first, s.first + k
        if mc > self.cap_c:
            self._grow_candidates(int(1.5 * mc))
        if mc:
            L.march_write(*rays, *march, s.info, s.stash[:k], self.c_ri, self.c_ts, self.c_te)
        else:  # a single fake sample (ray 0, [1, 1]) keeps every downstream shape valid (ray_samplers.py:494-500)
            mc = 1
            self.c_ri[:1].zero_()
            self.c_ts[:1].fill_(1.0)
            self.c_te[:1].fill_(1.0)
            s.info[:k].zero_()
            s.info[0, 1] = 1
        L.ray_points(rays[0], rays[1], self.c_ri, self.c_ts, self.c_te, mc, self.c_pos, self.c_dirs)
        L.field(self.model.field, self.c_pos, mc, self.c_enc, self.c_sel, self.c_dirs, self.app_const, self.c_sigma, self.c_rgb)
        depth = out["depth"][a:b, 0]
        L.render(self.c_ts, self.c_te, self.c_sigma, self.c_rgb, s.info, k, self.bg_mode, self.bg_vals, out["rgb"][a:b],
                 out["accumulation"][a:b, 0], depth, self.mid_lo[:k], self.mid_hi[:k])
        # expected depth clipped to the chunk's range of sample midpoints (renderers.py:381-383): ops over [k], not the samples
        torch.clamp(depth, min=self.mid_lo[:k].amin(), max=self.mid_hi[:k].amax(), out=depth)
        out["num_samples_per_ray"][a:b, 0].copy_(s.info[:k, 1])

    @profiler.time_function
    @torch.no_grad()
    def render(self, camera_ray_bundle) -> Dict[str, Tensor]:
        """-> the reference's output dict for a camera: `rgb` `[*image_shape, 3]`, `accumulation`, `depth` `[*image_shape, 1]`,
        `num_samples_per_ray` `[*image_shape, 1]` int64. Nears / fars on the bundle (a collider, a crop box) reach the marcher as
        t_min / t_max, as VolumetricSampler hands them on (ray_samplers.py:470-476)."""
        image_shape = camera_ray_bundle.origins.shape[:-1]
        o = camera_ray_bundle.origins.reshape(-1, 3)
        d = camera_ray_bundle.directions.reshape(-1, 3)
        nears, fars = getattr(camera_ray_bundle, "nears", None), getattr(camera_ray_bundle, "fars", None)
        has_bounds = nears is not None and fars is not None
        if has_bounds:
            nears, fars = nears.reshape(-1), fars.reshape(-1)

        def load_chunk(s: _Slot, a: int, k: int) -> None:
            s.origins[:k].copy_(o[a:a + k])
            s.directions[:k].copy_(d[a:a + k])
            if has_bounds:
                s.t_min[:k].copy_(nears[a:a + k])
                s.t_max[:k].copy_(fars[a:a + k])

        return eval_frame.as_image(self._render_rays(o.shape[0], load_chunk, has_bounds), image_shape)

    @profiler.time_function
    @torch.no_grad()
    def render_camera(self, c2w: Tensor, fx: float, fy: float, cx: float, cy: float, height: int, width: int,
                      lens=None) -> Dict[str, Tensor]:
        """`render` for ONE camera without a ray bundle, as EvalRenderer.render_camera: each chunk's rays are generated straight
        into its slot's buffers (nsamd_raygen_pinhole_grid; lens = (camera_type, distortion): nsamd_raygen_lens_grid). Same bits
        as `render` on the bundle `camera.generate_rays(camera_indices=0, keep_shape=True)` gives."""
        c2w, lens = eval_frame.prepare_view(c2w, lens, self.dev)
        view = (float(fx), float(fy), float(cx), float(cy), lens, int(width))

        def load_chunk(s: _Slot, a: int, k: int) -> None:
            self.launches.raygen(c2w, *view, a, k, s.origins, s.directions)

        return eval_frame.as_image(self._render_rays(int(height) * int(width), load_chunk, False), (int(height), int(width)))


def supported(model) -> Optional[str]:
    """None, or why this model's eval render has to stay on the module path."""
    if not all(hasattr(model, a) for a in ("occupancy_grid", "sampler", "field")):
        return "not an instant-ngp model"
    spec = model.field.mlp_base.encoding.spec
    if spec.num_levels != 16 or spec.out_dim != 32:
        return "the main-field kernels take 16 levels x 2 features"
    bgc = getattr(getattr(model, "renderer_rgb", None), "background_color", None)
    if isinstance(bgc, str) and bgc == "last_sample":
        return "background last_sample is not implemented for packed samples"
    return None


def runner_for(model, device) -> Optional[NgpEvalRenderer]:
    """The model's cached NgpEvalRenderer (rebuilt when the chunk size changed) for an eval render of rays on `device`, or None:
    the module path (training mode, not a GPU, NSAMD_EVAL_RUNNER=0, or a configuration `supported` refuses)."""
    if not eval_frame.runner_enabled(model, device) or supported(model) is not None:
        return None
    runner = getattr(model, "_ngp_eval_runner", None)
    if runner is None or runner.chunk != model.config.eval_num_rays_per_chunk:
        runner = model._ngp_eval_runner = NgpEvalRenderer(model)
    return runner
