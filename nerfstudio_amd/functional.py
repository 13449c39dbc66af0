"""torch.autograd glue over the nsamd C ABI (include/nsamd.h).

Each public function here is one stage of the nerfacto hot path running as hand-written gfx950
kernels. PyTorch only provides device memory, the stream and the autograd graph — no arithmetic of the path is done
by torch ops. Reference citations are relative to /root/reference/nerfstudio/.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _native as N


_GRID_CACHE: dict = {}

# When True, the backward kernels of the fused fields accumulate straight into `param.grad` whenever that buffer
# already exists (e.g. the views of arena.ParamArena) and autograd receives None for those inputs. This removes a
# zero-fill, a read-modify-write and an AccumulateGrad pass over every parameter (67 MB for the main hash table) per
# step. Semantics are those of gradient accumulation into a pre-zeroed .grad; off by default.
DIRECT_GRAD = False


def _grad_target(param: Tensor, needed: bool):
    """-> (buffer to accumulate into, value to return to autograd)."""
    if not needed:
        return None, None
    if DIRECT_GRAD and getattr(param, "grad", None) is not None and param.grad.is_contiguous():
        return param.grad, None
    buf = torch.zeros_like(param)
    return buf, buf


# ---------------------------------------------------------------------------------------------------------------
# configuration records
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class HashGridSpec:
    """Hyper-parameters of one multiresolution hash grid (HashEncoding ctor, field_components/encodings.py:321-347)."""

    num_levels: int
    min_res: int
    max_res: int
    log2_hashmap_size: int
    features_per_level: int = 2

    def __post_init__(self):
        if self.features_per_level != 2:
            raise ValueError("nerfstudio_amd hash grids are built for features_per_level=2 (every nerfacto config)")
        if not (0 < self.num_levels <= N.MAX_LEVELS):
            raise ValueError(f"num_levels must be in [1, {N.MAX_LEVELS}]")

    @property
    def table_size(self) -> int:
        return 2**self.log2_hashmap_size

    @property
    def out_dim(self) -> int:
        return self.num_levels * self.features_per_level

    @property
    def growth_factor(self) -> float:
        if self.num_levels > 1:
            return math.exp((math.log(self.max_res) - math.log(self.min_res)) / (self.num_levels - 1))
        return 1.0

    def scalings(self) -> Tensor:
        """floor(min_res * growth**level) evaluated in fp32 on the host, exactly like encodings.py:342-344 (where
        `np.float64 ** LongTensor` dispatches to torch's __rpow__ and yields fp32)."""
        levels = torch.arange(self.num_levels)
        return torch.floor(self.min_res * self.growth_factor**levels).to(torch.float32)

    def reachable_prefix(self):
        """(rows, index): the leading `rows` rows of the `[L*T, F]` table belong to the coarse levels whose lattice
        (res + 1)^3 is smaller than the table, and `index` (int64, sorted) lists the rows of that prefix a position in
        [0, 1]^3 can ever touch. The torch path hashes every level (encodings.py:398-415), so on those levels all other
        rows keep a zero gradient for ever — SURVEY.md 8a: 332 k of the first 2.6 M rows of the nerfacto main table —
        and a data-parallel exchange only needs the listed ones. Host arithmetic in wrap-around uint32, as the kernels."""
        import numpy as np

        T = self.table_size
        scal = self.scalings().tolist()
        parts, levels = [], 0
        for lvl, s_ in enumerate(scal):
            res = int(s_)
            if (res + 1) ** 3 >= T:
                break
            c = np.arange(res + 1, dtype=np.uint32)
            with np.errstate(over="ignore"):
                h = c[:, None, None] ^ (c[None, :, None] * np.uint32(2654435761)) ^ (c[None, None, :] * np.uint32(805459861))
            parts.append(np.unique((h & np.uint32(T - 1)).astype(np.int64)) + lvl * T)
            levels += 1
        index = torch.from_numpy(np.concatenate(parts)) if parts else torch.zeros(0, dtype=torch.int64)
        return levels * T, index

    def native(self) -> N.Grid:
        g = _GRID_CACHE.get(self)
        if g is None:
            g = N.make_grid(self.num_levels, self.log2_hashmap_size, self.scalings().tolist())
            _GRID_CACHE[self] = g
        return g


@dataclass
class PointSpec:
    """Sample points either as explicit `[M,3]` positions or as rays + bin edges (never materialised)."""

    positions: Optional[Tensor] = None
    origins: Optional[Tensor] = None
    directions: Optional[Tensor] = None
    t_bins: Optional[Tensor] = None

    @property
    def ray_mode(self) -> bool:
        return self.positions is None

    @property
    def num_points(self) -> int:
        if self.positions is not None:
            return self.positions.shape[0]
        return self.t_bins.shape[0] * (self.t_bins.shape[1] - 1)

    @property
    def samples_per_ray(self) -> int:
        return 0 if self.positions is not None else self.t_bins.shape[1] - 1

    def tensors(self) -> Tuple[Optional[Tensor], ...]:
        return (self.positions, self.origins, self.directions, self.t_bins)

    def native(self) -> N.Points:
        N.require_cuda(*self.tensors())
        return N.make_points(self.positions, self.origins, self.directions, self.t_bins, self.samples_per_ray)

    def needs_position_grad(self) -> bool:
        if self.positions is not None:
            return self.positions.requires_grad
        return bool(self.origins.requires_grad or self.directions.requires_grad)


def _f32c(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _spec_from_flat(positions, origins, directions, t_bins) -> PointSpec:
    return PointSpec(_f32c(positions), _f32c(origins), _f32c(directions), _f32c(t_bins))


_SCATTER_WS: dict = {}
_FIELD_WS: dict = {}


def field_bwd_workspace(device) -> Tuple[Tensor, int]:
    """Scratch for the per-workgroup weight-gradient partials of nsamd_field_mlp_bwd (<= 1024 workgroups x 12544)."""
    ws = _FIELD_WS.get(str(device))
    if ws is None:
        ws = torch.empty(1024 * 12544, device=device, dtype=torch.float32)
        _FIELD_WS[str(device)] = ws
    return ws, ws.numel()


_SCATTER_WS_MAX = 8  # cached workspaces (least recently used ones are dropped: a main-table workspace is ~0.75 GB)


DENSITY_WS_FLOATS = 1024 * 1156  # <= 1024 workgroups x (64 x 16 + 2 x 64 + 1, padded to 16 B) partial sums


def density_bwd_workspace(device, slot: int = 0) -> Tensor:
    """Scratch rows for the weight-gradient partials of nsamd_density_mlp_bwd[_gated] (summed in a fixed order). One
    buffer per (device, slot): calls that may overlap on different streams take different slots."""
    key = (str(device), "density", slot)
    ws = _FIELD_WS.get(key)
    if ws is None:
        ws = torch.empty(DENSITY_WS_FLOATS, device=device, dtype=torch.float32)
        _FIELD_WS[key] = ws
    return ws


_SCATTER_BUCKET = 1 << 16  # workspaces are sized for M rounded up to a multiple of this many points


def _cached_workspace(grid: HashGridSpec, device, num_points: int, kind, plan) -> Tuple[Optional[Tensor], int]:
    """A scatter workspace out of `_SCATTER_WS`, keyed (grid, bucket, device, kind). `plan(M)` is the library's query for M
    points: (words it wants — 0 when that path does not apply —, leading words that must start as zero). Only those state
    words are initialised (the kernels leave them at zero); the bulk never is.
    Cached per M rounded up to 64 k points: the packed instant-ngp path changes M every step (occupancy-grid sampling,
    DynamicBatch), and a cache keyed by the exact M would allocate a fresh ~GB workspace per step. A cached
    workspace serves every M of its bucket — the kernels lay the buffer out for the M of the call — and is re-allocated
    only if the library asks for more words than it holds. At most _SCATTER_WS_MAX entries; evicting one waits for the
    device first (a side-stream scatter may still be reading it). One workspace serves one call at a time: callers that
    overlap scatters on different streams must use different (grid, bucket) keys or serialise (train_step does)."""
    bucket = max(1, -(-int(num_points) // _SCATTER_BUCKET)) * _SCATTER_BUCKET
    key = (grid, bucket, str(device), kind)
    ws = _SCATTER_WS.get(key)
    if ws is not None:
        need = plan(num_points)[0] if num_points != bucket else ws.numel()  # (sized for the bucket's own M)
        if 0 < need <= ws.numel():
            _SCATTER_WS[key] = _SCATTER_WS.pop(key)  # most recently used last
            return ws, ws.numel()
        if need <= 0:
            return None, 0
        torch.cuda.synchronize(device)  # (never seen: the plan grows with M) replace it by a larger one
        _SCATTER_WS.pop(key)
    plans = [plan(m) for m in {bucket, max(int(num_points), 1)}]
    words, states = max(p[0] for p in plans), max(p[1] for p in plans)
    if words <= 0:
        return None, 0
    ws = torch.empty(words, device=device, dtype=torch.float32)
    ws[:states].zero_()
    while len(_SCATTER_WS) >= _SCATTER_WS_MAX:
        torch.cuda.synchronize(device)  # no kernel on any stream may still be using the evicted buffer
        _SCATTER_WS.pop(next(iter(_SCATTER_WS)))
    _SCATTER_WS[key] = ws
    return ws, ws.numel()


def _scatter_workspace(grid: HashGridSpec, device, num_points: int = 0, write_only: bool = False) -> Tuple[Optional[Tensor], int]:
    """Device scratch for the table-gradient scatter (csrc/scatter.hip): per (level, tile) a queue of 16-B records, the
    per-workgroup segment counts, a spill list (nsamd_hashgrid_encode_bwd_workspace; the state words are header + cursors,
    a few KB that depend on the grid only). Cached by `_cached_workspace` under kind `write_only`."""
    lib, g = N.load(), grid.native()
    return _cached_workspace(grid, device, num_points, write_only, lambda m: (
        int(lib.nsamd_hashgrid_encode_bwd_workspace(g, m, 1 if write_only else 0)),
        int(lib.nsamd_hashgrid_encode_bwd_workspace_state(g, m))))


def _producer_scatter_workspace(grid: HashGridSpec, device, num_points: int) -> Tuple[Optional[Tensor], int]:
    """Scratch of nsamd_field_mlp_bwd_scatter (the main field's backward emits the scatter's records itself): one static
    segment per (MLP workgroup, table tile) + dynamic areas + the worst-case spill list, ~1.4 GB for the nerfacto main table at
    196 608 points. Cached by `_cached_workspace` under kind "producer"."""
    lib, g = N.load(), grid.native()

    def plan(m):
        state = C.c_int64(0)
        words = int(lib.nsamd_field_mlp_bwd_scatter_workspace(g, m, C.byref(state)))
        return words, int(state.value)

    return _cached_workspace(grid, device, num_points, "producer", plan)


def scatter_events(ws: Tensor) -> Tuple[int, int, int]:
    """(spilled, unordered, lost) record counts of a scatter workspace since it was created
    (nsamd_hashgrid_scatter_events): `unordered` > 0 means some call was exact but not bit-reproducible."""
    ev = (C.c_uint32 * 3)()
    N.check(N.load().nsamd_hashgrid_scatter_events(N.ptr(ws), C.cast(ev, C.c_void_p), N.stream()), "scatter_events")
    return int(ev[0]), int(ev[1]), int(ev[2])


# ---------------------------------------------------------------------------------------------------------------
# launch records and launches shared by the autograd Functions below and the explicit schedules (train_step,
# eval_render, ngp_step, trainer): `hash_forward`, `table_scatter`, `ray_terms_launch`, `field_forward`, `field_backward`,
# `density_forward`, `density_backward` here and every `*_launch` further down take tensors and records, never a module, and
# are the only callers of their entry points: outputs are the caller's, counts that no shape gives are integers, nothing is
# allocated, copied or waited for (each is a node of a captured iteration), and the one check is the contiguity assert of
# `N.ptr` / `N.ptr_array` on each argument. `_f32c` / `N.require_cuda` (device, dtype, making contiguous) stay with
# the allocating wrappers, the only callers that receive foreign tensors. Records are built at launch time, never cached:
# they hold raw addresses, and an arena built later re-homes the parameters.
# ---------------------------------------------------------------------------------------------------------------
def density_mlp(W0: Tensor, b0: Tensor, W1: Tensor, b1: Tensor, average_init_density: float) -> N.DensityMlp:
    """nsamd_density_mlp of a proposal network's MLP (HashMLPDensityField: `mlp_base[1].param_tensors()`)."""
    return N.DensityMlp(N.ptr(W0), N.ptr(b0), N.ptr(W1), N.ptr(b1), W0.shape[1], W0.shape[0], float(average_init_density))


def field_params(fld):
    """(the ten MLP tensors of a NerfactoField in nsamd_field_mlp order, its appearance table or None)."""
    emb = fld.embedding_appearance.embedding.weight if fld.embedding_appearance is not None else None
    return [*fld.mlp_base.mlp.param_tensors(), *fld.mlp_head.param_tensors()], emb


def field_mlp(params: Sequence[Tensor], appearance: Optional[Tensor], average_init_density: float,
              ray_terms: Optional[Tensor] = None, ray_inputs: Optional[Tensor] = None) -> N.FieldMlp:
    """nsamd_field_mlp: the ten MLP tensors, the appearance table and, when the per-ray terms of head layer 0 are in use
    (include/nsamd.h), their buffers."""
    fm = N.FieldMlp(*(N.ptr(p) for p in params), N.ptr(appearance), appearance.shape[0] if appearance is not None else 0,
                    float(average_init_density))
    fm.ray_terms, fm.ray_inputs = N.ptr(ray_terms), N.ptr(ray_inputs)
    return fm


def field_mlp_grads(params: Sequence[Tensor], appearance: Optional[Tensor], grad_of) -> N.FieldMlpGrads:
    """nsamd_field_mlp_grads: `grad_of(tensor)` -> the buffer its gradient accumulates into; appearance None: no gradient of
    the appearance table."""
    return N.FieldMlpGrads(*(N.ptr(grad_of(p)) for p in params), N.ptr(grad_of(appearance)) if appearance is not None else None)


def hash_forward(pts: N.Points, M: int, transform: int, box: N.Aabb, table: Tensor, grid: HashGridSpec, enc: Tensor,
                 stride_p: int, stride_k: int, sel: Optional[Tensor]) -> None:
    """nsamd_hashgrid_encode_fwd on the current stream: the hash features of M points after the position normalisation
    `transform` / `box` into `enc` (point p, feature k at p * stride_p + k * stride_k) and, unless None, the selector `sel`."""
    N.check(N.load().nsamd_hashgrid_encode_fwd(pts, M, transform, box, N.ptr(table), grid.native(), N.ptr(enc), stride_p,
                                               stride_k, N.ptr(sel), N.stream()), "hashgrid_encode_fwd")


def table_scatter(pts: N.Points, M: int, transform: int, box: N.Aabb, table: Tensor, grid: HashGridSpec, denc: Tensor,
                  stride_p: int, stride_k: int, dtable: Optional[Tensor], dpos: Optional[Tensor] = None,
                  write_only: bool = False) -> None:
    """The hash table's gradient scatter of M points from their encoded-feature gradient `denc` (point p, feature k at
    p * stride_p + k * stride_k), on the current stream: `dtable` written (nsamd_hashgrid_encode_bwd_set, write_only) or
    accumulated into (nsamd_hashgrid_encode_bwd, which can also return dL/dposition in `dpos`)."""
    lib = N.load()
    ws, ws_n = _scatter_workspace(grid, denc.device, M, write_only=write_only)
    fn = lib.nsamd_hashgrid_encode_bwd_set if write_only else lib.nsamd_hashgrid_encode_bwd
    N.check(fn(pts, M, transform, box, N.ptr(table), grid.native(), N.ptr(denc), stride_p, stride_k, N.ptr(dtable), N.ptr(dpos),
               N.ptr(ws), ws_n, N.stream()), "hashgrid_encode_bwd")


def ray_terms_apply(dir_group: int, M: int) -> bool:
    """The ray-terms rule (include/nsamd.h, nsamd_field_mlp.ray_terms): samples grouped by ray, whole 16-sample tiles per ray."""
    return dir_group % 16 == 0 and M % dir_group == 0 and M > 0


def ray_terms_launch(dirs: Tensor, cams: Optional[Tensor], app_const: Optional[Tensor], rays: int, mlp: N.FieldMlp,
                     terms: Tensor, inputs: Optional[Tensor], slot=None, slots: int = 0) -> None:
    """nsamd_field_ray_terms on the current stream: head layer 0's share of the 48 per-ray inputs (SH of the view direction,
    appearance row) into `terms` `[rays, 64]`, the inputs themselves into `inputs` `[rays, 48 | 16]` (None: not kept).
    slot (the device address of a float) and slots: `dirs` `[slots, rays, 3]` and `cams` `[slots, rays]` are a pool of batches
    and the rays are those of the slot, clamped as `select_batch_launch` clamps it (nsamd_field_mlp.batch_slot) — the bits of
    the selection followed by the plain launch, without the selection in front."""
    mlp.batch_slot, mlp.batch_slots = slot, slots
    try:
        N.check(N.load().nsamd_field_ray_terms(N.ptr(dirs), N.ptr(cams), N.ptr(app_const), rays, mlp, N.ptr(terms),
                                               N.ptr(inputs), N.stream()), "field_ray_terms")
    finally:
        mlp.batch_slot, mlp.batch_slots = None, 0  # (the caller's struct goes on to the forward)


def field_forward(table: Tensor, grid: HashGridSpec, transform: int, box: N.Aabb, pts: N.Points, M: int, enc: Tensor,
                  sel: Tensor, dirs: Tensor, cams: Optional[Tensor], app_const: Optional[Tensor], dir_group: int,
                  mlp: N.FieldMlp, density: Tensor, rgb: Optional[Tensor]) -> None:
    """Hash grid + MLPs of a NerfactoField on M points, on the current stream: encoded features `enc` (feature-major) and
    selector `sel`, then density and rgb (None: density only). Point p takes direction / camera row p // dir_group;
    cams None -> the appearance row `app_const` for every point."""
    hash_forward(pts, M, transform, box, table, grid, enc, 1, M, sel)
    N.check(N.load().nsamd_field_mlp_fwd(N.ptr(enc), N.ptr(sel), N.ptr(dirs), N.ptr(cams), N.ptr(app_const), dir_group, M, mlp,
                                         N.ptr(density), N.ptr(rgb), N.stream()), "field_mlp_fwd")


def field_backward(table: Tensor, grid: HashGridSpec, transform: int, box: N.Aabb, pts: N.Points, M: int, enc: Tensor,
                   sel: Tensor, dirs: Tensor, cams: Optional[Tensor], app_const: Optional[Tensor], dir_group: int,
                   mlp: N.FieldMlp, ddens: Tensor, drgb: Tensor, denc: Tensor, grads: N.FieldMlpGrads, fws: Tensor,
                   dtable: Optional[Tensor], write_only: bool, fuse: bool = True, keep_denc: bool = False, on_denc=None,
                   fused_launch=None, dpos: Optional[Tensor] = None) -> None:
    """Backward of `field_forward` from the density / rgb gradients: the MLPs' gradients into `grads` (`fws`: the
    field_bwd_workspace), the table's into `dtable`. When the table gradient is written (write_only), the grid has 16
    levels and the library plans a producer workspace, the MLP backward emits the table scatter's records itself
    (nsamd_field_mlp_bwd_scatter: no `denc` round trip, no route launch; `denc` is stored only with keep_denc) —
    `fused_launch(args)` issues it instead of the single launch when given (args: the entry point's arguments before the
    phase and the stream). Otherwise, and always with `dpos` (dL/dposition, which only the scatter can return),
    nsamd_field_mlp_bwd writes `denc`, then `on_denc()` runs, then the table scatter unless `dtable` and `dpos` are None."""
    lib, st = N.load(), N.stream()
    if fuse and write_only and dpos is None and grid.num_levels == 16:
        sws, sws_n = _producer_scatter_workspace(grid, denc.device, M)
        if sws is not None:
            args = (pts, transform, box, grid.native(), N.ptr(enc), N.ptr(sel), N.ptr(dirs), N.ptr(cams),
                    N.ptr(app_const), dir_group, M, mlp, N.ptr(ddens), N.ptr(drgb), N.ptr(denc) if keep_denc else None, grads,
                    N.ptr(fws), fws.numel(), N.ptr(dtable), N.ptr(sws), sws_n)
            if fused_launch is not None:
                fused_launch(args)
            else:
                N.check(lib.nsamd_field_mlp_bwd_scatter(*args, st), "field_mlp_bwd_scatter")
            return
    N.check(lib.nsamd_field_mlp_bwd(N.ptr(enc), N.ptr(sel), N.ptr(dirs), N.ptr(cams), N.ptr(app_const), dir_group, M, mlp,
                                    N.ptr(ddens), N.ptr(drgb), N.ptr(denc), grads, N.ptr(fws), fws.numel(), st), "field_mlp_bwd")
    if on_denc is not None:
        on_denc()
    if dtable is not None or dpos is not None:
        table_scatter(pts, M, transform, box, table, grid, denc, 1, M, dtable, dpos, write_only=write_only)


def density_forward(enc: Tensor, sel: Tensor, M: int, mlp: N.DensityMlp, density: Tensor, pre: Optional[Tensor]) -> None:
    """nsamd_density_mlp_fwd on the current stream: density `[M]` of the feature-major features `enc` and selector `sel`; `pre`:
    the pre-activation the backward reads (None: not kept)."""
    N.check(N.load().nsamd_density_mlp_fwd(N.ptr(enc), N.ptr(sel), M, mlp, N.ptr(density), N.ptr(pre), N.stream()),
            "density_mlp_fwd")


def density_backward(enc: Tensor, sel: Tensor, pre: Tensor, ddens: Tensor, M: int, mlp: N.DensityMlp, denc: Tensor,
                     grads: Sequence[Tensor], ws: Tensor) -> None:
    """The ungated nsamd_density_mlp_bwd on the current stream: from the density gradient `ddens` the encoded-feature gradient
    `denc` (feature-major) and the gradients of W0, b0, W1, b1 accumulated into `grads`; `ws`: a density_bwd_workspace."""
    N.check(N.load().nsamd_density_mlp_bwd(N.ptr(enc), N.ptr(sel), N.ptr(pre), N.ptr(ddens), M, mlp, N.ptr(denc),
                                           *(N.ptr(g) for g in grads), N.ptr(ws), ws.numel(), N.stream()), "density_mlp_bwd")


def _position_grads(spec: PointSpec, dpos: Optional[Tensor]):
    """dL/dpositions [M,3] (None: not wanted) -> gradients of whatever the spec was built from."""
    if dpos is None:
        return None, None, None
    if not spec.ray_mode:
        return dpos, None, None
    n, s1 = spec.t_bins.shape
    d = dpos.view(n, s1 - 1, 3)
    mid = ((spec.t_bins[:, :-1] + spec.t_bins[:, 1:]) / 2)[..., None]
    return None, d.sum(dim=1), (d * mid).sum(dim=1)


def _table_and_position_grads(ctx, spec, table, table_ref, grid, transform, box, denc, stride_p, stride_k):
    """End of the backward of a Function whose inputs begin (positions, origins, directions, t_bins, table): the table scatter
    from the encoded-feature gradient `denc` -> (gradients of the first three, what autograd gets for the table)."""
    ttable, rtable = _grad_target(table_ref, ctx.needs_input_grad[4])
    dpos = torch.empty((spec.num_points, 3), device=table.device, dtype=torch.float32) if any(ctx.needs_input_grad[:3]) else None
    if ttable is not None or dpos is not None:
        table_scatter(spec.native(), spec.num_points, transform, box, table, grid, denc, stride_p, stride_k, ttable, dpos)
    return (*_position_grads(spec, dpos), rtable)


# ---------------------------------------------------------------------------------------------------------------
# a8  stand-alone hash encoding (Encoding API: [M,3] in [0,1] -> [M, 2L])
# ---------------------------------------------------------------------------------------------------------------
class _HashEncodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, table: Tensor, grid: HashGridSpec):
        N.require_cuda(x, table)
        x = _f32c(x)
        M = x.shape[0]
        out = torch.empty((M, grid.out_dim), device=x.device, dtype=torch.float32)
        hash_forward(N.make_points(positions=x), M, N.XFORM_NONE, N.Aabb(), table, grid, out, grid.out_dim, 1, None)
        ctx.save_for_backward(x, table)
        ctx.grid = grid
        return out

    @staticmethod
    def backward(ctx, gout: Tensor):
        x, table = ctx.saved_tensors
        grid: HashGridSpec = ctx.grid
        dtable = torch.zeros_like(table) if ctx.needs_input_grad[1] else None
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        if dtable is not None or dx is not None:
            table_scatter(N.make_points(positions=x), x.shape[0], N.XFORM_NONE, N.Aabb(), table, grid, _f32c(gout),
                          grid.out_dim, 1, dtable, dx)
        return dx, dtable, None


def hashgrid_encode(x: Tensor, table: Tensor, grid: HashGridSpec) -> Tensor:
    """HashEncoding.pytorch_fwd semantics (encodings.py:417-458) on `[*bs,3]` -> `[*bs, 2L]`."""
    shape = x.shape[:-1]
    return _HashEncodeFn.apply(x.reshape(-1, 3), table, grid).view(*shape, grid.out_dim)


class _SpecEncodeFn(torch.autograd.Function):
    """Hash features of sample points given as a PointSpec (positions or rays + bins), with the fields' position
    normalisation (aabb or L-inf contraction) and selector fused into the gather kernel. -> (enc [M, 2L], selector [M])."""

    @staticmethod
    def forward(ctx, positions, origins, directions, t_bins, table, grid: HashGridSpec, transform: int, aabb):
        spec = _spec_from_flat(positions, origins, directions, t_bins)
        N.require_cuda(table)
        M = spec.num_points
        enc = torch.empty((M, grid.out_dim), device=table.device, dtype=torch.float32)
        sel = torch.empty((M,), device=table.device, dtype=torch.float32)
        box = aabb if isinstance(aabb, N.Aabb) else N.make_aabb(aabb)
        hash_forward(spec.native(), M, transform, box, table, grid, enc, grid.out_dim, 1, sel)
        ctx.spec, ctx.grid, ctx.transform, ctx.box, ctx.table_ref = spec, grid, transform, box, table
        ctx.save_for_backward(table)
        ctx.mark_non_differentiable(sel)
        return enc, sel

    @staticmethod
    def backward(ctx, genc: Tensor, _gsel):
        (table,) = ctx.saved_tensors
        gp, go, gd, rtable = _table_and_position_grads(ctx, ctx.spec, table, ctx.table_ref, ctx.grid, ctx.transform, ctx.box,
                                                       _f32c(genc), ctx.grid.out_dim, 1)
        return gp, go, gd, None, rtable, None, None, None


def spec_encode(spec: PointSpec, table: Tensor, grid: HashGridSpec, transform: int, aabb) -> Tuple[Tensor, Tensor]:
    """(hash features `[M, 2L]`, selector `[M]`) of the points of `spec` after the field's position normalisation
    (fields/density_fields.py:95-103 + encodings.py:417-458) — the encoding half of a field, for heads that are not one
    of the fused MLP shapes."""
    return _SpecEncodeFn.apply(spec.positions, spec.origins, spec.directions, spec.t_bins, table, grid, transform, aabb)


def sh4_encode(directions: Tensor) -> Tensor:
    """SHEncoding(levels=4).pytorch_fwd (encodings.py:791-794); no gradient (it is @torch.no_grad there)."""
    N.require_cuda(directions)
    shape = directions.shape[:-1]
    d = _f32c(directions.detach().reshape(-1, 3))
    out = torch.empty((d.shape[0], 16), device=d.device, dtype=torch.float32)
    N.check(N.load().nsamd_sh4_encode(N.ptr(d), d.shape[0], N.ptr(out), N.stream()), "sh4_encode")
    return out.view(*shape, 16)


_FREQS: dict = {}


def nerf_encode_launch(pts: N.Points, M: int, freqs: Tensor, include_input: bool, out: Tensor) -> None:
    """nsamd_nerf_encode on the current stream: M points at the frequencies `freqs` -> dense rows `[M, 6 F (+3)]` of `out`."""
    N.check(N.load().nsamd_nerf_encode(pts, M, N.ptr(freqs), freqs.shape[0], int(bool(include_input)), N.ptr(out), N.stream()),
            "nerf_encode")


def nerf_encode(spec: PointSpec, num_frequencies: int, min_freq_exp: float, max_freq_exp: float,
                include_input: bool = False) -> Tensor:
    """NeRFEncoding.forward (encodings.py:148-189, no covariances) on the points of `spec` -> `[M, 6 F (+3)]`. The
    frequencies are evaluated with torch on the host once (`2 ** linspace`), as the reference does per call. No gradient
    w.r.t. the points (vanilla-nerf has none to take: no camera optimiser, no learned warp)."""
    N.require_cuda(*spec.tensors())
    if any(t is not None and t.requires_grad for t in spec.tensors()):
        raise RuntimeError("nsamd NeRFEncoding has no backward: the encoded points must not require grad")
    dev = next(t for t in spec.tensors() if t is not None).device
    freqs = _frequencies(num_frequencies, min_freq_exp, max_freq_exp, dev)
    spec = _spec_from_flat(*spec.tensors())
    M = spec.num_points
    out = torch.empty((M, 6 * num_frequencies + (3 if include_input else 0)), device=dev, dtype=torch.float32)
    nerf_encode_launch(spec.native(), M, freqs, include_input, out)
    return out


def _frequencies(num_frequencies: int, min_freq_exp: float, max_freq_exp: float, dev) -> Tensor:
    """The device copy of `2 ** linspace(min, max, F)`, evaluated with torch on the host once per configuration."""
    key = (num_frequencies, float(min_freq_exp), float(max_freq_exp), dev)
    if key not in _FREQS:
        _FREQS[key] = (2 ** torch.linspace(min_freq_exp, max_freq_exp, num_frequencies)).to(dev)
    return _FREQS[key]


def ipe_encode_launch(pts: N.Points, M: int, pixel_area: Optional[Tensor], variances: Optional[Tensor], freqs: Tensor,
                      include_input: bool, out: Tensor) -> None:
    """nsamd_ipe_encode on the current stream: the integrated encoding of M Gaussians -> dense rows `[M, 6 F (+3)]` of `out`.
    Ray mode (`pts` holds rays and bin edges): `pixel_area [num_rays]`, the Gaussians are formed in the kernel; explicit mode
    (`pts.positions` = the means): `variances [M,3]`, the covariance diagonals."""
    N.check(N.load().nsamd_ipe_encode(pts, M, N.ptr(pixel_area), N.ptr(variances), N.ptr(freqs), freqs.shape[0],
                                      int(bool(include_input)), N.ptr(out), N.stream()), "ipe_encode")


def ipe_encode(spec: PointSpec, pixel_area: Optional[Tensor], variances: Optional[Tensor], num_frequencies: int,
               min_freq_exp: float, max_freq_exp: float, include_input: bool = False) -> Tensor:
    """NeRFEncoding.forward with covariances (encodings.py:162-186) -> `[M, 6 F (+3)]`: on the conical frustums of the samples
    of `spec`'s rays (`pixel_area`, one value per ray) or on explicit means `spec.positions` with the covariance diagonals
    `variances [M,3]`. No gradient (mip-NeRF has none to take: no camera optimiser, no learned warp)."""
    given = (*spec.tensors(), pixel_area, variances)
    N.require_cuda(*given)
    if any(t is not None and t.requires_grad for t in given):
        raise RuntimeError("nsamd integrated NeRFEncoding has no backward: the encoded Gaussians must not require grad")
    if (pixel_area if spec.ray_mode else variances) is None:
        raise ValueError("ipe_encode takes pixel_area with rays and variances with explicit means")
    dev = next(t for t in spec.tensors() if t is not None).device
    freqs = _frequencies(num_frequencies, min_freq_exp, max_freq_exp, dev)
    spec = _spec_from_flat(*spec.tensors())
    M = spec.num_points
    if spec.ray_mode:
        pixel_area, variances = _f32c(pixel_area.reshape(-1)), None
        if pixel_area.shape[0] != spec.t_bins.shape[0]:
            raise ValueError("ipe_encode: one pixel area per ray")
    else:
        pixel_area, variances = None, _f32c(variances.reshape(-1, 3))
        if variances.shape[0] != M:
            raise ValueError("ipe_encode: one covariance diagonal per mean")
    out = torch.empty((M, 6 * num_frequencies + (3 if include_input else 0)), device=dev, dtype=torch.float32)
    ipe_encode_launch(spec.native(), M, pixel_area, variances, freqs, include_input, out)
    return out


def nerf_encode_bwd_rays_launch(pts: N.Points, M: int, freqs: Tensor, include_input: bool, d_out: Tensor, d_out_stride: int,
                                d_origins: Tensor, d_directions: Tensor, accumulate: bool = False) -> None:
    """nsamd_nerf_encode_bwd_rays on the current stream: the gradient of nerf_encode_launch's rows (row p of `d_out` starts at
    p * d_out_stride floats) with respect to the M sample positions of the rays `pts`, reduced per ray into `d_origins` /
    `d_directions` `[n,3]` (written, or added to)."""
    N.check(N.load().nsamd_nerf_encode_bwd_rays(pts, M, N.ptr(freqs), freqs.shape[0], int(bool(include_input)), N.ptr(d_out),
                                                int(d_out_stride), N.ptr(d_origins), N.ptr(d_directions),
                                                1 if accumulate else 0, N.stream()), "nerf_encode_bwd_rays")


def contract_linf(x: Tensor) -> Tensor:
    """SceneContraction(order=inf).forward (spatial_distortions.py:66-69), forward only (the fused fields carry
    the Jacobian inside their own backward)."""
    N.require_cuda(x)
    shape = x.shape
    xf = _f32c(x.detach().reshape(-1, 3))
    out = torch.empty_like(xf)
    N.check(N.load().nsamd_contract_linf(N.ptr(xf), xf.shape[0], N.ptr(out), N.stream()), "contract_linf")
    return out.view(shape)


# ---------------------------------------------------------------------------------------------------------------
# a9  stand-alone dense layer / MLP of arbitrary width                              (field_components/mlp.py:160-179)
# ---------------------------------------------------------------------------------------------------------------
_ACT = {None: 0, "relu": 1, "sigmoid": 2, "softplus": 3}


def linear_launch(x: Tensor, W: Tensor, b: Optional[Tensor], M: int, act: int, y: Tensor) -> None:
    """nsamd_linear_fwd on the current stream: y = act(x W^T + b) on the first M rows of `x` `[., K]`, `W` `[N, K]`."""
    N.check(N.load().nsamd_linear_fwd(N.ptr(x), N.ptr(W), N.ptr(b), M, W.shape[1], W.shape[0], act, N.ptr(y), N.stream()),
            "linear_fwd")


def linear_backward_launch(x: Tensor, W: Tensor, y: Optional[Tensor], dy: Tensor, M: int, act: int, dx: Optional[Tensor],
                           dW: Optional[Tensor], db: Optional[Tensor]) -> None:
    """nsamd_linear_bwd on the current stream, on the first M rows: `dx` `[., K]` written, `dW` `[N, K]` / `db` `[N]` accumulated
    into (each optional); `y` is the forward's output (not read without an activation: may then be None)."""
    N.check(N.load().nsamd_linear_bwd(N.ptr(x), N.ptr(W), N.ptr(y), N.ptr(dy), M, W.shape[1], W.shape[0], act, N.ptr(dx),
                                      N.ptr(dW), N.ptr(db), N.stream()), "linear_bwd")


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, W: Tensor, b: Optional[Tensor], act: int):
        N.require_cuda(x, W, b)
        x = _f32c(x)
        M, K = x.shape
        Nout = W.shape[0]
        y = torch.empty((M, Nout), device=x.device, dtype=torch.float32)
        linear_launch(x, W, b, M, act, y)
        ctx.save_for_backward(x, W, y)
        ctx.act, ctx.has_bias = act, b is not None
        return y

    @staticmethod
    def backward(ctx, gy: Tensor):
        x, W, y = ctx.saved_tensors
        gy = _f32c(gy)
        M, K = x.shape
        Nout = W.shape[0]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.zeros_like(W) if ctx.needs_input_grad[1] else None
        db = torch.zeros((Nout,), device=x.device, dtype=torch.float32) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        linear_backward_launch(x, W, y, gy, M, ctx.act, dx, dW, db)
        return dx, dW, db, None


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor], activation: Optional[str] = None) -> Tensor:
    """act(x W^T + b) on `[*bs, K]` with `weight [N,K]` (nn.Linear layout); activation None | "relu" | "sigmoid" |
    "softplus"."""
    shape = x.shape[:-1]
    y = _LinearFn.apply(x.reshape(-1, x.shape[-1]), weight, bias, _ACT[activation])
    return y.view(*shape, weight.shape[0])


# ---------------------------------------------------------------------------------------------------------------
# a6  proposal density field: contraction -> hash grid -> MLP -> trunc_exp           (fields/density_fields.py:94-117)
# ---------------------------------------------------------------------------------------------------------------
class _DensityFieldFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, positions, origins, directions, t_bins, table, W0, b0, W1, b1, grid: HashGridSpec,
                transform: int, aabb, avg_density: float):
        spec = _spec_from_flat(positions, origins, directions, t_bins)
        N.require_cuda(table, W0, b0, W1, b1)
        M = spec.num_points
        dev = table.device
        enc = torch.empty((grid.out_dim, M), device=dev, dtype=torch.float32)  # feature-major
        sel = torch.empty((M,), device=dev, dtype=torch.float32)
        box = aabb if isinstance(aabb, N.Aabb) else N.make_aabb(aabb)
        hash_forward(spec.native(), M, transform, box, table, grid, enc, 1, M, sel)
        mlp = density_mlp(W0, b0, W1, b1, avg_density)
        density = torch.empty((M,), device=dev, dtype=torch.float32)
        pre = torch.empty((M,), device=dev, dtype=torch.float32)
        density_forward(enc, sel, M, mlp, density, pre)
        ctx.spec, ctx.grid, ctx.transform, ctx.box, ctx.avg = spec, grid, transform, box, avg_density
        ctx.param_refs = (table, W0, b0, W1, b1)
        ctx.save_for_backward(table, W0, b0, W1, b1, enc, sel, pre)
        return density

    @staticmethod
    def backward(ctx, gdens: Tensor):
        table, W0, b0, W1, b1, enc, sel, pre = ctx.saved_tensors
        spec: PointSpec = ctx.spec
        M = spec.num_points
        denc = torch.empty_like(enc)
        refs = ctx.param_refs
        (tW0, rW0), (tb0, rb0), (tW1, rW1), (tb1, rb1) = (_grad_target(r, True) for r in refs[1:])
        density_backward(enc, sel, pre, _f32c(gdens), M, density_mlp(W0, b0, W1, b1, ctx.avg), denc, (tW0, tb0, tW1, tb1),
                         density_bwd_workspace(table.device))
        gp, go, gd, rtable = _table_and_position_grads(ctx, spec, table, refs[0], ctx.grid, ctx.transform, ctx.box, denc, 1, M)
        return gp, go, gd, None, rtable, rW0, rb0, rW1, rb1, None, None, None, None


def density_field(spec: PointSpec, table: Tensor, W0: Tensor, b0: Tensor, W1: Tensor, b1: Tensor, grid: HashGridSpec,
                  transform: int, aabb: Optional[Tensor], average_init_density: float) -> Tensor:
    """HashMLPDensityField.get_density on M points -> density `[M]`."""
    return _DensityFieldFn.apply(spec.positions, spec.origins, spec.directions, spec.t_bins, table, W0, b0, W1, b1,
                                 grid, transform, aabb, float(average_init_density))


# ---------------------------------------------------------------------------------------------------------------
# a10 + a12  nerfacto main field                                                   (fields/nerfacto_field.py:203-310)
# ---------------------------------------------------------------------------------------------------------------
class _NerfactoFieldFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, positions, origins, directions, t_bins, table, bW0, bb0, bW1, bb1, hW0, hb0, hW1, hb1, hW2, hb2,
                appearance, view_dirs, camera_indices, appearance_const, dir_group: int, grid: HashGridSpec,
                transform: int, aabb, avg_density: float):
        spec = _spec_from_flat(positions, origins, directions, t_bins)
        params = (bW0, bb0, bW1, bb1, hW0, hb0, hW1, hb1, hW2, hb2)
        N.require_cuda(table, *params, view_dirs, appearance, camera_indices, appearance_const)
        if tuple(bW0.shape) != (64, 32) or tuple(bW1.shape) != (16, 64) or tuple(hW1.shape) != (64, 64) or \
                tuple(hW2.shape) != (3, 64) or hW0.shape[0] != 64 or hW0.shape[1] not in (31, 63):
            raise RuntimeError(
                "nsamd main-field kernels are built for the nerfacto shape: L=16,F=2 -> 64 -> 16, head 31|63 -> 64 -> 64 "
                f"-> 3; got base {tuple(bW0.shape)}/{tuple(bW1.shape)}, head {tuple(hW0.shape)}/{tuple(hW1.shape)}/"
                f"{tuple(hW2.shape)}")
        M = spec.num_points
        dev = table.device
        view_dirs = _f32c(view_dirs)
        cams = camera_indices.contiguous().to(torch.int64) if camera_indices is not None else None
        enc = torch.empty((grid.out_dim, M), device=dev, dtype=torch.float32)
        sel = torch.empty((M,), device=dev, dtype=torch.float32)
        box = aabb if isinstance(aabb, N.Aabb) else N.make_aabb(aabb)
        mlp = field_mlp(params, appearance, avg_density)
        density = torch.empty((M,), device=dev, dtype=torch.float32)
        rgb = torch.empty((M, 3), device=dev, dtype=torch.float32)
        ctx.ray_terms = ctx.ray_inputs = None
        if ray_terms_apply(dir_group, M):
            rays = M // dir_group
            has_app = cams is not None or appearance_const is not None
            ctx.ray_terms = torch.empty((rays, 64), device=dev, dtype=torch.float32)
            ctx.ray_inputs = torch.empty((rays, 48 if has_app else 16), device=dev, dtype=torch.float32)
            ray_terms_launch(view_dirs, cams, appearance_const, rays, mlp, ctx.ray_terms, ctx.ray_inputs)
            mlp.ray_terms, mlp.ray_inputs = N.ptr(ctx.ray_terms), N.ptr(ctx.ray_inputs)
        field_forward(table, grid, transform, box, spec.native(), M, enc, sel, view_dirs, cams, appearance_const, dir_group,
                      mlp, density, rgb)
        ctx.spec, ctx.grid, ctx.transform, ctx.box, ctx.avg, ctx.dir_group = spec, grid, transform, box, avg_density, dir_group
        ctx.cams, ctx.app_const, ctx.has_app = cams, appearance_const, appearance is not None
        ctx.param_refs = (table, *params, appearance)
        ctx.save_for_backward(table, *params, appearance if appearance is not None else table.new_empty(0), enc, sel,
                              view_dirs)
        return density, rgb

    @staticmethod
    def backward(ctx, gdens: Tensor, grgb: Tensor):
        table, *params, appearance, enc, sel, view_dirs = ctx.saved_tensors
        appearance = appearance if ctx.has_app else None
        spec: PointSpec = ctx.spec
        M = spec.num_points
        gdens = _f32c(gdens) if gdens is not None else torch.zeros((M,), device=table.device)
        grgb = _f32c(grgb) if grgb is not None else torch.zeros((M, 3), device=table.device)
        denc = torch.empty_like(enc)
        refs = ctx.param_refs
        tparams, gparams = zip(*(_grad_target(r, True) for r in refs[1:11]))
        tapp, gapp = _grad_target(refs[11], True) if (appearance is not None and ctx.cams is not None) else (None, None)
        mlp = field_mlp(params, appearance, ctx.avg, ctx.ray_terms, ctx.ray_inputs)
        grads = field_mlp_grads(tparams, tapp, lambda g: g)  # (the targets themselves)
        ttable, dtable = _grad_target(refs[0], ctx.needs_input_grad[4])
        dpos = torch.empty((M, 3), device=table.device, dtype=torch.float32) if any(ctx.needs_input_grad[:3]) else None
        field_backward(table, ctx.grid, ctx.transform, ctx.box, spec.native(), M, enc, sel, view_dirs, ctx.cams, ctx.app_const,
                       ctx.dir_group, mlp, gdens, grgb, denc, grads, field_bwd_workspace(table.device)[0], ttable,
                       write_only=False, fuse=False, dpos=dpos)
        gp, go, gd = _position_grads(spec, dpos)
        return (gp, go, gd, None, dtable, *gparams, gapp, None, None, None, None, None, None, None, None)


def nerfacto_field(spec: PointSpec, table: Tensor, base_params: Sequence[Tensor], head_params: Sequence[Tensor],
                   appearance: Optional[Tensor], view_dirs: Tensor, camera_indices: Optional[Tensor],
                   appearance_const: Optional[Tensor], dir_group: int, grid: HashGridSpec, transform: int,
                   aabb: Optional[Tensor], average_init_density: float) -> Tuple[Tensor, Tensor]:
    """NerfactoField.forward on M points -> (density `[M]`, rgb `[M,3]`).

    view_dirs `[num_dirs,3]` / camera_indices `[num_dirs]`: point p uses row p // dir_group.
    camera_indices None -> every point uses `appearance_const` `[32]` (eval: mean or zeros, nerfacto_field.py:253-261);
    both None -> the field has no appearance embedding.
    """
    return _NerfactoFieldFn.apply(spec.positions, spec.origins, spec.directions, spec.t_bins, table, *base_params,
                                  *head_params, appearance, view_dirs, camera_indices, appearance_const, int(dir_group),
                                  grid, transform, aabb, float(average_init_density))


# ---------------------------------------------------------------------------------------------------------------
# a4 / a13 / a14  samplers
# ---------------------------------------------------------------------------------------------------------------
_LINSPACE_CACHE: dict = {}


def _linspace(kind: str, num_samples: int, device) -> Tensor:
    """Host-evaluated torch.linspace tables (so the fp32 values are bit-identical to the reference's CPU path)."""
    key = (kind, num_samples, str(device))
    t = _LINSPACE_CACHE.get(key)
    if t is None:
        if kind == "edges":  # ray_samplers.py:100
            t = torch.linspace(0.0, 1.0, num_samples + 1)
        else:  # "u": ray_samplers.py:317 / :326
            nb = num_samples + 1
            t = torch.linspace(0.0, 1.0 - (1.0 / nb), steps=nb)
        t = t.to(device)
        _LINSPACE_CACHE[key] = t
    return t


def piecewise_bins_launch(nears: Tensor, fars: Tensor, edges: Tensor, jitter: Optional[Tensor], per_edge: int, spacing: int,
                          s_bins: Tensor, t_bins: Tensor) -> None:
    """nsamd_piecewise_bins on the current stream: the initial sampler's `[n, S+1]` spacing and Euclidean edges from `nears` /
    `fars` `[n]`, the linspace table `edges` and the draws `jitter` (None: bin centres; per_edge 1: one draw per edge)."""
    n, s1 = s_bins.shape
    N.check(N.load().nsamd_piecewise_bins(N.ptr(nears), N.ptr(fars), N.ptr(edges), N.ptr(jitter), per_edge, n, s1 - 1, spacing,
                                          N.ptr(s_bins), N.ptr(t_bins), N.stream()), "piecewise_bins")


@torch.no_grad()
def piecewise_bins(nears: Tensor, fars: Tensor, num_samples: int, jitter: Optional[Tensor], spacing: int = 0
                   ) -> Tuple[Tensor, Tensor]:
    """UniformLinDispPiecewiseSampler (ray_samplers.py:78-128, 225-248). nears/fars `[N]` or `[N,1]`;
    jitter = the U[0,1) draws: `[N,1]` (single_jitter), `[N,S+1]` (one per bin edge) or None (eval). Returns
    (s_bins, t_bins) `[N, S+1]`."""
    N.require_cuda(nears, fars, jitter)
    nears, fars = _f32c(nears.reshape(-1)), _f32c(fars.reshape(-1))
    n = nears.shape[0]
    per_edge = _jitter_layout(jitter, n, num_samples + 1)
    jitter = _f32c(jitter.reshape(-1)) if jitter is not None else None
    s_bins = torch.empty((n, num_samples + 1), device=nears.device, dtype=torch.float32)
    t_bins = torch.empty_like(s_bins)
    edges = _linspace("edges", num_samples, nears.device)
    piecewise_bins_launch(nears, fars, edges, jitter, per_edge, int(spacing), s_bins, t_bins)
    return s_bins, t_bins


def _jitter_layout(jitter: Optional[Tensor], num_rays: int, num_edges: int) -> int:
    """0: one draw per ray (or none), 1: one per bin edge; anything else is a caller error."""
    if jitter is None or jitter.numel() == num_rays:
        return 0
    if jitter.numel() != num_rays * num_edges:
        raise ValueError(f"jitter must hold one draw per ray ({num_rays}) or per bin edge ({num_rays} x {num_edges}), "
                         f"got {tuple(jitter.shape)}")
    return 1


def weights_launch(t_bins: Tensor, density: Tensor, weights: Tensor) -> None:
    """nsamd_weights_fwd on the current stream: `weights` `[n, S]` from the edges `[n, S+1]` and the densities (n * S values)."""
    n, s = weights.shape
    N.check(N.load().nsamd_weights_fwd(N.ptr(t_bins), N.ptr(density), n, s, N.ptr(weights), N.stream()), "weights_fwd")


def weights_backward_launch(t_bins: Tensor, density: Tensor, dweights: Tensor, ddensity: Tensor) -> None:
    """nsamd_weights_bwd on the current stream: the density gradient (n * S values) from `dweights` `[n, S]`."""
    n, s = dweights.shape
    N.check(N.load().nsamd_weights_bwd(N.ptr(t_bins), N.ptr(density), N.ptr(dweights), n, s, N.ptr(ddensity), N.stream()),
            "weights_bwd")


class _WeightsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t_bins: Tensor, density: Tensor):
        N.require_cuda(t_bins, density)
        t_bins, density = _f32c(t_bins), _f32c(density)
        w = torch.empty_like(density)
        weights_launch(t_bins, density, w)
        ctx.save_for_backward(t_bins, density)
        return w

    @staticmethod
    def backward(ctx, gw: Tensor):
        t_bins, density = ctx.saved_tensors
        gd = torch.empty_like(density)
        weights_backward_launch(t_bins, density, _f32c(gw), gd)
        return None, gd


def weights_from_density(t_bins: Tensor, density: Tensor) -> Tensor:
    """RaySamples.get_weights (cameras/rays.py:129-152): `[N,S+1]`, `[N,S]` -> `[N,S]`."""
    return _WeightsFn.apply(t_bins, density)


def pdf_resample_launch(s_bins_prev: Tensor, weights: Tensor, u_base: Tensor, jitter: Optional[Tensor], nears: Tensor,
                        fars: Tensor, anneal: float, anneal_dev: Optional[Tensor], histogram_padding: float, eps: float,
                        spacing: int, per_edge: int, include_original: bool, num_samples: int, s_bins: Tensor, t_bins: Tensor,
                        inds: Optional[Tensor]) -> None:
    """nsamd_pdf_resample on the current stream: `num_samples` + 1 new edges per ray drawn from the histogram `weights`
    `[n, S_prev]` over `s_bins_prev` into `s_bins` / `t_bins` (with include_original merged into the existing edges), the
    searchsorted result into `inds` (None: not kept). `anneal_dev`: the anneal exponent in device memory instead of `anneal`."""
    n, s_prev = weights.shape
    N.check(N.load().nsamd_pdf_resample(N.ptr(s_bins_prev), N.ptr(weights), s_prev, N.ptr(u_base), N.ptr(jitter), N.ptr(nears),
                                        N.ptr(fars), anneal, N.ptr(anneal_dev), histogram_padding, eps,
                                        1.0 / (2 * (num_samples + 1)), spacing, per_edge, int(include_original), n, num_samples,
                                        N.ptr(s_bins), N.ptr(t_bins), N.ptr(inds), N.stream()), "pdf_resample")


@torch.no_grad()
def pdf_resample(s_bins_prev: Tensor, weights: Tensor, num_samples: int, jitter: Optional[Tensor], nears: Tensor,
                 fars: Tensor, anneal: float = 1.0, histogram_padding: float = 0.01, eps: float = 1e-5,
                 return_indices: bool = False, anneal_dev: Optional[Tensor] = None, spacing: int = 0,
                 include_original: bool = False):
    """PDFSampler.generate_ray_samples (ray_samplers.py:276-372) incl. the weight anneal (ray_samplers.py:601). Returns
    (s_bins, t_bins[, inds]): `[N, S+1]` edges, or `[N, S_prev+S+2]` with include_original (the new edges merged into the
    existing ones, :356-357); inds int32 `[N, S+1]` (the searchsorted result of the new edges). jitter: `[N,1]`
    (single_jitter), `[N,S+1]` (one per new edge) or None (eval)."""
    N.require_cuda(s_bins_prev, weights, nears, fars, jitter)
    s_bins_prev, weights = _f32c(s_bins_prev), _f32c(weights.detach())
    nears, fars = _f32c(nears.reshape(-1)), _f32c(fars.reshape(-1))
    n, s_prev = weights.shape
    nb = num_samples + 1
    per_edge = _jitter_layout(jitter, n, nb)
    jitter = _f32c(jitter.reshape(-1)) if jitter is not None else None
    dev = weights.device
    s_bins = torch.empty((n, nb + (s_prev + 1 if include_original else 0)), device=dev, dtype=torch.float32)
    t_bins = torch.empty_like(s_bins)
    inds = torch.empty((n, nb), device=dev, dtype=torch.int32) if return_indices else None
    u_base = _linspace("u", num_samples, dev)
    pdf_resample_launch(s_bins_prev, weights, u_base, jitter, nears, fars, float(anneal), anneal_dev, float(histogram_padding),
                        float(eps), int(spacing), per_edge, bool(include_original), num_samples, s_bins, t_bins, inds)
    return (s_bins, t_bins, inds) if return_indices else (s_bins, t_bins)


def distance_gradient_scale_launch(t_bins: Tensor, d_density: Optional[Tensor], d_rgb: Optional[Tensor]) -> None:
    """nsamd_distance_gradient_scale on the current stream: the per-sample gradients of the samples between the edges `t_bins`
    `[n, S+1]` multiplied in place by clamp(((start + end) / 2)^2, 0, 1)."""
    n, s1 = t_bins.shape
    N.check(N.load().nsamd_distance_gradient_scale(N.ptr(t_bins), n, s1 - 1, N.ptr(d_density), N.ptr(d_rgb), N.stream()),
            "distance_gradient_scale")


class _DistanceGradientScaleFn(torch.autograd.Function):
    """scale_gradients_by_distance_squared (model_components/losses.py:534-569): identity forward; the gradient is multiplied
    by clamp(((start + end) / 2)^2, 0, 1) per sample (nsamd_distance_gradient_scale)."""

    @staticmethod
    def forward(ctx, density: Tensor, rgb: Tensor, t_bins: Tensor):
        ctx.save_for_backward(t_bins)
        return density.view_as(density), rgb.view_as(rgb)

    @staticmethod
    def backward(ctx, g_density, g_rgb):
        (t_bins,) = ctx.saved_tensors
        gd = _f32c(g_density).clone() if g_density is not None else None
        gr = _f32c(g_rgb).clone() if g_rgb is not None else None
        distance_gradient_scale_launch(t_bins, gd, gr)
        return gd, gr, None


def scale_gradients_by_distance_squared(density: Tensor, rgb: Tensor, t_bins: Tensor) -> Tuple[Tensor, Tensor]:
    """density `[N,S,1]`, rgb `[N,S,3]` of a ray batch with euclidean bin edges t_bins `[N,S+1]` -> the same values whose
    gradients are scaled by the squared distance (NerfactoModelConfig.use_gradient_scaling)."""
    N.require_cuda(density, rgb, t_bins)
    return _DistanceGradientScaleFn.apply(density, rgb, _f32c(t_bins))


# ---------------------------------------------------------------------------------------------------------------
# a16-a18  compositing
# ---------------------------------------------------------------------------------------------------------------
def _bg_args(background, device):
    """-> (mode, ctypes float[3] or None)."""
    if background is None or (isinstance(background, str) and background in ("random", "none")):
        return N.BG_NONE, None
    if isinstance(background, str):
        if background == "last_sample":
            return N.BG_LAST_SAMPLE, None
        named = {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}
        if background not in named:
            raise ValueError(f"unsupported background colour {background!r}")
        vals = named[background]
    else:
        vals = [float(v) for v in torch.as_tensor(background).reshape(3).tolist()]
    return N.BG_CONSTANT, (C.c_float * 3)(*vals)


def composite_launch(rgb: Optional[Tensor], weights: Tensor, t_bins: Optional[Tensor], bg_mode: int, bg_vals, eval_clamp: bool,
                     out_rgb: Optional[Tensor], acc: Optional[Tensor], depth: Optional[Tensor], median: Optional[Tensor],
                     median_index: Optional[Tensor], minmax_ws: Optional[Tensor]) -> None:
    """nsamd_composite_fwd on the current stream over `weights` `[n, S]`; every output is optional: the composited colour
    (eval_clamp: nan_to_num on the samples, clamp to [0, 1]), the accumulation, the expected depth (needs `minmax_ws`, 2 + 2
    ceil(n / 4) floats, for the global clip), the median depth and its int32 sample index."""
    n, s = weights.shape
    N.check(N.load().nsamd_composite_fwd(N.ptr(rgb), N.ptr(weights), N.ptr(t_bins), n, s, bg_mode, bg_vals, int(eval_clamp),
                                         N.ptr(out_rgb), N.ptr(acc), N.ptr(depth), N.ptr(median), N.ptr(median_index),
                                         N.ptr(minmax_ws), N.stream()),
            "composite_fwd" if out_rgb is not None else "composite_fwd(median)" if median is not None else "composite_fwd(acc)")


class _CompositeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb: Tensor, weights: Tensor, t_bins: Optional[Tensor], bg_mode: int, bg_vals, want_depth: bool):
        N.require_cuda(rgb, weights, t_bins)
        rgb, weights = _f32c(rgb), _f32c(weights)
        t_bins = _f32c(t_bins) if t_bins is not None else None
        n, s = weights.shape
        dev = weights.device
        out = torch.empty((n, 3), device=dev, dtype=torch.float32)
        acc = torch.empty((n,), device=dev, dtype=torch.float32)
        depth = torch.empty((n,), device=dev, dtype=torch.float32) if want_depth else None
        ws = torch.empty((2 + 2 * ((n + 3) // 4),), device=dev, dtype=torch.float32) if want_depth else None
        composite_launch(rgb, weights, t_bins if want_depth else None, bg_mode, bg_vals, False, out, acc, depth, None, None, ws)
        ctx.save_for_backward(rgb, weights, t_bins if want_depth else None, ws)
        ctx.bg_mode, ctx.bg_vals, ctx.want_depth = bg_mode, bg_vals, want_depth
        if want_depth:
            return out, acc, depth
        return out, acc, None

    @staticmethod
    def backward(ctx, g_out, g_acc, g_depth):
        rgb, weights, t_bins, ws = ctx.saved_tensors
        n, s = weights.shape
        g_out = _f32c(g_out) if g_out is not None else None
        g_acc = _f32c(g_acc) if g_acc is not None else None
        g_depth = _f32c(g_depth) if (g_depth is not None and ctx.want_depth) else None
        d_rgb = torch.empty_like(rgb)
        d_w = torch.empty_like(weights)
        N.check(N.load().nsamd_composite_bwd(N.ptr(rgb), N.ptr(weights), N.ptr(t_bins), n, s, ctx.bg_mode, ctx.bg_vals,
                                             N.ptr(g_out), N.ptr(g_acc), N.ptr(g_depth), N.ptr(ws), None, N.ptr(d_rgb),
                                             N.ptr(d_w), N.stream()), "composite_bwd")
        return d_rgb, d_w, None, None, None, None


def composite(rgb: Tensor, weights: Tensor, t_bins: Optional[Tensor] = None, background="last_sample",
              expected_depth: bool = True):
    """Training-mode RGB + accumulation (+ expected depth) in one launch, differentiable w.r.t. rgb and weights.
    rgb `[N,S,3]`, weights `[N,S]`, t_bins `[N,S+1]` -> (rgb `[N,3]`, accumulation `[N]`, depth `[N]` or None)."""
    mode, vals = _bg_args(background, weights.device)
    return _CompositeFn.apply(rgb, weights, t_bins, mode, vals, bool(expected_depth and t_bins is not None))


@torch.no_grad()
def composite_eval(rgb: Tensor, weights: Tensor, t_bins: Tensor, background="last_sample"):
    """Eval-mode compositing (nan_to_num on the samples, clamp to [0,1]; renderers.py:225-231):
    -> rgb `[N,3]`, accumulation `[N]`, expected depth `[N]`, median depth `[N]`."""
    N.require_cuda(rgb, weights, t_bins)
    rgb, weights, t_bins = _f32c(rgb), _f32c(weights), _f32c(t_bins)
    n, s = weights.shape
    dev = weights.device
    mode, vals = _bg_args(background, dev)
    out = torch.empty((n, 3), device=dev, dtype=torch.float32)
    acc = torch.empty((n,), device=dev, dtype=torch.float32)
    dexp = torch.empty((n,), device=dev, dtype=torch.float32)
    dmed = torch.empty((n,), device=dev, dtype=torch.float32)
    ws = torch.empty((2 + 2 * ((n + 3) // 4),), device=dev, dtype=torch.float32)
    composite_launch(rgb, weights, t_bins, mode, vals, True, out, acc, dexp, dmed, None, ws)
    return out, acc, dexp, dmed


@torch.no_grad()
def depth_median(weights: Tensor, t_bins: Tensor, return_index: bool = False):
    """DepthRenderer(method="median") (renderers.py:354-364) -> `[N]` (and the int32 sample index)."""
    N.require_cuda(weights, t_bins)
    weights, t_bins = _f32c(weights.detach()), _f32c(t_bins)
    n, s = weights.shape
    d = torch.empty((n,), device=weights.device, dtype=torch.float32)
    idx = torch.empty((n,), device=weights.device, dtype=torch.int32) if return_index else None
    composite_launch(None, weights, t_bins, N.BG_NONE, None, False, None, None, None, d, idx, None)
    return (d, idx) if return_index else d


@torch.no_grad()
def accumulation(weights: Tensor) -> Tensor:
    """AccumulationRenderer (renderers.py:293-317) without gradient -> `[N]` (use `composite` when training)."""
    N.require_cuda(weights)
    weights = _f32c(weights)
    n, s = weights.shape
    acc = torch.empty((n,), device=weights.device, dtype=torch.float32)
    composite_launch(None, weights, None, N.BG_NONE, None, False, None, acc, None, None, None, None)
    return acc


# ---------------------------------------------------------------------------------------------------------------
# a19  proposal losses
# ---------------------------------------------------------------------------------------------------------------
class _InterlevelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w_prop: Tensor, s_bins_prop: Tensor, w_fine: Tensor, s_bins_fine: Tensor):
        N.require_cuda(w_prop, s_bins_prop, w_fine, s_bins_fine)
        w_prop, s_bins_prop = _f32c(w_prop), _f32c(s_bins_prop)
        w_fine, s_bins_fine = _f32c(w_fine.detach()), _f32c(s_bins_fine.detach())
        n, sp = w_prop.shape
        sf = w_fine.shape[1]
        per_ray = torch.empty((n,), device=w_prop.device, dtype=torch.float32)
        dw = torch.empty_like(w_prop)
        N.check(N.load().nsamd_interlevel_loss(N.ptr(s_bins_fine), N.ptr(w_fine), sf, N.ptr(s_bins_prop), N.ptr(w_prop),
                                               sp, n, 1.0 / (n * sf), N.ptr(per_ray), N.ptr(dw), N.stream()),
                "interlevel_loss")
        ctx.save_for_backward(dw)
        return per_ray.sum() / (n * sf)  # torch.mean over [N, S_fine]  (losses.py:128)

    @staticmethod
    def backward(ctx, g):
        (dw,) = ctx.saved_tensors
        return dw * g, None, None, None


def interlevel_loss(weights_list: Sequence[Tensor], s_bins_list: Sequence[Tensor]) -> Tensor:
    """losses.py:113-131 (weights `[N,S_i]`, spacing bins `[N,S_i+1]`, last entry = the nerf level, detached)."""
    total = None
    for w, b in zip(weights_list[:-1], s_bins_list[:-1]):
        term = _InterlevelFn.apply(w, b, weights_list[-1], s_bins_list[-1])
        total = term if total is None else total + term
    return total


class _DistortionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights: Tensor, s_bins: Tensor):
        N.require_cuda(weights, s_bins)
        weights, s_bins = _f32c(weights), _f32c(s_bins)
        n, s = weights.shape
        per_ray = torch.empty((n,), device=weights.device, dtype=torch.float32)
        dw = torch.empty_like(weights)
        N.check(N.load().nsamd_distortion_loss(N.ptr(s_bins), N.ptr(weights), s, n, 1.0 / n, N.ptr(per_ray), N.ptr(dw),
                                               N.stream()), "distortion_loss")
        ctx.save_for_backward(dw)
        return per_ray.sum() / n  # torch.mean over rays (losses.py:153)

    @staticmethod
    def backward(ctx, g):
        (dw,) = ctx.saved_tensors
        return dw * g, None


def distortion_loss(weights: Tensor, s_bins: Tensor) -> Tensor:
    """losses.py:149-154 on the final level."""
    return _DistortionFn.apply(weights, s_bins)


DEPTH_DS_NERF, DEPTH_URF = 1, 2  # DepthLossType values the kernel covers (losses.py:41-46)


def depth_loss_launch(weights: Sequence[Tensor], t_bins: Sequence[Tensor], termination_depth: Tensor,
                      directions_norm: Optional[Tensor], predicted_depth: Optional[Tensor], sigma: float, loss_type: int,
                      scale: float, per_ray: Optional[Tensor], d_weights: Optional[Sequence[Optional[Tensor]]],
                      d_predicted: Optional[Tensor], accumulate: bool = False) -> None:
    """nsamd_depth_loss on dense fp32 device tensors (weights `[n,S_l]`, bins `[n,S_l+1]`, per-ray vectors `[n]`)."""
    levels, n = len(weights), termination_depth.shape[0]
    parr = N.ptr_array
    counts = (C.c_int32 * levels)(*[int(w.shape[1]) for w in weights])
    N.check(N.load().nsamd_depth_loss(levels, parr(t_bins), parr(weights), counts, n, N.ptr(termination_depth),
                                      N.ptr(directions_norm), N.ptr(predicted_depth), float(sigma), int(loss_type),
                                      float(scale), 1 if accumulate else 0, N.ptr(per_ray),
                                      parr(d_weights) if d_weights is not None else None, N.ptr(d_predicted), N.stream()),
            "depth_loss")


class _DepthLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, levels: int, sigma: float, loss_type: int, termination_depth, directions_norm, predicted_depth, *rest):
        weights, t_bins = rest[:levels], rest[levels:]
        N.require_cuda(termination_depth, directions_norm, predicted_depth, *weights, *t_bins)
        ws = [_f32c(w) for w in weights]
        bins = [_f32c(b.detach()) for b in t_bins]
        n = ws[0].shape[0]
        td = _f32c(termination_depth.detach().reshape(-1))
        dn = None if directions_norm is None else _f32c(directions_norm.detach().reshape(-1))
        urf = loss_type == DEPTH_URF
        pred = _f32c(predicted_depth.reshape(-1)) if urf else None
        per_ray = torch.empty((levels, n), device=td.device, dtype=torch.float32)
        # a level whose weights take no gradient (the proposal levels of a step that does not update them) gets no buffer
        dws = [torch.empty_like(w) if ctx.needs_input_grad[6 + i] else None for i, w in enumerate(ws)]
        dpred = torch.empty_like(pred) if (urf and ctx.needs_input_grad[5]) else None
        scale = 1.0 / (n * levels) if n > 0 else 0.0
        depth_loss_launch(ws, bins, td, dn, pred, sigma, loss_type, scale, per_ray, dws, dpred)
        ctx.levels, ctx.pred_shape = levels, None if predicted_depth is None else predicted_depth.shape
        ctx.dws, ctx.dpred = dws, dpred
        return per_ray.sum() * scale  # mean over rays of every level, averaged over the levels (depth_nerfacto.py:94-104)

    @staticmethod
    def backward(ctx, g):
        dws = [None if d is None else d * g for d in ctx.dws]
        dpred = None if ctx.dpred is None else (ctx.dpred * g).reshape(ctx.pred_shape)
        return (None, None, None, None, None, dpred, *dws, *([None] * ctx.levels))


def depth_loss(weights_list: Sequence[Tensor], t_bins_list: Sequence[Tensor], termination_depth: Tensor,
               predicted_depth: Optional[Tensor], sigma, directions_norm: Optional[Tensor], is_euclidean: bool,
               loss_type: int) -> Tensor:
    """The depth loss of depth-nerfacto over every sampling level, already averaged over the levels
    (models/depth_nerfacto.py:94-104 over losses.py:289-325): weights `[n,S_l]`, Euclidean bin edges `[n,S_l+1]`,
    termination_depth / predicted_depth / directions_norm `[n]` or `[n,1]`, loss_type 1 (DS_NERF) or 2 (URF). 0-dim."""
    loss_type = int(getattr(loss_type, "value", loss_type))
    if loss_type not in (DEPTH_DS_NERF, DEPTH_URF):
        raise NotImplementedError("Provided depth loss type not implemented.")  # losses.py:325
    if loss_type == DEPTH_URF and predicted_depth is None:
        raise ValueError("the URF depth loss needs predicted_depth")
    if not is_euclidean and directions_norm is None:
        raise ValueError("a depth that is not Euclidean needs directions_norm")
    levels = len(weights_list)
    return _DepthLossFn.apply(levels, float(sigma), loss_type, termination_depth, None if is_euclidean else directions_norm,
                              predicted_depth, *weights_list, *t_bins_list)


# ---------------------------------------------------------------------------------------------------------------
# normals of the nerfacto field, forward only (eval render)       (fields/base_field.py:79-99, models/nerfacto.py:325-329)
# ---------------------------------------------------------------------------------------------------------------
def field_normals_launch(pts: N.Points, M: int, transform: int, box: N.Aabb, table: Tensor, grid: HashGridSpec, enc: Tensor,
                         base_params: Sequence[Tensor], normals: Optional[Tensor], gradient: Optional[Tensor],
                         geo: Optional[Tensor], geo_stride: int = 15, geo_offset: int = 0) -> None:
    """nsamd_field_normals on dense fp32 device tensors, on the current stream: `enc` the feature-major `[32, M]` features the
    hash forward left, base_params = (W0, b0, W1, b1) of the base MLP; normals / gradient `[M,3]` and `geo` (rows of
    `geo_stride` floats, the 15 geometry features from column `geo_offset`) are each optional."""
    if tuple(enc.shape) != (32, M) or tuple(table.shape) != (grid.num_levels * grid.table_size, 2):
        raise ValueError(f"field_normals: enc {tuple(enc.shape)} / table {tuple(table.shape)} do not fit M = {M} and the grid")
    W0, b0, W1, b1 = base_params
    if tuple(W0.shape) != (64, 32) or tuple(W1.shape) != (16, 64) or b0.numel() != 64 or b1.numel() != 16:
        raise ValueError("field_normals: the base MLP must be 32 -> 64 -> 16")
    for t_ in (normals, gradient):
        if t_ is not None and t_.numel() != 3 * M:
            raise ValueError("field_normals: normals / gradient must hold [M, 3]")
    if geo is not None and (geo_offset < 0 or geo_stride < geo_offset + 15 or geo.numel() < M * geo_stride):
        raise ValueError("field_normals: geo rows do not hold 15 columns from geo_offset for M samples")
    N.check(N.load().nsamd_field_normals(pts, M, transform, box, N.ptr(table), grid.native(), N.ptr(enc), N.ptr(W0), N.ptr(b0),
                                         N.ptr(W1), N.ptr(b1), N.ptr(normals), N.ptr(gradient), N.ptr(geo), int(geo_stride),
                                         int(geo_offset), N.stream()), "field_normals")


def field_normals(spec: PointSpec, table: Tensor, grid: HashGridSpec, transform: int, aabb, enc: Tensor,
                  base_params: Sequence[Tensor], want_gradient: bool = False):
    """Analytic normals of the points of `spec` from their hash features `enc` (`[32, M]`, feature-major) and the base MLP
    (W0, b0, W1, b1) -> (normals `[M,3]` = -normalize(d pre-activation / d normalised position), the raw gradient `[M,3]` or
    None, the geometry features `[M,15]`). No gradient flows through it: the normals are constants, as in the reference."""
    N.require_cuda(table, enc, *base_params, *spec.tensors())
    spec = _spec_from_flat(*(None if t is None else t.detach() for t in spec.tensors()))
    M = spec.num_points
    new = lambda *s: torch.empty(s, device=table.device, dtype=torch.float32)  # noqa: E731
    normals, grad, geo = new(M, 3), (new(M, 3) if want_gradient else None), new(M, 15)
    box = aabb if isinstance(aabb, N.Aabb) else N.make_aabb(aabb)
    field_normals_launch(spec.native(), M, transform, box, table.detach(), grid, _f32c(enc.detach()),
                         [_f32c(p.detach()) for p in base_params], normals, grad, geo)
    return normals, grad, geo


def normals_composite_launch(weights: Tensor, normals: Optional[Tensor], pred_pre: Optional[Tensor],
                             normals_out: Optional[Tensor], pred_out: Optional[Tensor]) -> None:
    """nsamd_normals_composite on dense fp32 device tensors (weights `[n,S]`, per-sample `[n*S,3]`, outputs `[n,3]`)."""
    n, S = weights.shape
    N.check(N.load().nsamd_normals_composite(N.ptr(weights), N.ptr(normals), N.ptr(pred_pre), n, S, N.ptr(normals_out),
                                             N.ptr(pred_out), N.stream()), "normals_composite")


def normals_composite(weights: Tensor, normals: Tensor, pred_pre: Tensor) -> Tuple[Tensor, Tensor]:
    """Rendered and shaded normals of both channels (NormalsRenderer + NormalsShader over the analytic normals and over
    PredNormalsFieldHead of `pred_pre`, the head's pre-activation): weights `[n,S]` or `[n,S,1]`, per-sample `[n,S,3]` ->
    two `[n,3]` images in [0, 1]."""
    N.require_cuda(weights, normals, pred_pre)
    w = _f32c(weights.detach().reshape(weights.shape[0], -1))
    n, S = w.shape
    nr, pp = _f32c(normals.detach().reshape(n * S, 3)), _f32c(pred_pre.detach().reshape(n * S, 3))
    out_n, out_p = torch.empty((n, 3), device=w.device, dtype=torch.float32), torch.empty((n, 3), device=w.device,
                                                                                            dtype=torch.float32)
    normals_composite_launch(w, nr, pp, out_n, out_p)
    return out_n, out_p


def normals_losses_launch(weights: Tensor, normals: Tensor, pred_pre: Optional[Tensor], directions: Optional[Tensor],
                          orientation_scale: float, pred_scale: float, orientation_per_ray: Optional[Tensor],
                          pred_per_ray: Optional[Tensor], d_pred_pre: Optional[Tensor], d_directions: Optional[Tensor],
                          accumulate_directions: bool = False) -> None:
    """nsamd_normals_losses on dense fp32 device tensors, on the current stream (weights `[n,S]`, per-sample `[n*S,3]`, directions
    and `d_directions` `[n,3]`, per-ray terms `[n]`); every output is optional."""
    n, S = weights.shape
    N.check(N.load().nsamd_normals_losses(N.ptr(weights), N.ptr(normals), N.ptr(pred_pre), N.ptr(directions), n, S,
                                          float(orientation_scale), float(pred_scale), N.ptr(orientation_per_ray),
                                          N.ptr(pred_per_ray), N.ptr(d_pred_pre), N.ptr(d_directions),
                                          1 if accumulate_directions else 0, N.stream()), "normals_losses")


class _NormalsLossesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights: Tensor, normals: Tensor, pred_pre: Tensor, directions: Tensor):
        N.require_cuda(weights, normals, pred_pre, directions)
        w = _f32c(weights.detach().reshape(weights.shape[0], -1))
        n, S = w.shape
        nr, pp = _f32c(normals.detach().reshape(n * S, 3)), _f32c(pred_pre.detach().reshape(n * S, 3))
        v = _f32c(directions.detach().reshape(n, 3))
        new = lambda *shape: torch.empty(shape, device=w.device, dtype=torch.float32)  # noqa: E731
        orientation, pred = new(n), new(n)
        d_pre = new(n * S, 3) if ctx.needs_input_grad[2] else None
        d_dir = new(n, 3) if ctx.needs_input_grad[3] else None
        normals_losses_launch(w, nr, pp, v, 1.0, 1.0, orientation, pred, d_pre, d_dir)
        ctx.save_for_backward(*(t for t in (d_pre, d_dir) if t is not None))
        ctx.have = (d_pre is not None, d_dir is not None)
        ctx.shapes = (pred_pre.shape, directions.shape)
        return orientation, pred

    @staticmethod
    def backward(ctx, g_orientation: Tensor, g_pred: Tensor):
        saved = list(ctx.saved_tensors)
        d_pre = saved.pop(0) if ctx.have[0] else None
        d_dir = saved.pop(0) if ctx.have[1] else None
        n = g_pred.shape[0]
        if d_pre is not None:  # the kernel left d term / d x of every sample: times the ray's upstream gradient
            d_pre = (d_pre.view(n, -1, 3) * g_pred.reshape(n, 1, 1)).reshape(ctx.shapes[0])
        if d_dir is not None:
            d_dir = (d_dir * g_orientation.reshape(n, 1)).reshape(ctx.shapes[1])
        return None, None, d_pre, d_dir


def normals_losses(weights: Tensor, normals: Tensor, pred_pre: Tensor, directions: Tensor) -> Tuple[Tensor, Tensor]:
    """The two per-ray normals loss terms of a `predict_normals` model (models/nerfacto.py:335-344 over losses.py:201-222):
    (orientation_loss(weights, normals, directions), pred_normal_loss(weights, normals, normalize(tanh(pred_pre)))), each `[n]`,
    from weights `[n,S]` or `[n,S,1]`, per-sample analytic normals and the predicted-normals head's PRE-activation `[n,S,3]` and
    the rays' view directions `[n,3]`. Weights and normals are constants, as the reference detaches them; gradient flows to
    `pred_pre` and to `directions`."""
    return _NormalsLossesFn.apply(weights, normals, pred_pre, directions)


# ---------------------------------------------------------------------------------------------------------------
# a3  camera-pose corrections of the rays
# ---------------------------------------------------------------------------------------------------------------
CAMERA_MODES = {"SO3xR3": 1, "SE3": 2}


def camera_apply_launch(pose: Tensor, mode: int, raw_origins: Tensor, raw_directions: Tensor, cams: Tensor, origins: Tensor,
                        directions: Tensor) -> None:
    """nsamd_camera_apply on the current stream: origins + t(c), R(c) directions of the `[n, 3]` raw rays for the camera c =
    `cams[ray]` (int64) under the pose corrections `pose` `[num_cameras, 6]`, `mode` a CAMERA_MODES value."""
    N.check(N.load().nsamd_camera_apply(N.ptr(pose), mode, pose.shape[0], N.ptr(raw_origins), N.ptr(raw_directions), N.ptr(cams),
                                        raw_origins.shape[0], N.ptr(origins), N.ptr(directions), N.stream()), "camera_apply")


def camera_backward_launch(pose: Tensor, mode: int, raw_directions: Tensor, cams: Tensor, d_origins: Sequence[Tensor],
                           d_directions: Sequence[Tensor], trans_penalty: float, rot_penalty: float, dpose: Tensor,
                           reg_out: Optional[Tensor]) -> None:
    """nsamd_camera_backward on the current stream: the per-ray gradients dL/d(origins, directions) of up to four sampling
    levels (one `[n, 3]` pair per level) summed per camera and taken through the exponential map into `dpose`, plus the
    gradient of the L2 pose regulariser with the two penalties, whose value goes to `reg_out` (None: not wanted)."""
    up = N.RayGrads()
    for k, (go, gd) in enumerate(zip(d_origins, d_directions)):
        up.d_origins[k], up.d_directions[k] = N.ptr(go), N.ptr(gd)
    up.count = len(d_origins)
    N.check(N.load().nsamd_camera_backward(N.ptr(pose), mode, pose.shape[0], N.ptr(raw_directions), N.ptr(cams),
                                           raw_directions.shape[0], up, trans_penalty, rot_penalty, N.ptr(dpose), N.ptr(reg_out),
                                           N.stream()), "camera_backward")


class _CameraRaysFn(torch.autograd.Function):
    """CameraOptimizer.apply_to_raybundle (cameras/camera_optimizers.py:148-153) on the pose parameter: one launch forward
    (nsamd_camera_apply), one launch backward (nsamd_camera_backward: per-camera sums of dL/d(origins, directions) in double
    in a fixed order, then the exponential map's closed-form backward) instead of the index / exp-map / bmm chain of torch
    kernels and their autograd nodes. The regulariser (:179-185) stays with the caller's loss dict."""

    @staticmethod
    def forward(ctx, pose: Tensor, origins: Tensor, directions: Tensor, cams: Tensor, mode: int):
        N.require_cuda(pose, origins, directions, cams)
        raw_o, raw_d = _f32c(origins.reshape(-1, 3)), _f32c(directions.reshape(-1, 3))
        idx = cams.reshape(-1).contiguous().to(torch.int64)
        p = _f32c(pose)
        o, d = torch.empty_like(raw_o), torch.empty_like(raw_d)
        camera_apply_launch(p, mode, raw_o, raw_d, idx, o, d)
        ctx.save_for_backward(p, raw_d, idx)
        ctx.mode = mode
        ctx.pose_param = pose
        return o.reshape(origins.shape), d.reshape(directions.shape)

    @staticmethod
    def backward(ctx, g_o: Optional[Tensor], g_d: Optional[Tensor]):
        p, raw_d, idx = ctx.saved_tensors
        g_o = torch.zeros_like(raw_d) if g_o is None else _f32c(g_o.reshape(-1, 3))
        g_d = torch.zeros_like(raw_d) if g_d is None else _f32c(g_d.reshape(-1, 3))
        buf, ret = _grad_target(ctx.pose_param, True)
        camera_backward_launch(p, ctx.mode, raw_d, idx, [g_o], [g_d], 0.0, 0.0, buf, None)
        return ret, None, None, None, None


def camera_correct_rays(pose: Tensor, mode: str, origins: Tensor, directions: Tensor, camera_indices: Tensor):
    """origins + t(c), R(c) directions for the camera c of every ray; `pose` [num_cameras, 6] = (translation, rotation
    vector), mode "SO3xR3" / "SE3" (cameras/lie_groups.py:25-117). The rays themselves are treated as constants."""
    return _CameraRaysFn.apply(pose, origins, directions, camera_indices, CAMERA_MODES[mode])


def select_batch_launch(slot: Tensor, slots: int, pool_origins: Tensor, pool_directions: Tensor, pool_cameras: Tensor,
                        pool_target: Tensor, origins: Tensor, directions: Tensor, camera_indices: Tensor, target: Tensor) -> None:
    """nsamd_select_batch on the current stream: batch number `slot[0]` (a device value, so that a captured launch follows it) of
    a pool of `slots` batches of `origins.shape[0]` rays each into the four static buffers a schedule reads."""
    N.check(N.load().nsamd_select_batch(N.ptr(slot), slots, origins.shape[0], N.ptr(pool_origins), N.ptr(pool_directions),
                                        N.ptr(pool_cameras), N.ptr(pool_target), N.ptr(origins), N.ptr(directions),
                                        N.ptr(camera_indices), N.ptr(target), N.stream()), "select_batch")


# ---------------------------------------------------------------------------------------------------------------
# a1  ray generation: pinhole, and perspective / fisheye / equirectangular lenses with distortion
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def raygen_pinhole(ray_indices: Tensor, c2w: Tensor, fx: Tensor, fy: Tensor, cx: Tensor, cy: Tensor):
    """RayGenerator.forward for perspective cameras (ray_generators.py:41-56; cameras.py:598-634, 781-787, 887-909).
    -> origins `[N,3]`, directions `[N,3]`, pixel_area `[N,1]`, directions_norm `[N,1]`."""
    N.require_cuda(ray_indices, c2w, fx, fy, cx, cy)
    idx = ray_indices.contiguous().to(torch.int64)
    c2w = _f32c(c2w.reshape(-1, 3, 4))
    fx, fy, cx, cy = (_f32c(t.reshape(-1)) for t in (fx, fy, cx, cy))
    n = idx.shape[0]
    dev = idx.device
    o = torch.empty((n, 3), device=dev, dtype=torch.float32)
    d = torch.empty((n, 3), device=dev, dtype=torch.float32)
    pa = torch.empty((n, 1), device=dev, dtype=torch.float32)
    dn = torch.empty((n, 1), device=dev, dtype=torch.float32)
    N.check(N.load().nsamd_raygen_pinhole(N.ptr(idx), N.ptr(c2w), N.ptr(fx), N.ptr(fy), N.ptr(cx), N.ptr(cy), n,
                                          c2w.shape[0], N.ptr(o), N.ptr(d), N.ptr(pa), N.ptr(dn), N.stream()),
            "raygen_pinhole")
    return o, d, pa, dn


def raygen_grid_launch(c2w: Tensor, fx: float, fy: float, cx: float, cy: float, lens, width: int, first: int, count: int, rows: int,
                       origins: Tensor, directions: Tensor) -> None:
    """nsamd_raygen_pinhole_grid (lens None) or nsamd_raygen_lens_grid (lens = (camera type 1 - 3, its six distortion parameters on
    the device or None)) on the current stream: the rays of pixels first .. first + count - 1 of ONE camera's row-major grid of
    width `width` into the first `rows` >= count rows of the eval loops' input buffers, rows count .. rows - 1 repeating the last
    pixel. c2w `[3, 4]` on the device, intrinsics by value."""
    lib = N.load()
    if lens is None:
        N.check(lib.nsamd_raygen_pinhole_grid(N.ptr(c2w), float(fx), float(fy), float(cx), float(cy), int(width), first, count, rows,
                                              N.ptr(origins), N.ptr(directions), None, N.stream()), "raygen_pinhole_grid")
    else:
        N.check(lib.nsamd_raygen_lens_grid(N.ptr(c2w), float(fx), float(fy), float(cx), float(cy), int(lens[0]), N.ptr(lens[1]),
                                           int(width), first, count, rows, N.ptr(origins), N.ptr(directions), None, N.stream()),
                "raygen_lens_grid")


LENS_TYPES = {1: "PERSPECTIVE", 2: "FISHEYE", 3: "EQUIRECTANGULAR"}  # CameraType values the lens generator covers
_CAMERA_TYPE_NAMES = {**LENS_TYPES, 4: "OMNIDIRECTIONALSTEREO_L", 5: "OMNIDIRECTIONALSTEREO_R", 6: "VR180_L", 7: "VR180_R",
                      8: "ORTHOPHOTO", 9: "FISHEYE624"}  # cameras/cameras.py:41-52


def check_lens_types(camera_type: Tensor) -> None:
    """ValueError naming the first camera type outside PERSPECTIVE / FISHEYE / EQUIRECTANGULAR (the kernels are not launched
    for one: the indexed entry point cannot read device memory on the host, so this layer checks)."""
    for t in torch.unique(camera_type.detach().reshape(-1).cpu()).tolist():
        if int(t) not in LENS_TYPES:
            raise ValueError(f"the hip ray generator does not cover camera type {int(t)} "
                             f"({_CAMERA_TYPE_NAMES.get(int(t), 'unknown')}); it handles {sorted(LENS_TYPES.values())}")


@torch.no_grad()
def raygen_lens(ray_indices: Tensor, c2w: Tensor, fx: Tensor, fy: Tensor, cx: Tensor, cy: Tensor, camera_type: Tensor,
                distortion: Optional[Tensor] = None, check_types: bool = True):
    """RayGenerator.forward for perspective, fisheye and equirectangular cameras with per-camera distortion parameters
    `[C,6] = (k1, k2, k3, k4, p1, p2)` (cameras.py:598-656, 781-817, 887-909; camera_utils.py:375-478); `camera_type` `[C]`
    holds CameraType values 1 - 3 and may mix them. -> origins `[N,3]`, directions `[N,3]`, pixel_area `[N,1]`,
    directions_norm `[N,1]`. check_types=False: the caller has run `check_lens_types` on these cameras already (it reads the
    types back to the host)."""
    N.require_cuda(ray_indices, c2w, fx, fy, cx, cy, camera_type)
    if check_types:
        check_lens_types(camera_type)
    idx = ray_indices.contiguous().to(torch.int64)
    c2w = _f32c(c2w.reshape(-1, 3, 4))
    fx, fy, cx, cy = (_f32c(t.reshape(-1)) for t in (fx, fy, cx, cy))
    ctype = camera_type.reshape(-1).to(torch.int32).contiguous()
    num_cameras = c2w.shape[0]
    if not (fx.numel() == fy.numel() == cx.numel() == cy.numel() == ctype.numel() == num_cameras):
        raise ValueError("raygen_lens: c2w, fx, fy, cx, cy and camera_type must describe the same number of cameras")
    if distortion is not None:
        N.require_cuda(distortion)
        distortion = _f32c(distortion.reshape(-1, 6))
        if distortion.shape[0] != num_cameras:
            raise ValueError("raygen_lens: distortion must be [num_cameras, 6]")
    n = idx.shape[0]
    dev = idx.device
    o = torch.empty((n, 3), device=dev, dtype=torch.float32)
    d = torch.empty((n, 3), device=dev, dtype=torch.float32)
    pa = torch.empty((n, 1), device=dev, dtype=torch.float32)
    dn = torch.empty((n, 1), device=dev, dtype=torch.float32)
    N.check(N.load().nsamd_raygen_lens(N.ptr(idx), N.ptr(c2w), N.ptr(fx), N.ptr(fy), N.ptr(cx), N.ptr(cy), N.ptr(ctype),
                                       N.ptr(distortion) if distortion is not None else None, n, num_cameras, N.ptr(o),
                                       N.ptr(d), N.ptr(pa), N.ptr(dn), N.stream()), "raygen_lens")
    return o, d, pa, dn


@torch.no_grad()
def adam_hyper(step: int, lr: float, betas=(0.9, 0.999)) -> Tuple[float, float]:
    """(lr / (1 - b1^step), sqrt(1 - b2^step)) — the two step-dependent scalars of Adam, in double as torch/optim/adam.py
    evaluates them (step_size, bias_correction2_sqrt); they are rounded to fp32 once, when they reach the kernel."""
    return lr / (1.0 - betas[0] ** step), (1.0 - betas[1] ** step) ** 0.5


def adam_step(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step: int, lr: float,
              betas=(0.9, 0.999), eps: float = 1e-15, grad_scale: float = 1.0, hyper_dev: Optional[Tensor] = None) -> None:
    """torch.optim.Adam step over a flat fp32 arena (engine/optimizers.py:74-193; AdamOptimizerConfig eps=1e-15)."""
    N.require_cuda(params, grads, exp_avg, exp_avg_sq)
    N.check(N.load().nsamd_adam_step(N.ptr(params), N.ptr(grads), N.ptr(exp_avg), N.ptr(exp_avg_sq), params.numel(),
                                     float(lr), float(betas[0]), float(betas[1]), float(eps), int(step),
                                     float(grad_scale), N.ptr(hyper_dev), N.stream()), "adam_step")


# ---------------------------------------------------------------------------------------------------------------
# a21 / f4  packed-sample path of instant-ngp (csrc/packed.hip): occupancy-grid marching, packed transmittance scan with
# early termination, compaction, packed compositing            (ray_samplers.py:385-519, models/instant_ngp.py:172-217)
# ---------------------------------------------------------------------------------------------------------------
def _occgrid_native(binaries: Tensor, roi_aabb: Sequence[float], coarse: Optional[Tensor] = None) -> N.OccGrid:
    g = N.OccGrid()
    g.binaries = N.ptr(binaries)
    g.levels, g.resolution = int(binaries.shape[0]), int(binaries.shape[1])
    for i, v in enumerate(roi_aabb):
        g.aabb[i] = float(v)
    g.coarse = N.ptr(coarse) if coarse is not None and coarse.numel() else None
    return g


def occgrid_coarse_words(levels: int, resolution: int) -> int:
    """Words of the coarse (4x4x4-block) occupancy bitfield for a grid shape; 0 = the marcher takes none."""
    return int(N.load().nsamd_occgrid_coarse_words(int(levels), int(resolution)))


@torch.no_grad()
def occgrid_cell_positions(cells: Optional[Tensor], num: int, binaries: Tensor, roi_aabb: Sequence[float], jitter: Tensor) -> Tensor:
    """Positions `[num,3]` inside the grid cells `cells` (flat int64 indices; None = cells 0..num-1) at the fractional
    offsets `jitter [num,3]` (nsamd_occgrid_cell_positions)."""
    N.require_cuda(binaries, jitter, cells)
    x = torch.empty((num, 3), device=jitter.device, dtype=torch.float32)
    N.check(N.load().nsamd_occgrid_cell_positions(N.ptr(cells), num, _occgrid_native(binaries, roi_aabb), N.ptr(_f32c(jitter)),
                                                  N.ptr(x), N.stream()), "occgrid_cell_positions")
    return x


@torch.no_grad()
def occgrid_update(occs: Tensor, cells: Optional[Tensor], occ_new: Tensor, ema_decay: float, scratch: Tensor) -> None:
    """occs[c] = max(occs[c] * decay, new estimates of c) for the listed cells, in place (nsamd_occgrid_update)."""
    N.require_cuda(occs, occ_new, scratch, cells)
    assert scratch.numel() >= occs.numel() and occs.is_contiguous()
    N.check(N.load().nsamd_occgrid_update(N.ptr(occs), occs.numel(), N.ptr(cells), N.ptr(_f32c(occ_new.reshape(-1))),
                                          occ_new.numel(), float(ema_decay), N.ptr(scratch), N.stream()), "occgrid_update")


@torch.no_grad()
def occgrid_binarise(occs: Tensor, binaries: Tensor, coarse: Optional[Tensor], occ_thre: float, scratch: Tensor,
                     threshold_out: Optional[Tensor] = None) -> None:
    """binaries = occs > min(mean over the cells with occs >= 0, occ_thre) and its coarse bitfield (nsamd_occgrid_binarise).
    scratch: >= 1024 float64; threshold_out: optional `[2]` fp32 (threshold, mean)."""
    N.require_cuda(occs, binaries, scratch, coarse, threshold_out)
    assert scratch.dtype == torch.float64 and scratch.numel() >= 1024
    N.check(N.load().nsamd_occgrid_binarise(N.ptr(occs), int(binaries.shape[0]), int(binaries.shape[1]), float(occ_thre),
                                            N.ptr(binaries), N.ptr(coarse) if coarse is not None and coarse.numel() else None,
                                            N.ptr(scratch), N.ptr(threshold_out), N.stream()), "occgrid_binarise")


def packed_info_launch(counts: Tensor, n: int, info: Tensor, total: Tensor) -> None:
    """nsamd_packed_info on the current stream: `info` `[n, 2]` int64 (start, count) from per-ray `counts` `[n]` int32, their sum
    into the one-element int64 `total`. Here and below `n` is the number of rays: a schedule's buffers may be larger."""
    N.check(N.load().nsamd_packed_info(N.ptr(counts), n, N.ptr(info), N.ptr(total), N.stream()), "packed_info")


def occgrid_march_count_launch(origins: Tensor, directions: Tensor, t_min: Optional[Tensor], t_max: Optional[Tensor], n: int,
                               near: float, far: float, grid: N.OccGrid, step_size: float, cone_angle: float, jitter: Optional[Tensor],
                               counts: Tensor, stash: Optional[Tensor], stash_cap: int) -> None:
    """nsamd_occgrid_march_count_stash on the current stream: the count pass of the marcher over `[n, 3]` rays -> kept steps per
    ray in `counts`, the first `stash_cap` of them in `stash` `[n, stash_cap, 2]` (None / 0: nothing stashed)."""
    N.check(N.load().nsamd_occgrid_march_count_stash(N.ptr(origins), N.ptr(directions), N.ptr(t_min), N.ptr(t_max),
                                                     n, near, far, grid, step_size, cone_angle, N.ptr(jitter),
                                                     N.ptr(counts), N.ptr(stash), stash_cap, N.stream()),
            "occgrid_march_count_stash")


def occgrid_march_write_launch(origins: Tensor, directions: Tensor, t_min: Optional[Tensor], t_max: Optional[Tensor], n: int,
                               near: float, far: float, grid: N.OccGrid, step_size: float, cone_angle: float, jitter: Optional[Tensor],
                               info: Tensor, stash: Optional[Tensor], stash_cap: int, ray_indices: Tensor, t_starts: Tensor,
                               t_ends: Tensor) -> None:
    """nsamd_occgrid_march_write_stashed on the current stream: the write pass behind `occgrid_march_count_launch` and
    `packed_info_launch` — every ray's samples at its `info` offset of the packed outputs (sized for the total or larger)."""
    N.check(N.load().nsamd_occgrid_march_write_stashed(N.ptr(origins), N.ptr(directions), N.ptr(t_min), N.ptr(t_max),
                                                       n, near, far, grid, step_size, cone_angle, N.ptr(jitter),
                                                       N.ptr(info), N.ptr(stash), stash_cap, N.ptr(ray_indices), N.ptr(t_starts),
                                                       N.ptr(t_ends), N.stream()), "occgrid_march_write_stashed")


def packed_positions_launch(origins: Tensor, directions: Tensor, ray_indices: Tensor, t_starts: Tensor, t_ends: Tensor,
                            count: int, out: Tensor) -> None:
    """nsamd_packed_positions on the current stream: o[ray] + d[ray] (t_start + t_end) / 2 of the first `count` packed samples."""
    N.check(N.load().nsamd_packed_positions(N.ptr(origins), N.ptr(directions), N.ptr(ray_indices), N.ptr(t_starts), N.ptr(t_ends),
                                            count, N.ptr(out), N.stream()), "packed_positions")


def packed_visibility_launch(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Tensor, n: int, early_stop_eps: float,
                             alpha_thre: float, mask: Tensor, kept: Tensor) -> None:
    """nsamd_packed_visibility on the current stream: per packed sample of the `[n, 2]` rays of `packed_info` whether it is kept
    (uint8 `mask`), per ray how many are (int32 `kept`)."""
    N.check(N.load().nsamd_packed_visibility(N.ptr(t_starts), N.ptr(t_ends), N.ptr(sigmas), N.ptr(packed_info),
                                             n, early_stop_eps, alpha_thre, N.ptr(mask), N.ptr(kept),
                                             N.stream()), "packed_visibility")


def packed_compact_launch(mask: Tensor, packed_info: Tensor, kept_info: Tensor, n: int, t_starts: Tensor, t_ends: Tensor,
                          ray_indices_out: Tensor, t_starts_out: Tensor, t_ends_out: Tensor) -> None:
    """nsamd_packed_compact on the current stream: the samples `mask` keeps, moved to their `kept_info` offsets."""
    N.check(N.load().nsamd_packed_compact(N.ptr(mask), N.ptr(packed_info), N.ptr(kept_info), n, N.ptr(t_starts),
                                          N.ptr(t_ends), N.ptr(ray_indices_out), N.ptr(t_starts_out), N.ptr(t_ends_out),
                                          N.stream()), "packed_compact")


def packed_weights_launch(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Tensor, n: int, weights: Tensor) -> None:
    """nsamd_packed_weights_fwd on the current stream: rendering weights of the packed samples of the rays of `packed_info`."""
    N.check(N.load().nsamd_packed_weights_fwd(N.ptr(t_starts), N.ptr(t_ends), N.ptr(sigmas), N.ptr(packed_info),
                                              n, N.ptr(weights), None, N.stream()), "packed_weights_fwd")


def packed_weights_backward_launch(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, dweights: Tensor, packed_info: Tensor,
                                   n: int, dsigmas: Tensor) -> None:
    """nsamd_packed_weights_bwd on the current stream: the density gradient of `packed_weights_launch` from `dweights`."""
    N.check(N.load().nsamd_packed_weights_bwd(N.ptr(t_starts), N.ptr(t_ends), N.ptr(sigmas), N.ptr(dweights), N.ptr(packed_info),
                                              n, N.ptr(dsigmas), N.stream()), "packed_weights_bwd")


def packed_composite_launch(rgb: Tensor, weights: Tensor, t_starts: Optional[Tensor], t_ends: Optional[Tensor],
                            packed_info: Tensor, n: int, bg_mode: int, bg_vals, eval_mode: bool, out_rgb: Tensor, acc: Tensor,
                            depth: Optional[Tensor]) -> None:
    """nsamd_packed_composite_fwd on the current stream: colour `[n, 3]`, accumulation `[n]` and (with the sample intervals)
    expected depth `[n]` of the rays of `packed_info`; `bg_mode` / `bg_vals` as `_packed_bg` returns them."""
    N.check(N.load().nsamd_packed_composite_fwd(N.ptr(rgb), N.ptr(weights), N.ptr(t_starts), N.ptr(t_ends), N.ptr(packed_info),
                                                n, bg_mode, bg_vals, int(eval_mode), N.ptr(out_rgb),
                                                N.ptr(acc), N.ptr(depth), N.stream()), "packed_composite_fwd")


def packed_render_launch(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, rgb: Tensor, packed_info: Tensor, n: int, bg_mode: int,
                         bg_vals, eval_mode: bool, out_rgb: Tensor, acc: Tensor, depth: Tensor, mid_lo: Optional[Tensor],
                         mid_hi: Optional[Tensor]) -> None:
    """nsamd_packed_render_fwd (include/nsamd_render.h) on the current stream: `packed_weights_launch` followed by
    `packed_composite_launch` in one pass — the same bits, the weights never in memory — and (both or neither) the rays' minimum
    / maximum sample midpoint `mid_lo` / `mid_hi` `[n]`."""
    N.check(N.load().nsamd_packed_render_fwd(N.ptr(t_starts), N.ptr(t_ends), N.ptr(sigmas), N.ptr(rgb), N.ptr(packed_info), n,
                                             bg_mode, bg_vals, int(eval_mode), N.ptr(out_rgb), N.ptr(acc), N.ptr(depth),
                                             N.ptr(mid_lo), N.ptr(mid_hi), N.stream()), "packed_render_fwd")


def packed_ray_points_launch(origins: Tensor, directions: Tensor, ray_indices: Tensor, t_starts: Tensor, t_ends: Tensor,
                             count: int, positions: Tensor, sample_directions: Tensor) -> None:
    """nsamd_packed_ray_points (include/nsamd_render.h) on the current stream: `packed_positions_launch` of the first `count`
    packed samples and, beside the positions, each sample's row of `directions`."""
    N.check(N.load().nsamd_packed_ray_points(N.ptr(origins), N.ptr(directions), N.ptr(ray_indices), N.ptr(t_starts),
                                             N.ptr(t_ends), count, N.ptr(positions), N.ptr(sample_directions), N.stream()),
            "packed_ray_points")


def packed_composite_backward_launch(rgb: Tensor, weights: Tensor, ray_indices: Tensor, count: int, bg_mode: int, bg_vals,
                                     g_rgb: Tensor, g_acc: Optional[Tensor], d_rgb: Optional[Tensor], d_weights: Tensor) -> None:
    """nsamd_packed_composite_bwd on the current stream: gradients of the first `count` packed samples' colours (None: not
    wanted) and weights from the per-ray gradients of the composited colour and (None: none) the accumulation."""
    N.check(N.load().nsamd_packed_composite_bwd(N.ptr(rgb), N.ptr(weights), N.ptr(ray_indices), count, bg_mode, bg_vals,
                                                N.ptr(g_rgb), N.ptr(g_acc), N.ptr(d_rgb), N.ptr(d_weights), N.stream()),
            "packed_composite_bwd")


@torch.no_grad()
def packed_info_from_counts(counts: Tensor) -> Tuple[Tensor, int]:
    """nerfacc.pack_info from per-ray counts (int32 `[N]`) -> (`[N,2]` int64 (start, count), total). The total is read
    back to the host (the packed arrays are allocated to size, as nerfacc does)."""
    N.require_cuda(counts)
    n = counts.shape[0]
    info = torch.empty((n, 2), device=counts.device, dtype=torch.int64)
    total = torch.zeros((1,), device=counts.device, dtype=torch.int64)
    packed_info_launch(counts, n, info, total)
    return info, int(total.item())


@torch.no_grad()
def occgrid_march(origins: Tensor, directions: Tensor, binaries: Tensor, roi_aabb: Sequence[float], step_size: float,
                  near_plane: float = 0.0, far_plane: float = 1e10, t_min: Optional[Tensor] = None,
                  t_max: Optional[Tensor] = None, cone_angle: float = 0.0, jitter: Optional[Tensor] = None,
                  coarse: Optional[Tensor] = None, stash_cap: int = 128):
    """Ray marching through a multi-level occupancy grid (`binaries [levels,R,R,R]` uint8) -> (ray_indices int64 `[n]`,
    t_starts, t_ends fp32 `[n]`, packed_info `[N,2]`). Count pass, prefix, write pass. `coarse`: the grid's 4x4x4-block
    bitfield (occgrid_binarise) — empty-space skipping, same samples. `stash_cap` > 0: the count pass leaves every ray's first
    `stash_cap` kept steps in a scratch and the write pass copies them (a ray is marched once; same values), 0: march twice."""
    N.require_cuda(origins, directions, binaries)
    o, d = _f32c(origins), _f32c(directions)
    assert binaries.dtype == torch.uint8 and binaries.is_contiguous() and binaries.dim() == 4
    n = o.shape[0]
    dev = o.device
    grid = _occgrid_native(binaries, roi_aabb, coarse)
    tmin = None if t_min is None else _f32c(t_min.reshape(-1))
    tmax = None if t_max is None else _f32c(t_max.reshape(-1))
    jit = None if jitter is None else _f32c(jitter.reshape(-1))
    counts = torch.empty((n,), device=dev, dtype=torch.int32)
    march = (o, d, tmin, tmax, n, float(near_plane), min(float(far_plane), 3.0e38), grid, float(step_size), float(cone_angle), jit)
    stash = torch.empty((n, int(stash_cap), 2), device=dev, dtype=torch.float32) if stash_cap > 0 else None
    occgrid_march_count_launch(*march, counts, stash, int(stash_cap))
    info, total = packed_info_from_counts(counts)
    ray_indices = torch.empty((total,), device=dev, dtype=torch.int64)
    t_starts = torch.empty((total,), device=dev, dtype=torch.float32)
    t_ends = torch.empty((total,), device=dev, dtype=torch.float32)
    if total:
        occgrid_march_write_launch(*march, info, stash, int(stash_cap), ray_indices, t_starts, t_ends)
    return ray_indices, t_starts, t_ends, info


@torch.no_grad()
def packed_positions(origins: Tensor, directions: Tensor, ray_indices: Tensor, t_starts: Tensor, t_ends: Tensor) -> Tensor:
    """o[ray] + d[ray] (t_start + t_end) / 2 for packed samples -> `[n,3]`."""
    N.require_cuda(origins, directions, ray_indices, t_starts, t_ends)
    out = torch.empty((ray_indices.shape[0], 3), device=origins.device, dtype=torch.float32)
    packed_positions_launch(_f32c(origins), _f32c(directions), ray_indices, t_starts, t_ends, ray_indices.shape[0], out)
    return out


@torch.no_grad()
def packed_visibility_compact(ray_indices: Tensor, t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Tensor,
                              early_stop_eps: float = 1e-4, alpha_thre: float = 0.0):
    """nerfacc.render_visibility_from_density + masking (OccGridEstimator.sampling): keep the samples whose transmittance
    is still >= early_stop_eps and whose alpha reaches alpha_thre -> (ray_indices, t_starts, t_ends, packed_info, mask)."""
    N.require_cuda(ray_indices, t_starts, t_ends, sigmas, packed_info)
    n_rays = packed_info.shape[0]
    dev = t_starts.device
    mask = torch.empty((t_starts.shape[0],), device=dev, dtype=torch.uint8)
    kept = torch.empty((n_rays,), device=dev, dtype=torch.int32)
    packed_visibility_launch(t_starts, t_ends, _f32c(sigmas), packed_info, n_rays, float(early_stop_eps), float(alpha_thre), mask,
                             kept)
    info2, total = packed_info_from_counts(kept)
    ri = torch.empty((total,), device=dev, dtype=torch.int64)
    ts = torch.empty((total,), device=dev, dtype=torch.float32)
    te = torch.empty((total,), device=dev, dtype=torch.float32)
    if total:
        packed_compact_launch(mask, packed_info, info2, n_rays, t_starts, t_ends, ri, ts, te)
    return ri, ts, te, info2, mask


class _PackedWeightsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sigmas: Tensor, t_starts: Tensor, t_ends: Tensor, packed_info: Tensor):
        N.require_cuda(sigmas, t_starts, t_ends, packed_info)
        sigmas = _f32c(sigmas)
        w = torch.empty_like(sigmas)
        packed_weights_launch(t_starts, t_ends, sigmas, packed_info, packed_info.shape[0], w)
        ctx.save_for_backward(sigmas, t_starts, t_ends, packed_info)
        return w

    @staticmethod
    def backward(ctx, gw: Tensor):
        sigmas, t_starts, t_ends, info = ctx.saved_tensors
        ds = torch.empty_like(sigmas)
        packed_weights_backward_launch(t_starts, t_ends, sigmas, _f32c(gw), info, info.shape[0], ds)
        return ds, None, None, None


def packed_weights(sigmas: Tensor, t_starts: Tensor, t_ends: Tensor, packed_info: Tensor) -> Tensor:
    """nerfacc.render_weight_from_density(...)[0] on packed samples `[n]` (differentiable w.r.t. sigmas)."""
    return _PackedWeightsFn.apply(sigmas, t_starts, t_ends, packed_info)


def _packed_bg(background) -> Tuple[int, Optional[object]]:
    if isinstance(background, str):
        if background == "last_sample":
            raise NotImplementedError("Background color 'last_sample' not implemented for packed samples.")  # renderers.py:95-96
        if background == "random":
            return 0, None
        vals = {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}[background]
    else:
        vals = tuple(float(v) for v in background.reshape(-1)[:3].tolist())
    return 1, (C.c_float * 3)(*vals)


class _PackedCompositeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb: Tensor, weights: Tensor, ray_indices: Tensor, packed_info: Tensor, t_starts, t_ends, bg_mode: int,
                bg_vals, eval_mode: bool):
        N.require_cuda(rgb, weights, ray_indices, packed_info)
        rgb, weights = _f32c(rgb), _f32c(weights)
        n_rays = packed_info.shape[0]
        dev = rgb.device
        out = torch.empty((n_rays, 3), device=dev, dtype=torch.float32)
        acc = torch.empty((n_rays,), device=dev, dtype=torch.float32)
        depth = torch.empty((n_rays,), device=dev, dtype=torch.float32) if t_starts is not None else None
        packed_composite_launch(rgb, weights, t_starts, t_ends, packed_info, n_rays, bg_mode, bg_vals, eval_mode, out, acc, depth)
        ctx.save_for_backward(rgb, weights, ray_indices)
        ctx.bg = (bg_mode, bg_vals)
        ctx.mark_non_differentiable(*([depth] if depth is not None else []))
        return out, acc, depth

    @staticmethod
    def backward(ctx, g_rgb, g_acc, _g_depth):
        rgb, weights, ray_indices = ctx.saved_tensors
        n = weights.shape[0]
        d_rgb = torch.empty_like(rgb) if ctx.needs_input_grad[0] else None
        d_w = torch.empty_like(weights)
        g_rgb = _f32c(g_rgb) if g_rgb is not None else torch.zeros((int(ray_indices.max()) + 1 if n else 0, 3), device=rgb.device)
        packed_composite_backward_launch(rgb, weights, ray_indices, n, ctx.bg[0], ctx.bg[1], g_rgb, _f32c(g_acc), d_rgb, d_w)
        return d_rgb, d_w, None, None, None, None, None, None, None


def packed_composite(rgb: Tensor, weights: Tensor, ray_indices: Tensor, packed_info: Tensor, t_starts: Optional[Tensor] = None,
                     t_ends: Optional[Tensor] = None, background="random", eval_mode: bool = False):
    """accumulate_along_rays compositing of packed samples -> (rgb `[N,3]`, accumulation `[N]`, depth `[N]` or None)."""
    mode, vals = _packed_bg(background)
    return _PackedCompositeFn.apply(rgb, weights, ray_indices, packed_info, t_starts, t_ends, mode, vals, bool(eval_mode))


# ---------------------------------------------------------------------------------------------------------------
# mesh export: TSDF fusion (exporter/tsdf_utils.py:172-274)
# ---------------------------------------------------------------------------------------------------------------
def tsdf_integrate_launch(origin: Sequence[float], voxel_size: Sequence[float], truncation: float, values: Tensor, weights: Tensor,
                          colors: Optional[Tensor], w2c: Tensor, K: Tensor, depth: Tensor, color: Optional[Tensor]) -> None:
    """nsamd_tsdf_integrate (include/nsamd_export.h) on dense fp32 device tensors: values / weights `[X,Y,Z]` and colors `[X,Y,Z,3]` updated in place by
    the B views w2c `[B,3,4]`, K `[B,2,3]`, depth `[B,H,W]`, color `[B,H,W,3]` (or None: colours untouched). origin, voxel_size:
    three host floats each."""
    N.require_cuda(values, weights, colors, w2c, K, depth, color)
    vol = N.TsdfVolume()
    for i in range(3):
        vol.origin[i], vol.voxel_size[i], vol.dims[i] = float(origin[i]), float(voxel_size[i]), int(values.shape[i])
    vol.truncation = float(truncation)
    B, H, W = (int(s) for s in depth.shape)
    N.check(N.load().nsamd_tsdf_integrate(vol, N.ptr(values), N.ptr(weights), N.ptr(colors), N.ptr(w2c), N.ptr(K), B,
                                          N.ptr(depth), N.ptr(color), H, W, N.stream()), "tsdf_integrate")


# ---------------------------------------------------------------------------------------------------------------
# point-cloud export: ordered selection and the outlier rule's neighbour search (include/nsamd_pointcloud.h)
# ---------------------------------------------------------------------------------------------------------------
def points_select_launch(origins: Tensor, directions: Tensor, depth: Tensor, rgb: Tensor, alpha: Optional[Tensor],
                         normals01: Optional[Tensor], box: "N.CropBox", out_points: Tensor, out_colors: Tensor,
                         out_view_dirs: Tensor, out_normals: Optional[Tensor], cursor: Tensor, scratch: Tensor) -> None:
    """nsamd_points_select on dense device tensors: the rays kept of origins / directions / rgb `[n,3]`, depth / alpha `[n]`
    (alpha None: every ray passes the opacity test), normals01 `[n,3]` or None, appended in ray order at row cursor[0] of the
    `[cap,3]` outputs; cursor `[2]` int64 (rows so far, overflow flag), scratch: int64, `N.select_scratch_words(n)` words."""
    N.require_cuda(origins, directions, depth, rgb, alpha, normals01, out_points, out_colors, out_view_dirs, out_normals, cursor,
                   scratch)
    n = int(depth.numel())
    assert origins.numel() == directions.numel() == rgb.numel() == 3 * n and (alpha is None or alpha.numel() == n)
    assert (normals01 is None) == (out_normals is None) and (normals01 is None or normals01.numel() == 3 * n)
    assert cursor.dtype == scratch.dtype == torch.int64 and cursor.numel() >= 2 and scratch.numel() >= N.select_scratch_words(n)
    cap = int(out_points.shape[0])
    assert tuple(out_colors.shape) == tuple(out_view_dirs.shape) == (cap, 3) and (out_normals is None or out_normals.shape[0] == cap)
    N.check(N.load().nsamd_points_select(N.ptr(origins), N.ptr(directions), N.ptr(depth), N.ptr(rgb), N.ptr(alpha),
                                         N.ptr(normals01), n, box, N.ptr(out_points), N.ptr(out_colors), N.ptr(out_view_dirs),
                                         N.ptr(out_normals), cap, N.ptr(cursor), N.ptr(scratch), N.stream()), "points_select")


def select_below_launch(avg: Tensor, threshold: Tensor, out_indices: Tensor, count: Tensor, scratch: Tensor) -> None:
    """nsamd_select_below: out_indices `[n]` int64 receives, ascending, the i with 0 < avg[i] < threshold[0] (both float64 on the
    device), count `[1]` int64 their number."""
    N.require_cuda(avg, threshold, out_indices, count, scratch)
    n = int(avg.numel())
    assert avg.dtype == threshold.dtype == torch.float64 and out_indices.dtype == count.dtype == scratch.dtype == torch.int64
    assert out_indices.numel() >= n and scratch.numel() >= N.select_scratch_words(n)
    N.check(N.load().nsamd_select_below(N.ptr(avg), n, N.ptr(threshold), N.ptr(out_indices), N.ptr(count), N.ptr(scratch),
                                        N.stream()), "select_below")


def point_cell_keys_launch(points: Tensor, grid: "N.PointGrid", keys: Tensor) -> None:
    """nsamd_point_cell_keys: keys `[n]` int64, the grid cell of every row of points `[n,3]` fp32."""
    N.require_cuda(points, keys)
    n = int(points.shape[0])
    assert points.dtype == torch.float32 and keys.dtype == torch.int64 and keys.numel() >= n
    N.check(N.load().nsamd_point_cell_keys(N.ptr(points), n, grid, N.ptr(keys), N.stream()), "point_cell_keys")


def knn_mean_distance_launch(points: Tensor, order: Tensor, cell_start: Tensor, grid: "N.PointGrid", k: int, max_rings: int,
                             avg: Tensor, unfinished: Tensor) -> None:
    """nsamd_knn_mean_distance: avg `[n]` float64, the mean distance of every row of points `[n,3]` fp32 to its min(k, n) nearest
    rows (itself included). order `[n]` int32: the rows sorted by cell key; cell_start `[cells + 1]` int32; unfinished `[1 + n]`
    int32: word 0 receives the number of queries that fell to the brute-force phase."""
    if k > N.KNN_MAX_K:
        raise ValueError(f"knn_mean_distance: at most {N.KNN_MAX_K} neighbours are supported, got {k}")
    N.require_cuda(points, order, cell_start, avg, unfinished)
    n = int(points.shape[0])
    cells = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
    assert points.dtype == torch.float32 and avg.dtype == torch.float64 and avg.numel() >= n
    assert order.dtype == cell_start.dtype == unfinished.dtype == torch.int32
    assert order.numel() == n and cell_start.numel() == cells + 1 and unfinished.numel() >= n + 1
    N.check(N.load().nsamd_knn_mean_distance(N.ptr(points), n, N.ptr(order), N.ptr(cell_start), grid, int(k), int(max_rings),
                                             N.ptr(avg), N.ptr(unfinished), N.stream()), "knn_mean_distance")


# ---------------------------------------------------------------------------------------------------------------
# mesh export: marching cubes over the fused volume (include/nsamd_mesh.h)
# ---------------------------------------------------------------------------------------------------------------
def mesh_count_launch(vol: "N.MeshVolume", values: Tensor, scratch: Tensor, totals: Tensor) -> None:
    """nsamd_mesh_count: totals `[2]` int64 on the device receives the number of vertices and of triangles of the mesh of
    values `[X,Y,Z]` fp32; scratch: uint8, `N.mesh_scratch_bytes(values.numel())` bytes, kept for `mesh_emit_launch`."""
    N.require_cuda(values, scratch, totals)
    assert values.dtype == torch.float32 and tuple(values.shape) == tuple(vol.dims)
    assert totals.dtype == torch.int64 and totals.numel() >= 2
    assert scratch.dtype == torch.uint8 and scratch.numel() >= N.mesh_scratch_bytes(values.numel()) and scratch.data_ptr() % 8 == 0
    N.check(N.load().nsamd_mesh_count(vol, N.ptr(values), N.ptr(scratch), N.ptr(totals), N.stream()), "mesh_count")


def mesh_emit_launch(vol: "N.MeshVolume", values: Tensor, colors: Tensor, scratch: Tensor, vertices: Tensor, normals: Tensor,
                     vertex_colors: Tensor, faces: Tensor) -> None:
    """nsamd_mesh_emit after `mesh_count_launch` on the same volume and scratch: vertices, normals, vertex_colors `[V,3]` fp32
    and faces `[T,3]` int32, V and T the totals the count gave; colors `[X,Y,Z,3]` fp32."""
    N.require_cuda(values, colors, scratch, vertices, normals, vertex_colors, faces)
    V, T = int(vertices.shape[0]), int(faces.shape[0])
    assert values.dtype == colors.dtype == torch.float32 and tuple(colors.shape) == (*vol.dims, 3) == (*values.shape, 3)
    assert vertices.dtype == normals.dtype == vertex_colors.dtype == torch.float32 and faces.dtype == torch.int32
    assert tuple(vertices.shape) == tuple(normals.shape) == tuple(vertex_colors.shape) == (V, 3) and tuple(faces.shape) == (T, 3)
    assert scratch.dtype == torch.uint8 and scratch.numel() >= N.mesh_scratch_bytes(values.numel())
    N.check(N.load().nsamd_mesh_emit(vol, N.ptr(values), N.ptr(colors), N.ptr(scratch), V, T, N.ptr(vertices), N.ptr(normals),
                                     N.ptr(vertex_colors), N.ptr(faces), N.stream()), "mesh_emit")


# ---------------------------------------------------------------------------------------------------------------
# mesh export: one ray per texel of the texture atlas, the ray length, the 8-bit image (include/nsamd_texture.h)
# ---------------------------------------------------------------------------------------------------------------
def texel_rays_launch(atlas: "N.TexelAtlasPod", vertices: Tensor, normals: Tensor, faces: Tensor, raylen_dev: Tensor, first: int,
                      count: int, rows: int, origins: Tensor, directions: Tensor, nears: Tensor, fars: Tensor) -> None:
    """nsamd_texel_rays on the current stream: the rays of texels first .. first + count - 1 of the atlas' row-major grid into the
    first `rows` >= count rows of the eval loop's input buffers (origins, directions `[n,3]`, nears, fars `[n]`), rows count ..
    rows - 1 repeating the last texel. vertices, normals `[V,3]` fp32, faces `[F,3]` int32, raylen_dev `[1]` fp32."""
    N.require_cuda(vertices, normals, faces, raylen_dev, origins, directions, nears, fars)
    V = int(vertices.shape[0])
    assert vertices.dtype == normals.dtype == raylen_dev.dtype == torch.float32 and faces.dtype == torch.int32
    assert tuple(normals.shape) == (V, 3) == tuple(vertices.shape) and tuple(faces.shape) == (atlas.faces, 3) and raylen_dev.numel() >= 1
    assert origins.dtype == directions.dtype == nears.dtype == fars.dtype == torch.float32
    assert origins.shape[0] >= rows and directions.shape[0] >= rows and nears.numel() >= rows and fars.numel() >= rows
    N.check(N.load().nsamd_texel_rays(atlas, N.ptr(vertices), N.ptr(normals), N.ptr(faces), V, N.ptr(raylen_dev), int(first),
                                      int(count), int(rows), N.ptr(origins), N.ptr(directions), N.ptr(nears), N.ptr(fars),
                                      N.stream()), "texel_rays")


def mesh_raylen_launch(vertices: Tensor, faces: Tensor, scratch: Tensor, raylen_dev: Tensor) -> None:
    """nsamd_mesh_raylen: raylen_dev `[1]` fp32 receives twice the mean length of the faces' first edge (vertices `[V,3]` fp32, faces
    `[T,3]` int32, T >= 1); scratch: uint8, `N.RAYLEN_SCRATCH_BYTES` bytes."""
    N.require_cuda(vertices, faces, scratch, raylen_dev)
    assert vertices.dtype == raylen_dev.dtype == torch.float32 and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3
    assert scratch.dtype == torch.uint8 and scratch.numel() >= N.RAYLEN_SCRATCH_BYTES and scratch.data_ptr() % 8 == 0
    N.check(N.load().nsamd_mesh_raylen(N.ptr(vertices), int(vertices.shape[0]), N.ptr(faces), int(faces.shape[0]), N.ptr(scratch),
                                       N.ptr(raylen_dev), N.stream()), "mesh_raylen")


def texture_store_launch(rgb: Tensor, count: int, first: int, atlas_u8: Tensor) -> None:
    """nsamd_texture_store: the first `count` rows of rgb `[n,3]` fp32 as 8-bit levels into rows first .. first + count - 1 of the
    `[H W, 3]` (or `[H, W, 3]`) uint8 atlas."""
    N.require_cuda(rgb, atlas_u8)
    assert rgb.dtype == torch.float32 and atlas_u8.dtype == torch.uint8 and rgb.shape[0] >= count >= 0
    assert first >= 0 and 3 * (first + count) <= atlas_u8.numel()
    N.check(N.load().nsamd_texture_store(N.ptr(rgb), int(count), int(first), N.ptr(atlas_u8), N.stream()), "texture_store")


# ---------------------------------------------------------------------------------------------------------------
# eval frames: minimum / maximum, PSNR and SSIM, colormaps (include/nsamd_image.h)
# ---------------------------------------------------------------------------------------------------------------
def image_range_launch(x: Tensor, scratch: Tensor, range2: Tensor) -> None:
    """nsamd_image_range on the current stream: range2 `[2]` fp32 receives {min, max} of the fp32 values of x (a NaN makes both
    NaN); scratch: uint8, `N.RANGE_SCRATCH_BYTES` bytes."""
    N.require_cuda(x, scratch, range2)
    assert x.dtype == range2.dtype == torch.float32 and range2.numel() >= 2
    assert scratch.dtype == torch.uint8 and scratch.numel() >= N.RANGE_SCRATCH_BYTES and scratch.data_ptr() % 8 == 0
    N.check(N.load().nsamd_image_range(N.ptr(x), int(x.numel()), N.ptr(scratch), N.ptr(range2), N.stream()), "image_range")


def image_metrics_scratch_bytes(H: int, W: int, C: int) -> int:
    """nsamd_image_metrics_scratch_bytes: two fp64 partial sums per tile of NSAMD_SSIM_TILE^2 windows (host arithmetic only; 0 for
    a size the entry point refuses)."""
    return int(N.load().nsamd_image_metrics_scratch_bytes(int(H), int(W), int(C)))


def image_metrics_launch(pred: Tensor, target: Tensor, range_pred: Optional[Tensor], range_target: Optional[Tensor],
                         data_range: float, psnr_range: float, scratch: Tensor, out4: Tensor, ssim_map: Optional[Tensor]) -> None:
    """nsamd_image_metrics: out4 `[4]` fp32 receives {mse, psnr, ssim, R} of pred against target, both `[H,W,C]` fp32; R from the
    two `[2]` ranges on the device, or data_range when both are None. ssim_map: `[H-10,W-10,C]` fp32 or None."""
    N.require_cuda(pred, target, range_pred, range_target, scratch, out4, ssim_map)
    H, W, C = (int(s) for s in pred.shape)
    assert pred.dtype == target.dtype == out4.dtype == torch.float32 and tuple(target.shape) == (H, W, C) and out4.numel() >= 4
    assert (range_pred is None) == (range_target is None)
    assert range_pred is None or (range_pred.dtype == range_target.dtype == torch.float32 and min(range_pred.numel(), range_target.numel()) >= 2)
    assert scratch.dtype == torch.uint8 and scratch.numel() >= image_metrics_scratch_bytes(H, W, C) and scratch.data_ptr() % 8 == 0
    assert ssim_map is None or (ssim_map.dtype == torch.float32 and tuple(ssim_map.shape) == (H - 10, W - 10, C))
    N.check(N.load().nsamd_image_metrics(N.ptr(pred), N.ptr(target), H, W, C, N.ptr(range_pred), N.ptr(range_target), float(data_range),
                                         float(psnr_range), N.ptr(scratch), N.ptr(out4), N.ptr(ssim_map), N.stream()), "image_metrics")


def colormap_launch(values: Tensor, lut: Optional[Tensor], range2: Optional[Tensor], accumulation: Optional[Tensor],
                    params: "N.ColormapParams", out_rgb: Optional[Tensor], out_u8: Optional[Tensor]) -> None:
    """nsamd_colormap: the colours of the n fp32 values into out_rgb `[n,3]` fp32 and / or out_u8 `[n,3]` uint8. lut `[256,3]`
    fp32 (None: "gray"), range2 `[2]` fp32 = {min, max} of the values where the parameters need them, accumulation `[n]` fp32."""
    N.require_cuda(values, lut, range2, accumulation, out_rgb, out_u8)
    n = int(values.numel())
    assert values.dtype == torch.float32 and (lut is None or (lut.dtype == torch.float32 and tuple(lut.shape) == (256, 3)))
    assert range2 is None or (range2.dtype == torch.float32 and range2.numel() >= 2)
    assert accumulation is None or (accumulation.dtype == torch.float32 and accumulation.numel() == n)
    assert out_rgb is None or (out_rgb.dtype == torch.float32 and out_rgb.numel() == 3 * n)
    assert out_u8 is None or (out_u8.dtype == torch.uint8 and out_u8.numel() == 3 * n)
    N.check(N.load().nsamd_colormap(N.ptr(values), n, N.ptr(lut), N.ptr(range2), N.ptr(accumulation), params, N.ptr(out_rgb),
                                    N.ptr(out_u8), N.stream()), "colormap")


def image_range(x: Tensor, scratch: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """{min, max} of x as a `[2]` fp32 tensor on x's device; no host read."""
    x = x.contiguous()
    scratch = torch.empty(N.RANGE_SCRATCH_BYTES, dtype=torch.uint8, device=x.device) if scratch is None else scratch
    out = torch.empty(2, dtype=torch.float32, device=x.device) if out is None else out
    image_range_launch(x, scratch, out)
    return out


def image_metrics(pred: Tensor, target: Tensor, data_range: Optional[float] = None, psnr_range: float = 1.0, return_map: bool = False,
                  scratch: Optional[Tensor] = None, out: Optional[Tensor] = None):
    """{mse, psnr, ssim, R} of pred against target (`[H,W,C]` fp32) as a `[4]` fp32 tensor on their device, with the per-window
    SSIM map `[H-10,W-10,C]` when asked for. data_range None: R is the larger of the two images' max - min, formed on the device."""
    pred, target = pred.contiguous(), target.contiguous()
    H, W, C = (int(s) for s in pred.shape)
    nbytes = max(image_metrics_scratch_bytes(H, W, C), 2 * N.RANGE_SCRATCH_BYTES)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=pred.device) if scratch is None else scratch
    out = torch.empty(4, dtype=torch.float32, device=pred.device) if out is None else out
    ranges = None
    if data_range is None:
        ranges = torch.empty(2, 2, dtype=torch.float32, device=pred.device)
        image_range_launch(pred, scratch, ranges[0])
        image_range_launch(target, scratch[N.RANGE_SCRATCH_BYTES:], ranges[1])
    ssim_map = torch.empty(H - 10, W - 10, C, dtype=torch.float32, device=pred.device) if return_map else None
    image_metrics_launch(pred, target, None if ranges is None else ranges[0], None if ranges is None else ranges[1],
                         0.0 if data_range is None else data_range, psnr_range, scratch, out, ssim_map)
    return (out, ssim_map) if return_map else out


def colormap(values: Tensor, lut: Optional[Tensor], params: "N.ColormapParams", accumulation: Optional[Tensor] = None,
             range2: Optional[Tensor] = None, rgb: bool = True, u8: bool = False):
    """The colours of a one-channel image `[..., 1]` (or `[...]`): `[..., 3]` fp32, uint8, or both as a pair. range2 None: the
    minimum and maximum the parameters need come from image_range of the values."""
    values = values.contiguous()
    shape = tuple(values.shape[:-1]) if values.dim() > 1 and values.shape[-1] == 1 else tuple(values.shape)
    needs = bool(params.normalize) or (params.mode == N.COLORMAP_DEPTH and params.fixed != 3)
    if needs and range2 is None:
        range2 = image_range(values)
    acc = None if accumulation is None else accumulation.contiguous()
    out_rgb = torch.empty(*shape, 3, dtype=torch.float32, device=values.device) if rgb else None
    out_u8 = torch.empty(*shape, 3, dtype=torch.uint8, device=values.device) if u8 else None
    colormap_launch(values, lut, range2 if needs else None, acc, params, out_rgb, out_u8)
    return (out_rgb, out_u8) if rgb and u8 else (out_rgb if rgb else out_u8)
