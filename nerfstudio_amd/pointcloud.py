"""Point-cloud export: the part of `ns-export pointcloud` after the model, on the device.

Reference: nerfstudio/exporter/exporter_utils.py generate_point_cloud (:83-223) and scripts/exporter.py ExportPointCloud
(:97-186). There every batch is boolean-indexed twice over four tensors and appended to Python lists, the whole cloud goes to
the host in float64, and Open3D's remove_statistical_outlier builds a k-d tree and asks it for 20 neighbours per point. Here

    PointAccumulator            the cloud's buffers on one device; `add` is ONE launch of the selection kernel
                                (csrc/pointcloud.hip through functional.points_select_launch) per batch of rays: the kept rays
                                appended in ray order behind a device-side cursor. The running total comes back through a
                                pinned host word one batch late, so the loop never drains the device
    remove_statistical_outliers the exact mean distance to the k nearest neighbours over a uniform grid (one lane per query, a
                                brute-force workgroup for the queries the grid gives up on), Open3D's threshold in float64,
                                the kept indices by the selection's ordered compaction
    generate_point_cloud        the reference's function, arguments and defaults, over the two
    export_point_cloud          ExportPointCloud.main's fields; writes point_cloud.ply (`PointCloud.write_ply`: no Open3D)

The outlier rule restates Open3D's RemoveStatisticalOutliers from its source and documentation (Open3D was not available to
compare against): SearchKNN returns the query itself at distance 0; a point is valid when its mean distance is > 0; the
threshold is mean + std_ratio * std over the valid points with the n - 1 denominator; kept: valid and below the threshold.

This module imports nothing of nerfstudio at module level. There is no torch fallback: a CPU tensor with the native launches
raises RuntimeError.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _native as N
from . import _ply
from . import functional as F

NB_NEIGHBORS = 20  # exporter_utils.py:193
DEFAULT_MAX_RINGS = 6
DEFAULT_OCCUPANCY = 8.0  # points per cell of the grid box, on average over ALL its cells
DEFAULT_QUANTILES = (0.01, 0.99)  # the grid box without a crop box: per axis, between these fractions of the points
MAX_DIM = 256  # cells per axis


class Launches:
    """The four native launches (functional.py). CPU tests of the layers above pass an object with the same methods over the
    host build of csrc/pointcloud.h."""

    points_select = staticmethod(F.points_select_launch)
    select_below = staticmethod(F.select_below_launch)
    point_cell_keys = staticmethod(F.point_cell_keys_launch)
    knn_mean_distance = staticmethod(F.knn_mean_distance_launch)


class PointCloud:
    """points, colors, view_directions `[n,3]` fp32 on one device, normals `[n,3]` or None."""

    def __init__(self, points: Tensor, colors: Tensor, view_directions: Tensor, normals: Optional[Tensor] = None) -> None:
        n = int(points.shape[0])
        assert tuple(points.shape) == tuple(colors.shape) == tuple(view_directions.shape) == (n, 3)
        assert normals is None or tuple(normals.shape) == (n, 3)
        self.points, self.colors, self.view_directions, self.normals = points, colors, view_directions, normals

    def __len__(self) -> int:
        return int(self.points.shape[0])

    def index(self, ind: Tensor) -> "PointCloud":
        """The rows `ind` of every tensor: the reference's `view_directions[ind]` / `normals[ind]` bookkeeping (:196-213)."""
        return PointCloud(self.points[ind], self.colors[ind], self.view_directions[ind],
                          None if self.normals is None else self.normals[ind])

    def write_ply(self, path) -> None:
        """Binary little-endian PLY (_ply.write): x y z float32, red green blue uint8 (_ply.colors: colors * 255 truncated), then
        nx ny nz float32 when there are normals."""
        normals = [] if self.normals is None else _ply.floats(("nx", "ny", "nz"), self.normals)
        _ply.write(path, _ply.floats("xyz", self.points) + _ply.colors(self.colors) + normals)

    def to_open3d(self):
        """open3d.geometry.PointCloud with float64 arrays, as the reference builds it (:186-188, :214)."""
        try:
            import open3d as o3d
        except ImportError as e:
            raise ImportError(f"PointCloud.to_open3d needs the open3d package ({e}); write_ply does without it") from e
        pcd = o3d.geometry.PointCloud()
        pcd.points = o3d.utility.Vector3dVector(self.points.double().cpu().numpy())
        pcd.colors = o3d.utility.Vector3dVector(self.colors.double().cpu().numpy())
        if self.normals is not None:
            pcd.normals = o3d.utility.Vector3dVector(self.normals.double().cpu().numpy())
        return pcd


def _obb_world2box(crop_obb) -> Tuple[Sequence[float], Sequence[float]]:
    """(world2box rows, S / 2) of an object with R [3,3], T [3], S [3]: torch.inverse of the 4x4 in fp32 on the host, as
    OrientedBox.within computes it (data/scene_box.py:97-106)."""
    H = torch.eye(4, dtype=torch.float32)
    H[:3, :3] = torch.as_tensor(crop_obb.R).detach().cpu()
    H[:3, 3] = torch.as_tensor(crop_obb.T).detach().cpu()
    world2box = torch.inverse(H)[:3].reshape(-1).tolist()
    half = (torch.as_tensor(crop_obb.S).detach().cpu().to(torch.float32) / 2).tolist()
    return world2box, half


def obb_aabb(crop_obb) -> Tuple[Sequence[float], Sequence[float]]:
    """The axis-aligned bounds of the oriented box: T -+ |R| S / 2."""
    R = torch.as_tensor(crop_obb.R).detach().cpu().double()
    T = torch.as_tensor(crop_obb.T).detach().cpu().double()
    reach = R.abs() @ (torch.as_tensor(crop_obb.S).detach().cpu().double() / 2)
    return (T - reach).tolist(), (T + reach).tolist()


class PointAccumulator:
    """The cloud under construction: four `[capacity,3]` buffers (normals only `with_normals`), the device cursor and the
    selection's scratch. `add` appends a batch's kept rays with one launch and returns the running total it KNOWS: the cursor
    is copied to a pinned host word behind every launch and read one batch late, behind that copy's event alone."""

    def __init__(self, capacity: int, device, with_normals: bool = False, launches=Launches) -> None:
        self.capacity, self.device, self.launches = int(capacity), torch.device(device), launches
        f32 = dict(device=self.device, dtype=torch.float32)
        self.points, self.colors, self.view_directions = (torch.empty((self.capacity, 3), **f32) for _ in range(3))
        self.normals = torch.empty((self.capacity, 3), **f32) if with_normals else None
        # rows so far, overflow flag (both the kernel's), batches whose normals left [0, 1] (this class's)
        self.cursor = torch.zeros(3, device=self.device, dtype=torch.int64)
        self._scratch: Optional[Tensor] = None
        cuda = self.device.type == "cuda"
        self._host = [torch.zeros(3, dtype=torch.int64, pin_memory=cuda) for _ in range(2)]
        self._events = [torch.cuda.Event() if cuda else None for _ in range(2)]
        self.totals: list = []  # the total after every batch whose copy has been read
        self.batches = 0

    def _check(self, words: Tensor) -> int:
        if int(words[1]) != 0:
            raise RuntimeError(f"PointAccumulator: a batch ran past the capacity of {self.capacity} points; nothing of it was "
                               "written (batches larger than the first one?)")
        if int(words[2]) != 0:
            raise ValueError("Normal values from method output must be in [0, 1]")  # exporter_utils.py:151-153
        return int(words[0])

    def _read(self, slot: int) -> None:
        if self._events[slot] is not None:
            self._events[slot].synchronize()
        self.totals.append(self._check(self._host[slot]))

    def add(self, ray_bundle, outputs: Dict[str, Tensor], rgb_output_name: str = "rgb", depth_output_name: str = "depth",
            normal_output_name: Optional[str] = None, use_alpha: bool = False, box: Optional["N.CropBox"] = None) -> Optional[int]:
        """One batch (:142-178). use_alpha: the model renders over a "random" background, so the opacity is its accumulation
        (get_rgba_image); otherwise every ray passes the opacity test. Returns the total after the PREVIOUS batch (None at
        the first)."""
        for name in (rgb_output_name, depth_output_name, normal_output_name):
            if name is not None and name not in outputs:
                raise KeyError(f"Could not find {name!r} in the model outputs; available: {sorted(outputs)}")
        accumulation_name = rgb_output_name.replace("rgb", "accumulation")
        if accumulation_name not in outputs:  # get_rgba_image, models/base_model.py:216-218
            raise NotImplementedError(f"no output named {accumulation_name!r}: the model's outputs do not give an opacity")
        f32 = dict(device=self.device, dtype=torch.float32)
        origins = ray_bundle.origins.detach().to(**f32).reshape(-1, 3).contiguous()
        directions = ray_bundle.directions.detach().to(**f32).reshape(-1, 3).contiguous()
        n = int(origins.shape[0])
        depth = outputs[depth_output_name].detach().to(**f32).reshape(n).contiguous()
        rgb = outputs[rgb_output_name].detach().to(**f32).reshape(n, 3).contiguous()
        alpha = outputs[accumulation_name].detach().to(**f32).reshape(n).contiguous() if use_alpha else None
        normals01 = None
        if (normal_output_name is not None) != (self.normals is not None):
            raise ValueError("PointAccumulator: with_normals and normal_output_name go together")
        if normal_output_name is not None:
            normals01 = outputs[normal_output_name].detach().to(**f32).reshape(n, 3).contiguous()
            lo, hi = torch.aminmax(normals01)  # one reduction; a NaN fails both comparisons, as the reference's assert does
            self.cursor[2:3] += (~((lo >= 0.0) & (hi <= 1.0))).to(torch.int64)
        words = N.select_scratch_words(n)
        if self._scratch is None or self._scratch.numel() < words:
            self._scratch = torch.empty(words, device=self.device, dtype=torch.int64)
        self.launches.points_select(origins, directions, depth, rgb, alpha, normals01, box if box is not None else N.make_crop_box(),
                                    self.points, self.colors, self.view_directions, self.normals, self.cursor, self._scratch)
        slot = self.batches % 2
        self._host[slot].copy_(self.cursor, non_blocking=True)
        if self._events[slot] is not None:
            self._events[slot].record()
        self.batches += 1
        if self.batches >= 2:
            self._read(1 - slot)  # the batch before this one
        return self.totals[-1] if self.totals else None

    def finish(self, num_points: Optional[int] = None) -> PointCloud:
        """The cloud so far; with num_points, truncated to the total after the first batch at which it reached num_points —
        where the reference's loop stops (:125). Reads the last batch's total."""
        if self.batches > len(self.totals):
            self._read((self.batches - 1) % 2)
        total = self.totals[-1] if self.totals else 0
        if num_points is not None:
            total = next((t for t in self.totals if t >= num_points), total)
        return PointCloud(self.points[:total], self.colors[:total], self.view_directions[:total],
                          None if self.normals is None else self.normals[:total])


def point_grid_for(points: Tensor, aabb=None, quantiles: Tuple[float, float] = DEFAULT_QUANTILES,
                   occupancy: float = DEFAULT_OCCUPANCY, dims: Optional[Sequence[int]] = None) -> "N.PointGrid":
    """The uniform grid of the neighbour search. Its box is `aabb` ((lo, hi), e.g. the crop box's) or, per axis, the span
    between the `quantiles` fractions of the points — a scene without a crop has points at depth ~1000 that would collapse the
    object into one cell of their bounding box; points outside the box fall into its border cells, which keeps the search
    exact. Cubic cells sized for `occupancy` points per cell on average over the box, or `dims` cells along the axes."""
    n = int(points.shape[0])
    if aabb is not None:
        lo, hi = [float(v) for v in aabb[0]], [float(v) for v in aabb[1]]
    else:
        finite = torch.nan_to_num(points.detach(), nan=0.0, posinf=3.0e38, neginf=-3.0e38)
        ranks = [min(n, max(1, int(math.floor(q * (n - 1))) + 1)) for q in quantiles]
        box = torch.stack([torch.kthvalue(finite, r, dim=0).values for r in ranks]).tolist()  # the one host read of the build
        lo, hi = box
    extent = [max(h - l, 0.0) for l, h in zip(lo, hi)]
    longest = max(extent)
    if not (longest > 0.0 and math.isfinite(longest)):
        return N.make_point_grid(lo if all(math.isfinite(v) for v in lo) else [0.0] * 3, 1.0, [1, 1, 1])
    extent = [max(e, longest * 1e-6) for e in extent]
    if dims is not None:
        dims = [int(d) for d in dims]
        cell = max(e / d for e, d in zip(extent, dims))
    else:
        cell = (extent[0] * extent[1] * extent[2] * occupancy / max(n, 1)) ** (1.0 / 3.0)
        cell = max(cell, longest / MAX_DIM)
        dims = [max(1, min(MAX_DIM, int(math.ceil(e / cell)))) for e in extent]
    return N.make_point_grid(lo, cell, dims)


def knn_mean_distances(points: Tensor, k: int, grid: "N.PointGrid", max_rings: int = DEFAULT_MAX_RINGS,
                       launches=Launches) -> Tuple[Tensor, Tensor]:
    """(avg [n] float64, unfinished [1 + n] int32) of nsamd_knn_mean_distance over `grid`: cell keys, a stable sort, the cells'
    start offsets (torch ops), then the search. unfinished[0]: the queries that fell to the brute-force phase."""
    if k > N.KNN_MAX_K:
        raise ValueError(f"at most {N.KNN_MAX_K} neighbours are supported (NSAMD_KNN_MAX_K), got {k}")
    dev = points.device
    n = int(points.shape[0])
    points = points.detach().to(torch.float32).contiguous()
    cells = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
    keys = torch.empty(n, device=dev, dtype=torch.int64)
    launches.point_cell_keys(points, grid, keys)
    sorted_keys, order = torch.sort(keys, stable=True)
    cell_start = torch.searchsorted(sorted_keys, torch.arange(cells + 1, device=dev, dtype=torch.int64)).to(torch.int32)
    avg = torch.empty(n, device=dev, dtype=torch.float64)
    unfinished = torch.zeros(n + 1, device=dev, dtype=torch.int32)
    launches.knn_mean_distance(points, order.to(torch.int32), cell_start, grid, k, max_rings, avg, unfinished)
    return avg, unfinished


def outlier_threshold(avg: Tensor, std_ratio: float) -> Tensor:
    """`[1]` float64 on avg's device: mean + std_ratio * std over the valid (avg > 0) entries, n - 1 in the denominator."""
    valid = avg > 0
    count = valid.sum()
    mean = torch.where(valid, avg, torch.zeros_like(avg)).sum() / count
    dev2 = torch.where(valid, (avg - mean) ** 2, torch.zeros_like(avg)).sum()
    return (mean + std_ratio * torch.sqrt(dev2 / (count - 1))).reshape(1)


def remove_statistical_outliers(points: Tensor, nb_neighbors: int = NB_NEIGHBORS, std_ratio: float = 2.0, *, aabb=None,
                                quantiles: Tuple[float, float] = DEFAULT_QUANTILES, occupancy: float = DEFAULT_OCCUPANCY,
                                dims: Optional[Sequence[int]] = None, grid: Optional["N.PointGrid"] = None,
                                max_rings: int = DEFAULT_MAX_RINGS, launches=Launches, stats: Optional[dict] = None):
    """Open3D's remove_statistical_outlier on the device -> (kept_indices [m] int64 ascending, avg [n] float64, threshold). The
    result does not depend on the grid (`aabb`, `quantiles`, `occupancy`, `dims` or a ready `grid`: see `point_grid_for`) or on
    `max_rings` (0: every query takes the brute-force phase) — they only move work. stats (a dict) receives
    `brute_force_queries` and the grid."""
    if nb_neighbors < 1 or std_ratio <= 0:
        raise ValueError("Illegal input parameters, the number of neighbors and standard deviation ratio must be positive.")
    if nb_neighbors > N.KNN_MAX_K:
        raise ValueError(f"at most {N.KNN_MAX_K} neighbours are supported (NSAMD_KNN_MAX_K), got {nb_neighbors}")
    n = int(points.shape[0])
    dev = points.device
    if n == 0:
        return torch.empty(0, device=dev, dtype=torch.int64), torch.empty(0, device=dev, dtype=torch.float64), float("nan")
    if grid is None:
        grid = point_grid_for(points, aabb, quantiles, occupancy, dims)
    avg, unfinished = knn_mean_distances(points, nb_neighbors, grid, max_rings, launches)
    threshold = outlier_threshold(avg, float(std_ratio))
    kept = torch.empty(n, device=dev, dtype=torch.int64)
    count = torch.zeros(1, device=dev, dtype=torch.int64)
    scratch = torch.empty(N.select_scratch_words(n), device=dev, dtype=torch.int64)
    launches.select_below(avg, threshold, kept, count, scratch)
    if stats is not None:
        stats.update(brute_force_queries=int(unfinished[0]), dims=list(grid.dims), cell_size=float(grid.cell_size),
                     origin=list(grid.origin))
    return kept[:int(count)], avg, float(threshold)


def _default_batch_fn(pipeline) -> Callable:
    source = getattr(pipeline, "_batch_source", None)  # device-resident batches (pipeline.setup_device_batches)
    if source is not None:
        return lambda: source.next_batch()[0]
    return lambda: pipeline.datamanager.next_train(0)[0]


def _default_render_fn(pipeline) -> Callable:
    def render(ray_bundle):
        with torch.no_grad():
            return pipeline.model(ray_bundle)

    return render


def generate_point_cloud(pipeline, num_points: int = 1000000, remove_outliers: bool = True, estimate_normals: bool = False,
                         reorient_normals: bool = False, rgb_output_name: str = "rgb", depth_output_name: str = "depth",
                         normal_output_name: Optional[str] = None, crop_obb=None, std_ratio: float = 10.0, *,
                         batch_fn: Optional[Callable] = None, render_fn: Optional[Callable] = None, launches=Launches,
                         max_batches: Optional[int] = None, outlier_options: Optional[dict] = None) -> PointCloud:
    """exporter_utils.generate_point_cloud (:83-223) — its arguments and defaults — as a `PointCloud` on the pipeline's device,
    in the reference's order. batch_fn() -> RayBundle (default: the pipeline's device batch source when it trains from one,
    else `datamanager.next_train(0)[0]`); render_fn(ray_bundle) -> outputs (default: the model under no_grad). The loop ends
    at the batch after the one at which the total reached num_points (the total is read one batch late) and the cloud is cut
    where the reference's loop stops. max_batches: RuntimeError instead of the reference's endless loop when too few rays
    pass. outlier_options: keyword arguments of `remove_statistical_outliers`."""
    if estimate_normals and normal_output_name is not None:
        raise ValueError("Cannot estimate normals and use normal_output_name at the same time")  # :201-204
    if estimate_normals:
        raise NotImplementedError("estimate_normals: Open3D's PCA normals are not part of the device path; use the model's "
                                  "normals (normal_output_name)")
    if reorient_normals and normal_output_name is None:
        raise ValueError("reorient_normals needs normals: pass normal_output_name")
    batch_fn = _default_batch_fn(pipeline) if batch_fn is None else batch_fn
    render_fn = _default_render_fn(pipeline) if render_fn is None else render_fn
    use_alpha = getattr(getattr(pipeline.model, "renderer_rgb", None), "background_color", None) == "random"
    box = aabb = None
    if crop_obb is not None:
        box = N.make_crop_box(*_obb_world2box(crop_obb))
        aabb = obb_aabb(crop_obb)
    acc = None
    while True:
        ray_bundle = batch_fn()
        outputs = render_fn(ray_bundle)
        if acc is None:
            rays = int(ray_bundle.origins.reshape(-1, 3).shape[0])
            acc = PointAccumulator(num_points + 2 * rays, ray_bundle.origins.device, normal_output_name is not None, launches)
        known = acc.add(ray_bundle, outputs, rgb_output_name, depth_output_name, normal_output_name, use_alpha, box)
        if known is not None and known >= num_points:
            break
        if max_batches is not None and acc.batches >= max_batches:
            if acc.finish().points.shape[0] >= num_points:
                break
            raise RuntimeError(f"generate_point_cloud: {acc.totals[-1]} of {num_points} points after {max_batches} batches")
    cloud = acc.finish(num_points)
    if remove_outliers:
        options = dict(aabb=aabb, launches=launches)
        options.update(outlier_options or {})
        ind, _, _ = remove_statistical_outliers(cloud.points, NB_NEIGHBORS, std_ratio, **options)
        cloud = cloud.index(ind)  # points, colours and — the reference's `ind` bookkeeping — view directions and normals
    if reorient_normals:  # :217-221
        flip = torch.sum(cloud.view_directions * cloud.normals, dim=-1) > 0
        cloud.normals = torch.where(flip[:, None], -cloud.normals, cloud.normals)
    return cloud


def rpy_matrix(roll: float, pitch: float, yaw: float) -> Tensor:
    """Rz(yaw) Ry(pitch) Rx(roll) as `[3,3]` fp32 — what OrientedBox.from_params builds from its RPY angles
    (data/scene_box.py:110-118)."""
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    return torch.tensor([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                         [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                         [-sp, cp * sr, cp * cr]], dtype=torch.float32)


class OrientedBox:
    """R [3,3], T [3], S [3] (data/scene_box.py:86-93)."""

    def __init__(self, R, T, S) -> None:
        self.R, self.T, self.S = (torch.as_tensor(v, dtype=torch.float32) for v in (R, T, S))


def export_point_cloud(pipeline, output_dir, num_points: int = 1000000, remove_outliers: bool = True,
                       reorient_normals: bool = True, normal_method: str = "model_output", normal_output_name: str = "normals",
                       depth_output_name: str = "depth", rgb_output_name: str = "rgb",
                       obb_center: Optional[Tuple[float, float, float]] = None,
                       obb_rotation: Optional[Tuple[float, float, float]] = None,
                       obb_scale: Optional[Tuple[float, float, float]] = None, num_rays_per_batch: int = 32768,
                       std_ratio: float = 10.0, save_world_frame: bool = False, **kwargs) -> PointCloud:
    """ExportPointCloud.main (scripts/exporter.py:129-186) with its fields as arguments: writes output_dir/point_cloud.ply and
    returns the cloud. kwargs: the keyword-only arguments of `generate_point_cloud`."""
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    sampler = getattr(pipeline.datamanager, "train_pixel_sampler", None)
    if sampler is not None:
        sampler.num_rays_per_batch = num_rays_per_batch  # :144-146
    crop_obb = None
    if obb_center is not None and obb_rotation is not None and obb_scale is not None:
        crop_obb = OrientedBox(rpy_matrix(*obb_rotation), obb_center, obb_scale)
    cloud = generate_point_cloud(pipeline, num_points=num_points, remove_outliers=remove_outliers,
                                 reorient_normals=reorient_normals, estimate_normals=normal_method == "open3d",
                                 rgb_output_name=rgb_output_name, depth_output_name=depth_output_name,
                                 normal_output_name=normal_output_name if normal_method == "model_output" else None,
                                 crop_obb=crop_obb, std_ratio=std_ratio, **kwargs)
    if save_world_frame:  # :165-174: the inverse dataparser transform, on poses with the points as translations
        points = cloud.points.detach().cpu()
        poses = torch.eye(4, dtype=torch.float32)[None, :3, :].repeat(points.shape[0], 1, 1)
        poses[:, :3, 3] = points
        poses = pipeline.datamanager.train_dataparser_outputs.transform_poses_to_original_space(poses)
        cloud.points = poses[:, :3, 3].to(cloud.points.device)
    cloud.write_ply(output_dir / "point_cloud.ply")
    return cloud
