"""Mesh export: rendered depth and colour frames fused into a TSDF volume on the device (`ns-export tsdf`).

Reference: nerfstudio/exporter/tsdf_utils.py. Its `export_tsdf_mesh` (:277-389) renders every training camera, copies each frame
to numpy and back (exporter_utils.render_trajectory), and `TSDF.integrate_tsdf` (:172-274) then updates the volume with ~40
eager torch launches over `[batch, voxels]` temporaries — more than 13 GB of them for 256^3 voxels and 10 views, by the shapes
in that function, to update 470 MB of state. Here

    TSDFVolume          the volume's state on one device; `integrate` is ONE launch of the tsdf kernel (csrc/tsdf.hip through
                        functional.tsdf_integrate_launch) per batch of views: 20 B per voxel read, 20 B written where a view
                        was valid
    fuse_views          renders the cameras with EvalRenderer.render_camera — rays generated inside the chunk loop — into two
                        static device buffers of `views_per_launch` frames and integrates each full buffer: no frame goes to
                        the host, memory is bounded by `views_per_launch`
    TSDFVolume.get_mesh marching cubes at level 0 on the device (csrc/mesh.hip through functional.mesh_count_launch and
                        functional.mesh_emit_launch): an ordered compaction of the crossed edges and the cells' triangles into
                        an indexed `Mesh`; the host reads two counts to size the outputs, nothing else leaves the device
    write_mesh_ply      binary PLY of a `Mesh`: positions, normals, colours, faces
    export_tsdf_mesh    the reference's function, signature and defaults, over the two; by default marching cubes and the PLY
                        writer are the reference's (`TSDFVolume.to_reference`: skimage, pymeshlab)
    export_tsdf_mesh_on_device   the same with `device_mesh` and `write_mesh_ply`: no reference installation needed
    export_textured_tsdf_mesh_on_device   that, then the mesh textured through the model (texture.py): `mesh.obj`,
                        `material_0.mtl`, `material_0.png` — `ns-export tsdf` with its default texture_method="nerf"

Kept as the reference has them (csrc/tsdf.h): the weight clamp of :267, voxels behind a camera, voxel coordinates at the
voxel's corner, the truncation from the x voxel size alone. The device mesh (include/nsamd_mesh.h) restates marching cubes
over a generated triangle table, since skimage was not available to compare with: same surface, its own vertex and triangle
order; its normals are in world space where the reference's are in index space (they differ for anisotropic voxels only).

This module imports nothing of nerfstudio at module level: `to_reference` and the default mesh / writer functions import it
lazily. There is no torch fallback: a CPU tensor with the native launch raises RuntimeError.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from . import _ply
from . import eval_frame
from . import functional as F


def _import_reference():
    try:
        from nerfstudio.exporter import tsdf_utils
    except ImportError as e:
        raise ImportError("nerfstudio_amd.export: meshing and writing the mesh are the reference's own code "
                          "(nerfstudio.exporter.tsdf_utils.TSDF.get_mesh / export_mesh: skimage marching cubes, pymeshlab); "
                          f"install nerfstudio with its export dependencies to use them ({e})") from e
    return tsdf_utils


@dataclass
class Mesh:
    """The fields of the reference's exporter_utils.Mesh (:46-57) that TSDF.get_mesh fills: vertices `[V,3]` fp32, faces `[T,3]`
    (int32 here: indices into vertices), normals `[V,3]` fp32, colors `[V,3]` fp32 in [0, 1]."""

    vertices: Tensor
    faces: Tensor
    normals: Tensor
    colors: Tensor


class TSDFVolume:
    """values `[X,Y,Z]`, weights `[X,Y,Z]`, colors `[X,Y,Z,3]`: fp32, dense, on one device. origin, voxel_size: `[3]` fp32 on the
    host (the launch takes them by value)."""

    def __init__(self, values: Tensor, weights: Tensor, colors: Tensor, origin: Tensor, voxel_size: Tensor,
                 truncation_margin: float = 5.0) -> None:
        assert values.dim() == 3 and weights.shape == values.shape and tuple(colors.shape) == (*values.shape, 3)
        assert values.dtype == weights.dtype == colors.dtype == torch.float32
        assert values.device == weights.device == colors.device
        self.values, self.weights, self.colors = values.contiguous(), weights.contiguous(), colors.contiguous()
        self.origin = torch.as_tensor(origin, dtype=torch.float32).reshape(3).cpu()
        self.voxel_size = torch.as_tensor(voxel_size, dtype=torch.float32).reshape(3).cpu()
        self.truncation_margin = float(truncation_margin)

    @property
    def device(self) -> torch.device:
        return self.values.device

    @property
    def truncation(self) -> float:
        """tsdf_utils.py:80-85: the x voxel size times the margin, for every axis, also with anisotropic voxels."""
        return self.voxel_size[0].item() * self.truncation_margin

    @staticmethod
    def from_aabb(aabb, volume_dims, device="cpu") -> "TSDFVolume":
        """tsdf_utils.py:88-113: origin aabb[0], voxel_size (aabb[1] - aabb[0]) / dims; values -1, weights 0, colours 0."""
        aabb = torch.as_tensor(aabb, dtype=torch.float32).reshape(2, 3).cpu()
        dims = torch.as_tensor(volume_dims).reshape(3).to(torch.int64).cpu()
        voxel_size = (aabb[1] - aabb[0]) / dims
        shape = dims.tolist()
        return TSDFVolume(-torch.ones(shape, device=device), torch.zeros(shape, device=device),
                          torch.zeros(shape + [3], device=device), aabb[0], voxel_size)

    @torch.no_grad()
    def integrate(self, c2w: Tensor, K: Tensor, depth_images: Tensor, color_images: Optional[Tensor] = None,
                  mask_images: Optional[Tensor] = None, launch_fn: Optional[Callable] = None) -> None:
        """TSDF.integrate_tsdf (:172-274) as one launch. c2w `[B,4,4]` or `[B,3,4]`; K `[B,3,3]` (the third row is ignored, as
        the reference ignores it); depth `[B,1,H,W]`, `[B,H,W]` or `[B,H,W,1]` (four dimensions with shape[1] == 1 read as the
        reference's channel-first layout); colour `[B,H,W,3]` — what the kernel takes — or `[B,3,H,W]`, made contiguous
        channel-last once. launch_fn: stands in for functional.tsdf_integrate_launch (same arguments) in CPU tests."""
        if mask_images is not None:
            raise NotImplementedError("Mask images are not supported yet.")  # :190-191
        dev = self.device
        f32 = dict(device=dev, dtype=torch.float32)
        B = int(c2w.shape[0])
        c2w = c2w.to(**f32)
        if tuple(c2w.shape[1:]) == (3, 4):
            row = torch.tensor([0.0, 0.0, 0.0, 1.0], **f32).expand(B, 1, 4)
            c2w = torch.cat([c2w, row], dim=1)
        if tuple(c2w.shape[1:]) != (4, 4):
            raise ValueError(f"c2w must be [B,4,4] or [B,3,4], got {tuple(c2w.shape)}")
        # :210, one matrix at a time: torch picks its LU routine by the batch size, and a view's w2c must not depend on which
        # views share its launch (views one at a time == the batch, bit for bit); inv_ex: torch.inverse without its host check
        w2c = torch.stack([torch.linalg.inv_ex(m).inverse for m in c2w])[:, :3, :].contiguous() if B else c2w[:, :3, :].contiguous()
        if tuple(K.shape) != (B, 3, 3):
            raise ValueError(f"K must be [{B},3,3], got {tuple(K.shape)}")
        K = K.to(**f32)[:, :2, :].contiguous()
        depth = depth_images.to(**f32)
        if depth.dim() == 4:
            if depth.shape[1] == 1:
                depth = depth[:, 0]
            elif depth.shape[-1] == 1:
                depth = depth[..., 0]
        if depth.dim() != 3 or depth.shape[0] != B:
            raise ValueError(f"depth images must be [{B},1,H,W], [{B},H,W] or [{B},H,W,1], got {tuple(depth_images.shape)}")
        depth = depth.contiguous()
        H, W = int(depth.shape[1]), int(depth.shape[2])
        color = None
        if color_images is not None:
            color = color_images.to(**f32)
            if tuple(color.shape) == (B, H, W, 3):
                color = color.contiguous()
            elif tuple(color.shape) == (B, 3, H, W):
                color = color.permute(0, 2, 3, 1).contiguous()
            else:
                raise ValueError(f"colour images must be [{B},{H},{W},3] or [{B},3,{H},{W}], got {tuple(color_images.shape)}")
        launch = F.tsdf_integrate_launch if launch_fn is None else launch_fn
        launch(self.origin.tolist(), self.voxel_size.tolist(), self.truncation, self.values, self.weights, self.colors, w2c, K,
               depth, color)

    @torch.no_grad()
    def get_mesh(self, launch_fns: Optional[Tuple[Callable, Callable]] = None) -> Mesh:
        """TSDF.get_mesh (:115-136) on the volume's device: marching cubes at level 0 over clamp(values, -1, 1), no mask on the
        weights. Two launches of csrc/mesh.hip — count, emit — with one read of the two totals between them to size the outputs:
        the only synchronisation. launch_fns: a (count, emit) pair standing in for functional.mesh_count_launch and
        functional.mesh_emit_launch (same arguments) in CPU tests. With the native launches a CPU volume raises RuntimeError."""
        count, emit = (F.mesh_count_launch, F.mesh_emit_launch) if launch_fns is None else launch_fns
        dev = self.device
        vol = N.make_mesh_volume(self.origin.tolist(), self.voxel_size.tolist(), self.values.shape)
        scratch = torch.empty(N.mesh_scratch_bytes(self.values.numel()), dtype=torch.uint8, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        count(vol, self.values, scratch, totals)
        V, T = totals.tolist()
        vertices, normals, colors = (torch.empty((V, 3), dtype=torch.float32, device=dev) for _ in range(3))
        faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
        emit(vol, self.values, self.colors, scratch, vertices, normals, colors, faces)
        return Mesh(vertices=vertices, faces=faces, normals=normals, colors=colors)

    def voxel_coords(self) -> Tensor:
        """`[3,X,Y,Z]` as the reference builds them (:100-104), on the volume's device. The kernel never materialises them."""
        dev = self.device
        axes = [torch.arange(n, device=dev) for n in self.values.shape]
        grid = torch.stack(torch.meshgrid(axes, indexing="ij"), dim=0)
        return self.origin.to(dev).view(3, 1, 1, 1) + grid * self.voxel_size.to(dev).view(3, 1, 1, 1)

    def to_reference(self):
        """The reference's `TSDF` dataclass over the SAME tensors (voxel_coords are built only here): `get_mesh` (skimage marching
        cubes) and `export_mesh` (pymeshlab) remain the reference's own code."""
        tsdf_utils = _import_reference()
        dev = self.device
        return tsdf_utils.TSDF(self.voxel_coords(), self.values, self.weights, self.colors, self.voxel_size.to(dev),
                               self.origin.to(dev), self.truncation_margin)


def scaled_pinhole_cameras(cameras, downscale_factor) -> List[Tuple[Tensor, float, float, float, float, int, int]]:
    """(c2w [3,4], fx, fy, cx, cy, H, W) per camera at 1 / downscale_factor of its resolution — the numbers
    Cameras.rescale_output_resolution (cameras/cameras.py:987-1020) would leave in the object: fp32 products, H and W truncated
    to integers. The cameras object is only read. A camera that is not CameraType.PERSPECTIVE raises ValueError: the TSDF's
    projection is a pinhole one."""
    c2w = cameras.camera_to_worlds.detach().reshape(-1, 3, 4)
    n = int(c2w.shape[0])
    ctype = getattr(cameras, "camera_type", None)
    if ctype is not None:
        for i, t in enumerate(torch.as_tensor(ctype).reshape(-1).tolist()):
            if int(t) != eval_frame.PERSPECTIVE:
                raise ValueError(f"fuse_views: camera {i} is of type {F._CAMERA_TYPE_NAMES.get(int(t), int(t))}; the TSDF "
                                 "projects voxels through a pinhole, only CameraType.PERSPECTIVE cameras can be fused")
    scale = torch.tensor([1.0 / downscale_factor], dtype=torch.float32)
    col = lambda t: torch.as_tensor(t).detach().reshape(-1).cpu()  # noqa: E731
    fx, fy, cx, cy = ((col(t).float() * scale).tolist() for t in (cameras.fx, cameras.fy, cameras.cx, cameras.cy))
    height = (col(cameras.height) * scale).to(torch.int64).tolist()
    width = (col(cameras.width) * scale).to(torch.int64).tolist()
    return [(c2w[i], fx[i], fy[i], cx[i], cy[i], height[i], width[i]) for i in range(n)]


def fuse_views(model, cameras, volume: TSDFVolume, downscale_factor=2, views_per_launch: int = 10,
               depth_output_name: str = "depth", rgb_output_name: str = "rgb", render_fn: Optional[Callable] = None) -> int:
    """Render every camera of `cameras` at 1 / downscale_factor of its resolution — pinhole, distortion disabled, as
    tsdf_utils.py:330-339 asks — and fuse the frames into `volume`, `views_per_launch` views per launch, in camera order.
    Returns the number of launches. render_fn(c2w, fx, fy, cx, cy, H, W) -> dict of `[H,W,C]` device tensors replaces the
    model's own runner — NgpEvalRenderer for a model `ngp_eval_render.supported` accepts, else EvalRenderer — and is required for
    a model both refuse."""
    views = scaled_pinhole_cameras(cameras, downscale_factor)
    V = int(views_per_launch)
    if V < 1:
        raise ValueError(f"views_per_launch must be at least 1, got {views_per_launch}")
    dev = volume.device
    launches = 0
    with eval_frame.eval_mode(model):
        if render_fn is None:
            runner, reason = eval_frame.export_runner_for(model, dev)
            if reason == eval_frame.RUNNER_OFF:
                N.require_cuda(volume.values)  # (a volume on the host has no runner either: that is the error to give)
                raise RuntimeError(f"fuse_views: {reason}")
            if reason is not None:
                raise ValueError(f"fuse_views: {reason}; pass render_fn")
            render_fn = lambda *view: runner.render_camera(*view, lens=None)  # noqa: E731
        depth_buf = color_buf = None
        poses: List[Tensor] = []
        intrinsics: List[List[List[float]]] = []

        def flush() -> None:
            nonlocal launches
            k = len(poses)
            if k == 0:
                return
            volume.integrate(torch.stack(poses).to(dev), torch.tensor(intrinsics, dtype=torch.float32), depth_buf[:k], color_buf[:k])
            launches += 1
            poses.clear()
            intrinsics.clear()

        for c2w, fx, fy, cx, cy, H, W in views:
            if depth_buf is None or tuple(depth_buf.shape[1:]) != (H, W):
                flush()  # a camera of another size: what the buffers hold goes first
                depth_buf = torch.empty((V, H, W), device=dev, dtype=torch.float32)
                color_buf = torch.empty((V, H, W, 3), device=dev, dtype=torch.float32)
            out: Dict[str, Tensor] = render_fn(c2w, fx, fy, cx, cy, H, W)
            for name in (depth_output_name, rgb_output_name):
                if name not in out:
                    raise KeyError(f"fuse_views: no output named {name!r}; the renderer gives {sorted(out)}")
            k = len(poses)
            depth_buf[k].copy_(out[depth_output_name].reshape(H, W))
            color_buf[k].copy_(out[rgb_output_name].reshape(H, W, -1)[..., :3])
            poses.append(c2w)
            intrinsics.append([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
            if len(poses) == V:
                flush()
        flush()
    return launches


def _reference_mesh(volume: TSDFVolume):
    return volume.to_reference().get_mesh()


def _reference_write(mesh, filename: str) -> None:
    _import_reference().TSDF.export_mesh(mesh, filename=filename)


def device_mesh(volume: TSDFVolume) -> Mesh:
    """`mesh_fn` of export_tsdf_mesh: the volume's own marching cubes."""
    return volume.get_mesh()


def write_mesh_ply(mesh: Mesh, filename) -> None:
    """`write_fn` of export_tsdf_mesh. Binary little-endian PLY (_ply.write, as pointcloud.PointCloud.write_ply): per vertex
    x y z nx ny nz float32 and red green blue alpha uint8 — _ply.colors, alpha 255 — then per face
    `list uchar int vertex_indices`. An empty mesh writes a valid file with no elements' rows."""
    props = _ply.floats("xyz", mesh.vertices) + _ply.floats(("nx", "ny", "nz"), mesh.normals) + _ply.colors(mesh.colors)
    _ply.write(filename, props + [("alpha", "u1", 255)], mesh.faces.detach().to(torch.int32).cpu().numpy())


def export_tsdf_mesh(pipeline, output_dir: Path, downscale_factor: int = 2, depth_output_name: str = "depth",
                     rgb_output_name: str = "rgb", resolution: Union[int, Sequence[int]] = (256, 256, 256), batch_size: int = 10,
                     use_bounding_box: bool = True, bounding_box_min: Tuple[float, float, float] = (-1.0, -1.0, -1.0),
                     bounding_box_max: Tuple[float, float, float] = (1.0, 1.0, 1.0),
                     refine_mesh_using_initial_aabb_estimate: bool = False, refinement_epsilon: float = 1e-2, *,
                     render_fn: Optional[Callable] = None, mesh_fn: Optional[Callable] = None,
                     write_fn: Optional[Callable] = None) -> None:
    """tsdf_utils.export_tsdf_mesh (:277-389) — its arguments and defaults, so `ns-export tsdf` can call it in place of the
    reference's — with the frames rendered and fused on the device (`fuse_views`; batch_size = views per launch). The
    dataparser's cameras are only read (the reference rescales them in place). mesh_fn(volume) -> mesh and write_fn(mesh,
    filename) default to the reference's TSDF.get_mesh / TSDF.export_mesh; render_fn as in `fuse_views`."""
    device = pipeline.device
    assert pipeline.datamanager.train_dataset is not None
    dataparser_outputs = pipeline.datamanager.train_dataset._dataparser_outputs
    if not use_bounding_box:
        aabb = dataparser_outputs.scene_box.aabb
    else:
        aabb = torch.tensor([bounding_box_min, bounding_box_max])
    if isinstance(resolution, int):
        volume_dims = [resolution] * 3
    elif isinstance(resolution, (list, tuple)) and len(resolution) == 3:
        volume_dims = [int(r) for r in resolution]
    else:
        raise ValueError("Resolution must be an int or a list.")
    mesh_fn = _reference_mesh if mesh_fn is None else mesh_fn
    write_fn = _reference_write if write_fn is None else write_fn
    cameras = dataparser_outputs.cameras

    def fused(box) -> TSDFVolume:
        volume = TSDFVolume.from_aabb(box, volume_dims, device=device)
        fuse_views(pipeline.model, cameras, volume, downscale_factor=downscale_factor, views_per_launch=batch_size,
                   depth_output_name=depth_output_name, rgb_output_name=rgb_output_name, render_fn=render_fn)
        return volume

    mesh = mesh_fn(fused(aabb))
    if refine_mesh_using_initial_aabb_estimate:  # :365-386: a second volume over the mesh's bounds +- epsilon
        vertices_min = torch.min(mesh.vertices, dim=0).values - refinement_epsilon
        vertices_max = torch.max(mesh.vertices, dim=0).values + refinement_epsilon
        mesh = mesh_fn(fused(torch.stack([vertices_min, vertices_max]).cpu()))
    write_fn(mesh, str(Path(output_dir) / "tsdf_mesh.ply"))


def export_tsdf_mesh_on_device(pipeline, output_dir: Path, **kwargs) -> None:
    """export_tsdf_mesh with the mesh extracted on the device and written by `write_mesh_ply`: the whole of `ns-export tsdf`,
    the refinement pass over the mesh's bounds included, with no reference installed. kwargs: export_tsdf_mesh's."""
    kwargs.setdefault("mesh_fn", device_mesh)
    kwargs.setdefault("write_fn", write_mesh_ply)
    export_tsdf_mesh(pipeline, output_dir, **kwargs)


def export_textured_tsdf_mesh_on_device(pipeline, output_dir: Path, px_per_uv_triangle: int = 4, **kwargs) -> Mesh:
    """`ns-export tsdf` with its default texture_method="nerf" (scripts/exporter.py:211, 253-266) and no reference installed:
    export_tsdf_mesh_on_device — `tsdf_mesh.ply` — then the mesh, which never left the device, textured by
    texture.export_textured_mesh(unwrap_method="custom"): `mesh.obj`, `material_0.mtl`, `material_0.png`. Returns the mesh.
    There is NO decimation (the reference's target_num_faces goes through pymeshlab): the atlas holds (P + 3) P / 2 texels per
    face, so the volume's `resolution` is the lever on the number of faces and with it on the atlas size, which is logged.
    kwargs: export_tsdf_mesh's."""
    from . import texture

    meshes: List[Mesh] = []
    mesh_fn = kwargs.pop("mesh_fn", device_mesh)

    def keeping_mesh(volume: TSDFVolume) -> Mesh:
        meshes.append(mesh_fn(volume))
        return meshes[-1]

    export_tsdf_mesh_on_device(pipeline, output_dir, mesh_fn=keeping_mesh, **kwargs)
    mesh = meshes[-1]  # (after a refinement pass: the second volume's)
    texture.export_textured_mesh(mesh, pipeline, Path(output_dir), px_per_uv_triangle, unwrap_method="custom")
    return mesh
