"""Textured mesh export: one ray per texel rendered through the model, `mesh.obj` + `material_0.mtl` + `material_0.png`.

Reference: nerfstudio/exporter/texture_utils.py — the stage `ns-export tsdf` / `ns-export poisson` run after meshing
(texture_method="nerf"). Its `unwrap_mesh_per_uv_triangle` (:77-208) gathers `[H,W,3,3]` vertices and normals and `[H,W,3,2]`
texture coordinates to form barycentric weights in fp32 from differences of coordinates 1 / W apart (1e-3 of error at 50 000
faces), holds an `[H,W]` bundle and every output image at once, and `export_textured_mesh` (:322-493) writes the OBJ line by
line in Python. Here

    TexelAtlas            the layout in closed form (include/nsamd_texture.h): texel -> triangle and three integer-ratio weights
    render_texture        the texels' rays generated inside the eval chunk loop (EvalRenderer.render_texels: nsamd_texel_rays into
                          the schedule's static inputs, the chunk, nsamd_texture_store of its rgb rows); the ray length from
                          nsamd_mesh_raylen; the result a `[H,W,3]` uint8 image on the device
    write_png             8-bit RGB PNG with zlib and struct alone
    write_textured_obj    the reference's OBJ / MTL lines, formatted in bulk
    export_textured_mesh  the reference's function, signature and defaults; unwrap_method="custom" needs nothing of nerfstudio,
                          "xatlas" takes the reference's unwrap and renders its bundle — with its own nears and fars — through
                          the model

The 8-bit level of a colour is this project's rule (floor(clamp(v, 0, 1) * 255 + 0.5), NaN -> 0): the reference writes through
mediapy, which was not available to compare with. This module imports nothing of nerfstudio at module level. There is no torch
fallback: a model the eval runner does not cover raises NotImplementedError.
"""
from __future__ import annotations

import math
import struct
import sys
import zlib
from dataclasses import dataclass
from pathlib import Path
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _native as N
from . import eval_frame
from . import functional as F

MTL_LINES = ("# Generated with nerfstudio", "newmtl material_0", "Ka 1.000 1.000 1.000", "Kd 1.000 1.000 1.000",
             "Ks 0.000 0.000 0.000", "d 1.0", "illum 2", "Ns 1.00000000", "map_Kd material_0.png")  # texture_utils.py:414-424
OBJ_HEAD = ("# Generated with nerfstudio", "mtllib material_0.mtl", "usemtl material_0")  # :431


@dataclass(frozen=True)
class TexelAtlas:
    """The per-UV-triangle atlas of F faces at P texels per triangle side: two faces per square of (P + 3) x P texels,
    squares_w x squares_h squares (texture_utils.py:101-109)."""

    faces: int
    px: int
    squares_w: int
    squares_h: int

    @staticmethod
    def for_faces(num_faces: int, px_per_uv_triangle: int) -> "TexelAtlas":
        F_, P = int(num_faces), int(px_per_uv_triangle)
        if F_ < 1:
            raise ValueError(f"TexelAtlas: a mesh with {F_} faces has no texture")
        if P < 2:
            raise ValueError(f"TexelAtlas: px_per_uv_triangle must be at least 2, got {P} (at 1 a triangle has no area in the atlas)")
        nsq = (F_ + 1) // 2
        sw = math.isqrt(nsq - 1) + 1  # ceil(sqrt(nsq))
        sh = (nsq + sw - 1) // sw
        return TexelAtlas(F_, P, sw, sh)

    @property
    def width(self) -> int:
        return self.squares_w * (self.px + 3)

    @property
    def height(self) -> int:
        return self.squares_h * self.px

    def native(self) -> "N.TexelAtlasPod":
        return N.make_texel_atlas(self.faces, self.px, self.squares_w, self.squares_h)

    def texture_coordinates(self) -> Tensor:
        """`[F,3,2]` fp32 on the host: the corners of face t on texel centres of square ((t div 2) mod sw, (t div 2) div sw), formed
        in float64 and rounded once."""
        P = self.px
        t = np.arange(self.faces, dtype=np.int64)
        q = t // 2
        su, sv = (q % self.squares_w)[:, None], (q // self.squares_w)[:, None]
        upper = np.array([[0, 0], [P - 1, 0], [0, P - 1]], dtype=np.int64)
        lower = np.array([[P + 2, P - 1], [3, P - 1], [P + 2, 0]], dtype=np.int64)
        offs = np.where((t % 2 == 1)[:, None, None], lower[None], upper[None])  # [F,3,2]
        u = (su * (P + 3) + offs[..., 0] + 0.5) / float(self.width)
        v = (sv * P + offs[..., 1] + 0.5) / float(self.height)
        return torch.from_numpy(np.stack([u, v], axis=-1).astype(np.float32))


def refusal(model) -> Optional[str]:
    """None, or why `render_texture` cannot render this model's texels."""
    if hasattr(model, "occupancy_grid"):
        return "an instant-ngp model: its ray marcher takes no per-ray near and far"
    return eval_frame.export_support(model)[1]


@torch.no_grad()
def render_texture(model, mesh, px_per_uv_triangle: int, raylen_method: str = "edge", out_f32: Optional[Tensor] = None) -> Tensor:
    """-> `[H,W,3]` uint8 on the mesh's device: the texture of `mesh` (vertices, normals `[V,3]`, faces `[F,3]`) over
    TexelAtlas.for_faces(F, px_per_uv_triangle), every texel one ray through `model` in eval mode. The faces are validated
    against V once (one read of two numbers); the kernels clamp regardless. out_f32 `[H W, 3]`: the unquantised rgb (tests)."""
    if raylen_method not in ("edge", "none"):
        raise ValueError(f"Ray length method {raylen_method} not supported.")  # texture_utils.py:382
    reason = refusal(model)
    if reason is not None:
        raise NotImplementedError(f"render_texture: {reason}; there is no torch fallback")
    vertices = mesh.vertices.detach().to(torch.float32).contiguous()
    normals = mesh.normals.detach().to(torch.float32).contiguous()
    faces = mesh.faces.detach().to(torch.int32).contiguous()
    V = int(vertices.shape[0])
    if tuple(normals.shape) != (V, 3) or tuple(vertices.shape) != (V, 3):
        raise ValueError("Number of vertices and vertex normals must be equal")  # :98
    atlas = TexelAtlas.for_faces(int(faces.shape[0]), px_per_uv_triangle)
    lo, hi = (int(x) for x in torch.stack(torch.aminmax(faces)).tolist())
    if lo < 0 or hi >= V:
        raise ValueError(f"render_texture: the faces index vertices {lo} .. {hi}, the mesh has {V}")
    dev = vertices.device
    with eval_frame.eval_mode(model):
        runner, reason = eval_frame.export_runner_for(model, dev)
        if runner is None:
            N.require_cuda(vertices)
            raise RuntimeError(f"render_texture: {reason}")
        raylen_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        if raylen_method == "edge":
            scratch = torch.empty(N.RAYLEN_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
            F.mesh_raylen_launch(vertices, faces, scratch, raylen_dev)
        image = torch.empty((atlas.height, atlas.width, 3), dtype=torch.uint8, device=dev)
        runner.render_texels(atlas, SimpleNamespace(vertices=vertices, normals=normals, faces=faces), raylen_dev, image, out_f32)
    return image


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(filename, image) -> None:
    """`image` `[H,W,3]` uint8 (tensor or array) as an 8-bit RGB PNG, every row with filter 0, one IDAT chunk."""
    if isinstance(image, Tensor):
        image = image.detach().cpu().numpy()
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"write_png takes [H,W,3] uint8, got {image.dtype} {tuple(image.shape)}")
    H, W = int(image.shape[0]), int(image.shape[1])
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)  # column 0: the filter type
    rows[:, 1:] = image.reshape(H, 3 * W)
    with open(filename, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)))
        f.write(_png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(_png_chunk(b"IEND", b""))


def write_textured_obj(output_dir, vertices, normals, faces, texture_coordinates) -> None:
    """`mesh.obj` and `material_0.mtl` in output_dir as texture_utils.py:412-481 lays them out: every `v`, then per face its
    three `vt u 1-v`, every `vn`, then `f a/t/a b/t/b c/t/c` 1-based with the vt indices 3i+1 .. 3i+3. Numbers carry nine
    significant digits (an fp32 reads back exactly); the lines are formatted array by array."""
    out = Path(output_dir)
    as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, Tensor) else np.asarray(t)  # noqa: E731
    v, vn = as_np(vertices).astype(np.float64), as_np(normals).astype(np.float64)
    fc = as_np(faces).astype(np.int64)
    tc = as_np(texture_coordinates).astype(np.float64).reshape(-1, 2)
    if tc.shape[0] != 3 * fc.shape[0]:
        raise ValueError(f"{fc.shape[0]} faces need {3 * fc.shape[0]} texture coordinates, got {tc.shape[0]}")
    with open(out / "material_0.mtl", "w", encoding="utf-8") as f:
        f.writelines(line + "\n" for line in MTL_LINES)
    vt = np.stack([tc[:, 0], 1.0 - tc[:, 1]], axis=1)
    i = np.arange(fc.shape[0], dtype=np.int64)[:, None]
    corners = np.empty((fc.shape[0], 9), dtype=np.int64)
    for c in range(3):
        corners[:, 3 * c] = corners[:, 3 * c + 2] = fc[:, c] + 1
        corners[:, 3 * c + 1] = 3 * i[:, 0] + c + 1
    with open(out / "mesh.obj", "w", encoding="utf-8") as f:
        f.writelines(line + "\n" for line in OBJ_HEAD)
        np.savetxt(f, v, fmt="v %.9g %.9g %.9g")
        np.savetxt(f, vt, fmt="vt %.9g %.9g")
        np.savetxt(f, vn, fmt="vn %.9g %.9g %.9g")
        np.savetxt(f, corners, fmt="f %d/%d/%d %d/%d/%d %d/%d/%d")


def _import_xatlas_unwrap():
    try:
        from nerfstudio.exporter.texture_utils import unwrap_mesh_with_xatlas
    except ImportError as e:
        raise ImportError("nerfstudio_amd.texture: unwrap_method=\"xatlas\" is the reference's own unwrap "
                          "(nerfstudio.exporter.texture_utils.unwrap_mesh_with_xatlas: xatlas, mediapy); install nerfstudio with "
                          f"its export dependencies, or pass unwrap_method=\"custom\", which needs none of them ({e})") from e
    return unwrap_mesh_with_xatlas


@torch.no_grad()
def _render_bundle_texture(model, vertices: Tensor, faces: Tensor, origins: Tensor, directions: Tensor, raylen_method: str) -> Tensor:
    """texture_utils.py:374-406 for texel rays somebody else unwrapped: the bundle carries nears = 0 and fars = raylen, and
    get_outputs_for_camera_ray_bundle honours them. -> `[H,W,3]` uint8."""
    from .cameras.rays import RayBundle

    dev = origins.device
    raylen = torch.zeros(1, dtype=torch.float32, device=dev)
    if raylen_method == "edge":
        scratch = torch.empty(N.RAYLEN_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
        F.mesh_raylen_launch(vertices, faces, scratch, raylen)
    origins = origins - 0.5 * raylen * directions
    one = torch.ones_like(origins[..., 0:1])
    bundle = RayBundle(origins=origins, directions=directions, pixel_area=one, camera_indices=torch.zeros_like(one),
                       nears=torch.zeros_like(one), fars=one * raylen, metadata={"directions_norm": one})
    with eval_frame.eval_mode(model):
        rgb = model.get_outputs_for_camera_ray_bundle(bundle)["rgb"][..., :3]
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    image = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    F.texture_store_launch(rgb.reshape(-1, 3).to(torch.float32).contiguous(), H * W, 0, image)
    return image


def export_textured_mesh(mesh, pipeline, output_dir: Path, px_per_uv_triangle: Optional[int], unwrap_method: str = "xatlas",
                         raylen_method: str = "edge", num_pixels_per_side=1024) -> None:
    """texture_utils.export_textured_mesh (:322-493), its arguments and defaults: `mesh.obj`, `material_0.mtl` and
    `material_0.png` in output_dir, on the pipeline's device. "custom" is `render_texture` — no unwrap tensors, no bundle;
    "xatlas" imports the reference's unwrap lazily (its ImportError names "custom")."""
    if unwrap_method not in ("xatlas", "custom"):
        raise ValueError(f"Unwrap method {unwrap_method} not supported.")
    if raylen_method not in ("edge", "none"):
        raise ValueError(f"Ray length method {raylen_method} not supported.")
    device = pipeline.device
    out = Path(output_dir)
    vertices = mesh.vertices.to(device=device, dtype=torch.float32).contiguous()
    normals = mesh.normals.to(device=device, dtype=torch.float32).contiguous()
    faces = mesh.faces.to(device=device, dtype=torch.int32).contiguous()
    if unwrap_method == "custom":
        assert px_per_uv_triangle is not None
        image = render_texture(pipeline.model, SimpleNamespace(vertices=vertices, normals=normals, faces=faces), px_per_uv_triangle,
                               raylen_method)
        texture_coordinates = TexelAtlas.for_faces(int(faces.shape[0]), px_per_uv_triangle).texture_coordinates()
    else:
        unwrap = _import_xatlas_unwrap()
        texture_coordinates, origins, directions = unwrap(vertices, faces.long(), normals, num_pixels_per_side=num_pixels_per_side)
        image = _render_bundle_texture(pipeline.model, vertices, faces, origins.float(), directions.float(), raylen_method)
    out.mkdir(parents=True, exist_ok=True)
    write_png(out / "material_0.png", image)
    write_textured_obj(out, vertices, normals, faces, texture_coordinates)
    print(f"[nerfstudio_amd.texture] {int(vertices.shape[0])} vertices, {int(faces.shape[0])} faces unwrapped with the "
          f"{unwrap_method} method; texture {int(image.shape[1])}x{int(image.shape[0])} (WxH); OBJ, MTL and PNG in {out}", file=sys.stderr)
