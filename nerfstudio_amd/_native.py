"""ctypes binding of libnsamd.so — the C-ABI boundary declared in include/nsamd.h.

This is the ONLY place the product touches native code. It never falls back: if the shared library is missing or a
kernel reports an error a RuntimeError is raised (the reference's tcnn seam silently falls back to torch,
field_components/encodings.py:350-352 — a `implementation="hip"` request must not).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnsamd.so")

MAX_LEVELS = 32
XFORM_NONE, XFORM_CONTRACT, XFORM_AABB = 0, 1, 2
BG_NONE, BG_LAST_SAMPLE, BG_CONSTANT = 0, 1, 2

vp = C.c_void_p
i64 = C.c_int64
i32 = C.c_int32
f32 = C.c_float


class Grid(C.Structure):
    _fields_ = [("num_levels", i32), ("log2_table_size", i32), ("scalings", f32 * MAX_LEVELS)]


class Points(C.Structure):
    _fields_ = [("positions", vp), ("origins", vp), ("directions", vp), ("t_bins", vp), ("samples_per_ray", i32)]


class Aabb(C.Structure):
    _fields_ = [("lo", f32 * 3), ("hi", f32 * 3)]


class DensityMlp(C.Structure):
    _fields_ = [("W0", vp), ("b0", vp), ("W1", vp), ("b1", vp), ("in_dim", i32), ("hidden", i32),
                ("average_init_density", f32)]


class FieldMlp(C.Structure):
    _fields_ = [("base_W0", vp), ("base_b0", vp), ("base_W1", vp), ("base_b1", vp), ("head_W0", vp), ("head_b0", vp),
                ("head_W1", vp), ("head_b1", vp), ("head_W2", vp), ("head_b2", vp), ("appearance", vp),
                ("num_images", i32), ("average_init_density", f32), ("ray_terms", vp), ("ray_inputs", vp),
                ("saved_hb", vp), ("saved_rgb", vp), ("batch_slot", vp), ("batch_slots", i32)]


class OccGrid(C.Structure):
    _fields_ = [("binaries", vp), ("levels", i32), ("resolution", i32), ("aabb", f32 * 6), ("coarse", vp)]


class RayGrads(C.Structure):
    _fields_ = [("d_origins", vp * 4), ("d_directions", vp * 4), ("count", i32)]


class FieldMlpGrads(C.Structure):
    _fields_ = [("base_W0", vp), ("base_b0", vp), ("base_W1", vp), ("base_b1", vp), ("head_W0", vp), ("head_b0", vp),
                ("head_W1", vp), ("head_b1", vp), ("head_W2", vp), ("head_b2", vp), ("appearance", vp)]


class TsdfVolume(C.Structure):
    _fields_ = [("origin", f32 * 3), ("voxel_size", f32 * 3), ("dims", i32 * 3), ("truncation", f32)]


class CropBox(C.Structure):
    """nsamd_crop_box (include/nsamd_pointcloud.h): world2box = rows of the 3x4 inverse of [R T; 0 1], half_scale = S / 2."""
    _fields_ = [("enabled", i32), ("world2box", f32 * 12), ("half_scale", f32 * 3)]


class PointGrid(C.Structure):
    """nsamd_point_grid: the uniform grid of the neighbour search."""
    _fields_ = [("origin", f32 * 3), ("cell_size", f32), ("dims", i32 * 3)]


class MeshVolume(C.Structure):
    """nsamd_mesh_volume (include/nsamd_mesh.h): the volume the mesh is extracted from."""
    _fields_ = [("origin", f32 * 3), ("voxel_size", f32 * 3), ("dims", i32 * 3)]


class TexelAtlasPod(C.Structure):
    """nsamd_texel_atlas (include/nsamd_texture.h): the layout of the per-UV-triangle atlas."""
    _fields_ = [("faces", i32), ("px", i32), ("squares_w", i32), ("squares_h", i32)]


class ColormapParams(C.Structure):
    """nsamd_colormap_params (include/nsamd_image.h): mode, options and fixed planes of one colormap launch."""
    _fields_ = [("mode", i32), ("normalize", i32), ("invert", i32), ("fixed", i32), ("colormap_min", C.c_double),
                ("colormap_max", C.c_double), ("near_plane", C.c_double), ("far_plane", C.c_double)]


class ProposalLevelBwd(C.Structure):
    """nsamd_proposal_level_bwd: one proposal level's gated backward chain (nsamd_proposal_levels_bwd)."""
    _fields_ = [("num_rays", i64), ("samples_per_ray", i32),
                ("t_bins", vp), ("density", vp), ("dweights", vp), ("ddensity", vp), ("gate", vp), ("ray_mask", vp),
                ("enc", vp), ("selector", vp), ("pre", vp), ("mlp", DensityMlp), ("denc", vp),
                ("dW0", vp), ("db0", vp), ("dW1", vp), ("db1", vp), ("mlp_workspace", vp), ("mlp_workspace_floats", i64),
                ("origins", vp), ("directions", vp), ("transform", C.c_int), ("aabb", Aabb), ("table", vp), ("grid", Grid),
                ("dtable", vp), ("scatter_workspace", vp), ("scatter_workspace_floats", i64)]


# name -> argtypes (restype is int unless listed in _RESTYPES). Mirrors include/nsamd.h one to one; the CPU test
# tests/test_abi.py checks that every symbol declared in the header is exported by the library and listed here.
_SIGNATURES = {
    "nsamd_hashgrid_encode_fwd": [Points, i64, C.c_int, Aabb, vp, Grid, vp, i64, i64, vp, vp],
    "nsamd_hashgrid_encode_bwd": [Points, i64, C.c_int, Aabb, vp, Grid, vp, i64, i64, vp, vp, vp, i64, vp],
    "nsamd_hashgrid_encode_bwd_set": [Points, i64, C.c_int, Aabb, vp, Grid, vp, i64, i64, vp, vp, vp, i64, vp],
    "nsamd_hashgrid_encode_bwd_rays": [Points, i64, C.c_int, Aabb, vp, Grid, vp, i64, i64, vp, vp, C.c_int, vp],
    "nsamd_hashgrid_encode_bwd_gated": [Points, i64, C.c_int, Aabb, vp, Grid, vp, i64, i64, vp, vp, i64, vp, vp, vp],
    "nsamd_hashgrid_encode_bwd_rays_gated": [Points, i64, C.c_int, Aabb, vp, Grid, vp, i64, i64, vp, vp, C.c_int, vp, vp, vp],
    "nsamd_hashgrid_encode_bwd_workspace": [Grid, i64, C.c_int],
    "nsamd_hashgrid_encode_bwd_workspace_state": [Grid, i64],
    "nsamd_hashgrid_scatter_events": [vp, vp, vp],
    "nsamd_sh4_encode": [vp, i64, vp, vp],
    "nsamd_nerf_encode": [Points, i64, vp, i32, i32, vp, vp],
    "nsamd_nerf_encode_bwd_rays": [Points, i64, vp, i32, i32, vp, i64, vp, vp, C.c_int, vp],
    "nsamd_ipe_encode": [Points, i64, vp, vp, vp, i32, i32, vp, vp],
    "nsamd_contract_linf": [vp, i64, vp, vp],
    "nsamd_density_mlp_fwd": [vp, vp, i64, DensityMlp, vp, vp, vp],
    "nsamd_density_field_fwd": [Points, i64, C.c_int, Aabb, vp, Grid, DensityMlp, vp, vp, vp, vp, vp],
    "nsamd_density_mlp_bwd": [vp, vp, vp, vp, i64, DensityMlp, vp, vp, vp, vp, vp, vp, i64, vp],
    "nsamd_density_mlp_bwd_gated": [vp, vp, vp, vp, i64, DensityMlp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp],
    "nsamd_field_mlp_fwd": [vp, vp, vp, vp, vp, i64, i64, FieldMlp, vp, vp, vp],
    "nsamd_field_mlp_bwd": [vp, vp, vp, vp, vp, i64, i64, FieldMlp, vp, vp, vp, FieldMlpGrads, vp, i64, vp],
    "nsamd_field_ray_terms": [vp, vp, vp, i64, FieldMlp, vp, vp, vp],
    "nsamd_field_mlp_bwd_scatter": [Points, C.c_int, Aabb, Grid, vp, vp, vp, vp, vp, i64, i64, FieldMlp, vp, vp, vp, FieldMlpGrads, vp,
                                    i64, vp, vp, i64, vp],
    "nsamd_field_mlp_bwd_scatter_phase": [Points, C.c_int, Aabb, Grid, vp, vp, vp, vp, vp, i64, i64, FieldMlp, vp, vp, vp, FieldMlpGrads,
                                          vp, i64, vp, vp, i64, C.c_int, vp],
    "nsamd_field_mlp_bwd_scatter_workspace": [Grid, i64, C.POINTER(C.c_int64)],
    "nsamd_proposal_levels_bwd": [C.POINTER(ProposalLevelBwd), i32, i32, vp],
    "nsamd_field_normals": [Points, i64, C.c_int, Aabb, vp, Grid, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp],
    "nsamd_normals_composite": [vp, vp, vp, i64, i32, vp, vp, vp],
    "nsamd_normals_losses": [vp, vp, vp, vp, i64, i32, f32, f32, vp, vp, vp, vp, i32, vp],
    "nsamd_linear_fwd": [vp, vp, vp, i64, i32, i32, C.c_int, vp, vp],
    "nsamd_linear_bwd": [vp, vp, vp, vp, i64, i32, i32, C.c_int, vp, vp, vp, vp],
    "nsamd_piecewise_bins": [vp, vp, vp, vp, i32, i64, i32, C.c_int, vp, vp, vp],
    "nsamd_weights_fwd": [vp, vp, i64, i32, vp, vp],
    "nsamd_weights_bwd": [vp, vp, vp, i64, i32, vp, vp],
    "nsamd_weights_bwd_gate": [vp, vp, vp, i64, i32, vp, vp, vp, i32, vp],
    "nsamd_pdf_resample": [vp, vp, i32, vp, vp, vp, vp, f32, vp, f32, f32, f32, C.c_int, i32, i32, i64, i32, vp, vp, vp, vp],
    "nsamd_proposal_resample": [vp, vp, vp, i32, vp, vp, vp, vp, f32, vp, f32, f32, f32, C.c_int, i64, i32, vp, vp, vp, vp, vp],
    "nsamd_composite_fwd": [vp, vp, vp, i64, i32, C.c_int, C.POINTER(f32), C.c_int, vp, vp, vp, vp, vp, vp, vp],
    "nsamd_render_train": [vp, vp, vp, i64, i32, C.c_int, C.POINTER(f32), vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "nsamd_render_train_bwd": [vp, vp, vp, vp, i64, i32, C.c_int, C.POINTER(f32), vp, vp, vp, vp, vp, vp],
    "nsamd_composite_bwd": [vp, vp, vp, i64, i32, C.c_int, C.POINTER(f32), vp, vp, vp, vp, vp, vp, vp, vp],
    "nsamd_distance_gradient_scale": [vp, i64, i32, vp, vp, vp],
    "nsamd_mse_loss": [vp, vp, i64, f32, vp, vp, vp],
    "nsamd_interlevel_loss": [vp, vp, i32, vp, vp, i32, i64, f32, vp, vp, vp],
    "nsamd_distortion_loss": [vp, vp, i32, i64, f32, vp, vp, vp],
    "nsamd_proposal_losses": [vp, vp, i32, i32, vp, vp, vp, i64, f32, f32, vp, vp, vp, vp, vp],
    "nsamd_depth_loss": [i32, vp, vp, vp, i64, vp, vp, vp, f32, i32, f32, i32, vp, vp, vp, vp],
    "nsamd_train_loss_values": [vp, vp, i32, vp, i64, i32, f32, f32, vp, vp],
    "nsamd_occgrid_march_count_stash": [vp, vp, vp, vp, i64, f32, f32, OccGrid, f32, f32, vp, vp, vp, i32, vp],
    "nsamd_occgrid_march_write_stashed": [vp, vp, vp, vp, i64, f32, f32, OccGrid, f32, f32, vp, vp, vp, i32, vp, vp, vp, vp],
    "nsamd_occgrid_coarse_words": [i32, i32],
    "nsamd_occgrid_cell_positions": [vp, i64, OccGrid, vp, vp, vp],
    "nsamd_occgrid_update": [vp, i64, vp, vp, i64, f32, vp, vp],
    "nsamd_occgrid_binarise": [vp, i32, i32, f32, vp, vp, vp, vp, vp],
    "nsamd_packed_info": [vp, i64, vp, vp, vp],
    "nsamd_packed_weights_fwd": [vp, vp, vp, vp, i64, vp, vp, vp],
    "nsamd_packed_weights_bwd": [vp, vp, vp, vp, vp, i64, vp, vp],
    "nsamd_packed_visibility": [vp, vp, vp, vp, i64, f32, f32, vp, vp, vp],
    "nsamd_packed_compact": [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp],
    "nsamd_packed_composite_fwd": [vp, vp, vp, vp, vp, i64, C.c_int, C.POINTER(f32), C.c_int, vp, vp, vp, vp],
    "nsamd_packed_composite_bwd": [vp, vp, vp, i64, C.c_int, C.POINTER(f32), vp, vp, vp, vp, vp],
    "nsamd_packed_positions": [vp, vp, vp, vp, vp, i64, vp, vp],
    "nsamd_raygen_pinhole": [vp, vp, vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp],
    "nsamd_raygen_pinhole_grid": [vp, f32, f32, f32, f32, i32, i64, i64, i64, vp, vp, vp, vp],
    "nsamd_raygen_lens": [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp],
    "nsamd_raygen_lens_grid": [vp, f32, f32, f32, f32, i32, vp, i32, i64, i64, i64, vp, vp, vp, vp],
    "nsamd_rows_gather": [vp, vp, i64, i32, vp, vp],
    "nsamd_rows_scatter": [vp, vp, i64, i32, vp, vp],
    "nsamd_select_batch": [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "nsamd_sample_batch": [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, C.c_uint64, i32, i64, vp, vp, vp, vp, vp, vp,
                           vp, vp, vp],
    "nsamd_select_bins": [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, C.c_int, vp, vp, vp],
    "nsamd_step_prologue": [vp, vp, i32, vp, vp, i64, vp, i64, C.c_uint64, vp],
    "nsamd_camera_apply": [vp, i32, i32, vp, vp, vp, i64, vp, vp, vp],
    "nsamd_camera_backward": [vp, i32, i32, vp, vp, i64, RayGrads, f32, f32, vp, vp, vp],
    "nsamd_adam_step": [vp, vp, vp, vp, i64, C.c_double, C.c_double, C.c_double, C.c_double, i32, f32, vp, vp],
    "nsamd_version": [],
    "nsamd_status_string": [C.c_int],
    "nsamd_device_info": [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.c_char_p, i32],
    "nsamd_probe_mfma16": [vp, vp, vp, vp],
    "nsamd_probe_mfma_bf16": [vp, vp, vp, vp],
}
# The same for include/nsamd_export.h, the mesh-export part of the ABI (tests/test_tsdf_cpu.py checks header, library and binding).
_EXPORT_SIGNATURES = {
    "nsamd_tsdf_integrate": [TsdfVolume, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, vp],
}
# And for include/nsamd_render.h, the eval render of the packed path (tests/test_ngp_eval_render_cpu.py checks the three).
_RENDER_SIGNATURES = {
    "nsamd_packed_render_fwd": [vp, vp, vp, vp, vp, i64, C.c_int, C.POINTER(f32), C.c_int, vp, vp, vp, vp, vp, vp],
    "nsamd_packed_ray_points": [vp, vp, vp, vp, vp, i64, vp, vp, vp],
}
# And for include/nsamd_pointcloud.h, point-cloud export (tests/test_pointcloud_cpu.py checks the three).
_POINTCLOUD_SIGNATURES = {
    "nsamd_points_select": [vp, vp, vp, vp, vp, vp, i64, CropBox, vp, vp, vp, vp, i64, vp, vp, vp],
    "nsamd_select_below": [vp, i64, vp, vp, vp, vp, vp],
    "nsamd_point_cell_keys": [vp, i64, PointGrid, vp, vp],
    "nsamd_knn_mean_distance": [vp, i64, vp, vp, PointGrid, i32, i32, vp, vp, vp],
}
# And for include/nsamd_mesh.h, the mesh extraction of mesh export (tests/test_mesh_cpu.py checks the three).
_MESH_SIGNATURES = {
    "nsamd_mesh_count": [MeshVolume, vp, vp, vp, vp],
    "nsamd_mesh_emit": [MeshVolume, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp],
}
# And for include/nsamd_texture.h, the texturing of an exported mesh (tests/test_texture_cpu.py checks the three).
_TEXTURE_SIGNATURES = {
    "nsamd_texel_rays": [TexelAtlasPod, vp, vp, vp, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp],
    "nsamd_mesh_raylen": [vp, i64, vp, i64, vp, vp, vp],
    "nsamd_texture_store": [vp, i64, i64, vp, vp],
}
# And for include/nsamd_image.h, the eval image metrics and colormaps (tests/test_image_metrics_cpu.py checks the three).
_IMAGE_SIGNATURES = {
    "nsamd_image_range": [vp, i64, vp, vp, vp],
    "nsamd_image_metrics_scratch_bytes": [i64, i64, i32],
    "nsamd_image_metrics": [vp, vp, i64, i64, i32, vp, vp, f32, f32, vp, vp, vp, vp],
    "nsamd_colormap": [vp, i64, vp, vp, vp, ColormapParams, vp, vp, vp],
}
SELECT_BLOCK = 256  # NSAMD_SELECT_BLOCK
MESH_BLOCK = 256  # NSAMD_MESH_BLOCK
RAYLEN_SCRATCH_BYTES = 8 * 1024  # NSAMD_RAYLEN_SCRATCH_BYTES
RANGE_SCRATCH_BYTES = 8 * 1024  # NSAMD_RANGE_SCRATCH_BYTES
SSIM_TILE = 32  # NSAMD_SSIM_TILE
SSIM_WINDOW = 11  # NSAMD_SSIM_WINDOW
COLORMAP_PLAIN, COLORMAP_DEPTH = 0, 1  # NSAMD_COLORMAP_PLAIN, NSAMD_COLORMAP_DEPTH
KNN_MAX_K = 32  # NSAMD_KNN_MAX_K
KNN_MAX_CELLS = 1 << 24  # NSAMD_KNN_MAX_CELLS
_RESTYPES = {"nsamd_version": C.c_char_p, "nsamd_status_string": C.c_char_p,
             "nsamd_hashgrid_encode_bwd_workspace": C.c_int64, "nsamd_hashgrid_encode_bwd_workspace_state": C.c_int64,
             "nsamd_field_mlp_bwd_scatter_workspace": C.c_int64,
             "nsamd_occgrid_coarse_words": C.c_int64, "nsamd_image_metrics_scratch_bytes": C.c_int64}

_lib = None
ERR_UNSUPPORTED = -2  # nsamd_status NSAMD_ERR_UNSUPPORTED

# Optional live kernel timing (bench.py's `roofline` leg): when PROFILE is a dict, every launch through the binding is
# bracketed by a pair of HIP events recorded on torch's current stream — the stream the kernels are enqueued on.
PROFILE: Optional[dict] = None


class _Entry:
    """One C-ABI entry point; transparently records (start, end) events per call when profiling is enabled."""

    __slots__ = ("fn", "name")

    def __init__(self, fn, name):
        self.fn, self.name = fn, name

    def __call__(self, *args):
        prof = PROFILE
        if prof is None:
            return self.fn(*args)
        key = self.name
        if self.name == "nsamd_density_field_fwd":
            key = f"{self.name}[M={args[1]}]"
        elif self.name.startswith("nsamd_hashgrid_encode"):
            key = f"{self.name}[L={args[5].num_levels},M={args[1]}]"
        elif self.name.startswith("nsamd_density_mlp"):
            key = f"{self.name}[M={args[2] if self.name.endswith('fwd') else args[4]}]"
        elif self.name == "nsamd_field_mlp_bwd_scatter_phase":
            key = f"{self.name}[{ {1: 'gradients+records', 2: 'dw_reduce', 4: 'apply'}.get(args[21], args[21]) }]"
        elif self.name == "nsamd_adam_step":
            key = f"{self.name}[n={args[4]}]"
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        r = self.fn(*args)
        e1.record()
        prof.setdefault(key, []).append((e0, e1))
        return r


class _Lib:
    pass


def load():
    """Load libnsamd.so (once). Raises RuntimeError when it has not been built — there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("NSAMD_LIB", LIB_PATH)  # (a probe / instrumented build of the same sources, scripts/probe_*)
    if not os.path.exists(path):
        raise RuntimeError(
            f"nerfstudio_amd: native library not found at {path}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C nerfstudio_amd/csrc`). "
            "There is no CPU/torch fallback for implementation='hip'."
        )
    cdll = C.CDLL(path)
    lib = _Lib()
    lib.cdll = cdll
    for name, argtypes in {**_SIGNATURES, **_EXPORT_SIGNATURES, **_RENDER_SIGNATURES, **_POINTCLOUD_SIGNATURES,
                           **_MESH_SIGNATURES, **_TEXTURE_SIGNATURES, **_IMAGE_SIGNATURES}.items():
        fn = getattr(cdll, name)  # AttributeError here = header / library mismatch
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, C.c_int)
        setattr(lib, name, _Entry(fn, name) if fn.restype is C.c_int and name not in ("nsamd_device_info",) else fn)
    _lib = lib
    return lib


def profile_summary(prof: dict) -> dict:
    """{key: (calls, total_ms, mean_ms)} from recorded event pairs (call after a device synchronise)."""
    out = {}
    for key, pairs in prof.items():
        ms = [a.elapsed_time(b) for a, b in pairs]
        out[key] = (len(ms), float(sum(ms)), float(sum(ms) / max(1, len(ms))))
    return out


def status_string(status: int) -> str:
    return load().nsamd_status_string(status).decode()


def check(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"nsamd: {what} failed with status {status}: {status_string(status)}")


def ptr(t: Optional[torch.Tensor]):
    """Device pointer of a tensor (None -> NULL). The tensor must be contiguous; callers keep it alive."""
    if t is None:
        return None
    assert t.is_contiguous(), "nsamd kernels take dense row-major tensors"
    return t.data_ptr()


def ptr_array(tensors):
    """Host array of the device pointers of `tensors` (None -> NULL), for the entry points that take one pointer per level."""
    return (vp * len(tensors))(*[ptr(t) for t in tensors])


# torch.cuda.current_stream() / `with torch.cuda.stream(s)` with no device argument resolve "the current device" through
# torch._utils._get_available_device_type -> torch.cuda.is_available() -> a device-count query of the driver: ~20 us per call on
# this ROCm build, 14 - 16 of them per eagerly launched iteration = a third of the host's share of an eager / data-parallel step
# (profiles/r06_s30_eager_host_cprofile.txt: 3170 x _cuda_getDeviceCount in 225 iterations). The helpers below name the device.
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # (private torch entry points: the public route is the fallback)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


if _RAW_STREAM is None or _GET_DEVICE is None:
    def stream() -> int:
        return torch.cuda.current_stream().cuda_stream
else:
    def stream() -> int:
        """The raw hipStream_t of torch's current stream (kernels must run on it, SURVEY.md §8b threading)."""
        return _RAW_STREAM(_GET_DEVICE())


def current_stream() -> "torch.cuda.Stream":
    """torch.cuda.current_stream() of the current device, without the device-count query."""
    if _GET_DEVICE is None:
        return torch.cuda.current_stream()
    return torch.cuda.current_stream(_GET_DEVICE())


class on_stream:
    """`with on_stream(s):` — torch.cuda.stream(s) for a stream of the CURRENT device, without the two device-count queries."""

    __slots__ = ("s", "prev")

    def __init__(self, s) -> None:
        self.s = s

    def __enter__(self):
        self.prev = current_stream()
        torch.cuda.set_stream(self.s)
        return self.s

    def __exit__(self, *exc):
        torch.cuda.set_stream(self.prev)
        return False


def require_cuda(*tensors: Optional[torch.Tensor]) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "nerfstudio_amd: implementation='hip' runs on an MI355X only; got a CPU tensor "
                "(there is no CPU fallback — use the reference's implementation='torch' for CPU runs)."
            )


def make_grid(num_levels: int, log2_table_size: int, scalings) -> Grid:
    if num_levels > MAX_LEVELS:
        raise ValueError(f"at most {MAX_LEVELS} hash levels are supported, got {num_levels}")
    g = Grid()
    g.num_levels = int(num_levels)
    g.log2_table_size = int(log2_table_size)
    for i, s in enumerate(scalings):
        g.scalings[i] = float(s)
    return g


def make_points(positions=None, origins=None, directions=None, t_bins=None, samples_per_ray: int = 0) -> Points:
    p = Points()
    p.positions = ptr(positions)
    p.origins = ptr(origins)
    p.directions = ptr(directions)
    p.t_bins = ptr(t_bins)
    p.samples_per_ray = int(samples_per_ray)
    return p


def make_aabb(aabb: Optional[torch.Tensor]) -> Aabb:
    a = Aabb()
    if aabb is not None:
        vals = aabb.detach().cpu().reshape(2, 3).tolist()
        for i in range(3):
            a.lo[i] = vals[0][i]
            a.hi[i] = vals[1][i]
    return a


def select_scratch_words(n: int) -> int:
    """NSAMD_SELECT_SCRATCH_WORDS(n): int64 words of scratch the two selection entry points need for n entries."""
    return 1 + ((n + SELECT_BLOCK - 1) // SELECT_BLOCK + 1) // 2


def make_crop_box(world2box=None, half_scale=None) -> CropBox:
    """world2box: 12 host floats (rows of the 3x4 matrix), half_scale: 3; None: the box is disabled."""
    b = CropBox()
    if world2box is not None:
        b.enabled = 1
        for i, v in enumerate(world2box):
            b.world2box[i] = float(v)
        for i, v in enumerate(half_scale):
            b.half_scale[i] = float(v)
    return b


def make_point_grid(origin, cell_size: float, dims) -> PointGrid:
    g = PointGrid()
    for i in range(3):
        g.origin[i], g.dims[i] = float(origin[i]), int(dims[i])
    g.cell_size = float(cell_size)
    return g


def mesh_scratch_bytes(n: int) -> int:
    """NSAMD_MESH_SCRATCH_BYTES(n): bytes of scratch the two mesh entry points need for a volume of n voxels."""
    return 16 + 8 * ((n + MESH_BLOCK - 1) // MESH_BLOCK) + 4 * n


def make_mesh_volume(origin, voxel_size, dims) -> MeshVolume:
    v = MeshVolume()
    for i in range(3):
        v.origin[i], v.voxel_size[i], v.dims[i] = float(origin[i]), float(voxel_size[i]), int(dims[i])
    return v


def make_texel_atlas(faces: int, px: int, squares_w: int, squares_h: int) -> TexelAtlasPod:
    a = TexelAtlasPod()
    a.faces, a.px, a.squares_w, a.squares_h = int(faces), int(px), int(squares_w), int(squares_h)
    return a


def make_colormap_params(depth: bool = False, normalize: bool = False, colormap_min: float = 0.0, colormap_max: float = 1.0,
                         invert: bool = False, near_plane: Optional[float] = None, far_plane: Optional[float] = None) -> ColormapParams:
    p = ColormapParams()
    p.mode, p.normalize, p.invert = (COLORMAP_DEPTH if depth else COLORMAP_PLAIN), int(bool(normalize)), int(bool(invert))
    p.fixed = (1 if near_plane is not None else 0) | (2 if far_plane is not None else 0)
    p.colormap_min, p.colormap_max = float(colormap_min), float(colormap_max)
    p.near_plane, p.far_plane = float(near_plane or 0.0), float(far_plane or 0.0)
    return p


def device_info() -> dict:
    lib = load()
    cus, wf, lds = i32(), i32(), i32()
    name = C.create_string_buffer(64)
    check(lib.nsamd_device_info(C.byref(cus), C.byref(wf), C.byref(lds), name, 64), "nsamd_device_info")
    return {"num_cus": cus.value, "wavefront_size": wf.value, "lds_bytes_per_cu": lds.value, "arch": name.value.decode()}
