"""What surrounds the two device-side eval chunk loops (eval_render.EvalRenderer, ngp_eval_render.NgpEvalRenderer), once: reading
a `Cameras` object, the `render_camera` prologue, a frame's output buffers, the eval appearance row, the gate in front of the
runners, the models' "which path renders this camera / this bundle" and the exporters' choice of a runner. Host code only: the
chunk loops stay in their modules (one replays a captured graph over padded static buffers, the other is eager and sliced).
"""
import contextlib
import os
from collections import namedtuple
from typing import Dict, Optional

import torch
from torch import Tensor

from . import functional as F

PERSPECTIVE = 1  # CameraType.PERSPECTIVE (cameras/cameras.py:41-52)
RUNNER_OFF = "the device-side eval renderer is switched off (NSAMD_EVAL_RUNNER=0)"
# c2w [3, 4]; camera_type: CameraType's value, PERSPECTIVE without the attribute; distortion: distortion_params as a tensor, or None
CameraView = namedtuple("CameraView", "c2w fx fy cx cy height width camera_type distortion")


def read_camera(camera) -> Optional[CameraView]:
    """A single `Cameras` object (cameras/cameras.py) as a CameraView, or None for several cameras and missing intrinsics."""
    try:
        c2w = camera.camera_to_worlds
        if c2w.dim() == 3:
            if c2w.shape[0] != 1:
                return None
            c2w = c2w[0]
        ctype = getattr(camera, "camera_type", None)
        ctype = PERSPECTIVE if ctype is None else int(torch.as_tensor(ctype).reshape(-1)[0])
        dist = getattr(camera, "distortion_params", None)
        dist = None if dist is None else torch.as_tensor(dist)
        one = lambda t: float(torch.as_tensor(t).reshape(-1)[0])  # noqa: E731
        h, w = int(one(camera.height)), int(one(camera.width))
        if h <= 0 or w <= 0 or torch.as_tensor(camera.fx).numel() != 1:
            return None
        return CameraView(c2w[:3, :4], one(camera.fx), one(camera.fy), one(camera.cx), one(camera.cy), h, w, ctype, dist)
    except (AttributeError, TypeError, ValueError, IndexError):
        return None


def pinhole_camera_args(camera):
    """(c2w [3,4], fx, fy, cx, cy, H, W) of a single perspective `Cameras` object whose distortion parameters, however many, are
    all zero or absent; None for a camera that needs the general ray generator (another type, distortion, several cameras)."""
    view = read_camera(camera)
    if view is None or view.camera_type != PERSPECTIVE or (view.distortion is not None and bool(torch.any(view.distortion != 0))):
        return None
    return view[:7]


def lens_camera_args(camera):
    """`pinhole_camera_args`' tuple plus (camera_type, distortion `[6]` or None) for a single `Cameras` object of a type in
    F.LENS_TYPES; None for several cameras, missing intrinsics, other types and a distortion that is not six wide."""
    view = read_camera(camera)
    if view is None or view.camera_type not in F.LENS_TYPES:
        return None
    dist = None if view.distortion is None else view.distortion.float().reshape(-1)
    return None if dist is not None and dist.numel() != 6 else (*view[:8], dist)


def in_loop_camera_args(camera):
    """(render_camera's positional arguments, its `lens`) for the cameras Model.get_outputs_for_camera renders without a ray
    bundle: one undistorted pinhole camera (lens None), or one perspective camera with non-zero distortion. None otherwise:
    fisheye and equirectangular cameras take `camera.generate_rays` there (`render_camera(lens=...)` covers them all the same)."""
    args = pinhole_camera_args(camera)
    if args is not None:
        return args, None
    args = lens_camera_args(camera)
    if args is not None and args[7] == PERSPECTIVE:
        return args[:7], (args[7], args[8])
    return None


def prepare_view(c2w: Tensor, lens, device):
    """`render_camera`'s pose and lens as the ray generators take them: c2w `[3, 4]` fp32 on `device`; lens None, or
    (camera_type of F.LENS_TYPES, distortion `[6]` fp32 on `device` or None)."""
    c2w = c2w.reshape(3, 4).to(device=device, dtype=torch.float32).contiguous()
    if lens is not None:
        camera_type, dist = int(lens[0]), lens[1]
        if camera_type not in F.LENS_TYPES:
            raise ValueError(f"render_camera: camera type {camera_type} is not one of {sorted(F.LENS_TYPES)}")
        if dist is not None:
            dist = torch.as_tensor(dist).reshape(6).to(device=device, dtype=torch.float32).contiguous()
        lens = (camera_type, dist)
    return c2w, lens


def frame_outputs(total: int, device, channels: Dict[str, tuple]) -> Dict[str, Tensor]:
    """The frame's `[total, C]` output buffers from {name: (C, dtype)} (dtype None: the default one)."""
    return {name: torch.empty((total, c), device=device, dtype=dtype) for name, (c, dtype) in channels.items()}


def as_image(out: Dict[str, Tensor], shape) -> Dict[str, Tensor]:
    """The finished `[total, C]` outputs as `[*shape, C]`: a bundle's image_shape, or (H, W)."""
    return {name: v.view(*shape, -1) for name, v in out.items()}


def padded_loader(buffers, arrays, n: int):
    """load(a, k) for a chunk loop over static `[n, ...]` buffers: rows a .. a + k - 1 of every array into the first k rows of
    its buffer, and a short chunk (k < n) padded with copies of its last row."""
    def load(a: int, k: int) -> None:
        for buf, arr in zip(buffers, arrays):
            buf[:k].copy_(arr[a:a + k])
        if k < n:
            for buf, arr in zip(buffers, arrays):
                buf[k:].copy_(arr[a + k - 1:a + k].expand(n - k, *arr.shape[1:]))
    return load


def eval_appearance_row(fld, app_const: Optional[Tensor]) -> None:
    """Eval mode's appearance row (fields/nerfacto_field.py:253-261) into its buffer (None: no embedding): the mean, or zeros."""
    if app_const is not None and fld.use_average_appearance_embedding:
        torch.mean(fld.embedding_appearance.embedding.weight.detach(), dim=0, out=app_const)
    elif app_const is not None:
        app_const.zero_()


@contextlib.contextmanager
def eval_mode(model):
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def runner_enabled(model, device) -> bool:
    """The first condition of both `runner_for`: eval mode, rays on a GPU, NSAMD_EVAL_RUNNER not 0."""
    return not model.training and torch.device(device).type == "cuda" and os.environ.get("NSAMD_EVAL_RUNNER", "1") == "1"


def predicts_normals(model) -> bool:
    """Such a nerfacto model renders through the runner with the normals stages."""
    return bool(getattr(model.config, "predict_normals", False))


def export_support(model):
    """(the module whose runner renders this model for an exporter, None): ngp_eval_render for a model its `supported` accepts,
    else eval_render — or (None, why that one refuses)."""
    from . import eval_render, ngp_eval_render

    if ngp_eval_render.supported(model) is None:
        return ngp_eval_render, None
    reason = eval_render.supported(model, normals=predicts_normals(model))
    return (eval_render, None) if reason is None else (None, f"the eval renderer does not cover this model ({reason})")


def export_runner_for(model, device):
    """(the model's runner for an export on `device`, None), or (None, reason): `export_support`'s, or RUNNER_OFF."""
    module, reason = export_support(model)
    runner = module.runner_for(model, device) if module is not None else None
    return runner, (None if runner is not None else reason or RUNNER_OFF)


def outputs_for_camera(model, camera, obb_box, runner_fn, fallback=None):
    """Model.get_outputs_for_camera (models/base_model.py:166-175): a camera `in_loop_camera_args` accepts, without a crop box,
    through `runner.render_camera` when `runner_fn(model, the model's device)` — the model's own gate — hands out a runner;
    anything else is `fallback(camera, obb_box=obb_box)`, the reference's method, or without one that method's body: the camera's
    `[H, W]` bundle through get_outputs_for_camera_ray_bundle. A crop box is not read as a camera; a refused camera asks for no runner."""
    args = in_loop_camera_args(camera) if obb_box is None else None
    if args is not None:
        dev = getattr(model, "device", None)  # (nerfstudio's Model has the property; this package's own models do not)
        runner = runner_fn(model, dev if dev is not None else next(model.parameters()).device)
        if runner is not None:
            return runner.render_camera(*args[0], lens=args[1])
    if fallback is not None:
        return fallback(camera, obb_box=obb_box)
    return model.get_outputs_for_camera_ray_bundle(camera.generate_rays(camera_indices=0, keep_shape=True, obb_box=obb_box))


def outputs_for_bundle(model, bundle, runner_fn, fallback=None):
    """Model.get_outputs_for_camera_ray_bundle (models/base_model.py:178-205): `runner.render` when `runner_fn(model, the rays'
    device)` hands out a runner, else `fallback(bundle)`, the reference's loop, or without one `module_chunk_loop`."""
    runner = runner_fn(model, bundle.origins.device)
    if runner is not None:
        return runner.render(bundle)
    return fallback(bundle) if fallback is not None else module_chunk_loop(model, bundle)


def module_chunk_loop(model, bundle) -> Dict[str, Tensor]:
    """The reference's Python chunk loop (models/base_model.py:178-205) over `forward`, its tensor outputs shaped as the image."""
    image_shape, chunk = bundle.origins.shape[:-1], model.config.eval_num_rays_per_chunk
    outs: Dict[str, list] = {}
    for i in range(0, len(bundle), chunk):
        for k, v in model.forward(bundle.get_row_major_sliced_ray_bundle(i, i + chunk)).items():
            if torch.is_tensor(v):
                outs.setdefault(k, []).append(v)
    return {k: torch.cat(v).view(*image_shape, -1) for k, v in outs.items()}
