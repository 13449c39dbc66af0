"""Evaluation of a model of this package over a set of cameras: the models' get_image_metrics_and_images (models/nerfacto.py:393-431,
instant_ngp.py:239-273, vanilla_nerf.py:218-264, mipnerf.py:163-213) and the body of VanillaPipeline.get_average_image_metrics
(pipelines/base_pipeline.py:346-418), with PSNR and SSIM taken on the device (image_metrics.ImageMetrics) and the depth and
accumulation images coloured there (utils.colormaps). No torchmetrics, torchvision or mediapy: the numbers are the kernels', the
PNGs are texture.write_png's.

A frame's metrics are four floats on the device; `image_metrics_and_images` reads them once per call (the reference returns
Python floats), `average_image_metrics` once per set, after its loop."""
from __future__ import annotations

import time
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import eval_frame
from . import functional as F
from . import image_metrics as im
from .utils import colormaps


def _metrics(model) -> im.ImageMetrics:
    """the model's own ImageMetrics (its scratch), made on first use; SSIM's range from the two images, PSNR's 1.0"""
    if getattr(model, "_image_metrics", None) is None:
        model._image_metrics = im.ImageMetrics(data_range=None, psnr_range=1.0)
    return model._image_metrics


def _lpips(model):
    """the model's LPIPS callable, or None: the network's weights are not part of this package"""
    fn = getattr(model, "lpips", None)
    return fn if callable(fn) else None


def _nchw(image: Tensor) -> Tensor:
    return torch.moveaxis(image, -1, 0)[None, ...]


def two_pass(outputs: Dict[str, Tensor]) -> bool:
    """a coarse / fine model's outputs (vanilla NeRF, mip-NeRF)"""
    return "rgb_fine" in outputs


def frame_images(model, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]) -> Tuple[Tensor, Dict[str, Tensor], Dict[str, Tensor]]:
    """(the ground truth over the model's background, {"": rgb} or {"coarse": .., "fine": ..}: the predictions the metrics take,
    the reference's images_dict) of one frame; nothing is read back. `prop_depth_i` for the keys the outputs hold."""
    if two_pass(outputs):
        image = model.renderer_rgb.blend_background(batch["image"].to(outputs["rgb_coarse"].device))
        near, far = float(model.config.near_plane), float(model.config.far_plane)
        acc = [colormaps.apply_colormap(outputs[f"accumulation_{p}"]) for p in ("coarse", "fine")]
        depth = [colormaps.apply_depth_colormap(outputs[f"depth_{p}"], accumulation=outputs[f"accumulation_{p}"], near_plane=near,
                                                far_plane=far) for p in ("coarse", "fine")]
        images = {"img": torch.cat([image, outputs["rgb_coarse"], outputs["rgb_fine"]], dim=1), "accumulation": torch.cat(acc, dim=1),
                  "depth": torch.cat(depth, dim=1)}
        preds = {"coarse": outputs["rgb_coarse"], "fine": outputs["rgb_fine"]}
        if getattr(model, "clip_rgb_for_metrics", False):  # mip-NeRF (models/mipnerf.py:196-197)
            preds = {k: torch.clip(v, min=0, max=1) for k, v in preds.items()}
        return image, preds, images
    device = outputs["rgb"].device
    image = model.renderer_rgb.blend_background(batch["image"].to(device))
    acc = colormaps.apply_colormap(outputs["accumulation"])
    depth = colormaps.apply_depth_colormap(outputs["depth"], accumulation=outputs["accumulation"])
    images = {"img": torch.cat([image, outputs["rgb"]], dim=1), "accumulation": acc, "depth": depth}
    i = 0
    while f"prop_depth_{i}" in outputs:
        images[f"prop_depth_{i}"] = colormaps.apply_depth_colormap(outputs[f"prop_depth_{i}"], accumulation=outputs["accumulation"])
        i += 1
    return image, {"": outputs["rgb"]}, images


def read_rows(rows: Tensor) -> List[List[float]]:
    """THE host read of a metrics buffer `[N, 4]`"""
    return rows.detach().cpu().tolist()


def image_metrics_and_images(model, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]) -> Tuple[Dict[str, float], Dict[str, Tensor]]:
    """Model.get_image_metrics_and_images with the reference's keys and image layout: Python floats (one host read of the frame's
    rows), `[H, W', 3]` images. "lpips" / "fine_lpips" only when the model has a callable `lpips`."""
    image, preds, images = frame_images(model, outputs, batch)
    rows = torch.empty(len(preds), 4, dtype=torch.float32, device=image.device)
    for row, pred in zip(rows, preds.values()):
        _metrics(model).measure_into(image, pred, row)
    values = read_rows(rows)
    lpips = _lpips(model)
    if two_pass(outputs):
        coarse, fine = values
        metrics = {"psnr": fine[im.PSNR], "coarse_psnr": coarse[im.PSNR], "fine_psnr": fine[im.PSNR], "fine_ssim": fine[im.SSIM]}
        if lpips is not None:
            metrics["fine_lpips"] = float(lpips(_nchw(image), _nchw(preds["fine"])))
    else:
        metrics = {"psnr": values[0][im.PSNR], "ssim": values[0][im.SSIM]}
        if lpips is not None:
            metrics["lpips"] = float(lpips(_nchw(image), _nchw(preds[""])))
    return metrics, images


def image_u8(image: Tensor) -> Tensor:
    """an `[H, W, 3]` fp32 image as the uint8 levels a PNG holds (nsamd_texture.h's 8-bit rule), on the image's device"""
    image = image.detach().float().contiguous()
    out = torch.empty(image.shape, dtype=torch.uint8, device=image.device)
    F.texture_store_launch(image.view(-1, 3), image.numel() // 3, 0, out)
    return out


class _FrameClock:
    """a frame's time from an event pair on the frame's stream (read after the loop); the host clock where there is no device"""

    def __init__(self, device) -> None:
        self.events = torch.device(device).type == "cuda"
        self.pairs: list = []

    def start(self):
        if not self.events:
            return time.perf_counter()
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stop(self, started) -> None:
        self.pairs.append((started, self.start()))

    def seconds(self) -> List[float]:
        return [1e-3 * a.elapsed_time(b) if self.events else b - a for a, b in self.pairs]


@torch.no_grad()
def average_image_metrics(model, frames, image_prefix: str = "eval", output_path: Optional[Path] = None, get_std: bool = False) -> Dict[str, float]:
    """The averages of VanillaPipeline.get_average_image_metrics over `frames`, a sequence of (camera, batch): "psnr", "ssim"
    ("fine_ssim" and the two-pass models' other keys), "num_rays_per_sec", "fps", with their "_std" when get_std. Every frame's
    metrics go into one `[N, rows, 4]` device buffer that is read ONCE, after the loop, with the frames' event times; with an
    output_path every image of the frame is written as `<image_prefix>_<key>_<idx:04d>.png` from its 8-bit levels taken on the
    device. The frame is the model's own get_outputs_for_camera (eval_frame.outputs_for_camera for this package's models: the runner,
    or the module chunk loop for a frame it declines and for the two-pass models). "lpips" as image_metrics_and_images has it (a host read per frame: the callable's)."""
    frames = list(frames)
    if not frames:
        raise ValueError("average_image_metrics needs at least one (camera, batch)")
    if output_path is not None:
        output_path = Path(output_path)
        output_path.mkdir(exist_ok=True, parents=True)
    from .texture import write_png

    device = getattr(model, "device", None)  # (nerfstudio's Model has the property; this package's own models do not)
    rows, rays, extra = None, [], []
    clock = _FrameClock(device if device is not None else next(model.parameters()).device)
    lpips = _lpips(model)
    with eval_frame.eval_mode(model):
        for idx, (camera, batch) in enumerate(frames):
            started = clock.start()
            outputs = model.get_outputs_for_camera(camera)  # its runner, or, where that declines, the module chunk loop
            image, preds, images = frame_images(model, outputs, batch)
            if rows is None:
                rows = torch.empty(len(frames), len(preds), 4, dtype=torch.float32, device=image.device)
            for row, pred in zip(rows[idx], preds.values()):
                _metrics(model).measure_into(image, pred, row)
            if lpips is not None:
                extra.append(float(lpips(_nchw(image), _nchw(list(preds.values())[-1]))))
            if output_path is not None:
                for key, img in images.items():
                    write_png(output_path / f"{image_prefix}_{key}_{idx:04d}.png", image_u8(img))
            clock.stop(started)
            rays.append(int(image.shape[0]) * int(image.shape[1]))
    values = read_rows(rows.view(-1, 4))
    seconds = clock.seconds()
    n_rows = rows.shape[1]
    per_frame: List[Dict[str, float]] = []
    for idx in range(len(frames)):
        v = values[idx * n_rows:(idx + 1) * n_rows]
        if n_rows == 2:
            d = {"psnr": v[1][im.PSNR], "coarse_psnr": v[0][im.PSNR], "fine_psnr": v[1][im.PSNR], "fine_ssim": v[1][im.SSIM]}
        else:
            d = {"psnr": v[0][im.PSNR], "ssim": v[0][im.SSIM]}
        if lpips is not None:
            d["fine_lpips" if n_rows == 2 else "lpips"] = extra[idx]
        d["num_rays_per_sec"] = rays[idx] / seconds[idx]
        d["fps"] = d["num_rays_per_sec"] / rays[idx]
        per_frame.append(d)
    out: Dict[str, float] = {}
    for key in per_frame[0]:
        column = torch.tensor([d[key] for d in per_frame])
        if get_std:
            std, mean = torch.std_mean(column)
            out[key], out[f"{key}_std"] = float(mean), float(std)
        else:
            out[key] = float(torch.mean(column))
    return out
