"""PSNR and SSIM of an evaluation frame on the device (include/nsamd_image.h: THE METRICS): what the reference gets from
torchmetrics' PeakSignalNoiseRatio(data_range=1.0) and structural_similarity_index_measure, by one tiled HIP kernel and a
finishing launch, with no host read until the caller asks for the numbers.

Images are `[H, W, C]` fp32, channel-last, as the eval runners return them; `structural_similarity_index_measure` takes the
library's `[B, C, H, W]` and can be assigned wherever the reference assigns the library's function. There is no torch fallback:
a CPU tensor is an error (nerfstudio_amd._native.require_cuda)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _native as N
from . import functional as F

MSE, PSNR, SSIM, RANGE = 0, 1, 2, 3  # the columns of a result


def _check(pred: Tensor, target: Tensor) -> None:
    if pred.dim() != 3 or tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"expected two [H, W, C] images of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    H, W, C = pred.shape
    if H < N.SSIM_WINDOW or W < N.SSIM_WINDOW:
        raise ValueError(f"SSIM's {N.SSIM_WINDOW} x {N.SSIM_WINDOW} window needs an image of at least that size, got {H} x {W}")
    if not 1 <= C <= 4:
        raise ValueError(f"1 to 4 channels are supported, got {C}")


class ImageMetrics:
    """Owns the scratch of the metrics launches for frames up to the largest size it has seen (grown on demand, never in a
    captured region: call once before capturing)."""

    def __init__(self, data_range: Optional[float] = None, psnr_range: float = 1.0) -> None:
        self.data_range, self.psnr_range = data_range, float(psnr_range)
        self.scratch: Optional[Tensor] = None
        self.ranges: Optional[Tensor] = None

    def _buffers(self, pred: Tensor) -> None:
        H, W, C = pred.shape
        need = 2 * N.RANGE_SCRATCH_BYTES + F.image_metrics_scratch_bytes(H, W, C)
        if self.scratch is None or self.scratch.device != pred.device or self.scratch.numel() < need:
            self.scratch = torch.empty(need, dtype=torch.uint8, device=pred.device)
            self.ranges = torch.empty(2, 2, dtype=torch.float32, device=pred.device)

    def measure_into(self, pred: Tensor, target: Tensor, row: Tensor, ssim_map: Optional[Tensor] = None,
                     ranges: Optional[Tensor] = None) -> Tensor:
        """{mse, psnr, ssim, R} of pred against target into `row` (`[4]` fp32: row i of an `[N, 4]` buffer); no synchronisation.
        ranges: `[2, 2]` fp32 {min, max} of pred and of target where the caller has them (a batch's); else taken here."""
        pred, target = pred.detach().float().contiguous(), target.detach().float().contiguous()
        _check(pred, target)
        self._buffers(pred)
        metrics_scratch = self.scratch[2 * N.RANGE_SCRATCH_BYTES:]
        if self.data_range is None:
            if ranges is None:
                ranges = self.ranges
                F.image_range_launch(pred, self.scratch, ranges[0])
                F.image_range_launch(target, self.scratch[N.RANGE_SCRATCH_BYTES:], ranges[1])
            F.image_metrics_launch(pred, target, ranges[0], ranges[1], 0.0, self.psnr_range, metrics_scratch, row, ssim_map)
        else:
            F.image_metrics_launch(pred, target, None, None, float(self.data_range), self.psnr_range, metrics_scratch, row, ssim_map)
        return row

    def measure(self, pred: Tensor, target: Tensor) -> Tensor:
        """a fresh `[4]` device tensor {mse, psnr, ssim, R}; no synchronisation"""
        return self.measure_into(pred, target, torch.empty(4, dtype=torch.float32, device=pred.device))


def psnr(pred: Tensor, target: Tensor, data_range: float = 1.0) -> Tensor:
    """PeakSignalNoiseRatio(data_range)(pred, target) of two `[H, W, C]` images: a 0-dim device tensor. A convenience: it runs
    the whole metrics launch (SSIM with a data range of 1 included) and keeps one of its four results."""
    return ImageMetrics(data_range=1.0, psnr_range=data_range).measure(pred, target)[PSNR]


def ssim(pred: Tensor, target: Tensor, data_range: Optional[float] = None, return_map: bool = False):
    """SSIM of two `[H, W, C]` images: a 0-dim device tensor, with the `[H-10, W-10, C]` per-window values when asked for"""
    _check(pred, target)
    H, W, C = pred.shape
    ssim_map = torch.empty(H - 10, W - 10, C, dtype=torch.float32, device=pred.device) if return_map else None
    out = ImageMetrics(data_range=data_range).measure_into(pred, target, torch.empty(4, dtype=torch.float32, device=pred.device), ssim_map)
    return (out[SSIM], ssim_map) if return_map else out[SSIM]


def structural_similarity_index_measure(preds: Tensor, target: Tensor, data_range: Optional[float] = None) -> Tensor:
    """torchmetrics.functional.structural_similarity_index_measure with nerfstudio's defaults for `[B, C, H, W]` inputs: the mean
    over the batch of every image's SSIM. Without a data_range the library takes ONE range over the whole batch; so does this."""
    if preds.dim() != 4 or tuple(preds.shape) != tuple(target.shape):
        raise ValueError(f"expected two [B, C, H, W] batches of one shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    measure = ImageMetrics(data_range=data_range)
    rows = torch.empty(preds.shape[0], 4, dtype=torch.float32, device=preds.device)
    ranges = None
    if data_range is None:
        ranges = torch.stack((F.image_range(preds.detach().float()), F.image_range(target.detach().float())))
    for b in range(preds.shape[0]):
        measure.measure_into(preds[b].permute(1, 2, 0), target[b].permute(1, 2, 0), rows[b], ranges=ranges)
    return rows[:, SSIM].mean()
