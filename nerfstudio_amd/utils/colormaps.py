"""Colormaps of the evaluation images on the device: the functions of the reference's utils/colormaps.py with its signatures and
defaults, over nsamd_colormap (include/nsamd_image.h: THE COLORMAP, pinned bit for bit to the reference's CPU results in
tests/golden/colormaps.npz). The minimum and maximum a map needs — a depth map's near and far, normalize — come from
nsamd_image_range and stay on the device: no float(...) read, no assert read. Where the reference asserts on values outside
[0, 1] (apply_float_colormap), the kernel clips.

Every function also takes `lut=`, a `[256, 3]` fp32 table, in place of the name: matplotlib is then never imported."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from .. import functional as F

COLORMAP_NAMES = ("default", "turbo", "viridis", "magma", "inferno", "cividis", "gray", "pca")  # "default" is turbo
Colormaps = str  # one of COLORMAP_NAMES, or any other name matplotlib knows a 256-row table for
WHITE = torch.tensor([1.0, 1.0, 1.0])
BLACK = torch.tensor([0.0, 0.0, 0.0])
_LUTS: Dict[Tuple[str, str], Tensor] = {}


@dataclass(frozen=True)
class ColormapOptions:
    """How a one-channel image becomes colours; field names and defaults are the reference's (utils/colormaps.py:30-43).
    colormap: the table's name; normalize: stretch the image's minimum .. maximum to 0 .. 1 first; colormap_min / colormap_max:
    the values 0 and 1 are mapped to before the clip to [0, 1]; invert: read the table from its far end."""

    colormap: Colormaps = "default"
    normalize: bool = False
    colormap_min: float = 0
    colormap_max: float = 1
    invert: bool = False


def colormap_lut(colormap: str, device) -> Optional[Tensor]:
    """The `[256, 3]` fp32 table of a named colormap on `device` (None for "gray"), from matplotlib on first use, cached per
    device. "default" is turbo."""
    if colormap == "default":
        colormap = "turbo"
    if colormap == "gray":
        return None
    if colormap == "pca":
        raise NotImplementedError('the "pca" colormap (apply_pca_colormap) is not implemented on the device')
    key = (colormap, str(torch.device(device)))
    if key not in _LUTS:
        import matplotlib  # lazily, as the reference's callers meet it

        table = torch.tensor(matplotlib.colormaps[colormap].colors, dtype=torch.float32)
        assert tuple(table.shape) == (256, 3)
        _LUTS[key] = table.to(device)
    return _LUTS[key]


def set_colormap_lut(colormap: str, table: Tensor, device) -> None:
    """Give a named colormap its `[256, 3]` table on `device` (a process without matplotlib; a table of one's own)."""
    if tuple(table.shape) != (256, 3):
        raise ValueError(f"a colormap table is [256, 3], got {tuple(table.shape)}")
    table = table.to(device=device, dtype=torch.float32).contiguous()
    _LUTS[("turbo" if colormap == "default" else colormap, str(table.device))] = table  # ("cuda" lands on "cuda:0")


def _table(colormap: str, lut: Optional[Tensor], device) -> Optional[Tensor]:
    if lut is not None:
        return lut.to(device=device, dtype=torch.float32).contiguous()
    return colormap_lut(colormap, device)


def _one_channel(image: Tensor, what: str) -> None:
    if image.shape[-1] != 1 or not torch.is_floating_point(image):
        raise ValueError(f"{what} takes a one-channel floating-point image [..., 1], got {tuple(image.shape)} {image.dtype}")


def apply_colormap(image: Tensor, colormap_options: ColormapOptions = ColormapOptions(), eps: float = 1e-9,
                   lut: Optional[Tensor] = None) -> Tensor:
    """A 3-channel image is returned as it is, a one-channel float image goes through the colormap (normalize, the min / max
    window, invert as the options say), a bool image through apply_boolean_colormap. More than 3 channels — the reference's PCA
    map — is not implemented. eps is the reference's 1e-9: the kernel's constant."""
    if image.shape[-1] == 3:
        return image
    if image.shape[-1] == 1 and torch.is_floating_point(image):
        if eps != 1e-9:
            raise NotImplementedError("eps other than the reference's default 1e-9 is not implemented")
        o = colormap_options
        params = N.make_colormap_params(False, o.normalize, o.colormap_min, o.colormap_max, o.invert)
        return F.colormap(image.detach().float(), _table(o.colormap, lut, image.device), params)
    if image.dtype == torch.bool:
        return apply_boolean_colormap(image)
    if image.shape[-1] > 3:
        raise NotImplementedError(f"an image of {image.shape[-1]} channels takes the reference's PCA colormap (apply_pca_colormap), "
                                  "which is not implemented on the device")
    raise NotImplementedError


def apply_float_colormap(image: Tensor, colormap: Colormaps = "viridis", lut: Optional[Tensor] = None) -> Tensor:
    """The table's row (image * 255) truncated for every pixel of a one-channel image in [0, 1], a NaN read as 0; "gray" has
    no table and repeats the value three times."""
    _one_channel(image, "apply_float_colormap")
    return F.colormap(image.detach().float(), _table(colormap, lut, image.device), N.make_colormap_params())


def apply_depth_colormap(depth: Tensor, accumulation: Optional[Tensor] = None, near_plane: Optional[float] = None,
                         far_plane: Optional[float] = None, colormap_options: ColormapOptions = ColormapOptions(),
                         lut: Optional[Tensor] = None) -> Tensor:
    """A depth map's picture: (depth - near) / (far - near + 1e-10) clipped to [0, 1] goes through apply_colormap, and an
    accumulation, where given, blends the result towards white. near_plane / far_plane None: the image's minimum / maximum, taken on the device."""
    _one_channel(depth, "apply_depth_colormap")
    o = colormap_options
    params = N.make_colormap_params(True, o.normalize, o.colormap_min, o.colormap_max, o.invert, near_plane, far_plane)
    acc = None if accumulation is None else accumulation.detach().float()
    return F.colormap(depth.detach().float(), _table(o.colormap, lut, depth.device), params, accumulation=acc)


def apply_boolean_colormap(image: Tensor, true_color: Tensor = WHITE, false_color: Tensor = BLACK) -> Tensor:
    """`[..., 3]`: true_color where the one channel is set, false_color elsewhere (one torch.where)."""
    t, f = true_color.to(image.device), false_color.to(image.device)
    return torch.where(image[..., :1], t, f)
