"""Training batches sampled on the device: the images of a dataset kept in HBM as uint8 and ONE launch per step
(`nsamd_sample_batch`, csrc/batch.hip) that draws the pixels, gathers their colours and generates their rays — what the
reference's datamanager does on the host every iteration (data/datamanagers/base_datamanager.py:506-515:
`PixelSampler.sample`, data/pixel_samplers.py:137-174 and :265-318, on the CPU; the colour gather `image[c.cpu(), y.cpu(),
x.cpu()]`, :305-309; `RayGenerator`, model_components/ray_generators.py:41-56).

    DeviceImageStore    images [N,H,W,3] uint8 (+ mask [N,H,W] uint8) and the cameras' records on the device
    DeviceBatchSource   the launch over a store: `launch` into caller-owned buffers (trainer.HipTrainer captures it as a node
                        of the iteration), `next_batch` as a drop-in for `datamanager.next_train`

The draws are counter based (Philox keyed by the seed, counter = (ray, attempt, draw)): the batch of draw k is a function of
(seed, k) alone, the same whether the launch is issued eagerly or replayed from a hipGraph. The sampling law is the
reference's default one — uniform over (image, row, col), with lane-local rejection against a mask; everything that takes
another law or another layout is DECLINED by `DeviceImageStore.from_dataset` with a reason that names it.

This module imports nothing of nerfstudio: it reads a dataset through `len`, `get_data(i, image_type="uint8")` and `cameras`.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple, Union

import torch

PERSPECTIVE, FISHEYE, EQUIRECTANGULAR = 1, 2, 3  # CameraType values (cameras/cameras.py:41-52) the ray arithmetic covers
MAX_ATTEMPTS = 100  # PixelSamplerConfig.max_num_iterations (pixel_samplers.py:51)
DEFAULT_MAX_BYTES = 16 << 30  # of the 288 GB of an MI355X; 100 images of 800 x 800 are 192 MB
_MASK64 = 0xFFFFFFFFFFFFFFFF


def mix_seed(seed: int, rank: int = 0) -> int:
    """The 64-bit seed of a rank's streams — trainer.HipTrainer's `rng_seed` recipe: ranks that share torch's seed still draw
    different pixels (the reference: one generator per process)."""
    return ((int(seed) + 0x632BE59BD9B4E019 * int(rank)) * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D) & _MASK64


class DeviceImageStore:
    """The training images and cameras of one dataset on the device. `nbytes`: images + mask (the cameras are 100 B each)."""

    def __init__(self, images, mask, c2w, fx, fy, cx, cy, camera_type, distortion) -> None:
        assert images.dtype == torch.uint8 and images.dim() == 4 and images.shape[-1] == 3
        self.images = images.contiguous()
        self.num_images, self.height, self.width = (int(s) for s in images.shape[:3])
        self.mask = None if mask is None else mask.reshape(self.num_images, self.height, self.width).to(torch.uint8).contiguous()
        dev, n = images.device, self.num_images
        f32 = dict(device=dev, dtype=torch.float32)
        self.c2w = c2w.reshape(n, 3, 4).to(**f32).contiguous()
        self.fx, self.fy, self.cx, self.cy = (t.reshape(n).to(**f32).contiguous() for t in (fx, fy, cx, cy))
        self.camera_type = camera_type.reshape(n).to(device=dev, dtype=torch.int32).contiguous()
        self.distortion = None if distortion is None else distortion.reshape(n, 6).to(**f32).contiguous()
        self.device = dev

    @property
    def nbytes(self) -> int:
        return self.images.numel() + (self.mask.numel() if self.mask is not None else 0)

    @staticmethod
    def bytes_needed(num_images: int, height: int, width: int, masked: bool = False) -> int:
        return num_images * height * width * (4 if masked else 3)

    @classmethod
    def from_dataset(cls, dataset, device, max_bytes: int = DEFAULT_MAX_BYTES, patch_size: int = 1) -> Union["DeviceImageStore", str]:
        """-> the store, or the reason (a string that names the declined case) why this dataset keeps the host datamanager.
        Images and masks come from the reference's own uint8 cache type (`get_data(i, image_type="uint8")`,
        data/datasets/base_dataset.py:116-165: `alpha_color` already composited), the cameras from `dataset.cameras`."""
        if patch_size > 1:
            return f"patch_size {patch_size} > 1 (the patch pixel sampler draws blocks of pixels, pixel_samplers.py:424-512)"
        cams = dataset.cameras
        n = len(dataset)
        if n <= 0:
            return "an empty dataset"
        types = cams.camera_type.reshape(-1).to(torch.int64).cpu()
        if types.numel() != n:
            return f"{types.numel()} cameras for {n} images"
        for t in torch.unique(types).tolist():
            if t not in (PERSPECTIVE, FISHEYE, EQUIRECTANGULAR):
                return f"camera type {t} (outside perspective / fisheye / equirectangular)"
        if bool((types == EQUIRECTANGULAR).all()):
            return "every camera is equirectangular (sample_method_equirectangular draws uniformly on the sphere, pixel_samplers.py:176-204)"
        meta = getattr(cams, "metadata", None) or {}
        if meta.get("fisheye_crop_radius", None) is not None:
            return "fisheye_crop_radius (sample_method_fisheye draws inside the crop circle, pixel_samplers.py:206-263)"
        ds_meta = getattr(dataset, "metadata", None) or {}
        if hasattr(dataset, "depth_filenames") or "depth_filenames" in ds_meta:
            return "a depth dataset (the batch would need depth_image)"
        first = dataset.get_data(0, image_type="uint8")
        if "depth_image" in first:
            return "a depth dataset (the batch would need depth_image)"
        h, w = (int(s) for s in first["image"].shape[:2])
        masked = "mask" in first
        need = cls.bytes_needed(n, h, w, masked)
        if need > max_bytes:
            return f"a store of {need} bytes ({n} images of {h} x {w}) exceeds max_bytes = {max_bytes}"
        images = torch.empty((n, h, w, 3), dtype=torch.uint8)
        mask = torch.empty((n, h, w), dtype=torch.uint8) if masked else None
        for i in range(n):
            data = first if i == 0 else dataset.get_data(i, image_type="uint8")
            image = data["image"]
            if tuple(image.shape[:2]) != (h, w):
                return f"images of different sizes ({h} x {w} and {int(image.shape[0])} x {int(image.shape[1])})"
            if image.shape[-1] == 4:
                return "four-channel images that remain RGBA (no alpha_color to composite them over)"
            if image.dtype != torch.uint8 or image.shape[-1] != 3:
                return f"images of dtype {image.dtype} with {int(image.shape[-1])} channels (uint8 RGB expected)"
            images[i] = image
            if masked:
                if "mask" not in data:
                    return "masks on some images only"
                mask[i] = data["mask"].reshape(h, w) != 0
        dist = getattr(cams, "distortion_params", None)
        return cls(images.to(device), None if mask is None else mask.to(device), cams.camera_to_worlds, cams.fx, cams.fy, cams.cx,
                   cams.cy, types, dist)


def native_launch(store: DeviceImageStore, num_rays: int, seed: int, max_attempts: int, draw_counter, draw_offset: int, origins,
                  directions, camera_indices, target, pixel_area=None, directions_norm=None, indices=None, failed=None) -> None:
    """nsamd_sample_batch on torch's current stream. No fallback: a missing library or a refused launch raises."""
    from . import _native as N

    N.require_cuda(store.images, origins, directions, camera_indices, target, draw_counter)
    N.check(N.load().nsamd_sample_batch(
        N.ptr(store.images), N.ptr(store.mask), store.num_images, store.height, store.width, N.ptr(store.c2w), N.ptr(store.fx),
        N.ptr(store.fy), N.ptr(store.cx), N.ptr(store.cy), N.ptr(store.camera_type), N.ptr(store.distortion), N.ptr(draw_counter),
        int(draw_offset), int(seed), int(max_attempts), int(num_rays), N.ptr(origins), N.ptr(directions), N.ptr(pixel_area),
        N.ptr(directions_norm), N.ptr(camera_indices), N.ptr(target), N.ptr(indices), N.ptr(failed), N.stream()), "sample_batch")


class DeviceBatchSource:
    """`num_rays` rays per batch out of `store`. seed: the run's seed (torch.initial_seed()); the rank is mixed in (`mix_seed`).
    launch_fn: the launch itself (`native_launch`); tests of the host logic inject a stand-in, as TrainEngine.runner_factory."""

    def __init__(self, store: DeviceImageStore, num_rays: int, seed: int, rank: int = 0, max_attempts: int = MAX_ATTEMPTS,
                 launch_fn: Optional[Callable] = None, bundle_cls=None) -> None:
        self.store, self.num_rays, self.max_attempts = store, int(num_rays), int(max_attempts)
        self.seed = mix_seed(seed, rank)
        self.launch_fn = launch_fn or native_launch
        self.bundle_cls = bundle_cls
        dev = store.device
        self.draw_counter = torch.zeros(1, device=dev, dtype=torch.int64)  # the eager form's own counter
        self.failed = torch.zeros(1, device=dev, dtype=torch.int32)  # lanes that ran out of redraws, over all launches
        self._scratch = None

    def set_draw(self, draw: int) -> None:
        """The next `next_batch` takes draw number `draw` (a resumed run: the model's step, as the jitter's counter)."""
        self.draw_counter.fill_(int(draw))

    def failed_lanes(self) -> int:
        """Lanes that exhausted `max_attempts` redraws against the mask since the start. Reads the device: call it where
        the host synchronises anyway (logging, evaluation)."""
        return int(self.failed.item())

    def launch(self, origins, directions, camera_indices, target, draw_counter, draw_offset: int = 0, pixel_area=None,
               directions_norm=None, indices=None) -> None:
        """The bare launch into caller-owned buffers ([n,3] fp32, [n] int64, [n,3] fp32), on the current stream; the draw is
        `draw_counter[0] + draw_offset`, read on the device — nothing here changes from step to step, so the launch can be
        captured. The counter is not advanced."""
        self.launch_fn(self.store, self.num_rays, self.seed, self.max_attempts, draw_counter, draw_offset, origins, directions,
                       camera_indices, target, pixel_area=pixel_area, directions_norm=directions_norm, indices=indices,
                       failed=self.failed)

    def next_batch(self, advance: bool = True) -> Tuple[object, Dict[str, torch.Tensor]]:
        """-> (RayBundle, {"image" [n,3], "indices" [n,3] int64}) in fresh tensors on the store's device: one launch with this
        object's own counter, then `counter += 1` as a torch op (advance=False: the same batch again next time). The eager form
        — not the captured path; no host copy or synchronisation either."""
        n, dev = self.num_rays, self.store.device
        f32 = dict(device=dev, dtype=torch.float32)
        o, d, t = (torch.empty((n, 3), **f32) for _ in range(3))
        pa, dn = torch.empty((n, 1), **f32), torch.empty((n, 1), **f32)
        cams = torch.empty((n,), device=dev, dtype=torch.int64)
        idx = torch.empty((n, 3), device=dev, dtype=torch.int64)
        self.launch(o, d, cams, t, self.draw_counter, 0, pixel_area=pa, directions_norm=dn, indices=idx)
        if advance:
            self.draw_counter.add_(1)
        bundle_cls = self.bundle_cls
        if bundle_cls is None:
            from .cameras.rays import RayBundle as bundle_cls
        rb = bundle_cls(origins=o, directions=d, pixel_area=pa, camera_indices=cams[:, None], metadata={"directions_norm": dn})
        return rb, {"image": t, "indices": idx}
