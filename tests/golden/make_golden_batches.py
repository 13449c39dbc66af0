#!/usr/bin/env python3
"""Golden fixture for the pixel draw of a training batch — written by THE REFERENCE ITSELF (read-only import of the reference,
torch path, CPU). Authoring container only:

    python tests/golden/make_golden_batches.py      ->  tests/golden/pixel_batches.npz

Each case runs the reference's own `PixelSampler.collate_image_dataset_batch` (data/pixel_samplers.py:265-318 ->
`sample_method` :137-174: `(torch.rand(n, 3) * tensor([N, H, W])).long()`, then the gather `image[c, y, x]`) with `torch.rand`
replaced by RECORDED float32 uniforms, on an image batch derived from uint8 pixels the way the reference's dataset derives it
(`image / np.float32(255)`, data/datasets/base_dataset.py:107). Cases (`cases` in the fixture; arrays are `<case>_<name>`):

    small   3 images of 5 x 7
    single  1 image of 1 x 1

Recorded per case: `images` uint8 [N,H,W,3], `uniforms` float32 [n,3], and the reference's `indices` int64 [n,3] and `image`
float32 [n,3]. The uniforms hold 0, 1 - 2^-24, for every dimension the 24-bit neighbours of every k / dim (the products that
land on or next to an integer), float32(k / dim) itself, and seeded 24-bit draws.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (sets up the import path of the reference and its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STEP = np.float32(2.0 ** -24)


def uniforms_for(dims, rs, extra=64):
    """[n,3] float32 in [0, 1): column j exercises dimension dims[j]; the other columns of such a row are seeded draws."""
    cols = []
    for dim in dims:
        vals = [np.float32(0.0), np.float32(1.0) - STEP, STEP]
        for k in range(1, dim + 1):
            grid = np.float32(np.round(k / dim * 2.0 ** 24)) * STEP  # the 24-bit uniform nearest k / dim ...
            for off in (-2, -1, 0, 1, 2):                              # ... and its neighbours
                vals.append(grid + np.float32(off) * STEP)
            vals.append(np.float32(k / dim))                           # not on the 24-bit grid in general
            vals.append(np.nextafter(np.float32(k / dim), np.float32(0.0)))
        v = np.array(vals, np.float32)
        cols.append(v[(v >= 0) & (v < 1)])
    n = max(len(c) for c in cols) + extra
    out = (rs.randint(0, 1 << 24, size=(n, 3)).astype(np.float32) * STEP).astype(np.float32)
    for j, c in enumerate(cols):
        out[:len(c), j] = c
    return out


def run_case(images_u8, uniforms):
    from nerfstudio.data.pixel_samplers import PixelSampler, PixelSamplerConfig

    n = uniforms.shape[0]
    sampler = PixelSampler(PixelSamplerConfig(num_rays_per_batch=n))
    image = torch.from_numpy(images_u8 / np.float32(255))  # base_dataset.py:107
    assert image.dtype == torch.float32
    batch = {"image": image, "image_idx": torch.arange(images_u8.shape[0])}
    real_rand = torch.rand

    def recorded(*size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        assert shape == (n, 3), shape
        return torch.from_numpy(uniforms.copy())

    torch.rand = recorded
    try:
        out = sampler.collate_image_dataset_batch(batch, n)
    finally:
        torch.rand = real_rand
    return out["indices"].numpy().astype(np.int64), out["image"].numpy().astype(np.float32)


def main():
    rs = np.random.RandomState(20240611)
    fixture = {"cases": np.array(["small", "single"])}
    for name, (N, H, W) in (("small", (3, 5, 7)), ("single", (1, 1, 1))):
        images = rs.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
        images.reshape(-1)[:2] = (0, 255)
        uniforms = uniforms_for((N, H, W), rs)
        indices, image = run_case(images, uniforms)
        assert indices[:, 0].max() == N - 1 and indices[:, 1].max() == H - 1 and indices[:, 2].max() == W - 1
        fixture.update({f"{name}_images": images, f"{name}_uniforms": uniforms, f"{name}_indices": indices, f"{name}_image": image})
        print(name, uniforms.shape, "indices max", indices.max(axis=0))
    np.savez_compressed(os.path.join(HERE, "pixel_batches.npz"), **fixture)


if __name__ == "__main__":
    main()
