#!/usr/bin/env python3
"""Time of mip-NeRF's integrated positional encoding at the method's own sizes (1024 and 4096 rays x 128 samples, 16 frequencies
at exponents 0 .. 16, input appended): nsamd_ipe_encode in ray mode against the torch-op composition of the same arithmetic on
the same GPU — Frustums.get_gaussian_blob + the reference's formula (encodings.py:162-186) — and one MipNerfModel training
iteration (forward, backward, RAdam step; 1024 rays x (128 + 128) samples) with the kernel against the same iteration with that
composition. Device events around back-to-back calls after a warm-up of every shape, the two arms alternating. GPU box only:
    python scripts/bench_ipe.py [--launches 200 --iterations 20 --repeats 3]
Prints one JSON line (best and worst repeat per arm; the store rate of the kernel from the bytes its rows take)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfstudio_amd import functional as F  # noqa: E402
from nerfstudio_amd.cameras.rays import RayBundle, samples_from_bins  # noqa: E402
from nerfstudio_amd.mipnerf import MipNerfModel, MipNerfModelConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--iterations", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
NF, LO, HI, S = 16, 0.0, 16.0, 128


def torch_ipe(mean, cov):
    """NeRFEncoding.pytorch_fwd with covariances + the appended input, as the reference evaluates it."""
    freqs = 2 ** torch.linspace(LO, HI, NF, device=mean.device)
    scaled = ((2 * torch.pi * mean)[..., None] * freqs).reshape(*mean.shape[:-1], -1)
    var = (torch.diagonal(cov, dim1=-2, dim2=-1)[..., :, None] * freqs[None, :] ** 2).reshape(*mean.shape[:-1], -1)
    out = torch.exp(-0.5 * torch.cat(2 * [var], dim=-1)) * torch.sin(torch.cat([scaled, scaled + torch.pi / 2.0], dim=-1))
    return torch.cat([out, mean], dim=-1)


def rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 4.0])
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1)
    area = 8.1e-7 * (0.75 + 0.5 * torch.rand(n, 1, generator=g))
    return o.to(dev), d.to(dev), area.to(dev)


def timed(arms, calls):
    """{name: fn} -> {name: [ms per call, one per repeat]}, the arms alternating within every repeat."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(args.repeats):
        for name, fn in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / calls)
    return {name: {"ms_best": round(min(t), 4), "ms_worst": round(max(t), 4)} for name, t in times.items()}


out = {}
for n in (1024, 4096):
    o, d, area = rays(n, n)
    rb = RayBundle(origins=o, directions=d, pixel_area=area)
    t_bins = 2.0 + 4.0 * torch.sort(torch.rand(n, S + 1, generator=torch.Generator().manual_seed(n + 1)), dim=-1).values.to(dev)
    samples = samples_from_bins(rb, t_bins, t_bins, None)
    spec = F.PointSpec(origins=o, directions=d, t_bins=t_bins)

    def composition():
        blob = samples.frustums.get_gaussian_blob()
        return torch_ipe(blob.mean, blob.cov)

    kernel = lambda: F.ipe_encode(spec, area, None, NF, LO, HI, True)  # noqa: E731
    # what bounds the kernel: the same rows from explicit Gaussians (no frustum arithmetic), and from Gaussians wider than every
    # wavelength (every entry damped to exactly zero: no sine is evaluated, the stores and one expf per entry are left)
    blob = samples.frustums.get_gaussian_blob()
    means = F.PointSpec(positions=blob.mean.reshape(-1, 3).contiguous())
    variances = torch.diagonal(blob.cov, dim1=-2, dim2=-1).reshape(-1, 3).contiguous()
    wide = torch.full_like(variances, 1.0e3)
    with torch.no_grad():
        a, b = kernel().view(n, S, -1), composition()
        res = timed({"kernel": kernel, "torch composition": composition,
                     "kernel, explicit mode": lambda: F.ipe_encode(means, None, variances, NF, LO, HI, True),
                     "kernel, explicit mode, every entry damped to zero": lambda: F.ipe_encode(means, None, wide, NF, LO, HI, True)},
                    args.launches)
    res["largest difference of the two outputs"] = float((a - b).abs().max())
    res["entries of the kernel's rows that are exactly zero"] = round(float((a[..., :96] == 0).float().mean()), 3)
    res["kernel store rate GB/s (396 B per sample)"] = round(n * S * 396 / (res["kernel"]["ms_best"] * 1e-3) / 1e9, 1)
    out[f"{n} x {S} samples"] = res

n = 1024
o, d, area = rays(n, 7)
target = torch.rand(n, 3, generator=torch.Generator().manual_seed(8)).to(dev)
torch.manual_seed(0)
model = MipNerfModel(MipNerfModelConfig()).to(dev).train()
opt = torch.optim.RAdam(model.get_param_groups()["fields"], lr=5e-4, eps=1e-8)
kernel_route = model.field._integrated_encoding


def composition_route(ray_samples):
    with torch.no_grad():
        blob = ray_samples.frustums.get_gaussian_blob()
        return torch_ipe(blob.mean, blob.cov).reshape(-1, 99)


def iteration(route):
    def run():
        model.field._integrated_encoding = route
        losses = model.get_loss_dict(model(RayBundle(origins=o, directions=d, pixel_area=area)), {"image": target})
        opt.zero_grad()
        sum(losses.values()).backward()
        opt.step()
    return run


out[f"training iteration, {n} rays x (128 + 128) samples"] = timed(
    {"kernel": iteration(kernel_route), "torch composition": iteration(composition_route)}, args.iterations)
print(json.dumps({"metric": "integrated positional encoding, ms per call (device events, back-to-back calls, arms alternating)",
                  "launches": args.launches, "iterations": args.iterations, "repeats": args.repeats, "cases": out}))
