#!/usr/bin/env python3
"""Times of mesh export on the GPU (profiles/tsdf_export.txt): one TSDFVolume.integrate of --views frames of --size x --size into
a --dims^3 volume against the fp32 torch-op restatement of the reference's update (tests/tsdf_reference.integrate_torch) on the
same inputs, and the whole export.fuse_views of --fuse-views cameras rendered by a default-configuration nerfacto model. Each
figure: warm-up runs, then the median of --repeats runs, each ended by a device synchronise; peak memory is
torch.cuda.max_memory_allocated over the timed runs minus what was allocated before them.

    python scripts/bench_tsdf_export.py [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import tsdf_reference as tr  # noqa: E402
from nerfstudio_amd import functional as Fn  # noqa: E402
from nerfstudio_amd.export import TSDFVolume, fuse_views  # noqa: E402

AABB = [[-1.0, -1, -1], [1, 1, 1]]


def orbit(n):
    """n look-at poses [n,4,4] fp32 on a sphere of radius 2.6 about the origin."""
    k = np.arange(n)
    theta, z = k * 2.399963, 0.8 * np.cos(k * 0.7)
    r = np.sqrt(1 - z * z)
    return torch.from_numpy(np.stack([tr.look_at(2.6 * np.array([r[i] * np.cos(theta[i]), r[i] * np.sin(theta[i]), z[i]]))
                                      for i in range(n)]).astype(np.float32))


def timed(fn, warmup, repeats):
    """-> (median ms, [ms], peak bytes above the baseline)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), ms, torch.cuda.max_memory_allocated() - base


def write(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, default=256)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--fuse-views", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, lines = "cuda", []
    say = lambda s: (print(s, flush=True), lines.append(s))  # noqa: E731
    B, S, D = a.views, a.size, a.dims
    f = 0.9 * S
    K = torch.tensor([[f, 0, S / 2 + 0.37], [0, f, S / 2 - 0.21], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    c2w = orbit(B)
    depth = torch.stack([torch.from_numpy(tr.sphere_depth(c.double().numpy(), K[0].double().numpy(), S, S, 0.6)) for c in c2w])
    depth = depth.float()[:, None].to(dev)
    color = torch.rand(B, 3, S, S, device=dev)
    c2w, K = c2w.to(dev), K.to(dev)
    say(f"{torch.cuda.get_device_name(0)}; volume {D}^3 ({D ** 3 * 20 / 2 ** 20:.0f} MiB of state), {B} views of {S} x {S}; "
        f"median of {a.repeats} synchronised runs after warm-up")

    vol = TSDFVolume.from_aabb(AABB, [D] * 3, device=dev)
    channel_last = color.permute(0, 2, 3, 1).contiguous()
    med, ms, peak = timed(lambda: vol.integrate(c2w, K, depth, channel_last), 3, a.repeats)
    say(f"TSDFVolume.integrate (one tsdf kernel launch + {B} 4x4 inversions): {med:.3f} ms  "
        f"[{min(ms):.3f} .. {max(ms):.3f}]  peak memory above the volume and frames {peak / 2 ** 20:.1f} MiB")
    # the kernel alone: device events around 20 back-to-back launches on prepared arguments
    w2c = torch.stack([torch.linalg.inv_ex(m).inverse for m in c2w])[:, :3].contiguous()
    args = (vol.origin.tolist(), vol.voxel_size.tolist(), vol.truncation, vol.values, vol.weights, vol.colors, w2c,
            K[:, :2].contiguous(), depth[:, 0].contiguous(), channel_last)
    per_launch = []
    for _ in range(a.repeats + 1):  # (the first round is the warm-up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            Fn.tsdf_integrate_launch(*args)
        e1.record()
        torch.cuda.synchronize()
        per_launch.append(e0.elapsed_time(e1) / 20)
    kernel_ms = statistics.median(per_launch[1:])
    touched = int((vol.weights > 0).sum())
    traffic = touched * 40 + (D ** 3 - touched) * 20
    say(f"  the launch alone (device events, 20 launches back to back): {kernel_ms:.3f} ms  [{min(per_launch[1:]):.3f} .. "
        f"{max(per_launch[1:]):.3f}]; {touched} of {D ** 3} voxels touched: 20 B of state read per voxel, 20 B written per "
        f"touched voxel = {traffic / 2 ** 20:.0f} MiB, {traffic / kernel_ms / 1e6:.0f} GB/s (the frames' pixels not counted)")

    eager = TSDFVolume.from_aabb(AABB, [D] * 3, device=dev)
    run = lambda: tr.integrate_torch(eager.origin, eager.voxel_size, eager.truncation, eager.values, eager.weights,  # noqa: E731
                                     eager.colors, c2w, K, depth, color)
    med_e, ms_e, peak_e = timed(run, 2, a.repeats)
    say(f"fp32 torch-op restatement of integrate_tsdf, same GPU and inputs: {med_e:.3f} ms  [{min(ms_e):.3f} .. {max(ms_e):.3f}]  "
        f"peak memory {peak_e / 2 ** 30:.2f} GiB")
    say(f"  ratio {med_e / med:.1f} x in time over the whole call, {med_e / kernel_ms:.0f} x over the launch alone; "
        f"{peak_e / 2 ** 20:.0f} MiB against {peak / 2 ** 20:.2f} MiB of temporaries")
    del eager
    if a.fuse_views <= 0:
        return write(a.out, lines)

    from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig

    torch.manual_seed(0)
    model = NerfactoModel(NerfactoModelConfig(), torch.tensor(AABB), num_train_data=a.fuse_views).to(dev).eval()
    n = a.fuse_views
    col = lambda v, dt=torch.float32: torch.full((n, 1), v, dtype=dt)  # noqa: E731
    cams = types.SimpleNamespace(camera_to_worlds=orbit(n)[:, :3], fx=col(2 * f), fy=col(2 * f), cx=col(S + 0.74), cy=col(S - 0.42),
                                 height=col(2 * S, torch.int64), width=col(2 * S, torch.int64), camera_type=col(1, torch.int64))
    fused = TSDFVolume.from_aabb(AABB, [D] * 3, device=dev)
    med_f, ms_f, peak_f = timed(lambda: fuse_views(model, cams, fused, downscale_factor=2, views_per_launch=B), 1, 3)
    say(f"fuse_views, {n} cameras of {2 * S} x {2 * S} at downscale_factor=2, {B} views per launch (render + fuse, random-init "
        f"default nerfacto): {med_f:.1f} ms  [{min(ms_f):.1f} .. {max(ms_f):.1f}] = {med_f / n:.2f} ms per view; "
        f"peak memory above model and volume {peak_f / 2 ** 20:.1f} MiB")
    write(a.out, lines)


if __name__ == "__main__":
    main()
