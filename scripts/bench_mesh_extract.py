#!/usr/bin/env python3
"""Times of the mesh extraction on the GPU (profiles/mesh_extract.txt): nsamd_mesh_count and nsamd_mesh_emit on a --dims^3 volume
that holds a sphere fused from --views analytic depth frames, each against the bytes it must move, beside the existing
nsamd_tsdf_integrate launch on the same volume, and the whole TSDFVolume.get_mesh (two launches, one read of the totals, the
allocations). Kernel figures: device events around --batch launches back to back, the median of --repeats such runs after a
warm-up run. Bytes, from the shapes: the count pass reads the values (4 B per voxel) and writes one word per voxel (4 B) and two
per workgroup; the emit pass reads the values and the words again and writes 36 B per vertex (position, normal, colour; 12 B of
colour read) and 12 B per triangle. Neighbour reads are served by the caches and not counted. Shares are of the 8 TB/s HBM peak.

    python scripts/bench_mesh_extract.py [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import tsdf_reference as tr  # noqa: E402
from nerfstudio_amd import _native as N  # noqa: E402
from nerfstudio_amd import functional as Fn  # noqa: E402
from nerfstudio_amd.export import TSDFVolume  # noqa: E402

AABB = [[-1.0, -1, -1], [1, 1, 1]]
HBM_PEAK = 8.0e12  # bytes per second


def orbit(n):
    k = np.arange(n)
    theta, z = k * 2.399963, 0.8 * np.cos(k * 0.7)
    r = np.sqrt(1 - z * z)
    return torch.from_numpy(np.stack([tr.look_at(2.6 * np.array([r[i] * np.cos(theta[i]), r[i] * np.sin(theta[i]), z[i]]))
                                      for i in range(n)]).astype(np.float32))


def event_ms(fn, batch, repeats):
    """per-launch ms: device events around `batch` launches back to back; the first run is the warm-up"""
    out = []
    for _ in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / batch)
    return statistics.median(out[1:]), out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, default=256)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=20)
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
    depth = depth.float().to(dev)
    color = torch.rand(B, S, S, 3, device=dev)
    vol = TSDFVolume.from_aabb(AABB, [D] * 3, device=dev)
    vol.integrate(c2w.to(dev), K.to(dev), depth, color)
    n = D ** 3
    say(f"{torch.cuda.get_device_name(0)}; volume {D}^3 = {n} voxels, a sphere of radius 0.6 fused from {B} views of {S} x {S}; "
        f"device events around {a.batch} launches back to back, median of {a.repeats} runs after a warm-up run")

    mv = N.make_mesh_volume(vol.origin.tolist(), vol.voxel_size.tolist(), vol.values.shape)
    scratch = torch.empty(N.mesh_scratch_bytes(n), dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    Fn.mesh_count_launch(mv, vol.values, scratch, totals)
    V, T = totals.tolist()
    outs = [torch.empty((V, 3), device=dev) for _ in range(3)] + [torch.empty((T, 3), dtype=torch.int32, device=dev)]
    Fn.mesh_emit_launch(mv, vol.values, vol.colors, scratch, *outs)
    torch.cuda.synchronize()
    say(f"mesh: {V} vertices, {T} triangles; scratch {scratch.numel() / 2 ** 20:.1f} MiB, outputs {(36 * V + 12 * T) / 2 ** 20:.1f} MiB")

    blocks = (n + N.MESH_BLOCK - 1) // N.MESH_BLOCK
    count_bytes = 4 * n + 4 * n + 8 * blocks
    emit_bytes = 4 * n + 4 * n + 8 * blocks + 48 * V + 12 * T
    for name, fn, nbytes in (("nsamd_mesh_count (count + scan)", lambda: Fn.mesh_count_launch(mv, vol.values, scratch, totals), count_bytes),
                             ("nsamd_mesh_emit", lambda: Fn.mesh_emit_launch(mv, vol.values, vol.colors, scratch, *outs), emit_bytes)):
        med, ms = event_ms(fn, a.batch, a.repeats)
        say(f"{name}: {med:.4f} ms  [{min(ms):.4f} .. {max(ms):.4f}]; {nbytes / 2 ** 20:.0f} MiB to move = "
            f"{nbytes / med / 1e6:.0f} GB/s, {100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of the HBM peak "
            f"(the volume and the words, {8 * n / 2 ** 20:.0f} MiB, fit the 256 MiB Infinity Cache between back-to-back launches)")

    w2c = torch.stack([torch.linalg.inv_ex(m).inverse for m in c2w.to(dev)])[:, :3].contiguous()
    args = (vol.origin.tolist(), vol.voxel_size.tolist(), vol.truncation, vol.values.clone(), vol.weights.clone(), vol.colors.clone(),
            w2c, K.to(dev)[:, :2].contiguous(), depth, color)
    med, ms = event_ms(lambda: Fn.tsdf_integrate_launch(*args), a.batch, a.repeats)
    say(f"for scale, nsamd_tsdf_integrate of the {B} views into the same volume: {med:.4f} ms  [{min(ms):.4f} .. {max(ms):.4f}]")

    whole = []
    for _ in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh = vol.get_mesh()
        torch.cuda.synchronize()
        whole.append(1e3 * (time.perf_counter() - t0))
    assert mesh.vertices.shape[0] == V and mesh.faces.shape[0] == T
    say(f"TSDFVolume.get_mesh, host clock to a device synchronise (allocations, count, the read of the totals, emit): "
        f"{statistics.median(whole[1:]):.3f} ms  [{min(whole[1:]):.3f} .. {max(whole[1:]):.3f}]")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
