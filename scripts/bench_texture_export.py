#!/usr/bin/env python3
"""Times of the texture export on the GPU (profiles/texture_export.txt): on the mesh of a --dims^3 volume that holds a sphere
fused from --views analytic depth frames, at --px texels per triangle side,

    device      texture.render_texture: nsamd_mesh_raylen, then per chunk nsamd_texel_rays into the eval schedule's inputs, the
                chunk, nsamd_texture_store of its rgb rows
    restated    the reference's unwrap_mesh_per_uv_triangle + ray-length line + bundle restated as fp32 torch ops on the same GPU
                (the [H,W,3,3] gathers, barycentric weights from texture-coordinate differences), then EvalRenderer.render(bundle)
                with the bundle's own nears and fars, and the 8-bit image by torch ops

in --repeats alternating runs after one warm-up run of each (host clock around a device synchronise), with the peak device
memory of a run above what model and mesh hold, the texels whose 8-bit level differs between the two, and the nsamd_texel_rays
launch alone (device events around --batch launches of one chunk) against the bytes it must move: 32 B written per ray; the
mesh reads are served by the caches and not counted. Shares are of the 8 TB/s HBM peak. The model is an untrained default
nerfacto: the times are those of the schedule, not of a scene.

    python scripts/bench_texture_export.py [--dims 256] [--px 4] [--out FILE]
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
from nerfstudio_amd import eval_render, texture  # noqa: E402
from nerfstudio_amd import functional as Fn  # noqa: E402
from nerfstudio_amd.cameras.rays import RayBundle  # noqa: E402
from nerfstudio_amd.export import TSDFVolume  # noqa: E402
from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig  # noqa: E402

AABB = [[-1.0, -1, -1], [1, 1, 1]]
HBM_PEAK = 8.0e12  # bytes per second


def orbit(n):
    k = np.arange(n)
    theta, z = k * 2.399963, 0.8 * np.cos(k * 0.7)
    r = np.sqrt(1 - z * z)
    return torch.from_numpy(np.stack([tr.look_at(2.6 * np.array([r[i] * np.cos(theta[i]), r[i] * np.sin(theta[i]), z[i]]))
                                      for i in range(n)]).astype(np.float32))


def area2(p, a, b):
    return (p[..., 0] - a[..., 0]) * (b[..., 1] - a[..., 1]) - (p[..., 1] - a[..., 1]) * (b[..., 0] - a[..., 0])


def restated_bundle(vertices, faces, normals, atlas):
    """the reference's per-texel tensors in fp32 on the device: texture coordinates of every face, per texel the gathered corner
    coordinates, vertices and normals, the weights as ratios of parallelogram areas, the blended ray, the offset, the bundle"""
    dev = vertices.device
    P, W, H = atlas.px, atlas.width, atlas.height
    tc = atlas.texture_coordinates().to(dev)
    x, y = torch.meshgrid(torch.arange(W, device=dev), torch.arange(H, device=dev), indexing="xy")
    p = torch.stack([torch.linspace(0.5 / W, 1 - 0.5 / W, W, device=dev)[x], torch.linspace(0.5 / H, 1 - 0.5 / H, H, device=dev)[y]], -1)
    square = torch.div(y, P, rounding_mode="floor") * atlas.squares_w + torch.div(x, P + 3, rounding_mode="floor")
    lower = (x % (P + 3) + y % P) >= P + 1
    t = torch.clamp(square * 2 + lower, max=atlas.faces - 1)
    uv, tri = tc[t], faces.long()[t]
    v, n = vertices[tri], normals[tri]
    total = area2(uv[..., 2, :], uv[..., 0, :], uv[..., 1, :])
    w = [area2(p, uv[..., 1, :], uv[..., 2, :]) / total, area2(p, uv[..., 2, :], uv[..., 0, :]) / total,
         area2(p, uv[..., 0, :], uv[..., 1, :]) / total]
    origins = v[..., 0, :] * w[0][..., None] + v[..., 1, :] * w[1][..., None] + v[..., 2, :] * w[2][..., None]
    directions = torch.nn.functional.normalize(-(n[..., 0, :] * w[0][..., None] + n[..., 1, :] * w[1][..., None]
                                                 + n[..., 2, :] * w[2][..., None]), dim=-1)
    fv = vertices[faces.long()]
    raylen = 2.0 * torch.mean(torch.norm(fv[:, 1, :] - fv[:, 0, :], dim=-1))
    origins = origins - 0.5 * raylen * directions
    one = torch.ones_like(origins[..., 0:1])
    return RayBundle(origins=origins, directions=directions, pixel_area=one, camera_indices=torch.zeros_like(one),
                     nears=torch.zeros_like(one), fars=one * raylen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, default=256)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--px", type=int, default=4)
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
    vol = TSDFVolume.from_aabb(AABB, [D] * 3, device=dev)
    vol.integrate(c2w.to(dev), K.to(dev), depth.float().to(dev), torch.rand(B, S, S, 3, device=dev))
    mesh = vol.get_mesh()
    del vol
    torch.manual_seed(0)
    model = NerfactoModel(NerfactoModelConfig(), torch.tensor(AABB), 8).to(dev).eval()
    atlas = texture.TexelAtlas.for_faces(int(mesh.faces.shape[0]), a.px)
    total = atlas.width * atlas.height
    chunk = int(model.config.eval_num_rays_per_chunk)
    say(f"{torch.cuda.get_device_name(0)}; a sphere of radius 0.6 fused from {B} views of {S} x {S} into {D}^3 voxels: "
        f"{mesh.vertices.shape[0]} vertices, {atlas.faces} faces; px_per_uv_triangle {a.px}: atlas {atlas.width} x {atlas.height} = "
        f"{total} texels, {-(-total // chunk)} chunks of {chunk} rays; an untrained default nerfacto model")

    def device_arm():
        return texture.render_texture(model, mesh, a.px)

    def restated_arm():
        bundle = restated_bundle(mesh.vertices, mesh.faces, mesh.normals, atlas)
        rgb = eval_render.runner_for(model, dev).render(bundle)["rgb"]
        return torch.floor(torch.nan_to_num(rgb, nan=0.0).clamp(0, 1) * 255 + 0.5).to(torch.uint8)

    images, times, peaks = {}, {"device": [], "restated": []}, {"device": [], "restated": []}
    for run in range(a.repeats + 1):  # run 0: the warm-up of each arm (graph capture, allocator)
        for name, arm in (("device", device_arm), ("restated", restated_arm)):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            images[name] = arm()
            torch.cuda.synchronize()
            if run:
                times[name].append(1e3 * (time.perf_counter() - t0))
                peaks[name].append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
    diff = int((images["device"] != images["restated"]).any(-1).sum())
    for name in ("device", "restated"):
        ms = times[name]
        say(f"{name}: {statistics.median(ms):.1f} ms  [{min(ms):.1f} .. {max(ms):.1f}] = {total / statistics.median(ms) / 1e3:.1f} M texels/s; "
            f"peak memory above model and mesh {statistics.median(peaks[name]):.0f} MiB (the {3 * total / 2 ** 20:.0f} MiB image included)")
    say(f"restated / device: {statistics.median(times['restated']) / statistics.median(times['device']):.2f} x; "
        f"{diff} of {total} texels differ in some 8-bit level between the two (the restated weights are fp32 differences of "
        f"texture coordinates 1 / {atlas.width} apart)")

    runner = eval_render.runner_for(model, dev)
    s, pod = runner.step, atlas.native()
    raylen = torch.zeros(1, device=dev)
    Fn.mesh_raylen_launch(mesh.vertices, mesh.faces, torch.empty(8192, dtype=torch.uint8, device=dev), raylen)
    k = min(chunk, total)
    first = (total // 2 // chunk) * chunk if total >= 2 * chunk else 0
    runs = []
    try:
        for _ in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.batch):
                Fn.texel_rays_launch(pod, mesh.vertices, mesh.normals, mesh.faces, raylen, first, k, chunk, s.origins, s.directions, s.nears, s.fars)
            e1.record()
            torch.cuda.synchronize()
            runs.append(1e3 * e0.elapsed_time(e1) / a.batch)
    finally:
        runner._restore_bounds()
    med = statistics.median(runs[1:])
    say(f"nsamd_texel_rays alone, one chunk of {chunk} rays: {med:.2f} us  [{min(runs[1:]):.2f} .. {max(runs[1:]):.2f}]; {32 * chunk / 2 ** 10:.0f} KiB "
        f"to write = {32 * chunk / med / 1e3:.0f} GB/s, {100 * 32 * chunk / (med * 1e-6) / HBM_PEAK:.2f} % of the HBM peak (a launch of this size is "
        f"bounded by its latency, not by bytes); ray length {float(raylen[0]):.6f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
