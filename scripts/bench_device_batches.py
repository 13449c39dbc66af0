#!/usr/bin/env python3
"""What a device-resident batch source costs next to bench.py's pool of pre-generated batches: the same captured nerfacto
iteration (trainer.HipTrainer, 4096 rays) with its batch

    pool_ms          selected from a pool of batches in HBM, as bench.py builds it (nsamd_select_bins);
    source_ms        SAMPLED inside the captured iteration from an image store in HBM (HipTrainer(source=...): nsamd_sample_batch
                     — pixel draw, uint8 colour gather, ray generation — as a node of the replayed graph);
    eager_source_ms  sampled eagerly by `DeviceBatchSource.next_batch()` and handed to `set_batch` ahead of every replay (the
                     form the data-parallel segments and a trainer without the device prologue take).

The image set is procedural and generated on the device: 100 images of 800 x 800, perspective cameras on a shell around the
scene box. The three trainers live in one process and their timed windows ALTERNATE (pool, source, eager, pool, ...), so a
drift of the box moves all three. One JSON line: the median of the windows per arm, every window, the window-to-window spread
of `pool_ms` and whether `source_ms` lies inside it.

    python scripts/bench_device_batches.py [--steps 20] [--warmup 5] [--windows 7] [--time-limit 300]
"""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--images", type=int, default=100)
ap.add_argument("--height", type=int, default=800)
ap.add_argument("--width", type=int, default=800)
ap.add_argument("--time-limit", type=int, default=300, help="seconds after which the process dumps its stacks and exits")
args = ap.parse_args()
faulthandler.dump_traceback_later(args.time_limit, exit=True)  # a hung launch must not hold the GPU

from nerfstudio_amd import _native, functional as F  # noqa: E402
from nerfstudio_amd.arena import ParamArena  # noqa: E402
from nerfstudio_amd.device_batches import DeviceBatchSource, DeviceImageStore  # noqa: E402
from nerfstudio_amd.trainer import HipTrainer  # noqa: E402

_native.load()
F.DIRECT_GRAD = True
dev = torch.device("cuda")
n = bench.RAYS_PER_GPU


def procedural_store():
    """Smooth colour fields per image, quantised to uint8 on the device; cameras on a shell of radius 2.5 looking at the origin."""
    N, H, W = args.images, args.height, args.width
    g = torch.Generator(device=dev).manual_seed(7)
    y = torch.linspace(0, 1, H, device=dev)[None, :, None, None]
    x = torch.linspace(0, 1, W, device=dev)[None, None, :, None]
    freq = torch.rand((N, 1, 1, 3), device=dev, generator=g) * 9 + 1
    phase = torch.rand((N, 1, 1, 3), device=dev, generator=g) * 6.28
    images = torch.empty((N, H, W, 3), device=dev, dtype=torch.uint8)
    for i in range(N):  # (one image at a time: the float intermediate of the whole set would be 768 MB)
        images[i] = ((torch.sin(freq[i] * (x[0] + 1.7 * y[0]) + phase[i]) * 0.5 + 0.5) * 255).round().to(torch.uint8)
    rs = np.random.RandomState(11)
    pos = rs.standard_normal((N, 3))
    pos = 2.5 * pos / np.linalg.norm(pos, axis=-1, keepdims=True)
    back = pos / np.linalg.norm(pos, axis=-1, keepdims=True)
    right = np.cross(np.array([0.0, 0.0, 1.0]) + 0.01 * rs.standard_normal((N, 3)), back)
    right /= np.linalg.norm(right, axis=-1, keepdims=True)
    up = np.cross(back, right)
    c2w = torch.from_numpy(np.concatenate([np.stack([right, up, back], -1), pos[..., None]], -1).astype(np.float32))
    focal = torch.full((N,), 1.1 * W)
    return DeviceImageStore(images, None, c2w, focal, focal, torch.full((N,), W / 2.0), torch.full((N,), H / 2.0),
                            torch.ones(N, dtype=torch.int32), None)


store = procedural_store()
_, _, pool = bench.synthetic_batch(dev, seed=1000)
arms = {}
for arm in ("pool", "source", "eager_source"):
    model = bench.build_model(dev, seed=0)
    arena = ParamArena(model.get_param_groups_ordered(), lr=1e-2, eps=1e-15)
    src = DeviceBatchSource(store, n, seed=1234)
    if arm == "pool":
        rb, batch, _ = bench.synthetic_batch(dev, seed=1000)
    else:
        rb, batch = src.next_batch(advance=False)
    tr = HipTrainer(model, arena, rb, batch, world=1, use_graph=True, use_runner=True, pool=pool if arm == "pool" else None,
                    source=src if arm == "source" else None)

    def step(tr=tr, src=src, arm=arm):
        if arm == "eager_source":
            tr.set_batch(*src.next_batch())
        tr.train_iteration()

    for _ in range(2):
        step()
    tr.finish()
    assert tr.try_capture(warm=False), arm
    assert tr.source_inside == (arm == "source")
    for _ in range(max(0, args.warmup - 2)):
        step()
    tr.finish()
    arms[arm] = (tr, step)
torch.cuda.synchronize()

windows = {arm: [] for arm in arms}
for _ in range(args.windows):
    for arm, (tr, step) in arms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        tr.finish()
        torch.cuda.synchronize()
        windows[arm].append((time.perf_counter() - t0) / args.steps * 1e3)
losses = {arm: float(tr.last_loss()) for arm, (tr, _) in arms.items()}
assert all(np.isfinite(v) for v in losses.values()), losses
med = {arm: float(np.median(v)) for arm, v in windows.items()}
lo, hi = min(windows["pool"]), max(windows["pool"])
print(json.dumps({
    "metric": "ms per nerfacto training iteration, 4096 rays, replayed hipGraphs (alternating windows, one process)",
    "steps": args.steps, "windows": args.windows, "store": [args.images, args.height, args.width], "store_bytes": store.nbytes,
    "pool_ms": round(med["pool"], 4), "source_ms": round(med["source"], 4), "eager_source_ms": round(med["eager_source"], 4),
    "pool_ms_spread": {"min": round(lo, 4), "max": round(hi, 4), "relative": round((hi - lo) / med["pool"], 4)},
    "source_ms_inside_pool_spread": bool(lo <= med["source"] <= hi),
    "source_over_pool": round(med["source"] / med["pool"], 4), "eager_source_over_pool": round(med["eager_source"] / med["pool"], 4),
    "windows_ms": {arm: [round(x, 4) for x in v] for arm, v in windows.items()},
    "final_loss": {arm: round(v, 5) for arm, v in losses.items()}}))
faulthandler.cancel_dump_traceback_later()
