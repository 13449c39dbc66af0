#!/usr/bin/env python3
"""Time of the ray-generation kernels at the training batch (4096 rays by default): nsamd_raygen_pinhole against
nsamd_raygen_lens for distorted perspective cameras, fisheye cameras with k1..k4, and one Cameras mixing types 1, 2, 3 (waves
diverge by type). Device events around `--launches` back-to-back launches, after a warm-up of every shape. GPU box only:
    python scripts/bench_raygen.py [--rays 4096 --cameras 200 --launches 2000 --repeats 3]
Prints one JSON line (microseconds per launch, best and worst repeat)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfstudio_amd import functional as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--cameras", type=int, default=200)
ap.add_argument("--launches", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
C, H, W = args.cameras, 540, 960
rot = torch.linalg.qr(torch.randn(C, 3, 3, generator=g))[0]
c2w = torch.cat([rot, torch.randn(C, 3, 1, generator=g)], dim=-1).to(dev)
fx, fy = (torch.empty(C).uniform_(0.8 * W, 1.0 * W, generator=g).to(dev) for _ in range(2))
cx = (W / 2 + torch.empty(C).uniform_(-1, 1, generator=g)).to(dev)
cy = (H / 2 + torch.empty(C).uniform_(-1, 1, generator=g)).to(dev)
idx = torch.stack([torch.randint(0, C, (args.rays,), generator=g), torch.randint(0, H, (args.rays,), generator=g),
                   torch.randint(0, W, (args.rays,), generator=g)], dim=-1).to(dev)
colmap = torch.tensor([-0.12, 0.03, 0.0, 0.0, 1e-3, -2e-3]).expand(C, 6).contiguous().to(dev)
fish_k = torch.tensor([0.04, -0.006, 0.002, -0.0004, 0.0, 0.0]).expand(C, 6).contiguous().to(dev)
types = {t: torch.full((C,), t, dtype=torch.int32, device=dev) for t in (1, 2)}
fx_fish, fy_fish = fx / 2, fy / 2
mixed = (torch.arange(C, dtype=torch.int32) % 3 + 1).to(dev)
cases = {
    "raygen_pinhole": lambda: F.raygen_pinhole(idx, c2w, fx, fy, cx, cy),
    "raygen_lens perspective, no distortion": lambda: F.raygen_lens(idx, c2w, fx, fy, cx, cy, types[1], None, check_types=False),
    "raygen_lens perspective, k1 k2 p1 p2": lambda: F.raygen_lens(idx, c2w, fx, fy, cx, cy, types[1], colmap, check_types=False),
    "raygen_lens fisheye, k1..k4": lambda: F.raygen_lens(idx, c2w, fx_fish, fy_fish, cx, cy, types[2], fish_k, check_types=False),
    "raygen_lens types 1, 2, 3 mixed, distorted": lambda: F.raygen_lens(idx, c2w, fx, fy, cx, cy, mixed, colmap, check_types=False),
}
out = {}
for name, fn in cases.items():
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.launches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / args.launches)
    out[name] = {"us_best": round(min(times), 2), "us_worst": round(max(times), 2)}
print(json.dumps({"metric": "ray generation, us per launch incl. its four output allocations (device events, back-to-back launches)",
                  "rays": args.rays, "cameras": C, "launches": args.launches, "cases": out}))
