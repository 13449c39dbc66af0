#!/usr/bin/env python3
"""Training iterations of a `predict_normals` nerfacto model driven through the Model API (forward -> get_metrics_dict ->
get_loss_dict -> backward, gradients dropped with set_to_none as a trainer does; no optimiser): the explicit kernel schedule
(`fused_train_step`, fused_step.FusedTrainStep with the normals stage of train_step.NerfactoTrainStep) against the module path
(the composed field of fields/nerfacto_field.py under autograd) — same model, same process, windows of the two alternating,
a host clock around each window that ends in a device synchronise, after warm-up. GPU box only:
    python scripts/bench_normals_training.py [--rays 4096 --windows 7 --steps 20]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfstudio_amd.cameras.rays import RayBundle  # noqa: E402
from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = NerfactoModel(NerfactoModelConfig(predict_normals=True), torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=100)
model = model.to(dev).train()
n = args.rays
rs = np.random.RandomState(0)
d = rs.standard_normal((n, 3)).astype(np.float32)
d /= np.linalg.norm(d, axis=-1, keepdims=True)
origins = torch.from_numpy(rs.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)).to(dev)
directions = torch.from_numpy(d).to(dev)
cams = torch.from_numpy(rs.randint(0, 100, (n, 1))).to(dev)
batch = {"image": torch.from_numpy(rs.uniform(0, 1, (n, 3)).astype(np.float32)).to(dev)}


def step(fused):
    model.config.fused_train_step = fused
    model.zero_grad(set_to_none=True)
    rb = RayBundle(origins=origins, directions=directions, pixel_area=torch.full((n, 1), 1e-6, device=dev), camera_indices=cams)
    out = model(rb)
    losses = model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch))
    sum(losses.values()).backward()
    return losses


def window(fused):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(fused)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.steps


values = {}
for fused in (True, False):
    for _ in range(args.warmup):
        losses = step(fused)
    values[fused] = {k: float(v) for k, v in losses.items()}
    assert all(np.isfinite(v) for v in values[fused].values()), values[fused]
ms = {True: [], False: []}
for _ in range(args.windows):
    for fused in (True, False):
        ms[fused].append(window(fused))
med = {k: float(np.median(v)) for k, v in ms.items()}
print(json.dumps({"metric": "training iteration of a predict_normals model through the Model API, ms per step (no optimiser)",
                  "rays": n, "samples": list(model.config.num_proposal_samples_per_ray) + [model.config.num_nerf_samples_per_ray],
                  "windows": args.windows, "steps_per_window": args.steps,
                  "fused_ms": [round(v, 3) for v in ms[True]], "module_ms": [round(v, 3) for v in ms[False]],
                  "fused_ms_median": round(med[True], 3), "module_ms_median": round(med[False], 3),
                  "speedup": round(med[False] / med[True], 2), "data": "synthetic, random-init weights", "dtype": "f32"}))
