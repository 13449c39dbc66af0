#!/usr/bin/env python3
"""Eval render of a `predict_normals` nerfacto model, one 800 x 800 pinhole frame: the device-side chunk loop with the normals
stages (eval_render.EvalRenderer(normals=True): nsamd_field_normals, the predicted-normals MLP, nsamd_normals_composite inside
the captured chunk schedule) against the module path's Python chunk loop (NSAMD_EVAL_RUNNER=0: the field composed of the
stand-alone kernels, torch.autograd.grad for the analytic normals, torch.cat per chunk) — same model, same process, the two
alternating, HIP events after warm-up. GPU box only:  python scripts/bench_render_normals.py [--height 800 --width 800 --frames 3]
Prints one JSON line; --stages adds one eager chunk with an event pair around the three added stages."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfstudio_amd import eval_render  # noqa: E402
from nerfstudio_amd.model_components.ray_generators import RayGenerator  # noqa: E402
from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--height", type=int, default=800)
ap.add_argument("--width", type=int, default=800)
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--stages", action="store_true")
ap.add_argument("--device-only", action="store_true", help="time the device-side loop alone (a kernel trace of it)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = NerfactoModel(NerfactoModelConfig(predict_normals=True), torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=100)
model = model.to(dev).eval()
H, W = args.height, args.width


class Cams:
    pass


cams = Cams()
c2w = np.eye(4, dtype=np.float32)[:3]
c2w[:, 3] = (0.0, 0.0, 0.9)
cams.camera_to_worlds = torch.from_numpy(c2w)[None].to(dev)
cams.fx = cams.fy = torch.tensor([[0.9 * W]])
cams.cx, cams.cy = torch.tensor([[W / 2.0]]), torch.tensor([[H / 2.0]])
cams.height, cams.width = torch.tensor([[H]]), torch.tensor([[W]])
cams.camera_type = torch.tensor([[1]])
cams.distortion_params = None
yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
idx = torch.stack([torch.zeros_like(yy), yy, xx], dim=-1).reshape(-1, 3).to(dev)
bundle = RayGenerator(cams).to(dev)(idx).reshape((H, W))


def frame(device_loop):
    os.environ["NSAMD_EVAL_RUNNER"] = "1" if device_loop else "0"
    return model.get_outputs_for_camera_ray_bundle(bundle)


def timed(device_loop):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = frame(device_loop)
    b.record()
    torch.cuda.synchronize()
    assert out["normals"].shape == (H, W, 3) and bool(torch.isfinite(out["pred_normals"]).all())
    return a.elapsed_time(b)


loops = (True,) if args.device_only else (True, False)
for loop in loops:  # warm-up: graph capture, first launches
    frame(loop)
    frame(loop)
torch.cuda.synchronize()
ms = {True: [], False: []}
for _ in range(args.frames):
    for loop in loops:
        ms[loop].append(timed(loop))
res = {"metric": "eval render of a predict_normals model, ms per frame", "image": [H, W],
       "chunk": model.config.eval_num_rays_per_chunk, "device_loop_ms": [round(v, 2) for v in ms[True]],
       "module_loop_ms": [round(v, 2) for v in ms[False]], "device_loop_ms_median": round(float(np.median(ms[True])), 2),
       "module_loop_ms_median": round(float(np.median(ms[False])), 2) if ms[False] else None, "data": "synthetic, random-init weights", "dtype": "f32"}
if args.stages:
    os.environ["NSAMD_EVAL_RUNNER"] = "1"
    r = eval_render.runner_for(model, dev)
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    r.normals = False
    a.record()
    r._launch_chunk()
    b.record()
    r.normals = True
    r._launch_normals()
    c.record()
    torch.cuda.synchronize()
    res["one_chunk_eager_ms"] = {"plain_schedule": round(a.elapsed_time(b), 3), "normals_stages": round(b.elapsed_time(c), 3)}
    m = r.step.m_main
    res["field_normals_algorithmic_bytes_per_chunk"] = m * (1024 + 128 + 12 + 60)
print(json.dumps(res))
