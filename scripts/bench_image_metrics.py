#!/usr/bin/env python3
"""The eval image metrics and colormaps, measured (profiles/image_metrics.txt).

    python scripts/bench_image_metrics.py --cpu-table [--out FILE]     (no GPU: the error table the tests' bounds come from)
    python scripts/bench_image_metrics.py [--size 800] [--out FILE --append]    (one MI355X: the timings)

--cpu-table: the host build of csrc/image_metrics.h (tests/hostcheck/image_helpers.cc) against the float64 restatement
(tests/image_metrics_reference.py) on the tests' images at the CPU and the GPU tests' sizes, C = 3 and 1, R from the images and
R = 1: the largest per-window error and the largest error of the mean, next to the fp32 conv2d composition's. The tests hold the
host build and the kernels to 4 x the table's maxima (image_metrics_reference.WINDOW_BOUND, MEAN_BOUND).

The timings, at --size x --size x 3, each arm in --repeats alternating runs after a warm-up of each, medians and [min .. max]:
    metrics   nsamd_image_range x 2 + nsamd_image_metrics with device ranges: the launches alone (device events around --batch
              calls), ImageMetrics.measure (host clock around a call and a synchronise), and the same work as the fp32 torch
              composition the tests restate (reflect pad, conv2d over five stacked images, the elementwise tail, mse and
              log10), with the three host reads of the reference's float(...) calls
    colormaps the four maps of a nerfacto frame (accumulation, depth, two proposal depths) through nsamd_image_range +
              nsamd_colormap, and the reference's functions restated as torch ops on the same GPU with their host reads
              (float(min), float(max) per depth map, two asserts per table lookup)
    set       eval.average_image_metrics per frame over --frames cameras of an untrained default nerfacto model, against the
              render alone (Model.get_outputs_for_camera)
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import image_metrics_reference as im  # noqa: E402

GPU_SIZES = ((11, 64), (41, 42), (42, 43), (43, 76))  # 11 x 64 and the tile edges (T + 9) x (T + 10) ... for T = 32


def cpu_table(say):
    lib = im.host_library(tempfile.mkdtemp())
    say("host build of csrc/image_metrics.h against float64 (|error|, per window: the largest over the map; mean: of the SSIM value)")
    say(f"{'image':10s} {'size':>9s} {'R':>4s} | {'host window':>11s} {'host mean':>10s} | {'fp32 conv window':>16s} {'fp32 conv mean':>14s} | "
        f"{'mse rel':>8s} {'psnr abs':>8s}")
    worst = dict(window=0.0, mean=0.0, mse=0.0, psnr=0.0, ratio=np.inf)
    by_kind = {}
    for kind in im.KINDS:
        for H, W in im.SIZES + GPU_SIZES:
            for C in (3, 1):
                pred, target = im.image_pair(kind, H, W, C)
                for R in (None, 1.0):
                    ref = im.metrics(pred, target, R)
                    out, ssim_map = im.host_metrics(lib, pred, target, R)
                    f32 = im.ssim_map_conv(pred, target, ref["R"], torch.float32).numpy().astype(np.float64)
                    ew, em = np.abs(ssim_map - ref["map"]).max(), abs(float(out[2]) - ref["ssim"])
                    fw, fm = np.abs(f32 - ref["map"]).max(), abs(f32.mean() - ref["ssim"])
                    emse, epsnr = abs(float(out[0]) - ref["mse"]) / ref["mse"], abs(float(out[1]) - ref["psnr"])
                    say(f"{kind:10s} {f'{H}x{W}x{C}':>9s} {'dev' if R is None else '1':>4s} | {ew:11.2e} {em:10.2e} | {fw:16.2e} {fm:14.2e} | "
                        f"{emse:8.1e} {epsnr:8.1e}")
                    worst["window"], worst["mean"] = max(worst["window"], ew), max(worst["mean"], em)
                    by_kind[kind] = (max(by_kind.get(kind, (0, 0))[0], ew), max(by_kind.get(kind, (0, 0))[1], em))
                    worst["mse"], worst["psnr"] = max(worst["mse"], emse), max(worst["psnr"], epsnr)
                    if kind == "half_flat" and min(H, W) > 11:
                        worst["ratio"] = min(worst["ratio"], fm / em)
    say(f"maxima: per window {worst['window']:.2e}, mean {worst['mean']:.2e}, mse relative {worst['mse']:.1e}, psnr absolute {worst['psnr']:.1e}; "
        f"on the half-flat pairs the fp32 composition's error of the mean is at least {worst['ratio']:.0f} x the host build's")
    say("the tests' bounds, 4 x the maxima per kind of image (image_metrics_reference.BOUNDS): "
        + "; ".join(f"{k}: per window 4 x {w:.2e}, mean 4 x {m:.2e}" for k, (w, m) in by_kind.items()))


def torch_metrics(pred, target):
    """the library path as fp32 torch ops with its host reads: (psnr, ssim) as Python floats"""
    R = float(max(pred.max() - pred.min(), target.max() - target.min()))
    ssim = float(im.ssim_map_conv(pred, target, R, torch.float32).mean())
    psnr = float(10.0 * torch.log10(1.0 / torch.mean((pred - target) ** 2)))
    return psnr, ssim


def torch_depth_colormap(depth, acc, lut):
    """utils/colormaps.py:120-152 and :93-117 as torch ops, with their host reads"""
    near, far = float(torch.min(depth)), float(torch.max(depth))
    t = torch.clip((depth - near) / (far - near + 1e-10), 0, 1)
    t = torch.nan_to_num(torch.clip(t * 1.0 + 0.0, 0, 1), 0)
    rows = (t * 255).long()
    assert torch.min(rows) >= 0
    assert torch.max(rows) <= 255
    return lut[rows[..., 0]] * acc + (1 - acc)


def torch_plain_colormap(image, lut):
    t = torch.nan_to_num(torch.clip(image * 1.0 + 0.0, 0, 1), 0)
    rows = (t * 255).long()
    assert torch.min(rows) >= 0
    assert torch.max(rows) <= 255
    return lut[rows[..., 0]]


def alternate(arms, repeats):
    """{name: [ms per run]} of the arms run in turn, after one warm-up run of each"""
    times = {name: [] for name in arms}
    for run in range(repeats + 1):
        for name, arm in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            torch.cuda.synchronize()
            if run:
                times[name].append(1e3 * (time.perf_counter() - t0))
    return times


def line(name, ms, unit="ms"):
    return f"  {name:44s} {statistics.median(ms):8.3f} {unit}  [{min(ms):.3f} .. {max(ms):.3f}]"


def timings(a, say):
    from nerfstudio_amd import eval as eval_images
    from nerfstudio_amd.image_metrics import ImageMetrics
    from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig
    from nerfstudio_amd.utils import colormaps as cm

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, S = "cuda", a.size
    say(f"{torch.cuda.get_device_name(0)}; {S} x {S} x 3 frames; {a.repeats} alternating runs per arm after one warm-up of each")
    pred, target = (torch.from_numpy(x).to(dev) for x in im.image_pair("sinusoid", S, S, 3))
    measure = ImageMetrics()
    out = measure.measure(pred, target)
    psnr, ssim = torch_metrics(pred, target)
    say(f"metrics of the pair: kernels psnr {float(out[1]):.5f} ssim {float(out[2]):.7f}; fp32 torch composition psnr {psnr:.5f} ssim {ssim:.7f}")
    launches = []
    for _ in range(a.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch):
            measure.measure_into(pred, target, out)
        e1.record()
        torch.cuda.synchronize()
        launches.append(e0.elapsed_time(e1) / a.batch)
    say("metrics:")
    say(line(f"the four launches alone (device events / {a.batch})", launches[1:]))
    t = alternate({"ImageMetrics.measure + synchronise": lambda: measure.measure(pred, target),
                   "ImageMetrics.measure + read of the [4]": lambda: measure.measure(pred, target).tolist(),
                   "fp32 torch composition, 3 host reads": lambda: torch_metrics(pred, target)}, a.repeats)
    for name, ms in t.items():
        say(line(name, ms))

    torch.manual_seed(0)
    depth = [torch.rand(S, S, 1, device=dev) * 6 + 0.2 for _ in range(3)]
    acc = torch.rand(S, S, 1, device=dev)
    lut = torch.linspace(0, 1, 256, device=dev)[:, None].expand(256, 3).contiguous()

    def device_maps():
        cm.apply_colormap(acc, lut=lut)
        for d in depth:
            cm.apply_depth_colormap(d, accumulation=acc, lut=lut)

    def torch_maps():
        torch_plain_colormap(acc, lut)
        for d in depth:
            torch_depth_colormap(d, acc, lut)

    same = int((cm.apply_depth_colormap(depth[0], accumulation=acc, lut=lut) != torch_depth_colormap(depth[0], acc, lut)).any(-1).sum())
    say(f"colormaps (accumulation, depth, two proposal depths); {same} of {S * S} depth pixels differ from the torch restatement on this GPU "
        "(its x / scalar is x * (1 / scalar) there; the definition is the CPU's):")
    for name, ms in alternate({"kernels (3 ranges + 4 colormaps), synchronise": device_maps, "torch ops, 14 host reads": torch_maps}, a.repeats).items():
        say(line(name, ms))

    model = NerfactoModel(NerfactoModelConfig(), torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 8).to(dev).eval()
    cameras = im.orbit_cameras(a.frames, S, S)  # the tests' cameras
    frames = [(c, {"image": torch.rand(S, S, 3, device=dev)}) for c in cameras]

    def render_only():
        for c in cameras:
            model.get_outputs_for_camera(c)

    say(f"a set of {a.frames} cameras, untrained default nerfacto (ms per frame):")
    arms = {"render alone": render_only, "average_image_metrics": lambda: eval_images.average_image_metrics(model, frames)}
    for name, ms in alternate(arms, a.repeats).items():
        say(line(name, [m / a.frames for m in ms]))
    with tempfile.TemporaryDirectory() as tmp:
        arms = {"average_image_metrics + 5 PNGs per frame": lambda: eval_images.average_image_metrics(model, frames, output_path=tmp)}
        for name, ms in alternate(arms, 3).items():
            say(line(name, [m / a.frames for m in ms]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-table", action="store_true")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it")
    a = ap.parse_args()
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))  # noqa: E731
    if a.cpu_table:
        say("Eval image metrics and colormaps (include/nsamd_image.h, csrc/image_metrics.hip): the CPU error table the tests' bounds were")
        say("taken from, then the timings on one MI355X. Both parts are this script's output: --cpu-table --out FILE starts the file, the")
        say("GPU run with --out FILE --append adds to it.")
        say("")
        say("== python scripts/bench_image_metrics.py --cpu-table")
        cpu_table(say)
    else:
        say("")
        say(f"== python scripts/bench_image_metrics.py --size {a.size} --frames {a.frames} --repeats {a.repeats}")
        timings(a, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
