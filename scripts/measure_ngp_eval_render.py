"""Full-image eval render of the benchmark's synthetic instant-ngp workload (scripts/bench_ngp.py builds it), one 800 x 800 frame:

  (a) the module-path loop over `forward` (NSAMD_EVAL_RUNNER=0: what NGPModel.get_outputs_for_camera_ray_bundle ran before the runner)
  (b) ngp_eval_render.NgpEvalRenderer on the same bundle, prefetch on and off

7 frames each after warm-up, the routes ALTERNATING frame by frame in one process; a frame's time is a host clock around work
that ends in a device synchronise. Also per route and chunk: the native entry-point calls (counted by _native.PROFILE) and the
aten operators dispatched (TorchDispatchMode; views included — an upper bound of torch's launches, not a kernel count), from one
extra frame outside the timed ones. The lines go to --out (profiles/ngp_eval_render.txt). Needs a GPU; there is no fallback.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FRAMES, WARMUP = 7, 2


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngp_eval_render.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_ngp_eval_render needs a GPU"
    from torch.utils._python_dispatch import TorchDispatchMode

    from bench_ngp import build_ngp_model
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.cameras.rays import RayBundle
    from nerfstudio_amd.ngp_eval_render import NgpEvalRenderer

    dev = torch.device("cuda", 0)
    model, _ = build_ngp_model(dev)
    model.eval()
    S = args.size
    chunk = model.config.eval_num_rays_per_chunk
    chunks = (S * S + chunk - 1) // chunk
    # a camera 3.5 units from the centre of the region of interest, looking at it, ~53 degrees across
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.2], [0.0, 1.0, 0.0, -0.1], [0.0, 0.0, 1.0, 3.5]], device=dev)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    idx = torch.stack([torch.zeros_like(yy), yy, xx], dim=-1).reshape(-1, 3).to(dev)
    one = lambda v: torch.tensor([float(v)], device=dev)  # noqa: E731
    o, d, pa, _ = F.raygen_pinhole(idx, c2w[None], one(S), one(S), one(S / 2), one(S / 2))
    frame = RayBundle(origins=o.view(S, S, 3), directions=d.view(S, S, 3), pixel_area=pa.view(S, S, 1),
                      camera_indices=torch.zeros(S, S, 1, dtype=torch.long, device=dev))
    runners = {"runner, prefetch": NgpEvalRenderer(model, prefetch=True), "runner, no prefetch": NgpEvalRenderer(model, prefetch=False)}

    def module_path():
        os.environ["NSAMD_EVAL_RUNNER"] = "0"
        try:
            return model.get_outputs_for_camera_ray_bundle(frame)
        finally:
            del os.environ["NSAMD_EVAL_RUNNER"]

    routes = {"module-path loop": module_path, **{k: (lambda r=r: r.render(frame)) for k, r in runners.items()}}

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))

    outs, counts = {}, {}
    for name, fn in routes.items():
        for _ in range(WARMUP):
            outs[name] = fn()
        torch.cuda.synchronize()
        Count.n, N.PROFILE = 0, {}
        with Count():
            fn()
        torch.cuda.synchronize()
        counts[name] = (sum(len(v) for v in N.PROFILE.values()) / chunks, Count.n / chunks)
        N.PROFILE = None
    ref = outs["module-path loop"]
    samples = int(ref["num_samples_per_ray"].sum())
    for name, out in outs.items():
        assert torch.equal(out["num_samples_per_ray"].reshape(-1), ref["num_samples_per_ray"].reshape(-1)), name
    rgb_gap = max(float((out["rgb"] - ref["rgb"]).abs().max()) for out in outs.values())
    times = {name: [] for name in routes}
    for _ in range(FRAMES):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    lines = [f"instant-ngp eval render, {S} x {S} frame of the benchmark's synthetic workload ({N.device_info()['arch']}): {chunks} chunks of "
             f"{chunk} rays, {samples} samples per frame ({samples / (S * S):.1f} per ray); {FRAMES} frames per route after {WARMUP + 1} "
             "warm-up frames, routes alternating frame by frame; wall clock per frame around a device synchronise; sample counts of the "
             f"routes equal, largest |rgb difference| between them {rgb_gap:.2e}",
             "route | median ms | min ms | max ms | M rays/s (median) | native entry-point calls per chunk | aten operators dispatched per chunk"]
    for name, ms in times.items():
        med = statistics.median(ms)
        lines.append(f"{name} | {med:.2f} | {min(ms):.2f} | {max(ms):.2f} | {S * S / med / 1e3:.2f} | {counts[name][0]:.1f} | {counts[name][1]:.1f}")
    a, b, c = (times[k] for k in ("module-path loop", "runner, prefetch", "runner, no prefetch"))

    def verdict(x, y, what):  # x faster than y by more than the spread of the frames?
        gap, spread = statistics.median(y) - statistics.median(x), max(max(x) - min(x), max(y) - min(y))
        word = "beyond" if abs(gap) > spread else "WITHIN"
        return f"{what}: {statistics.median(y) / statistics.median(x):.3f} x (median gap {gap:+.2f} ms, largest spread of the two routes' frames {spread:.2f} ms: {word} the spread)"

    lines.append(verdict(b, a, "runner with prefetch against the module-path loop"))
    lines.append(verdict(b, c, "prefetch against no prefetch"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
