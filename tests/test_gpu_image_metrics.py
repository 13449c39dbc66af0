"""GPU tests of the eval image metrics: nsamd_image_metrics and nsamd_image_range (csrc/image_metrics.hip over
csrc/image_metrics.h) entry by entry against the float64 restatement of tests/image_metrics_reference.py under the bounds its
docstring gives (the ones tests/test_image_metrics_cpu.py holds the host build to), and a small nerfacto and a small instant-ngp
model end to end: get_image_metrics_and_images and eval.average_image_metrics on frames their runners render. Every comparison
prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import image_metrics_reference as im

pytestmark = pytest.mark.gpu
T = torch.from_numpy
POISON, GUARD = -77.0, 512
TILE = 32
SIZES = ((11, 11), (11, 64), (TILE + 9, TILE + 10), (TILE + 10, TILE + 11), (TILE + 11, 2 * TILE + 12), (64, 97))


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    info = _native.device_info()
    assert info["wavefront_size"] == 64 and info["arch"].startswith("gfx950"), info
    assert _native.SSIM_TILE == TILE
    return functional


def guarded(numel, dtype, fill):
    slab = torch.full((GUARD + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return slab, slab[GUARD:GUARD + numel]


def intact(slab, numel, fill):
    return bool((slab[:GUARD] == fill).all()) and bool((slab[GUARD + numel:] == fill).all())


def launch_metrics(F, pred, target, R=None, with_map=True):
    """-> ({mse, psnr, ssim, R} fp32 [4], map or None) on the host, through the launch helpers with guard regions around out4,
    the map and the scratch (asserted intact); R None: ranges from nsamd_image_range on the device"""
    from nerfstudio_amd import _native as N

    pred, target = T(np.ascontiguousarray(pred)).cuda(), T(np.ascontiguousarray(target)).cuda()
    H, W, Ch = pred.shape
    nbytes = F.image_metrics_scratch_bytes(H, W, Ch)
    assert nbytes == 16 * ((H - 10 + TILE - 1) // TILE) * ((W - 10 + TILE - 1) // TILE)
    slabs = [guarded(4, torch.float32, POISON), guarded((H - 10) * (W - 10) * Ch, torch.float32, POISON), guarded(nbytes, torch.uint8, 0x5A)]
    out, ssim_map, scratch = slabs[0][1], slabs[1][1].view(H - 10, W - 10, Ch), slabs[2][1]
    ranges = None
    if R is None:
        ranges = torch.empty(2, 2, device="cuda")
        range_scratch = torch.empty(2 * N.RANGE_SCRATCH_BYTES, dtype=torch.uint8, device="cuda")
        F.image_range_launch(pred, range_scratch, ranges[0])
        F.image_range_launch(target, range_scratch[N.RANGE_SCRATCH_BYTES:], ranges[1])
    F.image_metrics_launch(pred, target, None if ranges is None else ranges[0], None if ranges is None else ranges[1], 0.0 if R is None else R,
                           1.0, scratch, out, ssim_map if with_map else None)
    torch.cuda.synchronize()
    assert intact(slabs[0][0], 4, POISON) and intact(slabs[1][0], ssim_map.numel(), POISON) and intact(slabs[2][0], nbytes, 0x5A)
    if not with_map:
        assert bool((ssim_map == POISON).all())
    return out.cpu().numpy(), ssim_map.cpu().numpy() if with_map else None


# ---------------------------------------------------------------- nsamd_image_metrics ---------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("kind", im.KINDS)
def test_metrics_against_float64_per_window_and_on_the_scalars(F, kind, H, W):
    for Ch in (3, 1):
        pred, target = im.image_pair(kind, H, W, Ch)
        for R in (None, 1.0):
            ref = im.metrics(pred, target, R)
            out, ssim_map = launch_metrics(F, pred, target, R)
            im.check_against_float64(out, ssim_map, ref, kind, f"gpu {kind} {H}x{W}x{Ch} R={R}")
            plain, _ = launch_metrics(F, pred, target, R, with_map=False)
            assert np.array_equal(plain.view(np.uint32), out.view(np.uint32))  # bit-identical without the map


@pytest.mark.parametrize("H,W", ((41, 43), (64, 97)))
def test_half_flat_pair_beats_the_fp32_composition_on_the_same_gpu(F, H, W):
    pred, target = im.image_pair("half_flat", H, W, 3)
    for R in (None, 1.0):
        ref = im.metrics(pred, target, R)
        out, _ = launch_metrics(F, pred, target, R)
        f32 = im.ssim_map_conv(T(pred).cuda(), T(target).cuda(), ref["R"], torch.float32).double().mean().item()
        e_kernel, e_f32 = abs(float(out[2]) - ref["ssim"]), abs(f32 - ref["ssim"])
        print(f"half-flat {H}x{W} R={R}: kernel {e_kernel:.2e}, fp32 torch composition on this GPU {e_f32:.2e}")
        assert e_kernel <= 0.1 * e_f32


def test_same_bits_run_to_run_and_replayed_from_a_captured_graph(F):
    from nerfstudio_amd.image_metrics import ImageMetrics

    pred, target = (T(a).cuda() for a in im.image_pair("sinusoid", TILE + 11, 2 * TILE + 12, 3))
    measure = ImageMetrics()
    runs = [measure.measure(pred, target).cpu() for _ in range(3)]
    assert all(torch.equal(r.view(torch.int32), runs[0].view(torch.int32)) for r in runs[1:])
    row = torch.zeros(4, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        measure.measure_into(pred, target, row)  # (warm-up on the capture stream: the buffers exist)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        measure.measure_into(pred, target, row)
    row.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(row.cpu().view(torch.int32), runs[0].view(torch.int32))
    other = T(im.image_pair("ramp", TILE + 11, 2 * TILE + 12, 3)[0]).cuda()
    expect = measure.measure(other, target).cpu()
    pred.copy_(other)  # the graph reads the buffers it captured
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(row.cpu().view(torch.int32), expect.view(torch.int32))


def test_edge_cases_on_the_device(F):
    flat, other = np.full((20, 23, 3), 0.37, np.float32), np.full((20, 23, 3), 0.52, np.float32)
    out, ssim_map = launch_metrics(F, flat, other)  # R = 0: the formula's 0 / 0, not an error
    assert out[3] == 0 and np.isnan(out[2]) and np.isnan(ssim_map).all() and np.isfinite(out[:2]).all()
    out, ssim_map = launch_metrics(F, flat, flat.copy(), 1.0)
    assert out[0] == 0 and np.isposinf(out[1]) and abs(out[2] - 1) <= im.BOUNDS["sinusoid"][1]
    pred, target = im.image_pair("sinusoid", TILE + 11, 2 * TILE + 12, 3)
    pred[40, 70, 2] = np.nan
    out, ssim_map = launch_metrics(F, pred, target, 1.0)
    expect = np.zeros(ssim_map.shape, bool)
    expect[30:41, 60:71, 2] = True
    assert np.isnan(out[:3]).all() and np.array_equal(np.isnan(ssim_map), expect)
    out, _ = launch_metrics(F, pred, target)
    assert np.isnan(out).all()


# ---------------------------------------------------------------- nsamd_image_range -----------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 256 * 1024, 256 * 1024 + 1))
def test_range_against_aminmax(F, n):
    """(256 * 1024 values fill the grid's 1024 workgroups once; one more starts the stride)"""
    from nerfstudio_amd import _native as N

    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).cuda()
    slab, out = guarded(2, torch.float32, POISON)
    sslab, scratch = guarded(N.RANGE_SCRATCH_BYTES, torch.uint8, 0x5A)

    def run(v):
        F.image_range_launch(v, scratch, out)
        torch.cuda.synchronize()
        assert intact(slab, 2, POISON) and intact(sslab, N.RANGE_SCRATCH_BYTES, 0x5A)
        return out.cpu()

    lo, hi = torch.aminmax(x)
    assert run(x).tolist() == [float(lo), float(hi)]
    for at in sorted({0, n // 2, n - 1}):
        y = x.clone()
        y[at] = float("nan")
        assert bool(torch.isnan(run(y)).all()), at
    assert run(x).tolist() == [float(lo), float(hi)]  # and no NaN left behind in the scratch


# ---------------------------------------------------------------- end to end ------------------------------------------------------
H_, W_ = 48, 64


def small_model(kind):
    if kind == "nerfacto":
        from test_gpu_texture import make_model

        return make_model()
    from test_gpu_ngp_eval_render import _model

    return _model()


@pytest.fixture(scope="module")
def turbo():
    """the table comes from the fixture: nothing here needs matplotlib"""
    from conftest import load_golden
    from nerfstudio_amd.utils import colormaps

    lut = T(load_golden("colormaps")["lut_turbo"])
    colormaps.set_colormap_lut("turbo", lut, "cuda")
    return lut.cuda()


@pytest.mark.parametrize("kind", ("nerfacto", "ngp"))
def test_models_end_to_end(F, turbo, kind, monkeypatch, tmp_path):
    from nerfstudio_amd import eval as E
    from nerfstudio_amd.utils import colormaps
    from test_texture_cpu import read_png

    model = small_model(kind)
    cameras = im.orbit_cameras(3, H_, W_, focal=45.0)
    g = torch.Generator().manual_seed(7)
    batches = [{"image": torch.rand(H_, W_, 4, generator=g).cuda()} for _ in cameras]
    # one frame through the model's runner, its metrics against float64 on the same outputs
    outputs = model.get_outputs_for_camera(cameras[0])
    assert tuple(outputs["rgb"].shape) == (H_, W_, 3)
    metrics, images = model.get_image_metrics_and_images(outputs, batches[0])
    gt = model.renderer_rgb.blend_background(batches[0]["image"])
    ref = im.metrics(gt.cpu().numpy(), outputs["rgb"].cpu().numpy())
    print(f"{kind}: psnr {metrics['psnr']:.5f} (float64 {ref['psnr']:.5f}), ssim {metrics['ssim']:.7f} (float64 {ref['ssim']:.7f})")
    mean_bound = max(b[1] for b in im.BOUNDS.values())  # a rendered frame is none of the three kinds: the largest of their bounds
    assert abs(metrics["psnr"] - ref["psnr"]) <= im.psnr_bound(ref["psnr"]) and abs(metrics["ssim"] - ref["ssim"]) <= mean_bound
    props = [k for k in outputs if k.startswith("prop_depth_")]
    assert list(metrics) == ["psnr", "ssim"] and list(images) == ["img", "accumulation", "depth"] + sorted(props)
    assert torch.equal(images["depth"], colormaps.apply_depth_colormap(outputs["depth"], accumulation=outputs["accumulation"], lut=turbo))
    assert tuple(images["img"].shape) == (H_, 2 * W_, 3) and torch.equal(images["img"][:, :W_], gt)
    # the set: equal to per-frame calls bit for bit, one read, PNGs of the device's 8-bit maps
    frames = list(zip(cameras, batches))
    reads = []
    monkeypatch.setattr(E, "read_rows", lambda rows, read=E.read_rows: (reads.append(tuple(rows.shape)), read(rows))[1])
    out = E.average_image_metrics(model, frames, output_path=tmp_path, get_std=True)
    assert reads == [(3, 4)]
    per_frame = [model.get_image_metrics_and_images(model.get_outputs_for_camera(c), b) for c, b in frames]
    for key in ("psnr", "ssim"):
        std, mean = torch.std_mean(torch.tensor([m[key] for m, _ in per_frame]))
        assert out[key] == float(mean) and out[f"{key}_std"] == float(std), key
    assert out["fps"] > 0 and out["num_rays_per_sec"] == pytest.approx(out["fps"] * H_ * W_, rel=1e-5)
    for k, (_, pictures) in enumerate(per_frame):
        for key, image in pictures.items():
            assert np.array_equal(read_png(tmp_path / f"eval_{key}_{k:04d}.png"), E.image_u8(image).cpu().numpy()), (k, key)
    # the module path: its frames' metrics against float64 of ITS outputs under the recorded bounds, and how far the two paths'
    # averages lie apart (a figure: their rgb agree to the 2e-6 of the runners' own tests, not bit for bit)
    monkeypatch.setenv("NSAMD_EVAL_RUNNER", "0")
    try:
        module = E.average_image_metrics(model, frames)
        refs = [im.metrics(model.renderer_rgb.blend_background(b["image"]).cpu().numpy(), model.get_outputs_for_camera(c)["rgb"].cpu().numpy())
                for c, b in frames]
    finally:
        monkeypatch.delenv("NSAMD_EVAL_RUNNER")
    ref_psnr = float(torch.mean(torch.tensor([r["psnr"] for r in refs])))
    ref_ssim = float(np.mean([r["ssim"] for r in refs]))
    print(f"{kind}: module path psnr {module['psnr']:.7f} (float64 {ref_psnr:.7f}), ssim {module['ssim']:.9f} (float64 {ref_ssim:.9f}); "
          f"runner - module path: psnr {out['psnr'] - module['psnr']:.2e}, ssim {out['ssim'] - module['ssim']:.2e}")
    assert abs(module["psnr"] - ref_psnr) <= im.psnr_bound(ref_psnr) + float(np.spacing(np.float32(ref_psnr)))  # + the fp32 mean of three
    assert abs(module["ssim"] - ref_ssim) <= mean_bound + 2.0 ** -24


@pytest.mark.parametrize("kind", ("vanilla", "mipnerf"))
def test_two_pass_models_end_to_end(F, turbo, kind, monkeypatch, tmp_path):
    """NeRFModel / MipNerfModel: no runner, every frame is the module chunk loop; two rows of metrics per frame"""
    from nerfstudio_amd import eval as E
    from nerfstudio_amd.mipnerf import MipNerfModel, MipNerfModelConfig
    from nerfstudio_amd.vanilla_nerf import NeRFModel, VanillaModelConfig
    from test_texture_cpu import read_png

    torch.manual_seed(3)
    sizes = dict(num_coarse_samples=16, num_importance_samples=16, eval_num_rays_per_chunk=1000)  # 3072 rays: a short last chunk
    model = (NeRFModel(VanillaModelConfig(**sizes)) if kind == "vanilla" else MipNerfModel(MipNerfModelConfig(**sizes))).cuda().eval()
    cameras = im.orbit_cameras(2, H_, W_, focal=45.0)
    for c in cameras:  # inside the models' near and far planes
        c.camera_to_worlds[:, 3] *= 2.4
    g = torch.Generator().manual_seed(11)
    frames = [(c, {"image": torch.rand(H_, W_, 4, generator=g).cuda()}) for c in cameras]
    reads = []
    monkeypatch.setattr(E, "read_rows", lambda rows, read=E.read_rows: (reads.append(tuple(rows.shape)), read(rows))[1])
    out = E.average_image_metrics(model, frames, output_path=tmp_path)
    assert reads == [(4, 4)] and list(out) == ["psnr", "coarse_psnr", "fine_psnr", "fine_ssim", "num_rays_per_sec", "fps"]
    mean_bound = max(b[1] for b in im.BOUNDS.values())
    per_frame, refs = [], []
    for c, b in frames:
        outputs = model.get_outputs_for_camera(c)
        assert tuple(outputs["rgb_fine"].shape) == (H_, W_, 3) and tuple(outputs["depth_coarse"].shape) == (H_, W_, 1)
        per_frame.append(model.get_image_metrics_and_images(outputs, b))
        gt = model.renderer_rgb.blend_background(b["image"]).cpu().numpy()
        clip = (lambda a: np.clip(a, 0, 1)) if kind == "mipnerf" else (lambda a: a)
        refs.append((im.metrics(gt, clip(outputs["rgb_coarse"].cpu().numpy())), im.metrics(gt, clip(outputs["rgb_fine"].cpu().numpy()))))
    for (m, images), (rc, rf) in zip(per_frame, refs):
        print(f"{kind}: fine psnr {m['fine_psnr']:.5f} (float64 {rf['psnr']:.5f}), coarse {m['coarse_psnr']:.5f} ({rc['psnr']:.5f}), "
              f"fine ssim {m['fine_ssim']:.7f} ({rf['ssim']:.7f})")
        assert abs(m["fine_psnr"] - rf["psnr"]) <= im.psnr_bound(rf["psnr"]) and abs(m["coarse_psnr"] - rc["psnr"]) <= im.psnr_bound(rc["psnr"])
        assert abs(m["fine_ssim"] - rf["ssim"]) <= mean_bound and m["psnr"] == m["fine_psnr"]
        assert tuple(images["img"].shape) == (H_, 3 * W_, 3) and tuple(images["depth"].shape) == (H_, 2 * W_, 3)
    for key in ("psnr", "coarse_psnr", "fine_ssim"):  # the eval-mode render is deterministic: the set equals the per-frame calls
        assert out[key] == float(torch.mean(torch.tensor([m[key] for m, _ in per_frame]))), key
    for k, (_, images) in enumerate(per_frame):
        for key, image in images.items():
            assert np.array_equal(read_png(tmp_path / f"eval_{key}_{k:04d}.png"), E.image_u8(image).cpu().numpy()), (k, key)
