"""CPU tests of the eval image metrics (include/nsamd_image.h, nerfstudio_amd/image_metrics.py, nerfstudio_amd/eval.py, the
models' get_image_metrics_and_images): the two float64 restatements of SSIM against each other, the arithmetic of
nerfstudio_amd/csrc/image_metrics.h compiled for the host (tests/hostcheck/image_helpers.cc) and looped as the kernels compose it
against them and against the fp32 conv2d composition, its edge cases, the same build under the address and undefined-behaviour
sanitizers as a stand-alone program, the Python layer over launches served by the host build, the files parsed back, and the ABI.

Bounds: image_metrics_reference's docstring (4 x the host build's measured errors, profiles/image_metrics.txt)."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
import image_metrics_reference as im
from test_texture_cpu import read_png

T = torch.from_numpy
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")
HEADER = os.path.join(ROOT, "include", "nsamd_image.h")
NAMES = ["nsamd_colormap", "nsamd_image_metrics", "nsamd_image_metrics_scratch_bytes", "nsamd_image_range"]
TILE = 32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return im.host_library(tmp_path_factory.mktemp("hostcheck"))


# ---------------------------------------------------------------- the definition --------------------------------------------------
@pytest.mark.parametrize("kind", im.KINDS)
def test_the_two_float64_restatements_agree(kind):
    for H, W in im.SIZES:
        for Ch in (3, 1):
            pred, target = im.image_pair(kind, H, W, Ch)
            R = im.data_range(pred, target)
            a, b = im.ssim_map_correlate(pred, target, R), im.ssim_map_conv(pred, target, R).numpy()
            assert a.shape == (H - 10, W - 10, Ch) == b.shape
            print(f"{kind} {H}x{W}x{Ch}: the two restatements differ by {np.abs(a - b).max():.1e} per window")
            assert np.abs(a - b).max() <= 1e-10
    assert abs(im.weights().sum() - 1) < 1e-15 and len(im.weights()) == 11
    assert im.psnr(np.full((11, 11, 1), 0.5, np.float32), np.full((11, 11, 1), 0.25, np.float32)) == pytest.approx(10 * np.log10(16.0), abs=1e-12)


# ---------------------------------------------------------------- image_metrics.h on the host -------------------------------------
@pytest.mark.parametrize("H,W", im.SIZES)
@pytest.mark.parametrize("kind", im.KINDS)
def test_host_build_matches_float64_per_window_and_on_the_mean(lib, kind, H, W):
    for Ch in (3, 1):
        pred, target = im.image_pair(kind, H, W, Ch)
        for R in (None, 1.0):
            ref = im.metrics(pred, target, R)
            out, ssim_map = im.host_metrics(lib, pred, target, R)
            e_mean = im.check_against_float64(out, ssim_map, ref, kind, f"host {kind} {H}x{W}x{Ch} R={R}")
            plain, _ = im.host_metrics(lib, pred, target, R, with_map=False)
            assert np.array_equal(plain.view(np.uint32), out.view(np.uint32))  # the map changes nothing
            f32 = im.ssim_map_conv(pred, target, ref["R"], torch.float32).numpy().astype(np.float64)
            e_f32 = abs(f32.mean() - ref["ssim"])
            print(f"    the fp32 conv2d composition: per window {np.abs(f32 - ref['map']).max():.2e}, mean {e_f32:.2e}")
            if kind == "half_flat":  # THE condition of the pivot: a tenth of the composition's error, at most
                assert e_mean <= 0.1 * e_f32, (e_mean, e_f32)


def test_edge_cases(lib):
    pred, target = im.image_pair("sinusoid", 41, 43, 3)
    window, mean = im.BOUNDS["sinusoid"]
    out, ssim_map = im.host_metrics(lib, pred, pred.copy())
    assert out[0] == 0 and np.isposinf(out[1]) and abs(out[2] - 1) <= mean and np.abs(ssim_map - 1).max() <= window  # identical images
    flat = np.full((20, 23, 3), 0.37, np.float32)
    out, ssim_map = im.host_metrics(lib, flat, flat.copy(), R=1.0)
    assert abs(out[2] - 1) <= mean and np.abs(ssim_map - 1).max() <= window and out[3] == 1.0  # constant images, explicit range
    other = np.full((20, 23, 3), 0.52, np.float32)
    out, ssim_map = im.host_metrics(lib, flat, other, R=1.0)
    ref = im.metrics(flat, other, 1.0)
    assert abs(out[2] - ref["ssim"]) <= mean and abs(out[0] - ref["mse"]) <= 2.0 ** -23 * ref["mse"]
    out, ssim_map = im.host_metrics(lib, flat, other)  # no range given: R = 0, the formula's 0 / 0
    assert out[3] == 0 and np.isnan(out[2]) and np.isnan(ssim_map).all() and np.isfinite(out[:2]).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(im.metrics(flat, other)["ssim"])  # as the float64 formula
    poisoned = pred.copy()
    poisoned[17, 29, 1] = np.nan
    for R in (None, 1.0):
        out, ssim_map = im.host_metrics(lib, poisoned, target, R)
        assert np.isnan(out[:3]).all()
        touched = np.zeros((31, 33), bool)
        touched[7:18, 19:30] = True  # the windows over pixel (17, 29)
        expect = np.zeros((31, 33, 3), bool)
        expect[..., 1] = touched
        if R is None:  # the image's range is NaN, so R is
            assert np.isnan(ssim_map).all() and np.isnan(out[3])
        else:  # exactly the windows over the pixel
            assert np.array_equal(np.isnan(ssim_map), expect)
    mono = im.image_pair("ramp", 30, 31, 1)
    out, ssim_map = im.host_metrics(lib, *mono)
    im.check_against_float64(out, ssim_map, im.metrics(*mono), "ramp", "C = 1")
    four = im.image_pair("sinusoid", 12, 45, 4)
    out, ssim_map = im.host_metrics(lib, *four)
    im.check_against_float64(out, ssim_map, im.metrics(*four), "sinusoid", "C = 4")


@pytest.mark.parametrize("H,W", ((11, 11), (TILE + 9, TILE + 10), (TILE + 11, 2 * TILE + 12)))
def test_host_build_is_clean_under_the_sanitizers(tmp_path, H, W):
    """a stand-alone program with the sanitizers' runtimes linked in statically: it runs in the environment it inherits, as it
    is, and nothing of it runs inside python. The sizes put one window, a full tile less one and a second tile of one window
    and of two rows on the halo indexing."""
    exe = str(tmp_path / "image_main")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(HOSTCHECK, "image_main.cc"), os.path.join(HOSTCHECK, "image_helpers.cc")], check=True)
    pred, target = im.image_pair("sinusoid", H, W, 3)
    path = tmp_path / "images.bin"
    with open(path, "wb") as f:
        f.write(pred.tobytes() + target.tobytes())
    run = subprocess.run([exe, str(path), str(H), str(W), "3"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    windows, mse, psnr, ssim, R = re.fullmatch(r"windows (\d+) mse (\S+) psnr (\S+) ssim (\S+) range (\S+)", run.stdout.strip()).groups()
    ref = im.metrics(pred, target)
    assert int(windows) == (H - 10) * (W - 10) * 3 and float(R) == np.float32(ref["R"])
    im.check_against_float64([float(mse), float(psnr), float(ssim), float(R)], None, ref, "sinusoid", f"sanitized {H}x{W}")


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 256 * 1024, 256 * 1024 + 1, 300001))
def test_range_is_min_and_max_and_a_nan_makes_both_nan(lib, n):
    rs = np.random.RandomState(n)
    x = rs.standard_normal(n).astype(np.float32)
    launch = im.host_launches(lib)[0]
    out = torch.full((2,), -7.0)
    launch(T(x), torch.zeros(8 * 1024, dtype=torch.uint8), out)
    assert out.tolist() == [float(x.min()), float(x.max())]
    for at in sorted({0, n // 2, n - 1}):
        y = x.copy()
        y[at] = np.nan
        launch(T(y), torch.zeros(8 * 1024, dtype=torch.uint8), out)
        assert bool(torch.isnan(out).all()), at
    y = np.full(n, np.inf, np.float32)
    launch(T(y), torch.zeros(8 * 1024, dtype=torch.uint8), out)
    assert out.tolist() == [np.inf, np.inf]


# ---------------------------------------------------------------- the Python layer ------------------------------------------------
def test_module_functions_over_the_host_build(lib, monkeypatch):
    from nerfstudio_amd import image_metrics as M

    log = []
    im.inject(monkeypatch, lib, log)
    pred, target = im.image_pair("sinusoid", 41, 43, 3)
    ref = im.metrics(pred, target)
    window, mean = im.BOUNDS["sinusoid"]
    value, ssim_map = M.ssim(T(pred), T(target), return_map=True)
    assert value.dim() == 0 and abs(float(value) - ref["ssim"]) <= mean and np.abs(ssim_map.numpy() - ref["map"]).max() <= window
    assert [e[0] for e in log] == ["range", "range", "metrics"]
    fixed = M.ssim(T(pred), T(target), data_range=1.0)
    assert abs(float(fixed) - im.metrics(pred, target, 1.0)["ssim"]) <= mean and len(log) == 4
    assert abs(float(M.psnr(T(pred), T(target))) - ref["psnr"]) <= im.psnr_bound(ref["psnr"])
    assert abs(float(M.psnr(T(pred), T(target), data_range=2.0)) - im.psnr(pred, target, 2.0)) <= im.psnr_bound(ref["psnr"] + 7)
    # the library's layout and its one range over a batch
    p2, t2 = im.image_pair("ramp", 41, 43, 3)
    batch_p, batch_t = torch.stack([T(pred), T(p2)]).permute(0, 3, 1, 2), torch.stack([T(target), T(t2)]).permute(0, 3, 1, 2)
    R = im.data_range(np.stack([pred, p2]), np.stack([target, t2]))
    expect = 0.5 * (im.metrics(pred, target, R)["ssim"] + im.metrics(p2, t2, R)["ssim"])
    got = M.structural_similarity_index_measure(batch_p, batch_t)
    assert got.dim() == 0 and abs(float(got) - expect) <= max(mean, im.BOUNDS["ramp"][1])
    assert abs(float(M.structural_similarity_index_measure(batch_p[:1], batch_t[:1], data_range=1.0)) - im.metrics(pred, target, 1.0)["ssim"]) <= mean
    # ImageMetrics: rows of one buffer, no read
    rows = torch.full((3, 4), -7.0)
    measure = M.ImageMetrics()
    measure.measure_into(T(pred), T(target), rows[1])
    assert (rows[0] == -7).all() and (rows[2] == -7).all() and abs(float(rows[1, M.SSIM]) - ref["ssim"]) <= mean
    assert torch.equal(measure.measure(T(pred), T(target)), rows[1]) and float(rows[1, M.RANGE]) == np.float32(ref["R"])
    for shape in ((10, 43, 3), (41, 10, 3)):
        with pytest.raises(ValueError, match="at least that size"):
            M.ssim(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError, match="1 to 4 channels"):
        M.ssim(torch.zeros(20, 20, 5), torch.zeros(20, 20, 5))
    with pytest.raises(ValueError, match="one shape"):
        M.ssim(torch.zeros(20, 20, 3), torch.zeros(20, 21, 3))


def fake_model(kind, background="white", lpips=None):
    """what the four models' get_image_metrics_and_images reads of `self`, with the real renderer"""
    from nerfstudio_amd.model_components.renderers import RGBRenderer

    m = types.SimpleNamespace(renderer_rgb=RGBRenderer(background_color=background), _image_metrics=None,
                              config=types.SimpleNamespace(near_plane=2.0, far_plane=6.0, num_proposal_iterations=2))
    if lpips is not None:
        m.lpips = lpips
    if kind == "mipnerf":
        m.clip_rgb_for_metrics = True
    return m


def model_class(kind):
    from nerfstudio_amd import instant_ngp, mipnerf, nerfacto, vanilla_nerf

    return {"nerfacto": nerfacto.NerfactoModel, "ngp": instant_ngp.NGPModel, "vanilla": vanilla_nerf.NeRFModel, "mipnerf": mipnerf.MipNerfModel}[kind]


def frame(kind, H=24, W=29, seed=0):
    """(outputs, batch) of a frame: an RGBA ground truth, predictions that leave [0, 1] a little (mip-NeRF clips them)"""
    rs = np.random.RandomState(seed)
    pred, target = im.image_pair("sinusoid", H, W, 3, seed)
    alpha = np.clip(rs.uniform(0.3, 1.2, (H, W, 1)), 0, 1).astype(np.float32)
    batch = {"image": T(np.concatenate([target, alpha], -1))}
    f = lambda lo, hi: T(rs.uniform(lo, hi, (H, W, 1)).astype(np.float32))  # noqa: E731
    if kind in ("nerfacto", "ngp"):
        out = {"rgb": T(pred), "accumulation": f(0, 1), "depth": f(0.5, 7)}
        if kind == "nerfacto":
            out.update(prop_depth_0=f(0.5, 7), prop_depth_1=f(0.5, 7))
        return out, batch
    wide = T(pred) * 1.2 - 0.1
    return {"rgb_coarse": T(target * 0.9 + 0.03), "rgb_fine": wide, "accumulation_coarse": f(0, 1), "accumulation_fine": f(0, 1),
            "depth_coarse": f(1, 7), "depth_fine": f(1, 7)}, batch


@pytest.mark.parametrize("kind", ("nerfacto", "ngp", "vanilla", "mipnerf"))
def test_get_image_metrics_and_images_against_float64(lib, monkeypatch, kind):
    from conftest import load_golden
    from nerfstudio_amd import eval as E
    from nerfstudio_amd.utils import colormaps as cm

    im.inject(monkeypatch, lib)
    cm.set_colormap_lut("turbo", T(load_golden("colormaps")["lut_turbo"]), "cpu")  # the table comes from the fixture
    reads = []
    monkeypatch.setattr(E, "read_rows", lambda rows, read=E.read_rows: (reads.append(tuple(rows.shape)), read(rows))[1])
    cls, model = model_class(kind), fake_model(kind)
    assert cls.lpips is None
    outputs, batch = frame(kind)
    metrics, images = cls.get_image_metrics_and_images(model, outputs, batch)
    rgba = batch["image"]
    gt = (rgba[..., :3] * rgba[..., 3:] + (1 - rgba[..., 3:])).numpy()  # over white
    mean = im.BOUNDS["sinusoid"][1]
    H, W = gt.shape[:2]
    if kind in ("nerfacto", "ngp"):
        ref = im.metrics(gt, outputs["rgb"].numpy())
        assert list(metrics) == ["psnr", "ssim"] and reads == [(1, 4)]
        assert abs(metrics["psnr"] - ref["psnr"]) <= im.psnr_bound(ref["psnr"]) and abs(metrics["ssim"] - ref["ssim"]) <= mean
        assert list(images) == ["img", "accumulation", "depth"] + (["prop_depth_0", "prop_depth_1"] if kind == "nerfacto" else [])
        assert tuple(images["img"].shape) == (H, 2 * W, 3) and np.array_equal(images["img"][:, :W].numpy(), gt.astype(np.float32))
        assert torch.equal(images["img"][:, W:], outputs["rgb"])
        assert torch.equal(images["accumulation"], cm.apply_colormap(outputs["accumulation"]))
        for key, name in [("depth", "depth")] + ([("prop_depth_0",) * 2, ("prop_depth_1",) * 2] if kind == "nerfacto" else []):
            assert tuple(images[key].shape) == (H, W, 3)
            assert torch.equal(images[key], cm.apply_depth_colormap(outputs[name], accumulation=outputs["accumulation"]))
        if kind == "nerfacto":  # maps only for the keys the outputs hold
            del outputs["prop_depth_1"]
            assert list(cls.get_image_metrics_and_images(model, outputs, batch)[1]) == ["img", "accumulation", "depth", "prop_depth_0"]
    else:
        fine, coarse = outputs["rgb_fine"].numpy(), outputs["rgb_coarse"].numpy()
        if kind == "mipnerf":
            fine, coarse = np.clip(fine, 0, 1), np.clip(coarse, 0, 1)
            assert (outputs["rgb_fine"] < 0).any() and (outputs["rgb_fine"] > 1).any()
        rf, rc = im.metrics(gt, fine), im.metrics(gt, coarse)
        assert list(metrics) == ["psnr", "coarse_psnr", "fine_psnr", "fine_ssim"] and reads == [(2, 4)]
        assert metrics["psnr"] == metrics["fine_psnr"] and abs(metrics["fine_psnr"] - rf["psnr"]) <= im.psnr_bound(rf["psnr"])
        assert abs(metrics["coarse_psnr"] - rc["psnr"]) <= im.psnr_bound(rc["psnr"]) and abs(metrics["fine_ssim"] - rf["ssim"]) <= mean
        assert list(images) == ["img", "accumulation", "depth"]
        assert tuple(images["img"].shape) == (H, 3 * W, 3) and tuple(images["depth"].shape) == (H, 2 * W, 3) == tuple(images["accumulation"].shape)
        assert torch.equal(images["img"][:, W:2 * W], outputs["rgb_coarse"]) and torch.equal(images["img"][:, 2 * W:], outputs["rgb_fine"])  # unclipped
        for i, p in enumerate(("coarse", "fine")):
            assert torch.equal(images["depth"][:, i * W:(i + 1) * W], cm.apply_depth_colormap(
                outputs[f"depth_{p}"], accumulation=outputs[f"accumulation_{p}"], near_plane=2.0, far_plane=6.0))
            assert torch.equal(images["accumulation"][:, i * W:(i + 1) * W], cm.apply_colormap(outputs[f"accumulation_{p}"]))
    # a callable lpips adds its key, called as the reference calls it
    outputs, batch = frame(kind)
    calls = []
    stub = lambda a, b: (calls.append((tuple(a.shape), tuple(b.shape))), torch.tensor(0.125))[1]  # noqa: E731
    metrics, _ = cls.get_image_metrics_and_images(fake_model(kind, lpips=stub), outputs, batch)
    key = "lpips" if kind in ("nerfacto", "ngp") else "fine_lpips"
    assert metrics[key] == 0.125 and list(metrics)[-1] == key and calls == [((1, 3, H, W),) * 2]


def test_depth_nerfacto_keeps_its_own_method():
    from nerfstudio_amd.depth_nerfacto import DepthNerfactoModel
    from nerfstudio_amd.nerfacto import NerfactoModel

    assert DepthNerfactoModel.get_image_metrics_and_images is not NerfactoModel.get_image_metrics_and_images
    assert "depth_mse" in DepthNerfactoModel.get_image_metrics_and_images.__doc__


import refdrive  # noqa: E402

needs_reference = pytest.mark.skipif(not refdrive.available(), reason="the reference checkout is not on this machine")


@needs_reference
@pytest.mark.parametrize("kind", ("nerfacto", "ngp", "vanilla", "mipnerf"))
def test_images_and_keys_equal_the_reference_methods(lib, monkeypatch, kind):
    """the reference's own get_image_metrics_and_images bodies with psnr / ssim / lpips stubbed, on the CPU: the same keys in the
    same order, the same images bit for bit"""
    pytest.importorskip("matplotlib")  # the reference's own functions read matplotlib's tables
    refdrive.install()
    import importlib

    from nerfstudio.model_components.renderers import RGBRenderer as RefRenderer

    module, name = {"nerfacto": ("nerfacto", "NerfactoModel"), "ngp": ("instant_ngp", "NGPModel"), "vanilla": ("vanilla_nerf", "NeRFModel"),
                    "mipnerf": ("mipnerf", "MipNerfModel")}[kind]
    ref_class = getattr(importlib.import_module(f"nerfstudio.models.{module}"), name)
    im.inject(monkeypatch, lib)
    outputs, batch = frame(kind)
    stub = lambda a, b: torch.tensor(0.5)  # noqa: E731
    config = types.SimpleNamespace(num_proposal_iterations=2, collider_params={"near_plane": 2.0, "far_plane": 6.0})
    ref_self = types.SimpleNamespace(device=torch.device("cpu"), renderer_rgb=RefRenderer(background_color="white"), psnr=stub, ssim=stub,
                                     lpips=stub, config=config)
    ref_metrics, ref_images = ref_class.get_image_metrics_and_images(ref_self, outputs, batch)
    metrics, images = model_class(kind).get_image_metrics_and_images(fake_model(kind, lpips=stub), outputs, batch)
    assert list(metrics) == list(ref_metrics) and list(images) == list(ref_images)
    for key in images:
        assert images[key].shape == ref_images[key].shape and torch.equal(images[key], ref_images[key]), key


# ---------------------------------------------------------------- a set of frames -------------------------------------------------
H_, W_ = 24, 29


class SetCamera(im.PinholeCamera):
    """camera k (its pose's x translation) of a set; its bundle carries k and every pixel's index"""

    def __init__(self, k):
        c2w = torch.eye(4)[:3].clone()
        c2w[0, 3] = float(k)
        super().__init__(c2w, 30.0, H_, W_, "cpu")
        self.k = k

    def generate_rays(self, camera_indices=0, keep_shape=True, obb_box=None):
        from nerfstudio_amd.cameras.rays import RayBundle

        assert camera_indices == 0 and keep_shape and obb_box is None
        pixel = torch.arange(H_ * W_, dtype=torch.float32).view(H_, W_, 1)
        return RayBundle(origins=pixel.expand(H_, W_, 3).contiguous(), directions=torch.ones(H_, W_, 3), pixel_area=torch.ones(H_, W_, 1),
                         camera_indices=torch.full((H_, W_, 1), self.k, dtype=torch.long))


class SetModel(torch.nn.Module):
    """A model whose camera k renders frame k, through the REAL entry points of the class it stands in for
    (eval_frame.outputs_for_camera / outputs_for_bundle / module_chunk_loop): `forward` serves a chunk's rows of the frame (the
    module path), the stand-in runner the whole frame. Chunks of 100 rays do not divide the 696 of a frame."""

    lpips = None

    def __init__(self, frames, kind):
        from nerfstudio_amd.model_components.renderers import RGBRenderer

        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(1))
        self.renderer_rgb, self.frames, self.paths, self._image_metrics = RGBRenderer(background_color="white"), frames, [], None
        self.config = types.SimpleNamespace(num_proposal_iterations=2, eval_num_rays_per_chunk=100, near_plane=2.0, far_plane=6.0)
        self.real = model_class(kind)

    def forward(self, bundle):
        assert not self.training and len(bundle) <= 100
        k, rows = int(bundle.camera_indices[0, 0]), bundle.origins[:, 0].long()
        return {key: v.reshape(H_ * W_, -1)[rows] for key, v in self.frames[k][0].items()}

    def render_camera(self, c2w, fx, fy, cx, cy, height, width, lens=None):  # the stand-in runner is the model itself
        assert (fx, height, width, lens) == (30.0, H_, W_, None) and not self.training
        self.paths.append("runner")
        return self.frames[int(c2w[0, 3])][0]

    def get_outputs_for_camera(self, camera, obb_box=None):
        return self.real.get_outputs_for_camera(self, camera, obb_box)

    def get_outputs_for_camera_ray_bundle(self, bundle):
        out = self.real.get_outputs_for_camera_ray_bundle(self, bundle)
        self.paths.append("module")
        return out


def set_harness(lib, monkeypatch, kind, count=3):
    """(eval module, model, [(camera, batch)], the log of metric-buffer reads) with the launches served by the host build, the
    turbo table from the fixture and nerfacto's runner_for handing out the stand-in runner EXCEPT for the second frame"""
    from conftest import load_golden
    from nerfstudio_amd import eval as E
    from nerfstudio_amd import eval_render
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.utils import colormaps

    im.inject(monkeypatch, lib)
    colormaps.set_colormap_lut("turbo", T(load_golden("colormaps")["lut_turbo"]), "cpu")
    monkeypatch.setattr(F, "texture_store_launch", lambda rgb, count, first, out: out.view(-1, 3)[first:first + count].copy_(
        torch.floor(torch.nan_to_num(rgb[:count], nan=0.0).clamp(0, 1) * 255 + 0.5).to(torch.uint8)))
    frames = [frame(kind, seed=s) for s in range(count)]
    model = SetModel(frames, kind).train()
    monkeypatch.setattr(eval_render, "runner_for", lambda m, dev: None if len(m.paths) == 1 else m)  # the runner declines frame 1
    reads = []
    monkeypatch.setattr(E, "read_rows", lambda rows, read=E.read_rows: (reads.append(tuple(rows.shape)), read(rows))[1])
    return E, model, [(SetCamera(k), frames[k][1]) for k in range(count)], reads


def check_pngs(folder, prefix, per_frame):
    names = sorted(p.name for p in folder.iterdir())
    assert names == sorted(f"{prefix}_{key}_{k:04d}.png" for k, (_, images) in enumerate(per_frame) for key in images)
    for k, (_, images) in enumerate(per_frame):
        for key, image in images.items():
            png = read_png(folder / f"{prefix}_{key}_{k:04d}.png")
            assert np.array_equal(png, np.floor(np.clip(image.numpy(), 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)), (k, key)


def test_average_image_metrics_reads_once_and_writes_the_reference_file_names(lib, monkeypatch, tmp_path):
    E, model, frames, reads = set_harness(lib, monkeypatch, "nerfacto")
    out = E.average_image_metrics(model, frames, image_prefix="val", output_path=tmp_path / "renders", get_std=True)
    # frame 1, which the runner declined, came chunk by chunk through eval_frame.module_chunk_loop; its metrics joined the others'
    assert reads == [(3, 4)] and model.paths == ["runner", "module", "runner"] and model.training
    per_frame = [model.real.get_image_metrics_and_images(model, *model.frames[k]) for k in range(3)]
    assert reads == [(3, 4)] + [(1, 4)] * 3
    assert sorted(out) == sorted(["psnr", "psnr_std", "ssim", "ssim_std", "num_rays_per_sec", "num_rays_per_sec_std", "fps", "fps_std"])
    for key in ("psnr", "ssim"):
        std, mean = torch.std_mean(torch.tensor([m[key] for m, _ in per_frame]))
        assert out[key] == float(mean) and out[f"{key}_std"] == float(std)
    assert out["num_rays_per_sec"] > 0 and out["fps"] == pytest.approx(out["num_rays_per_sec"] / (H_ * W_), rel=1e-5)
    assert list(per_frame[0][1]) == ["img", "accumulation", "depth", "prop_depth_0", "prop_depth_1"]
    check_pngs(tmp_path / "renders", "val", per_frame)
    model.paths.clear()
    plain = E.average_image_metrics(model.eval(), frames)
    assert sorted(plain) == ["fps", "num_rays_per_sec", "psnr", "ssim"] and plain["psnr"] == out["psnr"] and not model.training
    assert not os.path.exists(tmp_path / "eval_img_0000.png")
    with pytest.raises(ValueError, match="at least one"):
        E.average_image_metrics(model, [])
    model.lpips = lambda a, b: torch.tensor(0.25)
    assert E.average_image_metrics(model, frames[:1])["lpips"] == 0.25


@pytest.mark.parametrize("kind", ("vanilla", "mipnerf"))
def test_average_image_metrics_of_a_two_pass_model(lib, monkeypatch, tmp_path, kind):
    """NeRFModel / MipNerfModel have no runner: every frame is their get_outputs_for_camera -> the camera's bundle -> the module
    chunk loop; two rows of metrics per frame in one [N, 2, 4] buffer, read once"""
    E, model, frames, reads = set_harness(lib, monkeypatch, kind, count=2)
    if kind == "mipnerf":
        model.clip_rgb_for_metrics = True
    out = E.average_image_metrics(model, frames, output_path=tmp_path, get_std=True)
    assert reads == [(4, 4)] and model.paths == ["module", "module"] and model.training
    per_frame = [model.real.get_image_metrics_and_images(model, *model.frames[k]) for k in range(2)]
    keys = ["psnr", "coarse_psnr", "fine_psnr", "fine_ssim", "num_rays_per_sec", "fps"]
    assert list(out) == [k for key in keys for k in (key, f"{key}_std")]
    for key in keys[:4]:
        std, mean = torch.std_mean(torch.tensor([m[key] for m, _ in per_frame]))
        assert out[key] == float(mean) and out[f"{key}_std"] == float(std), key
    assert out["psnr"] == out["fine_psnr"] != out["coarse_psnr"]
    assert list(per_frame[0][1]) == ["img", "accumulation", "depth"] and tuple(per_frame[0][1]["img"].shape) == (H_, 3 * W_, 3)
    check_pngs(tmp_path, "eval", per_frame)
    model.lpips = lambda a, b: torch.tensor(0.25)
    assert E.average_image_metrics(model, frames)["fine_lpips"] == 0.25


def test_modules_import_nothing_of_the_libraries():
    for name in ("image_metrics.py", "eval.py", os.path.join("utils", "colormaps.py")):
        src = open(os.path.join(ROOT, "nerfstudio_amd", name)).read()
        assert not re.findall(r"^\s*(?:import|from)\s+(?:nerfstudio|torchmetrics|torchvision|mediapy|PIL)\b", src, re.M), name


# ---------------------------------------------------------------- the entry points ------------------------------------------------
def test_entry_points_are_declared_bound_and_launched_from_one_place(tmp_path):
    from nerfstudio_amd import _native as N

    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(nsamd_[a-z0-9_]+)\s*\(", header))) == sorted(N._IMAGE_SIGNATURES) == NAMES
    others = (set(N._SIGNATURES) | set(N._EXPORT_SIGNATURES) | set(N._RENDER_SIGNATURES) | set(N._POINTCLOUD_SIGNATURES)
              | set(N._MESH_SIGNATURES) | set(N._TEXTURE_SIGNATURES))
    assert not set(N._IMAGE_SIGNATURES) & others
    cdll = C.CDLL(N.LIB_PATH)
    lib = N.load()
    for name in NAMES:
        assert hasattr(cdll, name) and callable(getattr(lib, name))
    vp, i64, i32, f32 = N.vp, N.i64, N.i32, N.f32
    assert N._IMAGE_SIGNATURES == {"nsamd_image_range": [vp, i64, vp, vp, vp],
                                   "nsamd_image_metrics_scratch_bytes": [i64, i64, i32],
                                   "nsamd_image_metrics": [vp, vp, i64, i64, i32, vp, vp, f32, f32, vp, vp, vp, vp],
                                   "nsamd_colormap": [vp, i64, vp, vp, vp, N.ColormapParams, vp, vp, vp]}
    assert C.sizeof(N.ColormapParams) == 48 and N._RESTYPES["nsamd_image_metrics_scratch_bytes"] is C.c_int64
    define = lambda name: int(re.search(rf"#define {name}\s+(\d+)", text).group(1))  # noqa: E731
    assert define("NSAMD_SSIM_TILE") == N.SSIM_TILE == TILE and define("NSAMD_SSIM_WINDOW") == N.SSIM_WINDOW == 11
    assert define("NSAMD_RANGE_MAX_BLOCKS") * 8 == N.RANGE_SCRATCH_BYTES and define("NSAMD_IMAGE_BLOCK") == 256
    assert (define("NSAMD_COLORMAP_PLAIN"), define("NSAMD_COLORMAP_DEPTH")) == (N.COLORMAP_PLAIN, N.COLORMAP_DEPTH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "nsamd_image.h"\n'
                   "int main(void) {\n"
                   "  nsamd_colormap_params plain = {NSAMD_COLORMAP_PLAIN, 0, 0, 0, 0.0, 1.0, 0.0, 0.0};\n"
                   "  nsamd_colormap_params odd = {7, 0, 0, 0, 0.0, 1.0, 0.0, 0.0};\n"
                   "  nsamd_colormap_params depth = {NSAMD_COLORMAP_DEPTH, 0, 0, NSAMD_COLORMAP_FIXED_NEAR, 0.0, 1.0, 0.5, 0.0};\n"
                   "  static double scratch[NSAMD_RANGE_SCRATCH_BYTES / 8];\n"
                   "  float x[8];\n"
                   "  if (sizeof(plain) != 48 || sizeof(scratch) != 8192) return 20;\n"
                   "  if (nsamd_image_metrics_scratch_bytes(800, 800, 3) != 16 * 25 * 25) return 1;\n"
                   "  if (nsamd_image_metrics_scratch_bytes(11, 42, 1) != 16 || nsamd_image_metrics_scratch_bytes(11, 43, 1) != 32) return 2;\n"
                   "  if (nsamd_image_metrics_scratch_bytes(10, 800, 3) != 0 || nsamd_image_metrics_scratch_bytes(800, 800, 5) != 0) return 3;\n"
                   "  if (nsamd_image_range(x, 0, scratch, x, NULL) != NSAMD_ERR_INVALID_ARG) return 4;\n"
                   "  if (nsamd_image_range(NULL, 8, scratch, x, NULL) != NSAMD_ERR_INVALID_ARG) return 5;\n"
                   "  if (nsamd_image_metrics(x, x, 10, 64, 3, NULL, NULL, 1.0f, 1.0f, scratch, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 6;\n"
                   "  if (nsamd_image_metrics(x, x, 64, 10, 3, NULL, NULL, 1.0f, 1.0f, scratch, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 7;\n"
                   "  if (nsamd_image_metrics(x, x, 64, 64, 5, NULL, NULL, 1.0f, 1.0f, scratch, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 8;\n"
                   "  if (nsamd_image_metrics(x, x, 64, 64, 0, NULL, NULL, 1.0f, 1.0f, scratch, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 9;\n"
                   "  if (nsamd_image_metrics(x, x, 64, 64, 3, NULL, NULL, 0.0f, 1.0f, scratch, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 10;\n"
                   "  if (nsamd_image_metrics(x, x, 64, 64, 3, NULL, NULL, -1.0f, 1.0f, scratch, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 11;\n"
                   "  if (nsamd_image_metrics(x, x, 64, 64, 3, x, NULL, 1.0f, 1.0f, scratch, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 12;\n"
                   "  if (nsamd_image_metrics(x, x, 64, 64, 3, NULL, NULL, 1.0f, 0.0f, scratch, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 13;\n"
                   "  if (nsamd_image_metrics(x, x, 64, 64, 3, NULL, NULL, 1.0f, 1.0f, scratch, NULL, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 14;\n"
                   "  if (nsamd_colormap(x, 8, x, NULL, NULL, plain, NULL, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 15;\n"
                   "  if (nsamd_colormap(x, 0, x, NULL, NULL, plain, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 16;\n"
                   "  if (nsamd_colormap(x, 8, x, NULL, NULL, odd, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 17;\n"
                   "  if (nsamd_colormap(x, 8, x, NULL, x, plain, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 18;\n"
                   "  if (nsamd_colormap(x, 8, x, NULL, NULL, depth, x, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 19;\n"
                   "  return 0;\n}\n")
    libdir = os.path.dirname(N.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(tmp_path / "use"), "-L", libdir,
                    "-lnsamd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([str(tmp_path / "use")], check=True)
    pkg = os.path.join(ROOT, "nerfstudio_amd")
    for name in NAMES:
        sites = [f for f in os.listdir(pkg) if f.endswith(".py") and f != "_native.py" and f".{name}(" in open(os.path.join(pkg, f)).read()]
        assert sites == ["functional.py"], name
    makefile = open(os.path.join(pkg, "csrc", "Makefile")).read()
    assert " image_metrics.hip" in makefile and " image_metrics.h " in makefile and "nsamd_image.h" in makefile
    assert "nsamd_image" not in open(os.path.join(ROOT, "include", "nsamd.h")).read()  # that header stays as it is


def test_host_build_answers_the_argument_table_as_the_library(lib):
    """No call here reaches a launch: every one fails a check (the pointers are host memory)."""
    from nerfstudio_amd import _native as N

    native = N.load()
    p = torch.zeros(4096, dtype=torch.int64).data_ptr()
    plain, depth = N.make_colormap_params(), N.make_colormap_params(depth=True)

    def variants(rng, bytes_, metrics, colormap, stream):
        assert rng(p, 0, p, p, *stream) == -1 and rng(p, -3, p, p, *stream) == -1 and rng(None, 4, p, p, *stream) == -1
        assert bytes_(800, 800, 3) == 10000 and bytes_(10, 11, 1) == 0 and bytes_(11, 11, 5) == 0 and bytes_(11, 11, 4) == 16
        base = dict(pred=p, target=p, H=64, W=64, C=3, rp=None, rt=None, R=1.0, Rp=1.0, scratch=p, out=p, m=None)
        for bad in (dict(H=10), dict(W=10), dict(C=5), dict(C=0), dict(R=0.0), dict(R=float("nan")), dict(rp=p), dict(rt=p), dict(Rp=0.0),
                    dict(pred=None), dict(target=None), dict(scratch=None), dict(out=None), dict(H=2 ** 20, W=2 ** 20)):
            a = dict(base, **bad)
            assert metrics(a["pred"], a["target"], a["H"], a["W"], a["C"], a["rp"], a["rt"], a["R"], a["Rp"], a["scratch"], a["out"], a["m"], *stream) == -1, bad
        for bad in (dict(n=0), dict(n=2 ** 31), dict(values=None), dict(rgb=None, u8=None), dict(params=N.make_colormap_params(normalize=True)),
                    dict(params=depth), dict(params=N.make_colormap_params(depth=True, near_plane=1.0)), dict(acc=p)):
            a = dict(dict(values=p, n=8, lut=p, r=None, acc=None, params=plain, rgb=p, u8=p), **bad)
            assert colormap(a["values"], a["n"], a["lut"], a["r"], a["acc"], a["params"], a["rgb"], a["u8"], *stream) == -1, bad

    variants(native.nsamd_image_range, native.nsamd_image_metrics_scratch_bytes, native.nsamd_image_metrics, native.nsamd_colormap, (None,))
    variants(lib.hc_image_range, lib.hc_image_metrics_scratch_bytes, lib.hc_image_metrics, lib.hc_colormap, ())
