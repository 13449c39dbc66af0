"""Float64 restatements of the eval image metrics (include/nsamd_image.h: THE METRICS), the fp32 composition the library path
runs, the test images, and launches served by the host build of csrc/image_metrics.h (tests/hostcheck/image_helpers.cc).

Two independent statements of SSIM, both float64 and channel-last `[H, W, C]`:
  ssim_map_correlate  scipy.ndimage.correlate1d with the 11 weights along both axes, then the interior crop;
  ssim_map_conv       reflect F.pad by 5, F.conv2d with the 2-D window (the outer product) over the five stacked images and the
                      crop of 5 from every side, composed as the library composes them.
They agree to 1e-10 per window when given the same R (tests/test_image_metrics_cpu.py holds them to it). `ssim_map_conv` with
dtype=torch.float32 IS the fp32 composition: E[x^2] - E[x]^2 in fp32, which is what the kernel's pivot is measured against.

BOUNDS of the kernel against float64 (profiles/image_metrics.txt has the table they come from, scripts/bench_image_metrics.py
--cpu-table writes it): the host build's largest errors over the three kinds of image below, at the CPU and the GPU tests' sizes,
C = 3 and 1, R from the images and R = 1, were measured on the CPU, per window and on the mean, and the tests hold the host build
and the GPU build to 4 x those maxima per kind of image — the GPU build may order an 11-tap sum differently within what
-ffp-contract=off allows. (The half-flat pair's figures are those of a tile that straddles the flat half and the textured one:
its pivot can sit on one side only.) mse is a float64 sum rounded once to fp32 (2^-24 relative; the bound is 2^-23); psnr adds
the rounding of its own value: 10 / ln 10 x 2^-23 + one spacing of the fp32 result."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")
SIGMA, TAPS, K1, K2 = 1.5, 11, 0.01, 0.03
# kind of image -> (per window, mean): 4 x the host build's measured maxima (profiles/image_metrics.txt)
BOUNDS = {"sinusoid": (4 * 1.93e-05, 4 * 9.60e-08), "half_flat": (4 * 1.21e-04, 4 * 1.79e-05), "ramp": (4 * 3.17e-05, 4 * 5.90e-07)}
MSE_RELATIVE_BOUND = 2.0 ** -23
SIZES = ((41, 43), (64, 97), (11, 11))


def weights():
    d = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    g = np.exp(-(d / SIGMA) ** 2 / 2)
    return g / g.sum()


def data_range(pred, target):
    """R as the library forms it without a data_range: the larger max - min, in the images' own fp32"""
    pred, target = np.asarray(pred), np.asarray(target)
    return float(max(pred.max() - pred.min(), target.max() - target.min()))


def _compose(mu_x, mu_y, e_xx, e_yy, e_xy, R, clamp):
    c1, c2 = (K1 * R) ** 2, (K2 * R) ** 2
    s_xx, s_yy, s_xy = e_xx - mu_x * mu_x, e_yy - mu_y * mu_y, e_xy - mu_x * mu_y
    s_xx, s_yy = clamp(s_xx), clamp(s_yy)
    return ((2 * mu_x * mu_y + c1) * (2 * s_xy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_xx + s_yy + c2))


def ssim_map_correlate(pred, target, R):
    """[H-10, W-10, C] float64"""
    from scipy.ndimage import correlate1d

    x, y = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    g = weights()
    blur = lambda a: correlate1d(correlate1d(a, g, axis=0, mode="reflect"), g, axis=1, mode="reflect")[5:-5, 5:-5]  # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        return _compose(blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y), float(R), lambda s: np.maximum(s, 0.0))


def ssim_map_conv(pred, target, R, dtype=torch.float64):
    """[H-10, W-10, C] in `dtype` (arrays, or tensors on any device): reflect pad, one depth-wise conv2d with the 2-D window over
    the five stacked images, the crop"""
    as_tensor = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).to(dtype).permute(2, 0, 1)[None]  # noqa: E731
    x, y = as_tensor(pred), as_tensor(target)
    channels = x.shape[1]
    g = torch.from_numpy(weights()).to(device=x.device, dtype=dtype)
    kernel = (g[:, None] * g[None, :]).expand(channels, 1, TAPS, TAPS).contiguous()
    x, y = F.pad(x, (5, 5, 5, 5), mode="reflect"), F.pad(y, (5, 5, 5, 5), mode="reflect")
    out = F.conv2d(torch.cat((x, y, x * x, y * y, x * y)), kernel, groups=channels)
    mu_x, mu_y, e_xx, e_yy, e_xy = out.split(1)
    value = _compose(mu_x, mu_y, e_xx, e_yy, e_xy, torch.tensor(float(R), dtype=dtype, device=x.device), lambda s: torch.clamp(s, min=0.0))
    return value[0, :, 5:-5, 5:-5].permute(1, 2, 0)


def mse(pred, target):
    d = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    return float((d * d).mean())


def psnr(pred, target, psnr_range=1.0):
    with np.errstate(divide="ignore"):
        return float(10.0 * np.log10(psnr_range ** 2 / np.float64(mse(pred, target))))


def psnr_bound(value):
    return 10.0 / np.log(10.0) * MSE_RELATIVE_BOUND + float(np.spacing(np.float32(abs(value))))


def check_against_float64(out4, ssim_map, ref, kind, what):
    """a result {mse, psnr, ssim, R} (and its map, or None) against `metrics(...)` of the same pair under BOUNDS[kind]; prints the
    figures before it asserts"""
    window, mean = BOUNDS[kind]
    out4 = np.asarray(out4, np.float64)
    e_map = float(np.abs(np.asarray(ssim_map, np.float64) - ref["map"]).max()) if ssim_map is not None else 0.0
    e_mean, e_mse, e_psnr = abs(out4[2] - ref["ssim"]), abs(out4[0] - ref["mse"]) / ref["mse"], abs(out4[1] - ref["psnr"])
    print(f"{what}: per window {e_map:.2e} (bound {window:.2e}), mean {e_mean:.2e} ({mean:.2e}), mse relative {e_mse:.1e} "
          f"({MSE_RELATIVE_BOUND:.1e}), psnr {e_psnr:.1e} ({psnr_bound(ref['psnr']):.1e})")
    assert e_map <= window and e_mean <= mean and e_mse <= MSE_RELATIVE_BOUND and e_psnr <= psnr_bound(ref["psnr"]), what
    assert np.float32(out4[3]) == np.float32(ref["R"]), what
    return e_mean


def metrics(pred, target, R=None, psnr_range=1.0):
    """{mse, psnr, ssim, R} in float64 with the per-window map: the definition"""
    R = data_range(pred, target) if R is None else float(R)
    ssim = ssim_map_correlate(pred, target, R)
    return dict(mse=mse(pred, target), psnr=psnr(pred, target, psnr_range), ssim=float(ssim.mean()), R=R, map=ssim)


# ---------------------------------------------------------------- the images ------------------------------------------------------
def image_pair(kind, H, W, C=3, seed=0):
    """(pred, target) [H, W, C] fp32 in [0, 1]"""
    rs = np.random.RandomState(1000 * seed + 7 * H + W + C)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "sinusoid":
        target = np.stack([0.5 + 0.4 * np.sin(0.31 * xx + 0.7 * c) * np.cos(0.23 * yy - 0.4 * c) for c in range(C)], -1)
        pred = target + 0.05 * rs.standard_normal(target.shape)
    elif kind == "half_flat":  # top half constant 0.7, prediction = target + 0.002 noise
        target = np.stack([0.5 + 0.3 * np.sin(0.4 * xx + c) * np.sin(0.3 * yy) for c in range(C)], -1)
        target[: H // 2] = 0.7
        pred = target + 0.002 * rs.standard_normal(target.shape)
    elif kind == "ramp":  # a horizontal ramp with 0.003 noise
        target = np.repeat((xx / max(W - 1, 1))[..., None], C, -1).astype(np.float64)
        pred = target + 0.003 * rs.standard_normal(target.shape)
    else:
        raise ValueError(kind)
    return np.clip(pred, 0, 1).astype(np.float32), np.clip(target, 0, 1).astype(np.float32)


KINDS = ("sinusoid", "half_flat", "ramp")


# ---------------------------------------------------------------- the host build --------------------------------------------------
_HOST = {}


def host_library(directory):
    """the host build of csrc/image_metrics.h (built once per session into `directory`), with argtypes set"""
    if "lib" in _HOST:
        return _HOST["lib"]
    from nerfstudio_amd import _native as N

    out = os.path.join(str(directory), "libimagecheck.so")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(HOSTCHECK, "image_helpers.cc")], check=True)
    lib = C.CDLL(out)
    for name, argtypes in N._IMAGE_SIGNATURES.items():
        fn = getattr(lib, name.replace("nsamd_", "hc_"))
        fn.argtypes = argtypes if name.endswith("scratch_bytes") else argtypes[:-1]  # no stream
        fn.restype = C.c_int64 if name.endswith("scratch_bytes") else C.c_int
    _HOST["lib"] = lib
    return lib


def _ptr(t):
    if t is None:
        return None
    assert t.is_contiguous() and not t.is_cuda
    return t.data_ptr()


def host_launches(lib, log=None):
    """(image_range_launch, image_metrics_launch, colormap_launch) with the arguments of nerfstudio_amd.functional's, over host
    tensors, served by the host build; `log` collects (name, ...) per launch"""
    log = [] if log is None else log

    def image_range_launch(x, scratch, range2):
        assert x.dtype == range2.dtype == torch.float32 and scratch.numel() >= 8 * 1024 and scratch.data_ptr() % 8 == 0
        log.append(("range", x.numel()))
        assert lib.hc_image_range(_ptr(x), x.numel(), _ptr(scratch), _ptr(range2)) == 0

    def image_metrics_launch(pred, target, range_pred, range_target, data_range, psnr_range, scratch, out4, ssim_map):
        H, W, Ch = pred.shape
        assert tuple(target.shape) == (H, W, Ch) and scratch.numel() >= lib.hc_image_metrics_scratch_bytes(H, W, Ch) > 0
        assert ssim_map is None or tuple(ssim_map.shape) == (H - 10, W - 10, Ch)
        log.append(("metrics", H, W, Ch, range_pred is not None))
        assert lib.hc_image_metrics(_ptr(pred), _ptr(target), H, W, Ch, _ptr(range_pred), _ptr(range_target), data_range, psnr_range,
                                    _ptr(scratch), _ptr(out4), _ptr(ssim_map)) == 0

    def colormap_launch(values, lut, range2, accumulation, params, out_rgb, out_u8):
        n = values.numel()
        assert (out_rgb is None or out_rgb.numel() == 3 * n) and (out_u8 is None or out_u8.numel() == 3 * n)
        log.append(("colormap", n, params.mode, lut is not None, out_rgb is not None, out_u8 is not None))
        assert lib.hc_colormap(_ptr(values), n, _ptr(lut), _ptr(range2), _ptr(accumulation), params, _ptr(out_rgb), _ptr(out_u8)) == 0

    return image_range_launch, image_metrics_launch, colormap_launch


def inject(monkeypatch, lib, log=None):
    """nerfstudio_amd.functional's three image launches served by the host build"""
    from nerfstudio_amd import functional

    r, m, c = host_launches(lib, log)
    monkeypatch.setattr(functional, "image_range_launch", r)
    monkeypatch.setattr(functional, "image_metrics_launch", m)
    monkeypatch.setattr(functional, "colormap_launch", c)


def host_metrics(lib, pred, target, R=None, psnr_range=1.0, with_map=True):
    """({mse, psnr, ssim, R} as a float32 array, map or None) of the host build; R None: the ranges from hc_image_range"""
    r, m, _ = host_launches(lib)
    pred, target = torch.from_numpy(np.ascontiguousarray(pred)), torch.from_numpy(np.ascontiguousarray(target))
    H, W, Ch = pred.shape
    scratch = torch.zeros(max(8 * 1024, lib.hc_image_metrics_scratch_bytes(H, W, Ch)), dtype=torch.uint8)
    ranges = None
    if R is None:
        ranges = torch.zeros(2, 2)
        r(pred, scratch, ranges[0])
        r(target, scratch, ranges[1])
    out = torch.full((4,), -7.0)
    ssim_map = torch.full((H - 10, W - 10, Ch), -7.0) if with_map else None
    m(pred, target, None if ranges is None else ranges[0], None if ranges is None else ranges[1], 0.0 if R is None else R, psnr_range,
      scratch, out, ssim_map)
    return out.numpy(), None if ssim_map is None else ssim_map.numpy()


# ---------------------------------------------------------------- cameras ---------------------------------------------------------
class PinholeCamera:
    """what eval_frame.read_camera reads of a `Cameras` object, with the `generate_rays` the module path asks for (nsamd_raygen_pinhole,
    which tests/golden pins to the reference's own generate_rays)"""

    def __init__(self, c2w, focal, H, W, device):
        self.camera_to_worlds = c2w.to(device)
        self.fx, self.fy = torch.tensor([focal]), torch.tensor([focal])
        self.cx, self.cy = torch.tensor([W / 2.0 + 0.25]), torch.tensor([H / 2.0 - 0.5])
        self.height, self.width = torch.tensor([H]), torch.tensor([W])
        self.camera_type, self.distortion_params = torch.tensor([1]), None

    def generate_rays(self, camera_indices=0, keep_shape=True, obb_box=None):
        from nerfstudio_amd import functional as Fn
        from nerfstudio_amd.cameras.rays import RayBundle

        H, W, dev = int(self.height), int(self.width), self.camera_to_worlds.device
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        idx = torch.stack([torch.zeros_like(yy), yy, xx], dim=-1).reshape(-1, 3).to(dev)
        o, d, pa, _ = Fn.raygen_pinhole(idx, self.camera_to_worlds[None], *(v.to(dev) for v in (self.fx, self.fy, self.cx, self.cy)))
        return RayBundle(origins=o.view(H, W, 3), directions=d.view(H, W, 3), pixel_area=pa.view(H, W, 1),
                         camera_indices=torch.zeros(H, W, 1, dtype=torch.long, device=dev))


def orbit_cameras(n, H, W, device="cuda", focal=None):
    """n cameras on a circle of radius 1.7 around the z axis, looking at the origin"""
    out = []
    for k in range(n):
        a = 0.4 + 2.1 * k
        eye = np.array([1.7 * np.cos(a), 1.7 * np.sin(a), 0.35 * np.sin(1.3 * k)])
        back = eye / np.linalg.norm(eye)
        right = np.cross([0.0, 0.0, 1.0], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        c2w = torch.from_numpy(np.stack([right, up, back, eye], 1).astype(np.float32))
        out.append(PinholeCamera(c2w, 0.9 * W if focal is None else focal, H, W, device))
    return out
