"""GPU tests of ray generation for distorted perspective, fisheye and equirectangular cameras (nsamd_raygen_lens,
nsamd_raygen_lens_grid; csrc/lens.h): against tests/golden/raygen_lenses.npz — the reference's own RayGenerator(Cameras(...))
and a float64 evaluation of the same formulas — and, bit for bit, between the routes that must agree (mixed against per-type
calls, lens against pinhole for undistorted perspective cameras, the in-loop grid form against the indexed form, the eval
render of a camera against the render of its bundle).

Bounds, from the fixture (tests/test_lens_cpu.py explains them): every ray within 2 x e_ref of float64 and 3 x e_ref of the
reference's fp32, where e_ref is the reference's own distance from float64 over the whole fixture — directions 2.717e-07
absolute, pixel_area 1.773e-05 relative, directions_norm 1.530e-07 relative; origins exact.
"""
import types

import numpy as np
import pytest
import torch

from lens_fixture import CASES, case_arrays, check_against_fixture
from oracle import nerfacto_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    info = _native.device_info()
    assert info["wavefront_size"] == 64 and info["arch"].startswith("gfx950"), info
    return functional


def dev(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.cuda()


KEYS = ("rgb", "accumulation", "depth", "expected_depth", "prop_depth_0", "prop_depth_1")
COLMAP = [-0.12, 0.03, 0.0, 0.0, 1e-3, -2e-3]
FISH_K = [0.04, -0.006, 0.002, -0.0004, 0.0, 0.0]


def lens_rays(F, c, idx=None, rows=None):
    """functional.raygen_lens on a fixture case (optionally other indices / a subset of its cameras)."""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    dist = c.get("distortion")
    return F.raygen_lens(dev(c["ray_indices"] if idx is None else idx), dev(pick(c["c2w"])), dev(pick(c["fx"])), dev(pick(c["fy"])),
                         dev(pick(c["cx"])), dev(pick(c["cy"])), dev(pick(c["camera_type"])),
                         None if dist is None else dev(pick(dist)))


@pytest.mark.parametrize("name", CASES)
def test_raygen_lens_golden(F, golden, name):
    g = golden("raygen_lenses")
    o, d, pa, dn = lens_rays(F, case_arrays(g, name))
    check_against_fixture(g, name, o.cpu().numpy(), d.cpu().numpy(), pa.cpu().numpy(), dn.cpu().numpy())


def test_ray_generator_of_mixed_cameras_equals_per_type_calls(F, golden):
    """One Cameras mixing types 1, 2, 3 through RayGenerator: the rays of each type equal, bit for bit, a call on a Cameras
    that holds the cameras of that type only (a wave that diverges by type computes what a uniform wave computes)."""
    from nerfstudio_amd.model_components.ray_generators import RayGenerator

    c = case_arrays(golden("raygen_lenses"), "mixed")
    T = torch.from_numpy
    cams = types.SimpleNamespace(camera_to_worlds=T(c["c2w"]), fx=T(c["fx"])[:, None], fy=T(c["fy"])[:, None], cx=T(c["cx"])[:, None],
                                 cy=T(c["cy"])[:, None], camera_type=T(c["camera_type"])[:, None], distortion_params=T(c["distortion"]))
    gen = RayGenerator(cams).cuda()
    assert not gen.pinhole
    idx = c["ray_indices"]
    rb = gen(dev(idx))
    assert rb.origins.shape == (idx.shape[0], 3) and torch.equal(rb.camera_indices[:, 0].cpu(), T(idx[:, 0]))
    seen = 0
    for t in (1, 2, 3):
        rows = np.flatnonzero(c["camera_type"] == t)
        keep = np.isin(idx[:, 0], rows)
        sub = idx[keep].copy()
        sub[:, 0] = np.searchsorted(rows, sub[:, 0])  # camera number within the per-type Cameras
        o, d, pa, dn = lens_rays(F, c, idx=sub, rows=rows)
        k = dev(np.flatnonzero(keep))
        assert torch.equal(rb.origins[k], o) and torch.equal(rb.directions[k], d), t
        assert torch.equal(rb.pixel_area[k], pa) and torch.equal(rb.metadata["directions_norm"][k], dn), t
        seen += int(keep.sum())
    assert seen == idx.shape[0]


def test_undistorted_perspective_cameras_give_the_bits_of_the_pinhole_kernel(F, golden):
    from nerfstudio_amd.model_components.ray_generators import RayGenerator

    g = golden("raygen")
    args = [dev(g[k]) for k in ("ray_indices", "c2w", "fx", "fy", "cx", "cy")]
    want = F.raygen_pinhole(*args)
    C_ = g["fx"].shape[0]
    ones = torch.ones(C_, dtype=torch.int32, device="cuda")
    for dist in (None, torch.zeros(C_, 6, device="cuda")):
        got = F.raygen_lens(*args, ones, dist)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    T = torch.from_numpy
    cams = types.SimpleNamespace(camera_to_worlds=T(g["c2w"]), fx=T(g["fx"]), fy=T(g["fy"]), cx=T(g["cx"]), cy=T(g["cy"]),
                                 camera_type=torch.ones(C_, 1, dtype=torch.int64), distortion_params=torch.zeros(C_, 6))
    gen = RayGenerator(cams).cuda()
    assert gen.pinhole
    rb = gen(args[0])
    assert torch.equal(rb.origins, want[0]) and torch.equal(rb.directions, want[1]) and torch.equal(rb.pixel_area, want[2])
    assert torch.equal(rb.metadata["directions_norm"], want[3])
    with pytest.raises(ValueError, match="camera type 9"):  # checked on the host: nothing is launched for it
        F.raygen_lens(*args, ones * 9, None)


def _frame_indices(H, W):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([torch.zeros_like(yy), yy, xx], dim=-1).reshape(-1, 3).cuda()


C2W = torch.tensor([[0.96, -0.10, 0.26, 0.3], [0.05, 0.98, 0.19, -0.2], [-0.27, -0.17, 0.95, 0.9]])


@pytest.mark.parametrize("camera_type,dist", [(1, COLMAP), (2, FISH_K), (2, None), (3, None), (1, None)])
def test_grid_form_equals_indexed_form(F, camera_type, dist):
    """nsamd_raygen_lens_grid chunk by chunk over a frame that is not a multiple of the chunk == nsamd_raygen_lens over the
    frame's index list, bit for bit; the padded tail of the last chunk repeats the frame's last pixel."""
    from nerfstudio_amd import _native as N

    H, W, n = 37, 41, 512  # 1517 rays: 2 full chunks + 493
    fx, fy, cx, cy = (H if camera_type == 3 else 0.9 * W), (H if camera_type == 3 else 0.8 * W), W / 2.0 + 0.25, H / 2.0 - 0.5
    one = lambda v: torch.tensor([v], device="cuda", dtype=torch.float32)  # noqa: E731
    c2w = C2W.cuda().contiguous()
    k = None if dist is None else torch.tensor(dist, device="cuda", dtype=torch.float32)
    o, d, pa, _ = F.raygen_lens(_frame_indices(H, W), c2w[None], one(fx), one(fy), one(cx), one(cy),
                                torch.tensor([camera_type], dtype=torch.int32, device="cuda"), None if k is None else k[None])
    bo, bd, bpa = (torch.empty((n, c), device="cuda") for c in (3, 3, 1))
    total = H * W
    for a in range(0, total, n):
        kk = min(a + n, total) - a
        for buf in (bo, bd, bpa):
            buf.fill_(float("nan"))
        N.check(N.load().nsamd_raygen_lens_grid(N.ptr(c2w), fx, fy, cx, cy, camera_type, N.ptr(k), W, a, kk, n, N.ptr(bo), N.ptr(bd),
                                                N.ptr(bpa), N.stream()), "raygen_lens_grid")
        assert torch.equal(bo[:kk], o[a:a + kk]) and torch.equal(bd[:kk], d[a:a + kk]) and torch.equal(bpa[:kk], pa[a:a + kk]), a
        if kk < n:
            assert torch.equal(bo[kk:], o[-1:].expand(n - kk, 3)) and torch.equal(bd[kk:], d[-1:].expand(n - kk, 3))
            assert torch.equal(bpa[kk:], pa[-1:].expand(n - kk, 1))
    assert kk == 493


class _Cam:
    """One camera as Model.get_outputs_for_camera sees it; generate_rays counts its calls and builds the bundle with
    RayGenerator (nsamd_raygen_lens, which the fixture pins to the reference's generate_rays)."""

    def __init__(self, H, W, camera_type, dist):
        self.H, self.W = H, W
        self.camera_to_worlds = C2W[None].cuda()
        self.fx, self.fy = torch.tensor([[0.9 * W]]).cuda(), torch.tensor([[0.8 * W]]).cuda()
        self.cx, self.cy = torch.tensor([[W / 2.0 + 0.25]]).cuda(), torch.tensor([[H / 2.0 - 0.5]]).cuda()
        self.height, self.width = torch.tensor([[H]]), torch.tensor([[W]])
        self.camera_type = torch.tensor([[camera_type]])
        self.distortion_params = None if dist is None else torch.tensor([dist]).cuda()
        self.calls = 0

    def generate_rays(self, camera_indices=0, keep_shape=True, obb_box=None):
        from nerfstudio_amd.model_components.ray_generators import RayGenerator

        self.calls += 1
        return RayGenerator(self).cuda()(_frame_indices(self.H, self.W)).reshape((self.H, self.W))


def _eval_model():
    from test_gpu_kernels import _hip_model, small_cfg

    cfg = small_cfg(12, 10, 5)
    model = _hip_model(cfg, orc.init_params(cfg, seed=3, table_std=0.4), training=False)
    model.config.eval_num_rays_per_chunk = 512
    return model


def test_eval_render_of_a_distorted_perspective_camera_generates_its_rays_inside_the_chunk_loop(F):
    """Model.get_outputs_for_camera for ONE perspective camera with OpenCV distortion: no generate_rays call, and the outputs
    of get_outputs_for_camera_ray_bundle on the RayGenerator bundle, bit for bit; the second frame replays the captured chunk.
    After a frame the runner's input buffers hold the last chunk: 493 rays of the bundle and 19 copies of its last ray."""
    from nerfstudio_amd import eval_render

    model = _eval_model()
    H, W = 37, 41  # 1517 rays: 2 full chunks + 493
    cam = _Cam(H, W, 1, COLMAP)
    bundle = cam.generate_rays()
    ref = model.get_outputs_for_camera_ray_bundle(bundle)
    pin = model.get_outputs_for_camera_ray_bundle(_Cam(H, W, 1, None).generate_rays())
    assert not torch.equal(pin["rgb"], ref["rgb"]), "the distortion must change the picture"
    cam.calls = 0
    for _ in range(2):
        out = model.get_outputs_for_camera(cam)
        assert cam.calls == 0, "the distorted perspective camera must not build a ray bundle"
        for k in KEYS:
            assert out[k].shape == ref[k].shape == (H, W, ref[k].shape[-1]), k
            assert torch.equal(out[k], ref[k]), f"{k}: max |d| = {float((out[k] - ref[k]).abs().max()):.3e}"
    s = eval_render.runner_for(model, torch.device("cuda")).step
    o, d = bundle.origins.reshape(-1, 3), bundle.directions.reshape(-1, 3)
    assert torch.equal(s.origins[:493], o[1024:]) and torch.equal(s.directions[:493], d[1024:])
    assert torch.equal(s.origins[493:], o[-1:].expand(19, 3)) and torch.equal(s.directions[493:], d[-1:].expand(19, 3))
    out = model.get_outputs_for_camera(cam, obb_box=object())  # a crop box: the bundle route
    assert cam.calls == 1 and torch.equal(out["rgb"], ref["rgb"])


@pytest.mark.parametrize("camera_type,dist", [(2, FISH_K), (3, None)])
def test_render_camera_with_a_lens_equals_the_bundle_route(F, camera_type, dist):
    """EvalRenderer.render_camera(lens=(type, distortion)) for a fisheye / an equirectangular camera == render of the
    RayGenerator bundle, bit for bit. (Model.get_outputs_for_camera still sends these two types through generate_rays.)"""
    from nerfstudio_amd import eval_render

    model = _eval_model()
    H, W = 37, 41
    cam = _Cam(H, W, camera_type, dist)
    ref = model.get_outputs_for_camera_ray_bundle(cam.generate_rays())
    args = eval_render.lens_camera_args(cam)
    assert args is not None and args[7] == camera_type
    runner = eval_render.runner_for(model, torch.device("cuda"))
    for _ in range(2):
        out = runner.render_camera(*args[:7], lens=args[7:])
        for k in KEYS:
            assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k
    cam.calls = 0
    out = model.get_outputs_for_camera(cam)
    assert cam.calls == 1 and torch.equal(out["rgb"], ref["rgb"])
    with pytest.raises(ValueError, match="camera type 9"):
        runner.render_camera(*args[:7], lens=(9, None))
