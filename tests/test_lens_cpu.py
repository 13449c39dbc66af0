"""CPU tests of ray generation for distorted perspective, fisheye and equirectangular cameras: the per-ray arithmetic of
nerfstudio_amd/csrc/lens.h (what nsamd_raygen_lens / nsamd_raygen_lens_grid run per lane), compiled for the host by
tests/hostcheck/lens_helpers.cc, against tests/golden/raygen_lenses.npz — the reference's own RayGenerator(Cameras(...)) and a
float64 evaluation of the same formulas (tests/golden/make_golden_lenses.py) — and the host logic around the kernels. The
library built here is test infrastructure: the product never loads it.

Bounds. They come from the fixture, not from the code under test: `e_ref_*` is the REFERENCE's fp32 distance from float64, the
maximum over the whole fixture, floored at one fp32 ulp of 1.0. Measured when the fixture was written:

    directions       2.717e-07 absolute   (perspective / fisheye cases 0.9 - 1.4e-07, equirectangular and mixed 2.1 - 2.7e-07)
    pixel_area       1.773e-05 relative
    directions_norm  1.530e-07 relative

An independent fp32 implementation gets the same rounding budget with a factor 2 for the device's sinf / cosf and division:
every ray must lie within 2 x e_ref of float64 and (triangle inequality) within 3 x e_ref of the reference's fp32 arrays;
origins are exact.
"""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from lens_fixture import case_arrays, check_against_fixture

F32P = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
I64P = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "liblenscheck.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "lens_helpers.cc")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.hc_raygen_lens.argtypes = [I64P, F32P, F32P, F32P, F32P, F32P, I32P, C.c_void_p, C.c_int64, F32P, F32P, F32P, F32P]
    lib.hc_raygen_lens.restype = None
    lib.hc_lens_undistort.argtypes = [F32P, C.c_int64, F32P, F32P]
    lib.hc_lens_undistort.restype = None
    lib.hc_lens_local_direction.argtypes = [C.c_int, F32P, C.c_int64, F32P]
    lib.hc_lens_local_direction.restype = None
    lib.hc_lens_has_distortion.argtypes = [F32P]
    return lib


def host_rays(hc, idx, c2w, fx, fy, cx, cy, ctype, dist):
    n = idx.shape[0]
    o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    pa, dn = np.empty((n, 1), np.float32), np.empty((n, 1), np.float32)
    dist = None if dist is None else np.ascontiguousarray(dist, np.float32)
    hc.hc_raygen_lens(np.ascontiguousarray(idx), np.ascontiguousarray(c2w), fx, fy, cx, cy, np.ascontiguousarray(ctype, np.int32),
                      None if dist is None else dist.ctypes.data, n, o, d, pa, dn)
    return o, d, pa, dn


def test_fixture_holds_the_families_and_its_bounds():
    g = load_golden("raygen_lenses")
    assert list(g["cases"]) == ["opencv", "fisheye", "equirect", "mixed", "grid_opencv", "grid_fisheye"]
    ulp = 2.0 ** -23
    for q in ("directions", "pixel_area", "directions_norm"):
        assert float(g[f"e_ref_{q}"]) == max(float(g[f"e_ref_{q}_measured"]), ulp)
    assert np.allclose(g["e_ref_by_case"].max(axis=0),
                       [float(g[f"e_ref_{q}_measured"]) for q in ("directions", "pixel_area", "directions_norm")], rtol=0, atol=0)
    assert 1e-7 <= float(g["e_ref_directions"]) <= 4e-7 and 1e-6 <= float(g["e_ref_pixel_area"]) <= 4e-5
    assert sorted(set(g["mixed_camera_type"].tolist())) == [1, 2, 3]
    assert (g["opencv_distortion"][:3] != 0).any(axis=1).all() and not g["opencv_distortion"][3].any()
    for name in g["cases"]:
        c = case_arrays(g, name)
        h, w = c["hw"]
        for cam in range(len(c["fx"])):  # both corner pixels of every camera
            rows = c["ray_indices"][c["ray_indices"][:, 0] == cam]
            assert (rows[:, 1:] == [0, 0]).all(axis=1).any() and (rows[:, 1:] == [h - 1, w - 1]).all(axis=1).any(), (name, cam)
    assert g["grid_opencv_ray_indices"].shape[0] == 24 * 32 == g["grid_fisheye_ray_indices"].shape[0]


@pytest.mark.parametrize("name", ["opencv", "fisheye", "equirect", "mixed", "grid_opencv", "grid_fisheye"])
def test_lens_functions_reproduce_the_reference_fixture(hc, name):
    g = load_golden("raygen_lenses")
    c = case_arrays(g, name)
    o, d, pa, dn = host_rays(hc, c["ray_indices"], c["c2w"], c["fx"], c["fy"], c["cx"], c["cy"], c["camera_type"],
                             c.get("distortion"))
    check_against_fixture(g, name, o, d, pa, dn)


def test_all_zero_parameters_pass_through_undistortion_bit_for_bit(hc):
    """The reference undistorts the whole batch when ANY camera has a non-zero parameter; lens.h tests per camera and skips
    the iteration for an all-zero row. No result changes: lens_undistort itself, run on zeros, returns its input bit for bit
    (the residual is exactly 0 and every step is 0 / -1), signed zeros and large coordinates included."""
    rs = np.random.RandomState(5)
    xy = np.concatenate([rs.uniform(-1.5, 1.5, (4096, 2)), rs.standard_normal((64, 2)) * 1e3,
                         [[0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [1e-30, -1e-30], [3.0e18, -2.0e18]]]).astype(np.float32)
    out = np.full_like(xy, np.nan)
    zeros = np.zeros(6, np.float32)
    hc.hc_lens_undistort(xy, xy.shape[0], zeros, out)
    np.testing.assert_array_equal(out.view(np.uint32), xy.view(np.uint32))
    assert hc.hc_lens_has_distortion(zeros) == 0
    for i in range(6):
        k = zeros.copy()
        k[i] = 1e-6
        assert hc.hc_lens_has_distortion(k) == 1
    # so a zero row next to distorted rows (the reference iterates on it, lens.h does not) gives the reference's rays: the
    # `opencv` case above holds such a camera; here its rays alone, against the reference's fp32 within one rounding of the tail
    g = load_golden("raygen_lenses")
    c = case_arrays(g, "opencv")
    keep = c["ray_indices"][:, 0] == 3
    assert keep.sum() >= 10 and not c["distortion"][3].any()
    o, d, pa, dn = host_rays(hc, c["ray_indices"][keep], c["c2w"], c["fx"], c["fy"], c["cx"], c["cy"], c["camera_type"],
                             c["distortion"])
    np.testing.assert_array_equal(o, c["origins"][keep])
    assert np.abs(d - c["directions"][keep]).max() <= 3 * float(g["e_ref_directions"])


def test_undistortion_inverts_the_opencv_model(hc):
    """lens_undistort solves distort(x, y) = (xd, yd): distorting its result in float64 gives the input back."""
    g = load_golden("raygen_lenses")
    rs = np.random.RandomState(6)
    xy = rs.uniform(-0.6, 0.6, (512, 2)).astype(np.float32)
    for k in g["opencv_distortion"][:3]:
        out = np.empty_like(xy)
        hc.hc_lens_undistort(xy, xy.shape[0], np.ascontiguousarray(k), out)
        x, y = out[:, 0].astype(np.float64), out[:, 1].astype(np.float64)
        k1, k2, k3, k4, p1, p2 = k.astype(np.float64)
        r = x * x + y * y
        d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        back = np.stack([d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x), d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y)], -1)
        assert np.abs(back - xy).max() <= 4 * 2.0 ** -23, k  # a few roundings of coordinates below 1


def test_pinhole_rays_through_the_lens_functions_match_the_pinhole_fixture(hc):
    """Type 1 without distortion through raygen_lens_one is the pinhole generator: raygen.npz within the tolerances of
    test_gpu_kernels.test_raygen_golden, with a null parameter pointer and with a zero row."""
    g = load_golden("raygen")
    C_ = g["fx"].shape[0]
    for dist in (None, np.zeros((C_, 6), np.float32)):
        o, d, pa, dn = host_rays(hc, g["ray_indices"], g["c2w"], g["fx"], g["fy"], g["cx"], g["cy"], np.ones(C_, np.int32), dist)
        np.testing.assert_array_equal(o, g["origins"])
        np.testing.assert_allclose(d, g["directions"], atol=2e-7, rtol=1e-5)
        np.testing.assert_allclose(pa, g["pixel_area"], atol=1e-6, rtol=2e-4)
        np.testing.assert_allclose(dn, g["directions_norm"], atol=1e-6, rtol=1e-6)


def test_local_directions_by_type(hc):
    uv = np.array([[0.3, -0.2], [-0.7, 0.45], [1e-3, 2e-3]], np.float32)
    out = np.empty((3, 3), np.float32)
    hc.hc_lens_local_direction(1, uv, 3, out)
    np.testing.assert_array_equal(out, np.concatenate([uv, -np.ones((3, 1), np.float32)], -1))
    u, v = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    hc.hc_lens_local_direction(2, uv, 3, out)
    th = np.sqrt(u * u + v * v)
    np.testing.assert_allclose(out, np.stack([u * np.sin(th) / th, v * np.sin(th) / th, -np.cos(th)], -1), atol=2e-7, rtol=0)
    assert np.abs(np.linalg.norm(out.astype(np.float64), axis=-1) - 1).max() < 3e-7  # fisheye directions are unit vectors
    hc.hc_lens_local_direction(3, uv, 3, out)
    th, ph = -np.pi * u, np.pi * (0.5 - v)
    np.testing.assert_allclose(out, np.stack([-np.sin(th) * np.sin(ph), np.cos(ph), -np.cos(th) * np.sin(ph)], -1), atol=3e-7,
                               rtol=0)
    big = np.array([[3.0, 3.0]], np.float32)  # theta is clipped to pi: straight backwards
    hc.hc_lens_local_direction(2, big, 1, out[:1])
    assert out[0, 2] == 1.0 and abs(out[0, 0]) < 1e-6


# ---------------------------------------------------------------- host logic ----------------------------------------
def cam(**over):
    base = dict(camera_to_worlds=torch.eye(4)[None, :3], fx=torch.tensor([[100.0]]), fy=torch.tensor([[101.0]]),
                cx=torch.tensor([[31.5]]), cy=torch.tensor([[24.25]]), height=torch.tensor([[48]]), width=torch.tensor([[64]]),
                camera_type=torch.tensor([[1]]), distortion_params=None)
    base.update(over)
    return types.SimpleNamespace(**base)


def test_ray_generator_accepts_lens_cameras_and_rejects_the_rest():
    from nerfstudio_amd.model_components.ray_generators import RayGenerator

    n = 3
    many = dict(camera_to_worlds=torch.eye(4)[None, :3].repeat(n, 1, 1), fx=torch.full((n, 1), 50.0), fy=torch.full((n, 1), 50.0),
                cx=torch.full((n, 1), 28.0), cy=torch.full((n, 1), 20.0))
    gen = RayGenerator(cam(**many, camera_type=torch.tensor([[1], [2], [3]]),
                           distortion_params=torch.tensor([[-0.12, 0.03, 0, 0, 1e-3, -2e-3], [0.0] * 6, [0.0] * 6])))
    assert not gen.pinhole and gen.camera_type.dtype == torch.int32 and gen.camera_type.tolist() == [1, 2, 3]
    assert gen.distortion.shape == (3, 6) and gen.distortion.dtype == torch.float32
    assert "camera_type" not in gen.state_dict() and "distortion" not in gen.state_dict()  # non-persistent buffers
    gen = RayGenerator(cam(**many, camera_type=torch.tensor([[2], [2], [2]])))  # fisheye, distortion_params None -> zeros
    assert not gen.pinhole and not gen.distortion.any() and gen.distortion.shape == (3, 6)
    gen = RayGenerator(cam(**many, camera_type=torch.tensor([[1], [1], [1]]), distortion_params=torch.zeros(n, 6)))
    assert gen.pinhole  # today's kernel for undistorted perspective cameras
    assert RayGenerator(types.SimpleNamespace(**many)).pinhole  # no camera_type attribute: perspective
    assert not RayGenerator(cam(distortion_params=torch.tensor([[0.1, 0, 0, 0, 0, 0]]))).pinhole
    with pytest.raises(ValueError, match="camera type 9.*FISHEYE624"):
        RayGenerator(cam(camera_type=torch.tensor([[9]])))
    with pytest.raises(ValueError, match="camera type 8.*ORTHOPHOTO"):
        RayGenerator(cam(**many, camera_type=torch.tensor([[1], [8], [3]])))
    with pytest.raises(ValueError, match="camera type 4"):
        RayGenerator(cam(camera_type=torch.tensor([[4]])))


def test_lens_camera_args_picks_one_camera_of_a_covered_type():
    from nerfstudio_amd.eval_render import in_loop_camera_args, lens_camera_args, pinhole_camera_args

    c2w, fx, fy, cx, cy, h, w, ctype, dist = lens_camera_args(cam())
    assert (fx, fy, cx, cy, h, w, ctype, dist) == (100.0, 101.0, 31.5, 24.25, 48, 64, 1, None) and c2w.shape == (3, 4)
    assert lens_camera_args(cam())[:7][1:] == pinhole_camera_args(cam())[1:]
    k = torch.tensor([[-0.12, 0.03, 0.0, 0.0, 1e-3, -2e-3]])
    for t in (1, 2, 3):
        args = lens_camera_args(cam(camera_type=torch.tensor([[t]]), distortion_params=k))
        assert args[7] == t and torch.equal(args[8], k[0]) and args[8].shape == (6,)
    assert lens_camera_args(cam(camera_to_worlds=torch.eye(4)[:3]))[7] == 1                          # an unbatched [3, 4] pose
    assert lens_camera_args(types.SimpleNamespace(**{k_: v for k_, v in vars(cam()).items() if k_ != "camera_type"}))[7] == 1
    assert lens_camera_args(cam(camera_to_worlds=torch.eye(4)[None, :3].repeat(2, 1, 1))) is None    # two cameras
    assert lens_camera_args(cam(fx=torch.tensor([[100.0], [101.0]]))) is None
    assert lens_camera_args(types.SimpleNamespace(camera_to_worlds=torch.eye(4)[None, :3])) is None  # no intrinsics
    for t in (4, 5, 6, 7, 8, 9):
        assert lens_camera_args(cam(camera_type=torch.tensor([[t]]))) is None
    # Model.get_outputs_for_camera: in the chunk loop for perspective cameras, distorted or not; other lenses keep the bundle
    assert in_loop_camera_args(cam())[1] is None and in_loop_camera_args(cam())[0][1:] == pinhole_camera_args(cam())[1:]
    args, lens = in_loop_camera_args(cam(distortion_params=k))
    assert len(args) == 7 and lens[0] == 1 and torch.equal(lens[1], k[0])
    assert in_loop_camera_args(cam(camera_type=torch.tensor([[2]]))) is None
    assert in_loop_camera_args(cam(camera_type=torch.tensor([[3]]), distortion_params=k)) is None
    assert in_loop_camera_args(cam(camera_type=torch.tensor([[9]]))) is None
    # pinhole_camera_args itself is unchanged
    assert pinhole_camera_args(cam(distortion_params=torch.zeros(1, 6))) is not None
    assert pinhole_camera_args(cam(camera_type=torch.tensor([[2]]))) is None
    assert pinhole_camera_args(cam(distortion_params=k)) is None
    assert pinhole_camera_args(cam(camera_to_worlds=torch.eye(4)[None, :3].repeat(2, 1, 1))) is None
    assert len(pinhole_camera_args(cam())) == 7


def test_lens_entry_points_validate_before_launching():
    """Null pointers, no cameras or a negative count: NSAMD_ERR_INVALID_ARG (-1) with nothing launched; a camera type outside
    1 - 3 by value: NSAMD_ERR_UNSUPPORTED (-2); an empty launch is a no-op. The indexed form's types are device memory: the
    Python layer checks them."""
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import functional as F

    lib = N.load()
    assert lib.nsamd_raygen_lens(None, None, None, None, None, None, None, None, 5, 1, None, None, None, None, None) == -1
    assert lib.nsamd_raygen_lens(None, None, None, None, None, None, None, None, 0, 1, None, None, None, None, None) == 0
    assert lib.nsamd_raygen_lens(None, None, None, None, None, None, None, None, 0, 0, None, None, None, None, None) == -1
    assert lib.nsamd_raygen_lens(None, None, None, None, None, None, None, None, -1, 1, None, None, None, None, None) == -1
    assert lib.nsamd_raygen_lens_grid(None, 50.0, 50.0, 1.0, 1.0, 1, None, 8, 0, 5, 8, None, None, None, None) == -1
    assert lib.nsamd_raygen_lens_grid(None, 50.0, 50.0, 1.0, 1.0, 1, None, 8, 0, -1, 8, None, None, None, None) == -1
    assert lib.nsamd_raygen_lens_grid(None, 50.0, 50.0, 1.0, 1.0, 1, None, 8, 0, 5, 4, None, None, None, None) == -1
    assert lib.nsamd_raygen_lens_grid(None, 50.0, 50.0, 1.0, 1.0, 1, None, 0, 0, 5, 8, None, None, None, None) == -1
    assert lib.nsamd_raygen_lens_grid(None, 50.0, 50.0, 1.0, 1.0, 2, None, 8, 0, 0, 0, None, None, None, None) == 0
    for t in (0, 4, 9, -1):
        assert lib.nsamd_raygen_lens_grid(None, 50.0, 50.0, 1.0, 1.0, t, None, 8, 0, 5, 8, None, None, None, None) == -2
    F.check_lens_types(torch.tensor([1, 2, 3, 3]))
    with pytest.raises(ValueError, match="camera type 9"):
        F.check_lens_types(torch.tensor([[1], [9]]))
