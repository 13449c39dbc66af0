"""nsamd_camera_apply / nsamd_camera_backward (csrc/camera.hip) through the Python launch layer, entry by entry against the float64
reference of tests/camera_reference.py (the torch mirror of the exponential maps in double, autograd through it, the upstream
level sum in fp32 in list order) — what the .hip file adds to the per-camera arithmetic of camera.h, which the host tests cover:
the per-ray gather of the pose, the clamp of the camera index, the level sum, the per-camera double accumulation with every
thread striding over all rays, the 256-wide tree, the regulariser's extra workgroup and its `k += 256` loop, `dpose +=`, the
nullable regulariser output, n = 0. The bounds and their derivation (one u per fp32 operation of cam_exp_map and of the 3-term
dot product in the kernel's order, sinf / cosf charged 2 ulp, the amplification through 1 - cos and the divisions by t^2 / t^3
carried by the error rules; backward: the four fp32 roundings of `dpose += (float)dp + (float)dr`, those with a zero operand not
charged, plus 2^-40 of the sum of the absolute values of the terms entering the entry — 2^16 below the fp32 roundings) are in
that module's docstring; tests/test_camera_reference_cpu.py shows without a GPU that they reject per-camera sums in fp32, the
levels in reverse order, `dpose =` and a regulariser loop that starts at tid + 256.

Shapes, each the smallest that bites:
* forward (n, C) = (1, 1), (255, 3), (256, 3), (257, 3) — one workgroup less one lane, exactly one, one lane of a second — and
  (1000, 300); over every special pose (|w| ~ 5e-4, around and within 1e-5 of both branch points, zero, pure translation /
  rotation, |w| = 3.1 and 5, |v| = 50). SO3xR3 origins are the same bits as fl(raw_o + v).
* backward C = 3, n = 769 = 3 x 256 + 1, all rays on camera 1: four trips of thread 0, three of the others, every slot of the
  tree live; cameras 0 and 2 get the regulariser's gradient only. C = 300, n = 1000: the regulariser workgroup's loop takes a
  second trip (300 > 256), many cameras are empty. C = 1 with n = 1, 255, 256, 257. upstream.count 0 .. 4 with levels from 1e-6
  to 1e3 built so that the fp32 order of the sum matters; 5 and -1 refused. n = 0. dpose pre-filled with zero and with random
  values; regulariser pointer null and given (same dpose bits); penalties (0, 0), (1e-2, 1e-3) and the config defaults; all
  poses zero (the regulariser's gradient is exactly 0, SO3xR3 on its clamped branch); two launches, the same bits; camera
  indices -1 and C land on cameras 0 and C - 1 in both kernels.

Measured on MI355X (profiles/camera_pose_float64_ratios.txt), worst |err| / bound, and the same under a 1-ulp charge of sinf / cosf:
    forward  SO3xR3  directions 0.750 (0.750)        origins: the same bits as fl(raw_o + v)
    forward  SE3     directions 0.492 (0.492)        origins 0.773 (0.773)
    backward SO3xR3  dpose 0.980                     regulariser 0.558
    backward SE3     dpose 0.974                     regulariser 0.558
per family: forward n = 1 / 255 / 256 / 257 / 1000 directions 0.43 / 0.75 / 0.67 / 0.71 / 0.51 (SO3xR3), SE3 origins 0.52 / 0.77 /
0.76 / 0.77 / 0.65; backward dpose C = 3 n = 769 0.84 - 0.91 over the level counts, C = 300 0.98, C = 1 0.63 - 0.81, n = 0 0.96,
zero poses 0.91, clamped indices 0.62. The two charges agree to 0.003: at every worst entry the roundings of the fp32 operations
around them carry the bound, not sinf / cosf, so these cases would pass a 1-ulp charge as well. test_trig_budget measures the
charge itself through the SE3 forward, 40 000 angles from 1.01e-2 to 7: cosf 0.948 ulp at the worst (|w| = 1.301431), the sine
chain at most 0.370 ulp beyond its two roundings — the device is inside 1 ulp there, the 2-ulp charge has that much room.
A correctly rounded result uses up to half an ulp where the backward bound charges u |x| >= half an ulp, hence ratios close
to 1 there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import camera_reference as cr
from float64_check import SAFE, TINY, check_entries, report

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
MODES = ["SO3xR3", "SE3"]


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native
    from nerfstudio_amd import functional as F

    _native.load()
    return F


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def penalties():
    from nerfstudio_amd.cameras.camera_optimizers import CameraOptimizerConfig

    cfg = CameraOptimizerConfig()
    return [(0.0, 0.0), (1e-2, 1e-3), (cfg.trans_l2_penalty, cfg.rot_l2_penalty)]


# ---------------------------------------------------------------------------------------------------------------- forward
def apply(F, mode, pose, raw_o, raw_d, cams):
    """-> (origins, directions) [n, 3] on the device; one NaN row behind each must stay NaN."""
    n = raw_o.shape[0]
    o, d = torch.full((n + 1, 3), NAN, device="cuda"), torch.full((n + 1, 3), NAN, device="cuda")
    F.camera_apply_launch(dev(pose), F.CAMERA_MODES[mode], dev(raw_o), dev(raw_d), dev(cams), o[:n], d[:n])
    torch.cuda.synchronize()
    assert bool(torch.isnan(o[n]).all()) and bool(torch.isnan(d[n]).all()), "written past the last ray"
    return o[:n], d[:n]


def one_ulp_ratio(name, got, ref, bound1, worst):
    r = np.abs(got.detach().cpu().double().numpy() - ref) / (bound1 * SAFE + TINY)
    worst[name] = max(worst.get(name, 0.0), float(r.max()) if r.size else 0.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,num_cameras", [(1, 1), (255, 3), (256, 3), (257, 3), (1000, 300)])
def test_forward_per_entry(F, mode, n, num_cameras):
    seeds = {1: range(29), 3: range(0, 30, 3), 300: [0]}[num_cameras]  # every special pose is seen at every C
    worst = {}
    for seed in seeds:
        pose = cr.poses(num_cameras, seed)
        raw_o, raw_d, cams = cr.rays(n, num_cameras, 10 * n + seed)
        o, d = apply(F, mode, pose, raw_o, raw_d, cams)
        o64, d64 = cr.forward64(mode, pose, raw_o, raw_d, cams)
        _, oe, _, de = cr.forward_tracked(mode, pose, raw_o, raw_d, cams)
        _, oe1, _, de1 = cr.forward_tracked(mode, pose, raw_o, raw_d, cams, trig_ulp=1.0)
        if mode == "SO3xR3":  # fl(raw_o + v): no rounding precedes the sum
            want = raw_o + pose[cams, :3]
            assert want.dtype == F32 and torch.equal(bits(o), bits(torch.from_numpy(want))), "SO3xR3 origins: other bits"
        else:
            check_entries("origins", o, o64, oe, worst)
            one_ulp_ratio("origins (1-ulp charge)", o, o64, oe1, worst)
        check_entries("directions", d, d64, de, worst)
        one_ulp_ratio("directions (1-ulp charge)", d, d64, de1, worst)
    report(f"camera_apply {mode} n = {n} C = {num_cameras}", worst)


@pytest.mark.parametrize("mode", MODES)
def test_forward_empty_and_clamped_indices(F, mode):
    """n = 0 returns OK and writes nothing; camera indices -1 and C give the rows of cameras 0 and C - 1 (the kernel clamps
    before any read: a defined input)."""
    num_cameras = 5
    pose = cr.poses(num_cameras, 19)
    raw_o, raw_d, cams = cr.rays(8, num_cameras, 1, cams=[0, -1, 4, 5, 2, -1, 5, 3])
    o, d = apply(F, mode, pose, raw_o, raw_d, cams)
    o2, d2 = apply(F, mode, pose, raw_o, raw_d, cr.clamp_cams(cams, num_cameras))
    assert torch.equal(bits(o), bits(o2)) and torch.equal(bits(d), bits(d2))
    o64, d64 = cr.forward64(mode, pose, raw_o, raw_d, cams)
    _, oe, _, de = cr.forward_tracked(mode, pose, raw_o, raw_d, cams)
    worst = {}
    if mode == "SO3xR3":
        assert torch.equal(bits(o), bits(torch.from_numpy(raw_o + pose[cr.clamp_cams(cams, num_cameras), :3])))
    else:
        check_entries("origins", o, o64, oe, worst)
    check_entries("directions", d, d64, de, worst)
    report(f"camera_apply {mode} clamped indices", worst)
    apply(F, mode, pose, raw_o[:0], raw_d[:0], cams[:0])  # (asserts that nothing was written)


def test_trig_budget(F):
    """The charge the forward bound rests on, measured through the SE3 forward itself: for w = (x, 0, 0), v = 0 and the ray
    direction (0, 1, 0) the kernel's operations reduce to d[1] = cosf(th) EXACTLY (b w1 w1 + cs with w1 = 0, times 1, plus
    zeros) and d[2] = fl(fl(sinf(th) / th) x), with th = sqrtf(fl(x x)) as numpy forms it. Over |w| from the branch point 1e-2
    to 7 (past 2 pi; the pose set reaches 5): cosf within 2 ulp of cos — relative, also next to its zeros, as the bound charges
    it — and the sine chain within 2 ulp plus its two roundings, on the x with th == x."""
    rs = np.random.RandomState(0)
    x = np.concatenate([10.0 ** rs.uniform(np.log10(1.01e-2), np.log10(7.0), 20000), rs.uniform(1.01e-2, 7.0, 20000)]).astype(F32)
    n = x.size
    pose = np.zeros((n, 6), F32)
    pose[:, 3] = x
    th32 = np.sqrt(x * x)
    assert th32.dtype == F32 and (th32 >= F32(1.005e-2)).all()  # none on the Taylor branch
    raw_d = np.tile(np.array([0, 1, 0], F32), (n, 1))
    _, d = apply(F, "SE3", pose, np.zeros((n, 3), F32), raw_d, np.arange(n, dtype=np.int64))
    d = d.cpu().double().numpy()
    th = th32.astype(np.float64)
    ulp = 2.0**-23
    e_cos = np.abs(d[:, 1] - np.cos(th)) / (np.abs(np.cos(th)) * ulp)
    same = th32 == x
    e_sin = (np.abs(d[same, 2] - np.sin(th[same])) - 2 * cr.U * np.abs(np.sin(th[same]))) / (np.abs(np.sin(th[same])) * ulp)
    print(f"\ncosf through camera_apply: worst {e_cos.max():.3f} ulp at |w| = {th[np.argmax(e_cos)]:.6f}; sinf through sn / th * th "
          f"({int(same.sum())} of {n} points): at most {e_sin.max():.3f} ulp beyond its two roundings (budget 2 each)")
    assert same.sum() > n // 2
    assert e_cos.max() <= 2.0 and e_sin.max() <= 2.0


# --------------------------------------------------------------------------------------------------------------- backward
def backward(F, mode, pose, raw_d, cams, lo, ld, pens, old, with_reg=True):
    """-> (dpose [C, 6], regulariser value [1] or None) on the device; a NaN row behind dpose must stay NaN."""
    num_cameras = pose.shape[0]
    buf = torch.full((num_cameras + 1, 6), NAN, device="cuda")
    buf[:num_cameras] = dev(old)
    reg = torch.full((2,), NAN, device="cuda") if with_reg else None
    F.camera_backward_launch(dev(pose), F.CAMERA_MODES[mode], dev(raw_d), dev(cams), [dev(x) for x in lo], [dev(x) for x in ld],
                             pens[0], pens[1], buf[:num_cameras], reg[:1] if with_reg else None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[num_cameras]).all()) and (reg is None or bool(torch.isnan(reg[1]))), "written past the end"
    return buf[:num_cameras], (reg[:1] if with_reg else None)


def check_backward(F, mode, pose, raw_d, cams, lo, ld, pens, old, worst, tag=""):
    """One case: per entry against float64, the regulariser's value, the same dpose bits without the regulariser output and
    from a second launch. Returns the reference."""
    ref = cr.backward64(mode, pose, raw_d, cams, lo, ld, pens[0], pens[1], old)
    got, reg = backward(F, mode, pose, raw_d, cams, lo, ld, pens, old)
    check_entries("dpose" + tag, got, ref["dpose"], ref["dpose_bound"], worst)
    check_entries("regulariser" + tag, reg, [ref["reg"]], [ref["reg_bound"]], worst)
    again, _ = backward(F, mode, pose, raw_d, cams, lo, ld, pens, old)
    assert torch.equal(bits(again), bits(got)), "two launches on the same inputs differ"
    no_reg, _ = backward(F, mode, pose, raw_d, cams, lo, ld, pens, old, with_reg=False)
    assert torch.equal(bits(no_reg), bits(got)), "dpose depends on the regulariser pointer"
    return ref, got


def prefills(num_cameras, seed):
    return [np.zeros((num_cameras, 6), F32), np.random.RandomState(seed).normal(0, 1, (num_cameras, 6)).astype(F32)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", [0, 1, 2, 3, 4])
def test_backward_one_camera_of_three(F, mode, count):
    """C = 3, n = 769 = 3 x 256 + 1, every ray on camera 1."""
    num_cameras, n = 3, 769
    worst = {}
    for seed in (39, 8, 15, 18, 19, 20, 21, 22, 27):  # camera 1 holds special pose (seed + 1) % 40
        pose = cr.poses(num_cameras, seed)
        _, raw_d, cams = cr.rays(n, num_cameras, seed, cams=1)
        lo, ld = cr.upstream_levels(n, count, 7 * seed + count)
        for pens in penalties():
            for old in prefills(num_cameras, seed):
                ref, _ = check_backward(F, mode, pose, raw_d, cams, lo, ld, pens, old, worst)
                assert (ref["dp"][[0, 2]] == 0).all() and (count == 0 or (ref["dp"][1] != 0).any())
    report(f"camera_backward {mode} C = 3 n = 769 on camera 1, {count} levels", worst)


@pytest.mark.parametrize("mode", MODES)
def test_backward_many_cameras(F, mode):
    """C = 300 > 256 (the regulariser's loop takes a second trip), n = 1000 random cameras, many of them empty."""
    num_cameras, n = 300, 1000
    worst = {}
    pose = cr.poses(num_cameras)
    _, raw_d, cams = cr.rays(n, num_cameras, 5)
    assert np.setdiff1d(np.arange(num_cameras), cams).size > 5
    for count in (4, 1):
        lo, ld = cr.upstream_levels(n, count, 11 + count)
        for pens in penalties():
            for old in prefills(num_cameras, 6):
                check_backward(F, mode, pose, raw_d, cams, lo, ld, pens, old, worst)
    report(f"camera_backward {mode} C = 300 n = 1000", worst)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_backward_single_camera(F, mode, n):
    worst = {}
    for seed in (0, 9, 16, 19, 20, 21, 22, 23, 28):
        pose = cr.poses(1, seed)
        _, raw_d, cams = cr.rays(n, 1, seed + n)
        lo, ld = cr.upstream_levels(n, 2, seed)
        for old in prefills(1, seed):
            check_backward(F, mode, pose, raw_d, cams, lo, ld, (1e-2, 1e-3), old, worst)
    report(f"camera_backward {mode} C = 1 n = {n}", worst)


@pytest.mark.parametrize("mode", MODES)
def test_backward_no_rays(F, mode):
    """n = 0 with count = 0: dpose += the regulariser's gradient only, and its value is written."""
    worst = {}
    for num_cameras in (1, 3, 300):
        pose = cr.poses(num_cameras, 2)
        for pens in penalties():
            for old in prefills(num_cameras, 1):
                ref, _ = check_backward(F, mode, pose, np.zeros((0, 3), F32), np.zeros(0, np.int64), [], [], pens, old, worst)
                assert (ref["dp"] == 0).all()
    report(f"camera_backward {mode} n = 0", worst)


@pytest.mark.parametrize("mode", MODES)
def test_backward_zero_poses(F, mode):
    """Every pose zero, the state training starts from: the regulariser's gradient is exactly zero (so with no ray dpose keeps
    its bits) and its value is 0; SO3xR3 takes its clamped branch."""
    num_cameras, n = 3, 769
    pose = np.zeros((num_cameras, 6), F32)
    worst = {}
    old = prefills(num_cameras, 3)[1]
    got, reg = backward(F, mode, pose, np.zeros((0, 3), F32), np.zeros(0, np.int64), [], [], (1e-2, 1e-3), old)
    assert torch.equal(bits(got), bits(torch.from_numpy(old))) and float(reg) == 0.0
    _, raw_d, cams = cr.rays(n, num_cameras, 4)
    lo, ld = cr.upstream_levels(n, 4, 5)
    for o in prefills(num_cameras, 3):
        ref, _ = check_backward(F, mode, pose, raw_d, cams, lo, ld, (1e-2, 1e-3), o, worst)
        assert (ref["dr"] == 0).all() and ref["reg"] == 0.0
    report(f"camera_backward {mode} zero poses", worst)


@pytest.mark.parametrize("mode", MODES)
def test_backward_clamped_indices_and_refusals(F, mode):
    """Camera indices -1 and C land on cameras 0 and C - 1 (the same bits as the clamped list, consistent with the forward);
    upstream.count = 5 and -1 are refused with nothing written."""
    from nerfstudio_amd import _native as N

    num_cameras, n = 4, 300
    pose = cr.poses(num_cameras, 20)
    _, raw_d, cams = cr.rays(n, num_cameras, 6)
    cams[::7], cams[3::11] = -1, num_cameras
    lo, ld = cr.upstream_levels(n, 3, 2)
    old = prefills(num_cameras, 2)[1]
    worst = {}
    _, got = check_backward(F, mode, pose, raw_d, cams, lo, ld, (1e-2, 1e-3), old, worst)
    clamped, _ = backward(F, mode, pose, raw_d, cr.clamp_cams(cams, num_cameras), lo, ld, (1e-2, 1e-3), old)
    assert torch.equal(bits(clamped), bits(got))
    report(f"camera_backward {mode} clamped indices", worst)
    # refusals
    t_pose, t_d, t_c = dev(pose), dev(raw_d), dev(cr.clamp_cams(cams, num_cameras))
    levels = [dev(x) for x in lo] + [dev(lo[0])]
    dpose, reg = torch.full((num_cameras, 6), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    for count in (5, -1):
        up = N.RayGrads()
        for k in range(4):
            up.d_origins[k], up.d_directions[k] = N.ptr(levels[k]), N.ptr(levels[k])
        up.count = count
        status = N.load().nsamd_camera_backward(N.ptr(t_pose), F.CAMERA_MODES[mode], num_cameras, N.ptr(t_d), N.ptr(t_c), n, up,
                                                C.c_float(1e-2), C.c_float(1e-3), N.ptr(dpose), N.ptr(reg), N.stream())
        torch.cuda.synchronize()
        assert status != 0 and "invalid argument" in N.status_string(status)
        assert bool(torch.isnan(dpose).all()) and bool(torch.isnan(reg).all())
