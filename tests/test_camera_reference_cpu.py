"""tests/camera_reference.py (what tests/test_gpu_camera_pose.py holds nsamd_camera_apply / nsamd_camera_backward to) pinned,
without a GPU, to what already exists:

* per camera to csrc/camera.h as the host compiler builds it (tests/hostcheck: hc_cam_exp_map, hc_cam_exp_map_bwd) — the very
  functions the kernels run per camera — within the module's own per-entry bounds; the per-camera sums are formed in numpy from
  rays whose values are multiples of 1/8, so that they are exact and fp32 holds them (hc_cam_exp_map_bwd takes them as fp32);
* on the rays and poses of tests/golden/camera_opt.npz to that fixture's corrected origins and directions (the reference's own
  fp32 evaluation, in the same operation order: within the forward bound);
* the value track of the bound's restatement of cam_exp_map to the torch mirror (1e-12: the same function);
* and it shows that the inputs and bounds reject a model of each defect the GPU test is there to catch: per-camera sums
  accumulated in fp32 (256 strided partial sums and the tree, as the kernel lays them out), the upstream levels summed in
  reverse order, `dpose =` for `+=`, a regulariser mean that misses the first 256 cameras.
Every test prints its worst |err| / bound before it asserts."""
import numpy as np
import pytest
import torch

import camera_reference as cr
from float64_check import SAFE, TINY, check_entries, report
from test_kernel_helpers_cpu import hc  # noqa: F401  (the fixture that builds tests/hostcheck)

F32 = np.float32


def _mirror(mode, pose):
    return cr._exp_map(mode)(torch.from_numpy(pose.astype(np.float64))).numpy()


def _tracked(mode, pose, ulp=2.0):
    R, t = cr.exp_map_tracked(mode, pose, ulp)
    val, err = np.zeros((pose.shape[0], 3, 4)), np.zeros((pose.shape[0], 3, 4))
    for i in range(3):
        for j in range(3):
            val[:, i, j], err[:, i, j] = R[3 * i + j].v, R[3 * i + j].e
        val[:, i, 3], err[:, i, 3] = t[i].v, t[i].e
    return val, err


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_exp_map_against_camera_h_on_the_host(hc, mode):
    pose = cr.poses(300)
    C = pose.shape[0]
    want = _mirror(mode, pose)
    val, err = _tracked(mode, pose)
    np.testing.assert_allclose(val, want, rtol=1e-12, atol=1e-13)  # the restatement is the mirror's function
    got = np.zeros((C, 3, 4), F32)
    hc.hc_cam_exp_map(cr.MODES[mode], pose, C, got.reshape(-1))
    worst = {}
    check_entries("R|t", got, want, err, worst)
    one = _tracked(mode, pose, 1.0)[1]
    worst["R|t under a 1-ulp charge"] = float((np.abs(got - want) / (one * SAFE + TINY)).max())
    report(f"camera.h exp map on the host, {mode}", worst)
    if mode == "SO3xR3":
        assert np.array_equal(got[:, :, 3], pose[:, :3])
    # the bound is of the size of the roundings it counts: nowhere above 2e-5 |v| + 4e-6 (the |v| = 50 pose just above the SE3
    # branch point is the largest), and a few u for the ordinary poses
    scale = 1.0 + np.linalg.norm(pose[:, :3].astype(np.float64), axis=1)
    assert (err.max(axis=(1, 2)) <= 2e-5 * scale).all() and np.median(err.max(axis=(1, 2))) <= 40 * cr.U


def _eighths(rs, shape, lim=32):
    return (rs.randint(-lim, lim + 1, shape) / 8.0).astype(F32)


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
@pytest.mark.parametrize("pens", [(0.0, 0.0), (1e-2, 1e-3)])
def test_backward_against_camera_h_on_the_host(hc, mode, pens):
    rs = np.random.RandomState(5)
    C, n = 300, 4000
    pose = cr.poses(C)
    cams = rs.randint(0, C - 20, n).astype(np.int64)  # the last 20 cameras see no ray
    raw_d, go, gd = _eighths(rs, (n, 3), 8), _eighths(rs, (n, 3)), _eighths(rs, (n, 3))
    ref = cr.backward64(mode, pose, raw_d, cams, [go], [gd], pens[0], pens[1], np.zeros((C, 6), F32))
    up = np.zeros((C, 3, 4))
    np.add.at(up[:, :, :3], cams, gd.astype(np.float64)[:, :, None] * raw_d.astype(np.float64)[:, None, :])
    np.add.at(up[:, :, 3], cams, go.astype(np.float64))
    up32 = up.astype(F32)
    assert np.array_equal(up32.astype(np.float64), up), "the per-camera sums are exact in fp32 by construction"
    got = np.zeros((C, 6), F32)
    hc.hc_cam_exp_map_bwd(cr.MODES[mode], pose, up32.reshape(-1), C, pens[0], pens[1], 1, got.reshape(-1))
    worst = {}
    check_entries("dpose", got, ref["dpose"], ref["dpose_bound"], worst)
    # the Jacobian the bound's abs-sum uses reproduces the autograd gradient
    np.testing.assert_allclose(np.einsum("cijk,cij->ck", ref["jac"], up), ref["dp"], rtol=1e-9, atol=1e-9)
    report(f"camera.h backward on the host, {mode}, penalties {pens}", worst)
    assert (ref["dr"] == 0).all() == (pens == (0.0, 0.0))
    assert (ref["dp"][C - 20:] == 0).all()


def test_golden_fixture_within_the_forward_bound(golden):
    g = golden("camera_opt")
    worst = {}
    for mode in ("SO3xR3", "SE3"):
        pose = g["pose_adjustment"]
        cr.check_branches(pose)
        o, d = cr.forward64(mode, pose, g["origins"], g["directions"], g["cams"])
        ov, oe, dv, de = cr.forward_tracked(mode, pose, g["origins"], g["directions"], g["cams"])
        np.testing.assert_allclose(ov, o, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(dv, d, rtol=1e-12, atol=1e-13)
        check_entries(f"{mode} origins", g[f"{mode}_origins"], o, oe, worst)
        check_entries(f"{mode} directions", g[f"{mode}_directions"], d, de, worst)
    report("golden camera_opt", worst)


def test_level_sum_is_the_sequential_fp32_sum_and_its_order_matters():
    n = 769
    (lo, ld) = cr.upstream_levels(n, 4, 1)
    s = cr.level_sum32(lo, n)
    seq = np.zeros((n, 3), F32)
    for i in range(n):
        for k in range(3):
            acc = F32(0.0)
            for lv in lo:
                acc = F32(acc + lv[i, k])
            seq[i, k] = acc
    assert np.array_equal(s.view(np.int32), seq.view(np.int32))
    rev = cr.level_sum32(lo[::-1], n)
    assert (rev != s).mean() > 0.9 and np.abs(rev.astype(np.float64) - s).max() > 1e-5
    mags = [float(np.abs(x).mean()) for x in lo]
    assert mags[0] > 5e2 and mags[2] < 2e-6 and max(mags) / min(mags) > 1e8


# ------------------------------------------------------------------------------------------------ models of the defects
def _kernel_sums(raw_d, cams, C, go, gd, acc_dtype):
    """camera_backward_kernel's per-camera sums: thread tid adds its rays tid, tid + 256, ... in order, then the 256-wide tree."""
    n = raw_d.shape[0]
    out = np.zeros((C, 3, 4))
    terms = np.concatenate([(gd.astype(np.float64)[:, :, None] * raw_d.astype(np.float64)[:, None, :]),
                            go.astype(np.float64)[:, :, None]], axis=2)  # [n, 3, 4]: the products are formed in double
    for c in range(C):
        acc = np.zeros((256, 3, 4), acc_dtype)
        for i in np.flatnonzero(cams == c):
            acc[i % 256] = (acc[i % 256] + terms[i].astype(acc_dtype)).astype(acc_dtype)
        m = 128
        while m > 0:
            acc[:m] = (acc[:m] + acc[m:2 * m]).astype(acc_dtype)
            m >>= 1
        out[c] = acc[0]
    return out


def _model_dpose(ref, sums, old, assign=False):
    dp = np.einsum("cijk,cij->ck", ref["jac"], sums)
    add = (dp.astype(F32) + ref["dr"].astype(F32)).astype(F32)
    return add if assign else (old + add).astype(F32)


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_bounds_reject_models_of_the_defects(mode):
    """The GPU test's first backward case (C = 3, 769 rays on camera 1, four levels) through a numpy model of the kernel: the
    faithful model passes; each defect fails the per-entry check."""
    C, n = 3, 769
    pose = cr.poses(C, seed=8)
    _, raw_d, cams = cr.rays(n, C, 2, cams=1)
    lo, ld = cr.upstream_levels(n, 4, 3)
    old = np.random.RandomState(4).normal(0, 1, (C, 6)).astype(F32)
    zero = np.zeros((C, 6), F32)

    def passes(got, ref):
        try:
            check_entries("dpose", got, ref["dpose"], ref["dpose_bound"], {})
            return True
        except AssertionError:
            return False

    go, gd = cr.level_sum32(lo, n), cr.level_sum32(ld, n)
    for pens in ((0.0, 0.0), (1e-2, 1e-3)):
        ref_old = cr.backward64(mode, pose, raw_d, cams, lo, ld, pens[0], pens[1], old)
        ref_zero = cr.backward64(mode, pose, raw_d, cams, lo, ld, pens[0], pens[1], zero)
        good = _kernel_sums(raw_d, cams, C, go, gd, np.float64)
        assert passes(_model_dpose(ref_old, good, old), ref_old) and passes(_model_dpose(ref_zero, good, zero), ref_zero)
        # sums accumulated in float
        assert not passes(_model_dpose(ref_zero, _kernel_sums(raw_d, cams, C, go, gd, F32), zero), ref_zero)
        # levels summed in reverse order
        rev = _kernel_sums(raw_d, cams, C, cr.level_sum32(lo[::-1], n), cr.level_sum32(ld[::-1], n), np.float64)
        assert not passes(_model_dpose(ref_zero, rev, zero), ref_zero)
        # dpose = instead of +=
        assert not passes(_model_dpose(ref_old, good, old, assign=True), ref_old)
    # the regulariser's mean without the cameras a loop from tid + 256 skips
    pose = cr.poses(300)
    ref = cr.backward64(mode, pose, np.zeros((0, 3), F32), np.zeros(0, np.int64), [], [], 1e-2, 1e-3, np.zeros((300, 6), F32))
    tp, rp = float(F32(1e-2)), float(F32(1e-3))
    p64 = pose.astype(np.float64)

    def value(first):
        return F32(F32(np.linalg.norm(p64[first:, :3], axis=1).sum() / 300) * F32(tp) + F32(np.linalg.norm(p64[first:, 3:], axis=1).sum() / 300) * F32(rp))

    assert abs(float(value(0)) - ref["reg"]) <= ref["reg_bound"] * SAFE
    assert abs(float(value(256)) - ref["reg"]) > 1e3 * ref["reg_bound"]
