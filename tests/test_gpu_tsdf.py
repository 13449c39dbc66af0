"""GPU tests of nsamd_tsdf_integrate (csrc/tsdf.hip over csrc/tsdf.h), export.TSDFVolume and export.fuse_views.

Float64 parity under the rule of tests/tsdf_reference.py: on the voxels no fp32 evaluation can legitimately decide differently
(at most 3 % of a case are unsafe) the weights equal float64's exactly and values / colours lie within MARGIN = 4 times the
reference's own fp32 distance from float64 on the same case (tests/golden/tsdf.npz; where the fixture has no case, the distance
of the fp32 torch-op restatement, tsdf_reference.integrate_torch, on the same GPU and inputs). Every test prints its ratios before
it asserts; the ones seen on MI355X are in profiles/tsdf_float64_ratios.txt.
"""
import types

import numpy as np
import pytest
import torch

import tsdf_reference as tr
from oracle import nerfacto_oracle as orc

pytestmark = pytest.mark.gpu
T = torch.from_numpy
KEYS = ("values", "weights", "colors")


@pytest.fixture(scope="module", autouse=True)
def generators_left_as_found():
    """Building the end-to-end model draws from torch's global generators; tests that run after this module (some initialise
    their modules unseeded) see the stream they saw before it existed."""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu)


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    info = _native.device_info()
    assert info["wavefront_size"] == 64 and info["arch"].startswith("gfx950"), info
    return functional


@pytest.fixture(scope="module")
def g(golden):
    return golden("tsdf")


def new_volume(g, name):
    from nerfstudio_amd.export import TSDFVolume

    return TSDFVolume.from_aabb(T(g[f"{name}_aabb"]), T(g[f"{name}_dims"]), device="cuda")


def state_of(volume):
    return {k: getattr(volume, k).cpu().numpy() for k in KEYS}


def case_tensors(g, name):
    return tuple(T(g[f"{name}_{k}"]).cuda() for k in ("c2w", "K", "depth", "color"))


def f64_of(g, name, start=None):
    inp = tr.case_inputs(g, name)
    origin, voxel_size, truncation = tr.volume_geometry(inp["aabb"], inp["dims"])
    v, w, c = tr.initial_state(inp["dims"]) if start is None else (start["values"], start["weights"], start["colors"])
    return tr.integrate_f64(origin, voxel_size, truncation, v, w, c, inp["c2w"], inp["K"], inp["depth"], inp["color"])


@pytest.mark.parametrize("name", tr.CASES)
def test_cases_against_float64_and_the_reference(F, g, name):
    c2w, K, depth, color = case_tensors(g, name)
    vol = new_volume(g, name)
    vol.integrate(c2w, K, depth, color)
    e = float(g[f"e_ref_values_{name}"]), float(g[f"e_ref_colors_{name}"])
    ref = {k: g[f"{name}_batch_{k}"] for k in KEYS}
    first = state_of(vol)
    tr.check(first, f64_of(g, name), *e, ref=ref, label=f"gpu {name} batch")
    vol.integrate(c2w, K, depth, color)
    tr.check(state_of(vol), f64_of(g, name, start=first), *e, label=f"gpu {name} twice")
    if name == "B":  # the camera's plane stays untouched, no NaN; a second pass leaves the values as they are
        plane = g["B_voxel_coords"][2] == 0.25
        assert not first["weights"][plane].any() and (first["values"][plane] == -1).all()
        assert np.array_equal(state_of(vol)["values"], first["values"]) and first["weights"].max() == 1.0
        assert int((first["weights"] > 0).sum()) == 106


@pytest.mark.parametrize("name", tr.CASES)
def test_batch_equals_views_one_at_a_time_and_runs_repeat_bit_for_bit(F, g, name):
    c2w, K, depth, color = case_tensors(g, name)
    batch, again, seq, plain = (new_volume(g, name) for _ in range(4))
    batch.integrate(c2w, K, depth, color)
    again.integrate(c2w, K, depth, color)
    for b in range(c2w.shape[0]):
        seq.integrate(c2w[b:b + 1], K[b:b + 1], depth[b:b + 1], color[b:b + 1])
    for k in KEYS:
        assert torch.equal(getattr(again, k), getattr(batch, k)), f"two runs: {k}"
        assert torch.equal(getattr(seq, k), getattr(batch, k)), f"one at a time: {k}"
    plain.colors.fill_(0.25)  # colours absent: the same values and weights, the colours array untouched
    plain.integrate(c2w, K, depth)
    assert torch.equal(plain.values, batch.values) and torch.equal(plain.weights, batch.weights)
    assert bool((plain.colors == 0.25).all())


# Volumes of one lane, of less than a wavefront's multiple and of one lane more than a workgroup. Bounds where the fixture has no
# case, from the number format: a camera coordinate (|.| <= 4) is three products and three sums, each within half an ulp of 4
# (2.4e-7), on a row of the device's inverse that is an ulp or so off times |p| <= 1.8: 1.5e-6 per coordinate at worst, 2.6e-6
# for the three in the distance, 7e-7 more for the squares, their sums and the root: 3.3e-6, over the truncation (>= 3.3 here)
# 1e-6 in the new value. An update adds two roundings of numbers <= 2 and halves what the state carried: 2^-22 in all, for the
# value and for the colour.
SMALL = [((1, 1, 1), [[0.25, 0.125, -0.25], [2.25, 2.125, 1.75]]), ((3, 1, 70), [[-1, -0.1, -1], [1, 0.1, 1]]),
         ((1, 1, 257), [[-0.2, -0.2, -1], [1.8, 1.8, 1]])]
POISON, GUARD = -77.0, 512


@pytest.mark.parametrize("dims,aabb", SMALL)
def test_small_volumes_store_nothing_outside_their_arrays(F, g, dims, aabb):
    from nerfstudio_amd.export import TSDFVolume

    n = int(np.prod(dims))
    host = TSDFVolume.from_aabb(aabb, dims)
    slabs = {k: torch.full((GUARD + getattr(host, k).numel() + GUARD,), POISON, device="cuda") for k in KEYS}
    inner = {k: slabs[k][GUARD:GUARD + getattr(host, k).numel()].view(getattr(host, k).shape) for k in KEYS}
    for k in KEYS:
        inner[k].copy_(getattr(host, k))
    vol = TSDFVolume(inner["values"], inner["weights"], inner["colors"], host.origin, host.voxel_size)
    assert all(getattr(vol, k).data_ptr() == inner[k].data_ptr() for k in KEYS)
    c2w, K, depth, color = case_tensors(g, "A")
    depth = torch.full_like(depth, 3.0)  # every voxel that lands in an image is in front of the surface
    vol.integrate(c2w, K, depth, color)
    torch.cuda.synchronize()
    for k in KEYS:
        size = getattr(host, k).numel()
        assert bool((slabs[k][:GUARD] == POISON).all()) and bool((slabs[k][GUARD + size:] == POISON).all()), k
    f64 = tr.integrate_f64(host.origin.numpy(), host.voxel_size.numpy(), host.truncation, host.values.numpy(), host.weights.numpy(),
                           host.colors.numpy(), g["A_c2w"], g["A_K"], depth.cpu().numpy(), g["A_color"])
    got, safe = state_of(vol), tr.safe_voxels(f64)
    dv, dc = tr.distance(got["values"], f64, "values", safe), tr.distance(got["colors"], f64, "colors", safe)
    print(f"tsdf gpu {dims}: {n} voxels, touched {int(f64['touched'].sum())}, unsafe {int((~safe).sum())}, values {dv:.3e}, "
          f"colors {dc:.3e}")
    assert f64["touched"].any() and host.truncation >= 3.3
    assert np.array_equal(got["weights"][safe].astype(np.float64), f64["weights"][safe])
    assert dv <= 1e-6 + 2.0 ** -22 and dc <= 2.0 ** -22


def test_no_views_and_bad_arguments(F, g):
    from nerfstudio_amd import _native as N

    vol = new_volume(g, "B")
    before = {k: getattr(vol, k).clone() for k in KEYS}
    empty = lambda *shape: torch.empty(shape, device="cuda")  # noqa: E731
    vol.integrate(empty(0, 4, 4), empty(0, 3, 3), empty(0, 1, 6, 8), empty(0, 3, 6, 8))  # B = 0: nothing launched
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(getattr(vol, k), before[k])
    c2w, K, depth, color = case_tensors(g, "B")
    w2c, K2 = torch.inverse(c2w)[:, :3].contiguous(), K[:, :2].contiguous()
    args = (vol.origin.tolist(), vol.voxel_size.tolist(), vol.truncation, vol.values, vol.weights, vol.colors, w2c, K2)
    with pytest.raises(RuntimeError, match="status -1"):  # H <= 0
        F.tsdf_integrate_launch(*args, empty(1, 0, 8), None)
    native = N.TsdfVolume()
    for i in range(3):
        native.origin[i], native.voxel_size[i], native.dims[i] = -1.0, 0.25, 8
    native.truncation = 1.25
    d = depth[:, 0].contiguous()
    with pytest.raises(RuntimeError, match="status -1"):  # a null values pointer
        N.check(N.load().nsamd_tsdf_integrate(native, None, N.ptr(vol.weights), N.ptr(vol.colors), N.ptr(w2c), N.ptr(K2), 1, N.ptr(d),
                                              None, 6, 8, N.stream()), "tsdf_integrate")
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(getattr(vol, k), before[k])
    vol.integrate(c2w.cpu(), K.cpu(), depth.cpu(), color.cpu())  # host inputs are moved to the volume's device
    assert int((vol.weights > 0).sum()) == 106


# ---------------------------------------------------------------- end to end ----------------------------------------------
def _eval_model():
    from test_gpu_kernels import _hip_model, small_cfg

    cfg = small_cfg(12, 10, 5)
    model = _hip_model(cfg, orc.init_params(cfg, seed=3, table_std=0.4), training=True)
    model.config.eval_num_rays_per_chunk = 512
    return model


def test_fuse_views_equals_integrating_the_rendered_frames(F):
    """fuse_views over three perspective cameras of 16 x 12 at downscale_factor=2 == integrating the frames render_camera returns
    for the scaled cameras, bit for bit (the frames are the same); the same frames through float64 under the module's rule, e_ref
    from the fp32 torch-op restatement on this GPU."""
    from nerfstudio_amd import eval_render
    from nerfstudio_amd.export import TSDFVolume, fuse_views, scaled_pinhole_cameras

    model = _eval_model()
    positions = ((1.9, 0.4, 0.5), (-0.5, 1.8, 0.7), (0.4, -0.7, 1.9))
    n = len(positions)
    col = lambda v, dt=torch.float32: torch.full((n, 1), v, dtype=dt)  # noqa: E731
    cams = types.SimpleNamespace(camera_to_worlds=torch.stack([T(tr.look_at(p).astype(np.float32))[:3] for p in positions]),
                                 fx=col(17.0), fy=col(16.5), cx=col(8.37), cy=col(5.79), height=col(12, torch.int64),
                                 width=col(16, torch.int64), camera_type=col(1, torch.int64))
    before = {k: v.clone() for k, v in vars(cams).items()}
    # The seeded model is untrained and renders depths of 60 - 75 (printed below). A box that large — truncation 77 — makes the
    # voxels' distances straddle them, so values strictly between -1 and 1 are compared too; the cameras then stand inside the
    # volume, voxels behind them included.
    aabb, dims = [[-90.0, -80, -70], [95, 85, 100]], (12, 12, 12)
    fused = TSDFVolume.from_aabb(aabb, dims, device="cuda")
    assert fuse_views(model, cams, fused, downscale_factor=2, views_per_launch=2) == 2  # launches of 2 and 1 views
    assert model.training and all(torch.equal(getattr(cams, k), v) for k, v in before.items())

    views = scaled_pinhole_cameras(cams, 2)
    assert [(v[5], v[6]) for v in views] == [(6, 8)] * n
    model.eval()
    runner = eval_render.runner_for(model, torch.device("cuda"))
    frames = [runner.render_camera(*v, lens=None) for v in views]
    depth = torch.stack([f["depth"] for f in frames]).permute(0, 3, 1, 2).contiguous()  # [B,1,H,W], the reference's layout
    color = torch.stack([f["rgb"] for f in frames]).permute(0, 3, 1, 2).contiguous()
    c2w = torch.cat([cams.camera_to_worlds, torch.tensor([0.0, 0, 0, 1]).expand(n, 1, 4)], 1).cuda()
    K = torch.tensor([[[v[1], 0.0, v[3]], [0.0, v[2], v[4]], [0.0, 0.0, 1.0]] for v in views]).cuda()
    direct = TSDFVolume.from_aabb(aabb, dims, device="cuda")
    direct.integrate(c2w, K, depth, color)
    for k in KEYS:
        assert torch.equal(getattr(fused, k), getattr(direct, k)), k

    host = TSDFVolume.from_aabb(aabb, dims)
    f64 = tr.integrate_f64(host.origin.numpy(), host.voxel_size.numpy(), host.truncation, host.values.numpy(), host.weights.numpy(),
                           host.colors.numpy(), c2w.cpu().numpy(), K.cpu().numpy(), depth.cpu().numpy(), color.cpu().numpy())
    eager = TSDFVolume.from_aabb(aabb, dims, device="cuda")
    tr.integrate_torch(eager.origin, eager.voxel_size, eager.truncation, eager.values, eager.weights, eager.colors, c2w, K, depth,
                       color)
    safe = tr.safe_voxels(f64)
    e_values = tr.distance(eager.values.cpu().numpy(), f64, "values", safe)
    e_colors = tr.distance(eager.colors.cpu().numpy(), f64, "colors", safe)
    inner = (f64["values"] > -1) & (f64["values"] < 1) & f64["touched"]
    print(f"tsdf gpu end to end: depth {float(depth.min()):.3f} .. {float(depth.max()):.3f}, touched {int(f64['touched'].sum())}, "
          f"{int(inner.sum())} of them strictly inside (-1, 1), from behind {int(f64['behind'].sum())}")
    assert int(f64["touched"].sum()) > 100 and int(inner.sum()) > 50
    tr.check(state_of(fused), f64, e_values, e_colors, ref=state_of(eager), label="gpu end to end")
