"""The instant-ngp eval render on the device (include/nsamd_render.h, nerfstudio_amd/ngp_eval_render.py).

* nsamd_packed_render_fwd BIT FOR BIT against nsamd_packed_weights_fwd -> nsamd_packed_composite_fwd over every geometry of
  tests/test_gpu_packed_float64.py (counts 0, 1, 63 / 64 / 65 ... 4097, empty first and last rays, no rays), eval_mode 0 / 1, both
  background modes, NaN and Inf colours on some samples: that file holds the two-launch route to float64 entry by entry, so
  equality carries its bounds. mid_lo / mid_hi bit for bit against numpy fp32 (ts + te) / 2 per ray, +-inf on empty rays.
* nsamd_packed_ray_points: positions bit for bit nsamd_packed_positions, directions bit for bit the gather; 0, 5, 4097 samples.
* NgpEvalRenderer on a small model (hash size 2^14, grid 16^3 x 2 levels, a blob of occupied cells, a 40 x 33 frame, chunk 256)
  against the module path — sample counts exactly, rgb / accumulation atol 2e-6, depth rtol 1e-5 / atol 1e-6, the tolerances
  tests/test_gpu_packed.py holds between the explicit training schedule and the module path (the two routes differ by the
  rounding of the positions) — and bit for bit against itself: prefetch on / off, bundle / render_camera, run / re-run, capacity
  64 / ample, chunk 256 / 1000 (but `depth`: the clip is per chunk).
* export.fuse_views on an instant-ngp model == integrating the frames render_camera returns.
Every output buffer of a direct launch is NaN / sentinel-filled first.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from oracle import nerfacto_oracle as orc
from test_gpu_packed_float64 import BG, GEOMETRIES, _dev, _nan, _p, composite_inputs, geometry_counts, info_from_counts, samples_case

pytestmark = pytest.mark.gpu
H, W, CHUNK = 33, 40, 256
KEYS = ("rgb", "accumulation", "depth", "num_samples_per_ray")


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


def _n():
    from nerfstudio_amd import _native as N

    return N


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- the two kernels ------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_packed_render_equals_weights_then_composite_bit_for_bit(F, geometry):
    N = _n()
    lib, st = N.load(), N.stream()
    counts = geometry_counts(geometry)
    info = info_from_counts(counts)
    nr = len(counts)
    seed = 60 + nr
    ts, te, sig = samples_case(counts, seed)
    ts2, te2, _, rgb, _, _ = composite_inputs(counts, seed, "random")  # colours in [-0.5, 1.5]: the eval clamp acts at both ends
    assert np.array_equal(ts, ts2) and np.array_equal(te, te2)
    n = len(ts)
    bad = rgb.copy()
    bad[::11] = np.nan
    bad[5::13, 1] = np.inf
    bad[7::17, 2] = -np.inf
    sig_hot = sig.copy()
    sig_hot[::3] *= 200.0  # rays whose transmittance underflows on the way: no early exit, 0 * NaN stays NaN without eval_mode
    info_d, tsd, ted = _dev(info), _dev(ts), _dev(te)
    bgv = (C.c_float * 3)(*BG)
    mid = ((ts + te).astype(np.float32) / np.float32(2.0)).astype(np.float32)
    lo_ref = np.array([mid[s:s + c].min() if c else np.inf for s, c in info], np.float32).reshape(-1)
    hi_ref = np.array([mid[s:s + c].max() if c else -np.inf for s, c in info], np.float32).reshape(-1)
    nan_rays = 0
    for colours, sigmas in ((rgb, sig), (bad, sig), (bad, sig_hot)):
        cd, sgd = _dev(colours), _dev(sigmas)
        for eval_mode in (0, 1):
            for bg_mode in (0, 1):
                bg = bgv if bg_mode else None
                w = _nan(n)
                N.check(lib.nsamd_packed_weights_fwd(_p(tsd), _p(ted), _p(sgd), _p(info_d), nr, _p(w), None, st), "weights_fwd")
                r_rgb, r_acc, r_dep = _nan(nr, 3), _nan(nr), _nan(nr)
                N.check(lib.nsamd_packed_composite_fwd(_p(cd), _p(w), _p(tsd), _p(ted), _p(info_d), nr, bg_mode, bg, eval_mode,
                                                       _p(r_rgb), _p(r_acc), _p(r_dep), st), "composite_fwd")
                o_rgb, o_acc, o_dep, lo, hi = _nan(nr, 3), _nan(nr), _nan(nr), _nan(nr), _nan(nr)
                N.check(lib.nsamd_packed_render_fwd(_p(tsd), _p(ted), _p(sgd), _p(cd), _p(info_d), nr, bg_mode, bg, eval_mode,
                                                    _p(o_rgb), _p(o_acc), _p(o_dep), _p(lo), _p(hi), st), "render_fwd")
                p_rgb, p_acc, p_dep = _nan(nr, 3), _nan(nr), _nan(nr)  # without the midpoint range: the same three outputs
                N.check(lib.nsamd_packed_render_fwd(_p(tsd), _p(ted), _p(sgd), _p(cd), _p(info_d), nr, bg_mode, bg, eval_mode,
                                                    _p(p_rgb), _p(p_acc), _p(p_dep), None, None, st), "render_fwd")
                torch.cuda.synchronize()
                tag = f"{geometry} eval{eval_mode} bg{bg_mode}"
                for name, got, plain, ref in (("rgb", o_rgb, p_rgb, r_rgb), ("acc", o_acc, p_acc, r_acc), ("depth", o_dep, p_dep, r_dep)):
                    assert torch.equal(_bits(got), _bits(ref)), f"{tag} {name}: {int((_bits(got) != _bits(ref)).sum())} entries differ"
                    assert torch.equal(_bits(plain), _bits(ref)), f"{tag} {name} (no midpoint range)"
                assert not bool(torch.isnan(r_acc).any()) and not bool(torch.isnan(r_dep).any())  # (written, and finite inputs)
                if eval_mode:
                    assert not bool(torch.isnan(o_rgb).any())
                elif colours is bad:
                    nan_rays += int(torch.isnan(o_rgb).any(dim=1).sum())
                np.testing.assert_array_equal(lo.cpu().numpy(), lo_ref)
                np.testing.assert_array_equal(hi.cpu().numpy(), hi_ref)
    if n >= 100:
        assert nan_rays > 0  # the NaN colours were seen where nothing removes them


@pytest.mark.parametrize("n", [0, 5, 4097])
def test_packed_ray_points_equals_positions_and_gather(F, n):
    N = _n()
    lib, st = N.load(), N.stream()
    rs = np.random.RandomState(90 + n)
    nr = 37
    o, d = rs.standard_normal((nr, 3)).astype(np.float32), rs.standard_normal((nr, 3)).astype(np.float32)
    ri = np.sort(rs.randint(0, nr, n)).astype(np.int64)
    ts = rs.uniform(0.05, 6.0, n).astype(np.float32)
    te = (ts + rs.uniform(0.005, 0.05, n)).astype(np.float32)
    od, dd, rid, tsd, ted = _dev(o), _dev(d), _dev(ri), _dev(ts), _dev(te)
    ref, pos, dirs = _nan(n, 3), _nan(n, 3), _nan(n, 3)
    N.check(lib.nsamd_packed_positions(_p(od), _p(dd), _p(rid), _p(tsd), _p(ted), n, _p(ref), st), "packed_positions")
    N.check(lib.nsamd_packed_ray_points(_p(od), _p(dd), _p(rid), _p(tsd), _p(ted), n, _p(pos), _p(dirs), st), "packed_ray_points")
    torch.cuda.synchronize()
    assert torch.equal(_bits(pos), _bits(ref)) and not bool(torch.isnan(pos).any())
    np.testing.assert_array_equal(dirs.cpu().numpy(), d[ri])
    # ... and through the launch helper, into buffers larger than the count (only the first n rows are written)
    pos2, dirs2 = _nan(n + 3, 3), _nan(n + 3, 3)
    F.packed_ray_points_launch(od, dd, _dev(np.concatenate([ri, [0, 0, 0]])), _dev(np.concatenate([ts, [1, 1, 1]]).astype(np.float32)),
                               _dev(np.concatenate([te, [1, 1, 1]]).astype(np.float32)), n, pos2, dirs2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(pos2[:n]), _bits(ref)) and bool(torch.isnan(pos2[n:]).all()) and bool(torch.isnan(dirs2[n:]).all())


# ---------------------------------------------------------------- the runner ------------------------------------------------
C2W = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.05], [0.0, 0.0, 1.0, 1.7]])
VIEW = (45.0, 45.0, W / 2.0 + 0.25, H / 2.0 - 0.5)


def _model(background="white", blob=True):
    from nerfstudio_amd.instant_ngp import InstantNGPModelConfig, NGPModel

    ocfg = orc.NerfactoCfg(main_grid=orc.HashGridCfg(16, 16, 2048, 14), prop_grids=(), num_images=4, average_init_density=1.0)
    params = orc.init_params(ocfg, seed=45, table_std=0.5)
    mc = InstantNGPModelConfig(grid_resolution=16, grid_levels=2, log2_hashmap_size=14, background_color=background, cone_angle=0.004,
                               render_step_size=0.02, eval_num_rays_per_chunk=CHUNK)
    model = NGPModel(mc, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4)
    missing, unexpected = model.load_state_dict({k: v.clone() for k, v in params.items() if k.startswith("field.")}, strict=False)
    assert not unexpected, unexpected
    with torch.no_grad():  # (the oracle's initialisation has no embedding rows of its own for this model)
        model.field.embedding_appearance.embedding.weight.copy_(
            torch.from_numpy(np.random.RandomState(5).standard_normal((4, 32)).astype(np.float32)) * 0.3)
    model = model.cuda().eval()
    if blob:  # a blob of occupied cells off the centre, and one of the coarse level between it and the camera
        g = torch.stack(torch.meshgrid(*[torch.arange(16.0)] * 3, indexing="ij"), dim=-1)
        model.occupancy_grid.binaries[0] = ((g - torch.tensor([9.0, 7.0, 8.0])).norm(dim=-1) < 4.5).to(torch.uint8).cuda()
        model.occupancy_grid.binaries[1] = ((g - torch.tensor([10.0, 8.0, 13.0])).norm(dim=-1) < 1.6).to(torch.uint8).cuda()
    return model


def _frame(F, with_bounds=False):
    """The bundle `generate_rays(camera_indices=0, keep_shape=True)` gives for the camera of C2W / VIEW (nsamd_raygen_pinhole, which
    tests/golden pins to the reference's own generate_rays)."""
    from nerfstudio_amd.cameras.rays import RayBundle

    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    idx = torch.stack([torch.zeros_like(yy), yy, xx], dim=-1).reshape(-1, 3).cuda()
    one = lambda v: torch.tensor([v]).cuda()  # noqa: E731
    o, d, pa, _ = F.raygen_pinhole(idx, C2W[None].cuda(), *(one(v) for v in VIEW))
    kw = {}
    if with_bounds:
        g = torch.Generator().manual_seed(3)
        kw["nears"] = (0.9 + 0.5 * torch.rand(H, W, 1, generator=g)).cuda()
        kw["fars"] = kw["nears"] + (0.3 + 0.8 * torch.rand(H, W, 1, generator=g)).cuda()
    return RayBundle(origins=o.view(H, W, 3), directions=d.view(H, W, 3), pixel_area=pa.view(H, W, 1),
                     camera_indices=torch.zeros(H, W, 1, dtype=torch.long).cuda(), **kw)


def _module_path(model, frame, monkeypatch):
    monkeypatch.setenv("NSAMD_EVAL_RUNNER", "0")
    try:
        return model.get_outputs_for_camera_ray_bundle(frame)
    finally:
        monkeypatch.delenv("NSAMD_EVAL_RUNNER")


def _close_to_module_path(out, ref):
    assert torch.equal(out["num_samples_per_ray"], ref["num_samples_per_ray"].view_as(out["num_samples_per_ray"]))
    np.testing.assert_allclose(out["rgb"].cpu().numpy(), ref["rgb"].cpu().numpy(), atol=2e-6)
    np.testing.assert_allclose(out["accumulation"].cpu().numpy(), ref["accumulation"].cpu().numpy(), atol=2e-6)
    np.testing.assert_allclose(out["depth"].cpu().numpy(), ref["depth"].cpu().numpy(), rtol=1e-5, atol=1e-6)


def _same_bits(a, b, keys=KEYS):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k], b[k]), f"{k}: {int((a[k] != b[k]).sum())} entries differ"


def test_runner_against_the_module_path_and_against_itself(F, monkeypatch):
    from nerfstudio_amd.ngp_eval_render import NgpEvalRenderer

    model = _model()
    frame = _frame(F)
    ref = _module_path(model, frame, monkeypatch)
    runner = NgpEvalRenderer(model)
    out = runner.render(frame)
    assert out["rgb"].shape == (H, W, 3) and out["num_samples_per_ray"].shape == (H, W, 1) and out["num_samples_per_ray"].dtype == torch.int64
    per_chunk = [int(c.sum()) for c in out["num_samples_per_ray"].reshape(-1).split(CHUNK)]
    assert len(per_chunk) == 6 and min(per_chunk) > 0 and float(out["accumulation"].max()) > 0.0  # the frame sees the blob
    assert int((out["num_samples_per_ray"] == 0).sum()) > 0  # ... and rays that see nothing
    _close_to_module_path(out, ref)
    _same_bits(runner.render(frame), out)                                         # run and re-run
    _same_bits(NgpEvalRenderer(model, prefetch=False).render(frame), out)          # read-then-launch, strictly in turn
    _same_bits(runner.render_camera(C2W.cuda(), *VIEW, H, W), out)                 # rays generated inside the chunk loop
    tiny = NgpEvalRenderer(model, cap_candidates=64)
    _same_bits(tiny.render(frame), out)
    assert tiny.cap_c >= max(per_chunk) > 64 and tiny.grown >= 1
    wide = NgpEvalRenderer(model, chunk=1000).render(frame)                        # another chunking: the clip range is per chunk
    _same_bits(wide, out, keys=("rgb", "accumulation", "num_samples_per_ray"))
    hit = out["accumulation"] > 0.1  # (a ray of little weight sits on its chunk's clip bound, which moves with the chunking)
    assert int(hit.sum()) > 0 and torch.equal(wide["depth"][hit], out["depth"][hit])
    # the model's own entry points take the runner (cached on the model) and give its bits
    _same_bits(model.get_outputs_for_camera_ray_bundle(frame), out)
    cam = types.SimpleNamespace(camera_to_worlds=C2W.cuda(), fx=torch.tensor([VIEW[0]]), fy=torch.tensor([VIEW[1]]),
                                cx=torch.tensor([VIEW[2]]), cy=torch.tensor([VIEW[3]]), height=torch.tensor([H]), width=torch.tensor([W]),
                                camera_type=torch.tensor([1]), distortion_params=None)
    _same_bits(model.get_outputs_for_camera(cam), out)
    assert model._ngp_eval_runner.chunk == CHUNK


@pytest.mark.parametrize("case", ["bounds", "random", "average_appearance"])
def test_runner_edge_cases_against_the_module_path(F, monkeypatch, case):
    """("white" without bounds and with the zero appearance row is the test above.)"""
    from nerfstudio_amd.ngp_eval_render import NgpEvalRenderer

    model = _model(background="random" if case == "random" else "white")
    if case == "average_appearance":
        model.field.use_average_appearance_embedding = True
    frame = _frame(F, with_bounds=case == "bounds")
    ref = _module_path(model, frame, monkeypatch)
    out = NgpEvalRenderer(model).render(frame)
    _close_to_module_path(out, ref)
    plain = NgpEvalRenderer(_model()).render(_frame(F))
    if case == "bounds":
        assert not torch.equal(plain["num_samples_per_ray"], out["num_samples_per_ray"])  # the interval matters on this frame
    else:
        assert torch.equal(plain["num_samples_per_ray"], out["num_samples_per_ray"]) and not torch.equal(plain["rgb"], out["rgb"])


@pytest.mark.parametrize("background", ["white", "random"])
def test_runner_all_empty_grid(F, monkeypatch, background):
    """No candidate in any chunk: the reference's fake sample (ray 0, [1, 1]) — num_samples_per_ray 1 on each chunk's first ray,
    depth 1, rgb = the background — and the module path gives the same."""
    from nerfstudio_amd.ngp_eval_render import NgpEvalRenderer

    model = _model(background=background, blob=False)
    frame = _frame(F)
    out = NgpEvalRenderer(model).render(frame)
    expect = torch.zeros(H * W, dtype=torch.int64)
    expect[::CHUNK] = 1
    assert torch.equal(out["num_samples_per_ray"].reshape(-1).cpu(), expect)
    assert torch.equal(out["depth"].cpu(), torch.ones(H, W, 1))
    assert torch.equal(out["accumulation"].cpu(), torch.zeros(H, W, 1))
    assert torch.equal(out["rgb"].cpu(), torch.full((H, W, 3), 1.0 if background == "white" else 0.0))
    ref = _module_path(model, frame, monkeypatch)
    _same_bits(out, {k: ref[k].view_as(out[k]) for k in KEYS})


def test_fuse_views_on_an_ngp_model_equals_integrating_its_frames(F):
    from nerfstudio_amd import export, ngp_eval_render

    model = _model()
    poses = C2W[None].repeat(3, 1, 1)
    poses[:, 0, 3] = torch.tensor([0.1, -0.2, 0.3])
    cams = types.SimpleNamespace(camera_to_worlds=poses, fx=torch.full((3, 1), 2 * VIEW[0]), fy=torch.full((3, 1), 2 * VIEW[1]),
                                 cx=torch.full((3, 1), 2 * VIEW[2]), cy=torch.full((3, 1), 2 * VIEW[3]), height=torch.full((3, 1), 2 * H),
                                 width=torch.full((3, 1), 2 * W), camera_type=torch.ones(3, 1))
    box = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    fused = export.TSDFVolume.from_aabb(box, [12, 10, 8], device="cuda")
    assert export.fuse_views(model, cams, fused, downscale_factor=2, views_per_launch=2) == 2
    runner = ngp_eval_render.runner_for(model, "cuda")
    assert runner is model._ngp_eval_runner
    by_hand = export.TSDFVolume.from_aabb(box, [12, 10, 8], device="cuda")
    K = torch.tensor([[VIEW[0], 0.0, VIEW[2]], [0.0, VIEW[1], VIEW[3]], [0.0, 0.0, 1.0]])
    frames = [runner.render_camera(poses[i].cuda(), *VIEW, H, W) for i in range(3)]
    for a, b in ((0, 2), (2, 3)):
        by_hand.integrate(poses[a:b].cuda(), K[None].repeat(b - a, 1, 1), torch.stack([f["depth"][..., 0] for f in frames[a:b]]),
                          torch.stack([f["rgb"] for f in frames[a:b]]))
    torch.cuda.synchronize()
    assert bool((fused.weights > 0).any())
    for name in ("values", "weights", "colors"):
        assert torch.equal(getattr(fused, name), getattr(by_hand, name)), name
