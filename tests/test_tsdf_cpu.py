"""CPU tests of mesh export (nerfstudio_amd/export.py over nsamd_tsdf_integrate): the float64 restatement against the fixture the
reference wrote, the per-voxel arithmetic of nerfstudio_amd/csrc/tsdf.h compiled for the host (tests/hostcheck/tsdf_helpers.cc)
and looped over the voxels as the kernel composes it, and every layer above the kernel — TSDFVolume, fuse_views,
export_tsdf_mesh, the entry point's validation — with the launch replaced by the host build or by the float64 restatement.

Fixture: tests/golden/tsdf.npz, written by the reference's own TSDF class (tests/golden/make_golden_tsdf.py). The cases, the
margins that make a voxel unsafe and the bounds are in tests/tsdf_reference.py: weights exact on safe voxels, values and colours
within MARGIN = 4 times the reference's own fp32 distance from float64 on the same case (measured when the fixture was written:
case A 4.4e-07 / 5.2e-08, case B 5.3e-08 / 0 — one view, the colour is copied —, case C 5.7e-07 / 4.5e-08).
"""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import tsdf_reference as tr

F32P = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
T = torch.from_numpy


@pytest.fixture(scope="module")
def g():
    return load_golden("tsdf")


def reference_state(g, name, tag):
    return {k: g[f"{name}_{tag}_{k}"] for k in ("values", "weights", "colors")}


def f64_of(g, name, start=None, color=True):
    inp = tr.case_inputs(g, name)
    origin, voxel_size, truncation = tr.volume_geometry(inp["aabb"], inp["dims"])
    v, w, c = tr.initial_state(inp["dims"]) if start is None else (start["values"], start["weights"], start["colors"])
    return tr.integrate_f64(origin, voxel_size, truncation, v, w, c, inp["c2w"], inp["K"], inp["depth"],
                            inp["color"] if color else None)


def bounds(g, name):
    return float(g[f"e_ref_values_{name}"]), float(g[f"e_ref_colors_{name}"])


# ---------------------------------------------------------------- fixture and float64 ---------------------------------
@pytest.mark.parametrize("name", tr.CASES)
def test_fixture_holds_the_cases_and_the_restatement_reproduces_the_reference(g, name):
    inp = tr.case_inputs(g, name)
    again = tr.make_case(name)  # the generator's inputs are reproducible
    for k, v in again.items():
        np.testing.assert_array_equal(v, inp[k])
    first = f64_of(g, name)
    safe = tr.safe_voxels(first)
    assert 1.0 - safe.mean() <= tr.UNSAFE_CAP  # the cap, for the reference alone
    e_values, e_colors = bounds(g, name)
    batch = reference_state(g, name, "batch")
    second = f64_of(g, name, start=batch)
    assert np.array_equal(tr.safe_voxels(second), safe)
    for tag, f64 in (("batch", first), ("twice", second), ("seq", first)):
        ref = reference_state(g, name, tag)
        assert np.array_equal(ref["weights"][safe].astype(np.float64), f64["weights"][safe])
        assert tr.distance(ref["values"], f64, "values", safe) <= e_values
        assert tr.distance(ref["colors"], f64, "colors", safe) <= e_colors
        assert not np.isnan(ref["values"]).any() and ref["weights"].max() <= 1.0
    plain, nocolor = f64_of(g, name, color=False), reference_state(g, name, "nocolor")
    assert np.array_equal(plain["values"], first["values"]) and not plain["colors"].any() and not nocolor["colors"].any()
    assert tr.distance(nocolor["values"], plain, "values", safe) <= e_values
    touched = batch["weights"] > 0
    assert list(g[f"{name}_counts"]) == [safe.size, touched.sum(), (first["behind"] & touched).sum(), (~safe).sum()]
    assert np.array_equal(first["touched"][safe], touched[safe])
    _, _, truncation = tr.volume_geometry(inp["aabb"], inp["dims"])
    assert truncation == float(g[f"{name}_truncation"]) == float(g[f"{name}_voxel_size"][0]) * 5.0  # the x size alone


def test_fixture_cases_cover_what_they_are_for(g):
    assert list(g["A_counts"][:3]) == [990, 465, 18] and g["A_counts"][0] % 256 != 0
    # B: the 64 voxels on the camera's plane stay untouched without a NaN; 12 touched voxels lie behind the camera; a second pass
    # leaves the values bit-identical (the mean of a value with itself) and the weights at 1
    assert list(g["B_counts"]) == [512, 106, 12, 0]
    plane = g["B_voxel_coords"][2] == 0.25
    assert plane.sum() == 64 and not g["B_batch_weights"][plane].any() and (g["B_batch_values"][plane] == -1).all()
    assert np.array_equal(g["B_twice_values"], g["B_batch_values"]) and g["B_twice_weights"].max() == 1.0
    vs = g["C_voxel_size"]
    assert len({float(v) for v in vs}) == 3 and float(g["C_truncation"]) == float(vs[0]) * 5.0
    for name in tr.CASES:  # the reference itself: views one at a time are the batch, bit for bit
        for k in ("values", "weights", "colors"):
            assert np.array_equal(g[f"{name}_seq_{k}"], g[f"{name}_batch_{k}"])
        assert np.array_equal(g[f"{name}_nocolor_values"], g[f"{name}_batch_values"])


# ---------------------------------------------------------------- tsdf.h on the host -------------------------------------
@pytest.fixture(scope="module")
def host_launch(tmp_path_factory):
    """functional.tsdf_integrate_launch's arguments served by the host build of csrc/tsdf.h; `.stores`: voxels written back."""
    from nerfstudio_amd import _native as N

    out = str(tmp_path_factory.mktemp("hostcheck") / "libtsdfcheck.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "tsdf_helpers.cc")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.hc_tsdf_integrate.argtypes = [N.TsdfVolume] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                                       C.POINTER(C.c_int64)]

    def launch(origin, voxel_size, truncation, values, weights, colors, w2c, K, depth, color):
        vol = N.TsdfVolume()
        for i in range(3):
            vol.origin[i], vol.voxel_size[i], vol.dims[i] = origin[i], voxel_size[i], values.shape[i]
        vol.truncation = truncation
        for t in (values, weights, colors, w2c, K, depth, color):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.device.type == "cpu")
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        stores = C.c_int64(-1)
        status = lib.hc_tsdf_integrate(vol, ptr(values), ptr(weights), ptr(colors), ptr(w2c), ptr(K), w2c.shape[0], ptr(depth),
                                       ptr(color), depth.shape[1], depth.shape[2], C.byref(stores))
        assert status == 0, status
        launch.stores = stores.value

    return launch


def new_volume(g, name):
    from nerfstudio_amd.export import TSDFVolume

    return TSDFVolume.from_aabb(T(g[f"{name}_aabb"]), T(g[f"{name}_dims"]))


def state_of(volume):
    return {k: getattr(volume, k).numpy().copy() for k in ("values", "weights", "colors")}


def case_tensors(g, name):
    return tuple(T(g[f"{name}_{k}"]) for k in ("c2w", "K", "depth", "color"))


@pytest.mark.parametrize("name", tr.CASES)
def test_header_arithmetic_reproduces_the_reference_and_float64(g, host_launch, name):
    c2w, K, depth, color = case_tensors(g, name)
    vol = new_volume(g, name)
    vol.integrate(c2w, K, depth, color, launch_fn=host_launch)
    e_values, e_colors = bounds(g, name)
    first = f64_of(g, name)
    tr.check(state_of(vol), first, e_values, e_colors, ref=reference_state(g, name, "batch"), label=f"host {name} batch")
    assert host_launch.stores == int(first["touched"].sum()) or not tr.safe_voxels(first).all()
    start = state_of(vol)
    vol.integrate(c2w, K, depth, color, launch_fn=host_launch)
    tr.check(state_of(vol), f64_of(g, name, start=start), e_values, e_colors, label=f"host {name} twice")
    if name == "B":
        plane = g["B_voxel_coords"][2] == 0.25
        assert not vol.weights.numpy()[plane].any() and np.array_equal(vol.values.numpy(), start["values"])
        assert np.array_equal(start["colors"], g["B_batch_colors"])  # one view: the colour is the pixel's, exactly


@pytest.mark.parametrize("name", tr.CASES)
def test_views_one_at_a_time_equal_the_batch_bit_for_bit_and_colours_may_be_absent(g, host_launch, name):
    c2w, K, depth, color = case_tensors(g, name)
    batch, seq, plain = new_volume(g, name), new_volume(g, name), new_volume(g, name)
    batch.integrate(c2w, K, depth, color, launch_fn=host_launch)
    for b in range(c2w.shape[0]):
        seq.integrate(c2w[b:b + 1], K[b:b + 1], depth[b:b + 1], color[b:b + 1], launch_fn=host_launch)
    for k in ("values", "weights", "colors"):
        assert torch.equal(getattr(seq, k), getattr(batch, k)), k
    plain.colors.fill_(0.25)
    plain.integrate(c2w, K, depth, launch_fn=host_launch)
    assert torch.equal(plain.values, batch.values) and torch.equal(plain.weights, batch.weights)
    assert (plain.colors == 0.25).all()  # untouched


# ---------------------------------------------------------------- TSDFVolume ----------------------------------------------
@pytest.mark.parametrize("name", tr.CASES)
def test_from_aabb_starts_where_the_reference_starts(g, name):
    vol = new_volume(g, name)
    for k in ("values", "weights", "colors"):
        np.testing.assert_array_equal(getattr(vol, k).numpy(), g[f"{name}_{k}0"])
    np.testing.assert_array_equal(vol.origin.numpy(), g[f"{name}_origin"])
    np.testing.assert_array_equal(vol.voxel_size.numpy(), g[f"{name}_voxel_size"])
    np.testing.assert_array_equal(vol.voxel_coords().numpy(), g[f"{name}_voxel_coords"])
    assert vol.truncation == float(g[f"{name}_truncation"]) and vol.truncation_margin == 5.0
    listed = type(vol).from_aabb(g[f"{name}_aabb"].tolist(), [int(d) for d in g[f"{name}_dims"]], device="cpu")
    assert torch.equal(listed.voxel_size, vol.voxel_size) and listed.values.shape == vol.values.shape


def test_every_accepted_layout_reaches_the_launch_as_the_same_dense_tensors(g):
    c2w, K, depth, color = case_tensors(g, "A")
    calls = []
    launch = tr.fake_launch(calls)
    layouts = [(c2w, K, depth, color), (c2w[:, :3], K, depth[:, 0], color.permute(0, 2, 3, 1).contiguous()),
               (c2w.double(), K.double(), depth.permute(0, 2, 3, 1), color.permute(0, 2, 3, 1)),
               (c2w, K * torch.tensor([[1.0], [1.0], [7.0]]), depth.expand(-1, 1, -1, -1), color)]  # K's third row is ignored
    results = []
    for args in layouts:
        vol = new_volume(g, "A")
        vol.integrate(*args, launch_fn=launch)
        results.append(state_of(vol))
    first = calls[0]
    assert first["w2c"].shape == (4, 3, 4) and first["K"].shape == (4, 2, 3) and first["depth"].shape == (4, 24, 32)
    assert first["color"].shape == (4, 24, 32, 3) and first["origin"] == [-1.0, -1.0, -1.0]
    assert first["truncation"] == float(g["A_truncation"])
    assert torch.equal(first["w2c"], torch.inverse(c2w)[:, :3]) and torch.equal(first["K"], K[:, :2])
    assert torch.equal(first["color"], color.permute(0, 2, 3, 1))
    for call in calls[1:]:
        for k in ("w2c", "K", "depth", "color"):
            assert call[k].dtype == torch.float32 and call[k].is_contiguous() and torch.equal(call[k], first[k]), k
    for r in results[1:]:
        for k in r:
            assert np.array_equal(r[k], results[0][k])
    tr.check(results[0], f64_of(g, "A"), *bounds(g, "A"), ref=reference_state(g, "A", "batch"), label="fake launch A")
    vol = new_volume(g, "A")
    vol.integrate(c2w, K, depth, launch_fn=launch)
    assert calls[-1]["color"] is None and not vol.colors.any()
    with pytest.raises(NotImplementedError, match="Mask images"):
        vol.integrate(c2w, K, depth, color, mask_images=torch.ones(4, 1, 24, 32, dtype=torch.bool), launch_fn=launch)
    for bad in ((c2w[:, :2], K, depth, color), (c2w, K[:, :2], depth, color), (c2w, K, depth[:2], color),
                (c2w, K, depth, color[:, :2])):
        with pytest.raises(ValueError):
            vol.integrate(*bad, launch_fn=launch)


def test_native_launch_refuses_host_tensors_and_meshing_needs_the_reference(g, monkeypatch):
    vol = new_volume(g, "B")
    before = state_of(vol)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.integrate(*case_tensors(g, "B"))
    for k, v in before.items():
        assert np.array_equal(getattr(vol, k).numpy(), v)
    monkeypatch.setitem(sys.modules, "nerfstudio.exporter", None)
    with pytest.raises(ImportError, match="nerfstudio"):
        vol.to_reference()
    text = open(os.path.join(ROOT, "nerfstudio_amd", "export.py")).read()
    assert not re.findall(r"^(?:import|from)\s+nerfstudio\b", text, re.M)  # nothing of nerfstudio at module level


def test_to_reference_hands_the_same_tensors_to_the_references_class(g, monkeypatch):
    seen = {}

    class TSDF:
        def __init__(self, voxel_coords, values, weights, colors, voxel_size, origin, truncation_margin=5.0):
            seen.update(locals())

    monkeypatch.setitem(sys.modules, "nerfstudio", types.ModuleType("nerfstudio"))
    monkeypatch.setitem(sys.modules, "nerfstudio.exporter", types.ModuleType("nerfstudio.exporter"))
    mod = types.ModuleType("nerfstudio.exporter.tsdf_utils")
    mod.TSDF = TSDF
    monkeypatch.setitem(sys.modules, "nerfstudio.exporter.tsdf_utils", mod)
    sys.modules["nerfstudio.exporter"].tsdf_utils = mod
    vol = new_volume(g, "C")
    assert isinstance(vol.to_reference(), TSDF)
    assert seen["values"] is vol.values and seen["weights"] is vol.weights and seen["colors"] is vol.colors
    np.testing.assert_array_equal(seen["voxel_coords"].numpy(), g["C_voxel_coords"])
    assert torch.equal(seen["origin"], vol.origin) and torch.equal(seen["voxel_size"], vol.voxel_size)


# ---------------------------------------------------------------- fuse_views ----------------------------------------------
class _Model(torch.nn.Module):
    config = types.SimpleNamespace()


def cameras_of(g, n=None, camera_type=1):
    n = g["rescale_fx"].shape[0] if n is None else n
    c2w = torch.stack([T(tr.look_at((2.0 + 0.1 * i, 0.3 * i, 0.5)).astype(np.float32))[:3] for i in range(n)])
    return types.SimpleNamespace(camera_to_worlds=c2w, camera_type=torch.full((n, 1), camera_type),
                                 **{k: T(g[f"rescale_{k}"][:n].copy()) for k in ("fx", "fy", "cx", "cy", "height", "width")})


def stub_render(calls, names=("depth", "rgb"), fail_at=None):
    def render(c2w, fx, fy, cx, cy, H, W):
        if fail_at is not None and len(calls) == fail_at:
            raise RuntimeError("render failed")
        calls.append((c2w, fx, fy, cx, cy, H, W))
        i = len(calls)
        out = {"depth": torch.full((H, W, 1), 1.0 + i), "rgb": torch.full((H, W, 3), i / 16.0), "accumulation": torch.ones(H, W, 1)}
        return {k: out[k] for k in names + ("accumulation",)}

    return render


def recording_volume(dims=(4, 4, 4), launch=None):
    """A small volume whose `integrate` goes to the float64 stand-in, which records its arguments in `.calls` (or to `launch`)."""
    from nerfstudio_amd.export import TSDFVolume

    vol = TSDFVolume.from_aabb([[-1.0, -1, -1], [1, 1, 1]], dims)
    vol.calls = []
    launch = tr.fake_launch(vol.calls) if launch is None else launch
    integrate = vol.integrate
    vol.integrate = lambda *a, **kw: integrate(*a, launch_fn=launch, **kw)
    return vol


@pytest.mark.parametrize("factor", [2, 3])
def test_fuse_views_scales_like_the_reference_without_touching_the_cameras(g, factor):
    from nerfstudio_amd.export import fuse_views

    cams = cameras_of(g)
    before = {k: v.clone() for k, v in vars(cams).items()}
    calls, vol = [], recording_volume()
    model = _Model().train()
    launches = fuse_views(model, cams, vol, downscale_factor=factor, views_per_launch=2, render_fn=stub_render(calls))
    n = len(calls)
    assert n == 5 and model.training
    for k, col in (("fx", 1), ("fy", 2), ("cx", 3), ("cy", 4), ("height", 5), ("width", 6)):
        want = g[f"rescale_f{factor}_{k}"].reshape(-1)
        got = np.array([c[col] for c in calls])
        np.testing.assert_array_equal(got.astype(want.dtype), want)  # the fp32 products, H and W truncated
        assert isinstance(calls[0][col], int if col > 4 else float)
    for k, v in before.items():  # the cameras object is only read
        assert torch.equal(getattr(cams, k), v) and getattr(cams, k).dtype == v.dtype
    # five cameras of five sizes: every size change flushes what the buffers hold
    assert launches == 5 and [c["depth"].shape[0] for c in vol.calls] == [1] * 5
    for i, call in enumerate(vol.calls):
        H, W = calls[i][5], calls[i][6]
        assert call["depth"].shape == (1, H, W) and call["color"].shape == (1, H, W, 3)
        assert (call["depth"] == 2.0 + i).all() and (call["color"] == (i + 1) / 16.0).all()
        want_K = torch.tensor([[calls[i][1], 0.0, calls[i][3]], [0.0, calls[i][2], calls[i][4]]])
        assert torch.equal(call["K"][0], want_K)
        assert torch.equal(call["w2c"][0], torch.inverse(torch.cat([cams.camera_to_worlds[i], torch.tensor([[0.0, 0, 0, 1]])]))[:3])


def same_size_cameras(g, n, sizes=None):
    cams = cameras_of(g, 1)
    rep = lambda t: t.repeat(n, 1)  # noqa: E731
    cams = types.SimpleNamespace(camera_to_worlds=torch.stack([T(tr.look_at((2.0, 0.2 * i, 0.4)).astype(np.float32))[:3]
                                                               for i in range(n)]),
                                 **{k: rep(getattr(cams, k)) for k in ("fx", "fy", "cx", "cy", "height", "width", "camera_type")})
    if sizes is not None:
        cams.height, cams.width = torch.tensor(sizes)[:, :1].clone(), torch.tensor(sizes)[:, 1:].clone()
    return cams


def test_fuse_views_batches_in_view_order_and_flushes_on_a_size_change(g, host_launch):
    from nerfstudio_amd.export import fuse_views

    calls, vol = [], recording_volume()
    cams = same_size_cameras(g, 7)
    assert fuse_views(_Model().eval(), cams, vol, downscale_factor=2, views_per_launch=3, render_fn=stub_render(calls)) == 3
    assert [c["depth"].shape[0] for c in vol.calls] == [3, 3, 1]
    order = torch.cat([c["depth"][:, 0, 0] for c in vol.calls])
    assert order.tolist() == [2.0 + i for i in range(7)]  # frames in view order
    w2c = torch.cat([c["w2c"] for c in vol.calls])
    hom = torch.cat([cams.camera_to_worlds, torch.tensor([0.0, 0, 0, 1]).expand(7, 1, 4)], 1)
    assert torch.equal(w2c, torch.inverse(hom)[:, :3])
    # a size change in the middle of a buffer: 2 views of 12 x 16, then 3 of 10 x 16 -> launches of 2 and 3
    calls, vol = [], recording_volume()
    cams = same_size_cameras(g, 5, sizes=[[24, 32]] * 2 + [[20, 32]] * 3)
    assert fuse_views(_Model().eval(), cams, vol, views_per_launch=4, render_fn=stub_render(calls)) == 2
    assert [tuple(c["depth"].shape) for c in vol.calls] == [(2, 12, 16), (3, 10, 16)]
    # the batches together are the views one by one (the header's arithmetic: the state is fp32 either way)
    one, batched = recording_volume(launch=host_launch), recording_volume(launch=host_launch)
    fuse_views(_Model().eval(), cams, one, views_per_launch=1, render_fn=stub_render([]))
    fuse_views(_Model().eval(), cams, batched, views_per_launch=4, render_fn=stub_render([]))
    assert (one.weights > 0).any() and torch.equal(one.values, batched.values) and torch.equal(one.colors, batched.colors)


def test_fuse_views_restores_the_mode_and_names_what_it_refuses(g):
    from nerfstudio_amd.export import fuse_views

    cams = same_size_cameras(g, 4)
    for training in (True, False):
        model = _Model().train(training)
        seen = []

        def render(*view, model=model, seen=seen):
            seen.append(model.training)
            return stub_render([])(*view)

        fuse_views(model, cams, recording_volume(), render_fn=render)
        assert seen == [False] * 4 and model.training is training  # rendered in eval mode, the previous mode restored
        with pytest.raises(RuntimeError, match="render failed"):
            fuse_views(model, cams, recording_volume(), render_fn=stub_render([], fail_at=2))
        assert model.training is training
    with pytest.raises(KeyError, match=r"'depth'.*accumulation.*rgb"):
        fuse_views(_Model(), cams, recording_volume(), render_fn=stub_render([], names=("rgb",)))
    with pytest.raises(KeyError, match="'colour'"):
        fuse_views(_Model(), cams, recording_volume(), rgb_output_name="colour", render_fn=stub_render([]))
    fisheye = cameras_of(g, 3)
    fisheye.camera_type[1] = 2
    calls = []
    with pytest.raises(ValueError, match="FISHEYE"):
        fuse_views(_Model(), fisheye, recording_volume(), render_fn=stub_render(calls))
    assert not calls
    ngp = _Model().train()  # no proposal networks: eval_render.supported gives a reason, and no render_fn was passed
    with pytest.raises(ValueError, match="not a nerfacto model"):
        fuse_views(ngp, cams, recording_volume())
    assert ngp.training
    with pytest.raises(ValueError, match="views_per_launch"):
        fuse_views(_Model(), cams, recording_volume(), views_per_launch=0, render_fn=stub_render([]))


# ---------------------------------------------------------------- export_tsdf_mesh ----------------------------------------
def test_export_tsdf_mesh_fuses_meshes_and_writes_with_a_refinement_pass(g, tmp_path, monkeypatch):
    import inspect

    from nerfstudio_amd import export

    monkeypatch.setattr(export.F, "tsdf_integrate_launch", tr.fake_launch())
    cams = same_size_cameras(g, 5)
    before = {k: v.clone() for k, v in vars(cams).items()}
    scene_box = types.SimpleNamespace(aabb=torch.tensor([[-2.0, -2, -2], [2, 2, 2]]))
    outputs = types.SimpleNamespace(cameras=cams, scene_box=scene_box)
    pipeline = types.SimpleNamespace(device="cpu", model=_Model().train(), datamanager=types.SimpleNamespace(
        train_dataset=types.SimpleNamespace(_dataparser_outputs=outputs)))
    volumes, written, calls = [], [], []

    def mesh_fn(volume):
        volumes.append(volume)
        return types.SimpleNamespace(vertices=torch.tensor([[-0.5, -0.25, 0.0], [0.5, 0.25, 0.125], [0.0, 0.0, -0.125]]))

    kw = dict(render_fn=stub_render(calls), mesh_fn=mesh_fn, write_fn=lambda mesh, filename: written.append((mesh, filename)))
    export.export_tsdf_mesh(pipeline, tmp_path, resolution=[6, 5, 4], batch_size=2, **kw)
    assert len(volumes) == 1 and len(calls) == 5 and written[0][1] == str(tmp_path / "tsdf_mesh.ply")
    vol = volumes[0]
    assert tuple(vol.values.shape) == (6, 5, 4) and vol.origin.tolist() == [-1.0, -1.0, -1.0] and (vol.weights > 0).any()
    assert torch.equal(vol.voxel_size, torch.tensor([2.0, 2.0, 2.0]) / torch.tensor([6, 5, 4]))
    export.export_tsdf_mesh(pipeline, tmp_path, resolution=4, use_bounding_box=False, refine_mesh_using_initial_aabb_estimate=True,
                            refinement_epsilon=0.5, **kw)
    assert len(volumes) == 3 and len(calls) == 15 and len(written) == 2  # the refinement renders and fuses again
    assert volumes[1].origin.tolist() == [-2.0, -2.0, -2.0] and tuple(volumes[1].values.shape) == (4, 4, 4)
    assert volumes[2].origin.tolist() == [-1.0, -0.75, -0.625]  # the mesh's bounds - epsilon
    assert torch.equal(volumes[2].voxel_size, (torch.tensor([1.0, 0.75, 0.625]) - torch.tensor([-1.0, -0.75, -0.625])) / 4)
    for k, v in before.items():
        assert torch.equal(getattr(cams, k), v)
    assert pipeline.model.training
    with pytest.raises(ValueError, match="Resolution"):
        export.export_tsdf_mesh(pipeline, tmp_path, resolution="256", **kw)
    # the reference's signature and defaults (tsdf_utils.py:277-290), so ns-export tsdf can call it in its place
    params = inspect.signature(export.export_tsdf_mesh).parameters
    positional = [(k, p.default) for k, p in params.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert positional == [("pipeline", inspect.Parameter.empty), ("output_dir", inspect.Parameter.empty), ("downscale_factor", 2),
                          ("depth_output_name", "depth"), ("rgb_output_name", "rgb"), ("resolution", (256, 256, 256)),
                          ("batch_size", 10), ("use_bounding_box", True), ("bounding_box_min", (-1.0, -1.0, -1.0)),
                          ("bounding_box_max", (1.0, 1.0, 1.0)), ("refine_mesh_using_initial_aabb_estimate", False),
                          ("refinement_epsilon", 1e-2)]


# ---------------------------------------------------------------- the entry point ------------------------------------------
EXPORT_HEADER = os.path.join(ROOT, "include", "nsamd_export.h")


def test_entry_point_is_declared_bound_and_launched_from_one_place(tmp_path):
    """include/nsamd_export.h, the library and _native._EXPORT_SIGNATURES agree, as tests/test_abi.py checks for include/nsamd.h:
    the header is plain C99, a C program that includes it links against the library and gets the argument checks' answers."""
    from nerfstudio_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(EXPORT_HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(nsamd_[a-z0-9_]+)\s*\(", header))) == sorted(N._EXPORT_SIGNATURES) == ["nsamd_tsdf_integrate"]
    assert not set(N._EXPORT_SIGNATURES) & set(N._SIGNATURES)
    assert hasattr(C.CDLL(N.LIB_PATH), "nsamd_tsdf_integrate") and callable(N.load().nsamd_tsdf_integrate)
    assert N._EXPORT_SIGNATURES["nsamd_tsdf_integrate"] == [N.TsdfVolume, N.vp, N.vp, N.vp, N.vp, N.vp, N.i32, N.vp, N.vp, N.i32,
                                                            N.i32, N.vp]
    assert C.sizeof(N.TsdfVolume) == 40
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", EXPORT_HEADER], check=True)
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "nsamd_export.h"\n'
                   "int main(void) {\n"
                   "  nsamd_tsdf_volume vol = {{0, 0, 0}, {1, 1, 1}, {2, 2, 2}, 5.0f};\n"
                   "  if (nsamd_tsdf_integrate(vol, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, 4, 4, NULL) != NSAMD_OK) return 1;\n"
                   "  if (nsamd_tsdf_integrate(vol, NULL, NULL, NULL, NULL, NULL, 1, NULL, NULL, 4, 4, NULL) != NSAMD_ERR_INVALID_ARG)"
                   " return 2;\n"
                   "  return 0;\n}\n")
    libdir = os.path.dirname(N.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.dirname(EXPORT_HEADER), str(src), "-o", str(tmp_path / "use"), "-L", libdir,
                    "-lnsamd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([str(tmp_path / "use")], check=True)
    pkg = os.path.join(ROOT, "nerfstudio_amd")
    sites = [f for f in os.listdir(pkg) if f.endswith(".py") and f != "_native.py"
             and ".nsamd_tsdf_integrate" in open(os.path.join(pkg, f)).read()]
    assert sites == ["functional.py"]
    makefile = open(os.path.join(pkg, "csrc", "Makefile")).read()
    assert " tsdf.hip" in makefile and " tsdf.h " in makefile and "nsamd_export.h" in makefile


def test_entry_point_validates_before_it_launches():
    """No call here reaches a launch: every one fails a check or has nothing to do (the pointers are host memory)."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    a = torch.zeros(64)
    p = a.data_ptr()

    def call(dims=(2, 2, 2), truncation=1.0, values=p, weights=p, colors=p, w2c=p, K=p, B=1, depth=p, color=p, H=2, W=2):
        vol = N.TsdfVolume()
        for i in range(3):
            vol.origin[i], vol.voxel_size[i], vol.dims[i] = -1.0, 0.5, dims[i]
        vol.truncation = truncation
        return lib.nsamd_tsdf_integrate(vol, values, weights, colors, w2c, K, B, depth, color, H, W, None)

    assert call(B=0) == 0 and call(dims=(0, 2, 2)) == 0 and call(dims=(2, 2, 0)) == 0  # nothing to do
    assert call(B=0, values=None) == 0
    for bad in (dict(values=None), dict(weights=None), dict(w2c=None), dict(K=None), dict(depth=None), dict(H=0), dict(H=-3),
                dict(W=0), dict(B=-1), dict(dims=(2, -1, 2)), dict(truncation=0.0), dict(truncation=float("nan"))):
        assert call(**bad) == -1, bad
    assert call(dims=(2**31 - 1, 2**10, 1)) == -2  # more voxels than one lane each in a launch grid
    with pytest.raises(RuntimeError, match="status -1"):
        N.check(call(values=None), "tsdf_integrate")
