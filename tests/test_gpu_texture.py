"""GPU tests of the texture export: nsamd_texel_rays / nsamd_mesh_raylen / nsamd_texture_store (csrc/texture.hip over
csrc/texture.h) entry by entry against the float64 restatement of tests/texture_reference.py under the bounds its docstring
derives (the ones tests/test_texture_cpu.py holds the host build to), EvalRenderer.render_texels and render(bundle) with the
bundle's own bounds against the module path bit for bit, and export.export_textured_tsdf_mesh_on_device end to end. Every
comparison prints its figures before it asserts."""
import os

import numpy as np
import pytest
import torch

import texture_reference as tx
import tsdf_reference as tr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
POISON, GUARD = -77.0, 512
CASES = ((1, 2), (2, 2), (7, 4), (37, 4), (3, 4), (128, 4), (127, 4), (37, 3))


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    info = _native.device_info()
    assert info["wavefront_size"] == 64 and info["arch"].startswith("gfx950"), info
    return functional


def guarded(numel, dtype, fill):
    slab = torch.full((GUARD + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return slab, slab[GUARD:GUARD + numel]


def intact(slab, numel, fill):
    return bool((slab[:GUARD] == fill).all()) and bool((slab[GUARD + numel:] == fill).all())


def device_mesh(vertices, normals, faces):
    return T(vertices).cuda(), T(normals).cuda(), T(faces).cuda()


def launch_rays(F, mesh, P, raylen, first=0, count=None, rows=None):
    """-> (origins, directions [rows,3], nears, fars [rows]) on the host; asserts that the guards around all four are intact"""
    from nerfstudio_amd.texture import TexelAtlas

    v, n, f = mesh
    atlas = TexelAtlas.for_faces(f.shape[0], P)
    count = atlas.width * atlas.height - first if count is None else count
    rows = count if rows is None else rows
    slabs = [guarded(3 * rows, torch.float32, POISON), guarded(3 * rows, torch.float32, POISON), guarded(rows, torch.float32, POISON),
             guarded(rows, torch.float32, POISON)]
    o, d, nr, fr = slabs[0][1].view(rows, 3), slabs[1][1].view(rows, 3), slabs[2][1], slabs[3][1]
    F.texel_rays_launch(atlas.native(), v, n, f, torch.tensor([raylen], dtype=torch.float32, device="cuda"), first, count, rows, o, d, nr, fr)
    torch.cuda.synchronize()
    for (slab, _), numel in zip(slabs, (3 * rows, 3 * rows, rows, rows)):
        assert intact(slab, numel, POISON)
    return o.cpu().numpy(), d.cpu().numpy(), nr.cpu().numpy(), fr.cpu().numpy()


def check_rays(o, d, ref, what):
    eo = np.abs(o.astype(np.float64) - ref["origins"])
    ed = np.abs(d.astype(np.float64) - ref["directions"])
    print(f"{what}: origins max err {eo.max():.3e} (bound at it {ref['origin_bound'].flat[eo.argmax()]:.3e}), "
          f"directions {ed.max():.3e} (bound {ref['direction_bound'].flat[ed.argmax()]:.3e})")
    assert (eo <= ref["origin_bound"]).all() and (ed <= ref["direction_bound"]).all(), what


# ---------------------------------------------------------------- nsamd_texel_rays ------------------------------------------------
@pytest.mark.parametrize("F_,P", CASES)
def test_texel_rays_against_float64(F, F_, P):
    vertices, normals, faces = tx.soup(F_)
    raylen = float(np.float32(tx.raylen(vertices, faces)))
    mesh = device_mesh(vertices, normals, faces)
    o, d, nr, fr = launch_rays(F, mesh, P, raylen)
    check_rays(o, d, tx.texel_rays(vertices, normals, faces, P, raylen), f"gpu F={F_} P={P}")
    assert (nr == 0).all() and (fr == np.float32(raylen)).all()
    o0, d0, _, fr0 = launch_rays(F, mesh, P, 0.0)  # raylen_method="none"
    check_rays(o0, d0, tx.texel_rays(vertices, normals, faces, P, 0.0), f"gpu F={F_} P={P} raylen 0")
    assert np.array_equal(d0, d) and (fr0 == 0).all()


@pytest.fixture(scope="module")
def full128(F):
    """the 1792 texels of soup(128) at P = 4 in one launch, the reference of the chunked launches: computed once, never written"""
    vertices, normals, faces = tx.soup(128)
    mesh = device_mesh(vertices, normals, faces)
    out = launch_rays(F, mesh, 4, 0.37)
    for a in out:
        a.setflags(write=False)
    return mesh, out


@pytest.mark.parametrize("count", (1, 63, 64, 65, 255, 256, 257))
def test_a_chunk_equals_its_rows_of_the_whole_and_pads_with_its_last_row(F, full128, count):
    mesh, (o, d, nr, fr) = full128
    first = 13 + 56 * 5  # neither on a row of the 56-wide atlas nor on a square
    for rows in (count, count + 37):
        co, cd, cn, cf = launch_rays(F, mesh, 4, 0.37, first, count, rows)
        assert np.array_equal(co[:count].view(np.uint32), o[first:first + count].view(np.uint32))
        assert np.array_equal(cd[:count].view(np.uint32), d[first:first + count].view(np.uint32))
        assert (cn == 0).all() and (cf == np.float32(0.37)).all()
        assert (co[count:].view(np.uint32) == co[count - 1].view(np.uint32)).all() and (cd[count:].view(np.uint32) == cd[count - 1].view(np.uint32)).all()


def test_any_split_into_chunks_gives_the_bits_of_one_launch(F, full128):
    mesh, (o, d, _, _) = full128
    for chunk in (100, 512, 1791):
        parts = [launch_rays(F, mesh, 4, 0.37, a, min(chunk, 1792 - a), chunk) for a in range(0, 1792, chunk)]
        ko = np.concatenate([p[0][:min(chunk, 1792 - a)] for p, a in zip(parts, range(0, 1792, chunk))])
        kd = np.concatenate([p[1][:min(chunk, 1792 - a)] for p, a in zip(parts, range(0, 1792, chunk))])
        assert np.array_equal(ko.view(np.uint32), o.view(np.uint32)) and np.array_equal(kd.view(np.uint32), d.view(np.uint32))


def test_face_indices_outside_the_mesh_are_clamped_and_a_zero_blend_gives_zero(F):
    vertices, normals, faces = tx.soup(37)
    wild = faces.copy()
    wild[1], wild[4, 2], wild[36, 0] = (-5, len(vertices), 2 ** 31 - 1), -2 ** 31, len(vertices) + 100000
    o, d, _, _ = launch_rays(F, device_mesh(vertices, normals, wild), 4, 0.5)
    check_rays(o, d, tx.texel_rays(vertices, normals, np.clip(wild, 0, len(vertices) - 1), 4, 0.5), "gpu clamped faces")
    flat = normals.copy()
    flat[faces[2]] = 0.0
    o, d, _, _ = launch_rays(F, device_mesh(vertices, flat, faces), 4, 0.5)
    ref = tx.texel_rays(vertices, flat, faces, 4, 0.5)
    zero = ref["blend_norm"] == 0
    assert zero.sum() >= 4 and (d[zero] == 0).all() and np.isfinite(d).all() and np.isfinite(o).all()
    check_rays(o, d, ref, "gpu zero blend")


# ---------------------------------------------------------------- nsamd_mesh_raylen -----------------------------------------------
@pytest.mark.parametrize("T_", (1, 255, 256, 257, 5000, 300000))  # 300000: more faces than the 1024 workgroups cover at once
def test_raylen_is_float64_rounded_once_and_repeats(F, T_):
    from nerfstudio_amd import _native as N

    rs = np.random.RandomState(T_)
    vertices = rs.uniform(-1, 1, (max(3, min(T_ // 2, 4000)), 3)).astype(np.float32)
    faces = rs.randint(0, len(vertices), (T_, 3)).astype(np.int32)
    faces[0, 0] = len(vertices) + 3  # clamped
    v, f = T(vertices).cuda(), T(faces).cuda()
    runs = []
    for _ in range(3):
        scratch_slab, scratch = guarded(N.RAYLEN_SCRATCH_BYTES, torch.uint8, 0xAB)
        out_slab, out = guarded(1, torch.float32, POISON)
        F.mesh_raylen_launch(v, f, scratch, out)
        torch.cuda.synchronize()
        assert intact(scratch_slab, N.RAYLEN_SCRATCH_BYTES, 0xAB) and intact(out_slab, 1, POISON)
        runs.append(out.cpu().numpy().copy())
    exact = tx.raylen(vertices, faces)
    print(f"T={T_}: raylen {float(runs[0][0]):.9g}, float64 {exact:.17g}")
    assert abs(float(runs[0][0]) - exact) <= np.spacing(np.float32(exact))  # 1 fp32 ulp
    assert runs[0].view(np.uint32) == runs[1].view(np.uint32) == runs[2].view(np.uint32)


# ---------------------------------------------------------------- nsamd_texture_store ---------------------------------------------
def test_texture_store_is_exact_at_every_offset_and_keeps_its_guards(F):
    rs = np.random.RandomState(4)
    special = np.array([0.0, 1.0, 0.5 / 255, -0.3, 1.7, np.nan, np.inf, -np.inf, -0.0, 254.5 / 255, 0.999, 1e-30], np.float32)
    rgb = rs.uniform(-0.1, 1.1, (1000, 3)).astype(np.float32)
    rgb.reshape(-1)[:len(special)] = special
    rgb.reshape(-1)[100:356] = (np.arange(256) / np.float32(255)).astype(np.float32)  # every level
    expected = tx.levels(rgb)
    assert np.array_equal(expected.reshape(-1)[100:356], np.arange(256))
    dev = T(rgb).cuda()
    for first in (0, 1, 2, 3, 7):
        for count in (1, 2, 5, 63, 64, 65, 1000):
            slab, image = guarded(3 * (first + count), torch.uint8, 7)
            F.texture_store_launch(dev, count, first, image.view(-1, 3))
            torch.cuda.synchronize()
            got = image.view(-1, 3).cpu().numpy()
            assert intact(slab, 3 * (first + count), 7) and (got[:first] == 7).all(), (first, count)
            assert np.array_equal(got[first:], expected[:count]), (first, count)


# ---------------------------------------------------------------- the runner ------------------------------------------------------
def make_model():
    from oracle import nerfacto_oracle as orc
    from test_gpu_kernels import _hip_model, small_cfg

    cfg = small_cfg(12, 10, 5)
    m = _hip_model(cfg, orc.init_params(cfg, seed=3, table_std=0.4), training=False)
    m.proposal_sampler.set_anneal(0.37)
    return m


@pytest.fixture(scope="module")
def model():
    return make_model()


CAMERA = (torch.tensor([[0.96, -0.10, 0.26, 0.3], [0.05, 0.98, 0.19, -0.2], [-0.27, -0.17, 0.95, 0.9]]), 36.9, 32.8, 20.75, 18.0, 37, 41)


def module_path(model, bundle, monkeypatch):
    monkeypatch.setenv("NSAMD_EVAL_RUNNER", "0")
    try:
        return model.get_outputs_for_camera_ray_bundle(bundle)
    finally:
        monkeypatch.setenv("NSAMD_EVAL_RUNNER", "1")


@pytest.mark.parametrize("P", (4, 3))
def test_render_texels_equals_the_module_path_on_the_same_rays(F, model, monkeypatch, P):
    """a twice-subdivided octahedron of radius 0.3 (128 faces): 56 x 32 = 1792 texels at P = 4 (3 chunks of 512 and 256), 1152
    at P = 3. The module path renders the bundle of the float64-checked texel rays with its nears and fars; the runner generates
    the same rays inside its loop: rgb bit for bit, eager and replayed, at chunk 512 and 256; the image is the rule on that rgb;
    and a camera frame after the texels equals one before (the planes came back)."""
    from nerfstudio_amd.cameras.rays import RayBundle
    from nerfstudio_amd.eval_render import EvalRenderer
    from nerfstudio_amd.texture import TexelAtlas
    from types import SimpleNamespace

    vertices, normals, faces = tx.octahedron(2, 0.3)
    assert faces.shape == (128, 3)
    v, n, f = device_mesh(vertices, normals, faces)
    mesh = SimpleNamespace(vertices=v, normals=n, faces=f)
    atlas = TexelAtlas.for_faces(128, P)
    total = atlas.width * atlas.height
    assert total == {4: 1792, 3: 1152}[P]
    raylen_dev = torch.zeros(1, device="cuda")
    F.mesh_raylen_launch(v, f, torch.empty(8192, dtype=torch.uint8, device="cuda"), raylen_dev)
    raylen = float(raylen_dev[0])
    assert abs(raylen - tx.raylen(vertices, faces)) <= np.spacing(np.float32(raylen))
    o, d, nr, fr = (torch.empty(total, 3, device="cuda"), torch.empty(total, 3, device="cuda"), torch.empty(total, device="cuda"),
                    torch.empty(total, device="cuda"))
    F.texel_rays_launch(atlas.native(), v, n, f, raylen_dev, 0, total, total, o, d, nr, fr)
    check_rays(o.cpu().numpy(), d.cpu().numpy(), tx.texel_rays(vertices, normals, faces, P, raylen), f"octahedron P={P}")
    H, W = atlas.height, atlas.width
    bundle = RayBundle(origins=o.view(H, W, 3), directions=d.view(H, W, 3), pixel_area=torch.ones(H, W, 1, device="cuda"),
                       camera_indices=torch.zeros((H, W, 1), dtype=torch.int64, device="cuda"), nears=nr.view(H, W, 1), fars=fr.view(H, W, 1))
    for chunk, graphs in ((512, (False, True)), (256, (True,))):
        model.config.eval_num_rays_per_chunk = chunk
        ref = module_path(model, bundle, monkeypatch)["rgb"].reshape(-1, 3)
        assert torch.isfinite(ref).all() and float(ref.std()) > 1e-3  # the field is not constant over the sphere
        for use_graph in graphs:
            runner = EvalRenderer(model, use_graph=use_graph)
            before = runner.render_camera(CAMERA[0].cuda(), *CAMERA[1:])
            rgb = torch.full((total, 3), POISON, device="cuda")
            image = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            runner.render_texels(atlas, mesh, raylen_dev, image, rgb)
            what = f"P={P} chunk={chunk} {'graph' if use_graph else 'eager'}"
            assert torch.equal(rgb, ref), f"{what}: max |d| = {float((rgb - ref).abs().max()):.3e}"
            assert np.array_equal(image.cpu().numpy().reshape(-1, 3), tx.levels(ref.cpu().numpy())), what
            assert bool((runner.step.nears == 0).all()) and bool((runner.step.fars == float(model.config.far_plane)).all())
            after = runner.render_camera(CAMERA[0].cuda(), *CAMERA[1:])
            assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before), what
    model.config.eval_num_rays_per_chunk = 512


def test_render_keeps_a_bundles_own_bounds_and_gives_the_planes_back(F, model, monkeypatch):
    """render(bundle) for a bundle that carries nears and fars equals the module path — which leaves such a bundle alone — bit
    for bit in every output; one without them renders between 0 and far_plane as before, also right after a bounded one."""
    from oracle import nerfacto_oracle as orc
    from nerfstudio_amd.cameras.rays import RayBundle
    from nerfstudio_amd.eval_render import EvalRenderer

    model.config.eval_num_rays_per_chunk = 512
    H, W = 37, 41  # 1517 rays: 2 full chunks + 493
    o, d, _, _ = orc.synthetic_rays(H * W, 5, seed=9)
    rs = np.random.RandomState(2)
    nears = T(rs.uniform(0.0, 0.3, (H, W, 1)).astype(np.float32)).cuda()
    fars = nears + T(rs.uniform(0.5, 3.0, (H, W, 1)).astype(np.float32)).cuda()
    common = dict(origins=o.cuda().view(H, W, 3), directions=d.cuda().view(H, W, 3), pixel_area=torch.full((H, W, 1), 1e-6).cuda(),
                  camera_indices=torch.zeros((H, W, 1), dtype=torch.int64).cuda())
    bounded, plain = RayBundle(nears=nears, fars=fars, **common), RayBundle(**common)
    ref_bounded, ref_plain = module_path(model, bounded, monkeypatch), module_path(model, plain, monkeypatch)
    keys = {"rgb", "accumulation", "depth", "expected_depth", "prop_depth_0", "prop_depth_1"}
    assert keys <= set(ref_bounded) and not torch.equal(ref_bounded["rgb"], ref_plain["rgb"])
    assert float(ref_bounded["depth"].max()) <= float(fars.max())  # no sample past a ray's own far
    for use_graph in (False, True):
        runner = EvalRenderer(model, use_graph=use_graph)
        for bundle, ref, what in ((bounded, ref_bounded, "bounded"), (plain, ref_plain, "plain after bounded"), (bounded, ref_bounded, "again")):
            out = runner.render(bundle)
            for k in keys:
                assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), \
                    f"{k} ({what}, {'graph' if use_graph else 'eager'}): max |d| = {float((out[k] - ref[k]).abs().max()):.3e}"
    assert torch.equal(bounded.nears, nears) and torch.equal(bounded.fars, fars)  # the bundle is only read
    through = model.get_outputs_for_camera_ray_bundle(bounded)  # the entry point the reference's export_textured_mesh calls
    assert all(torch.equal(through[k], ref_bounded[k]) for k in keys)


# ---------------------------------------------------------------- end to end ------------------------------------------------------
def test_textured_export_of_a_fused_sphere_end_to_end(F, tmp_path):
    """analytic depth views of a sphere fused into a 32^3 volume, meshed and textured on the device through a field that answers
    one colour everywhere: the four files parse, the counts agree, and every in-triangle texel holds that colour"""
    from types import SimpleNamespace

    from nerfstudio_amd import export
    from test_mesh_cpu import read_mesh_ply
    from test_texture_cpu import check_files

    H, W, R = 48, 64, 0.6
    positions = ((2.0, 0.3, 0.4), (-1.8, 0.9, 0.2), (0.2, -2.0, 0.6), (0.3, 0.4, 2.1))
    n = len(positions)
    cameras = SimpleNamespace(camera_to_worlds=T(np.stack([tr.look_at(p)[:3] for p in positions]).astype(np.float32)),
                              camera_type=torch.ones(n, 1, dtype=torch.int64), fx=torch.full((n, 1), 70.0), fy=torch.full((n, 1), 70.0),
                              cx=torch.full((n, 1), 32.0), cy=torch.full((n, 1), 24.0), height=torch.full((n, 1), H), width=torch.full((n, 1), W))
    colour = np.array([51, 128, 204], np.uint8)

    def render(c2w, fx, fy, cx, cy, h, w):
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        depth = tr.sphere_depth(np.vstack([c2w.cpu().numpy().astype(np.float64), [0, 0, 0, 1]]), K, h, w, R)
        return {"depth": T(depth.astype(np.float32)).cuda().view(h, w, 1), "rgb": T(colour / np.float32(255)).cuda().expand(h, w, 3)}

    flat = make_model().train()  # the export renders in eval mode and gives the mode back
    flat.config.eval_num_rays_per_chunk = 4096
    with torch.no_grad():  # sigmoid(0 x + b) = the colour for every sample; background "last_sample" composites it unchanged
        last = flat.field.mlp_head.layers[-1]
        last.weight.zero_()
        last.bias.copy_(torch.logit(T(colour / np.float64(255))).float())
    outputs = SimpleNamespace(cameras=cameras, scene_box=SimpleNamespace(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]])))
    pipeline = SimpleNamespace(device="cuda", model=flat, datamanager=SimpleNamespace(train_dataset=SimpleNamespace(_dataparser_outputs=outputs)))
    mesh = export.export_textured_tsdf_mesh_on_device(pipeline, tmp_path, px_per_uv_triangle=4, downscale_factor=1, resolution=32,
                                                      batch_size=4, render_fn=render)
    assert flat.training and mesh.vertices.is_cuda
    assert sorted(os.listdir(tmp_path)) == ["material_0.mtl", "material_0.png", "mesh.obj", "tsdf_mesh.ply"]
    vertex, face = read_mesh_ply(tmp_path / "tsdf_mesh.ply")
    Fn = int(mesh.faces.shape[0])
    assert len(face) == Fn > 500 and len(vertex) == mesh.vertices.shape[0]
    png = check_files(tmp_path, mesh.vertices.cpu().numpy(), mesh.normals.cpu().numpy(), mesh.faces.cpu().numpy(), 4)
    t, w = tx.texel_sites(Fn, 4)
    inside = (w >= 0).all(1)
    texels = png.reshape(-1, 3)[inside]
    print(f"end to end: {Fn} faces, atlas {png.shape[1]}x{png.shape[0]}, {int(inside.sum())} in-triangle texels, "
          f"levels {texels.min(0)} .. {texels.max(0)}")
    assert inside.sum() >= 10 * Fn and (texels == colour[None]).all()
