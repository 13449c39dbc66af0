"""CPU tests of the texture export (include/nsamd_texture.h, nerfstudio_amd/texture.py, EvalRenderer.render_texels, render with
a bundle's own bounds, export.export_textured_tsdf_mesh_on_device): the arithmetic of nerfstudio_amd/csrc/texture.h compiled for
the host (tests/hostcheck/texture_helpers.cc) and looped as the kernels compose it against the float64 restatement
(tests/texture_reference.py) and against the fixture the reference's own unwrap_mesh_per_uv_triangle wrote
(tests/golden/texture.npz), the same build under the address and undefined-behaviour sanitizers as a stand-alone program, the
Python layer over launches served by the restatement, the files parsed back, and the ABI.

Bounds: texture_reference's docstring derives them from the operation count (C_BLEND = 5 roundings per blended term, the
normalisation's 4, the offset's 2). Against the fixture the reference's fp32 gets, on top, its own recorded deviation from float64
(`ref_vs_f64_*`): the allowance is the reference's, not the kernel's."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import types
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import texture_reference as tx

T = torch.from_numpy
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")
HEADER = os.path.join(ROOT, "include", "nsamd_texture.h")
NAMES = ["nsamd_mesh_raylen", "nsamd_texel_rays", "nsamd_texture_store"]
GOLDEN_CASES = ((1, 2), (2, 2), (7, 4), (37, 4))
CASES = GOLDEN_CASES + ((3, 4), (128, 4), (127, 4), (37, 3))  # + odd, full, one clamped slot, P = 3


def _ptr(t):
    if t is None:
        return None
    assert t.is_contiguous()
    return t.data_ptr()


@pytest.fixture(scope="module")
def g():
    return load_golden("texture")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """(texel_rays, mesh_raylen, texture_store) with the arguments of nerfstudio_amd.functional's launches, served by the host
    build of texture.h"""
    from nerfstudio_amd import _native as N

    out = str(tmp_path_factory.mktemp("hostcheck") / "libtexturecheck.so")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(HOSTCHECK, "texture_helpers.cc")], check=True)
    lib = C.CDLL(out)
    for name, argtypes in N._TEXTURE_SIGNATURES.items():
        getattr(lib, name.replace("nsamd_", "hc_")).argtypes = argtypes[:-1]  # no stream

    def texel_rays(atlas, vertices, normals, faces, raylen_dev, first, count, rows, origins, directions, nears, fars):
        assert origins.shape[0] >= rows and directions.shape[0] >= rows and nears.numel() >= rows and fars.numel() >= rows
        assert lib.hc_texel_rays(atlas, _ptr(vertices), _ptr(normals), _ptr(faces), vertices.shape[0], _ptr(raylen_dev), first, count,
                                 rows, _ptr(origins), _ptr(directions), _ptr(nears), _ptr(fars)) == 0

    def mesh_raylen(vertices, faces, scratch, raylen_dev):
        assert scratch.numel() >= N.RAYLEN_SCRATCH_BYTES and scratch.data_ptr() % 8 == 0
        assert lib.hc_mesh_raylen(_ptr(vertices), vertices.shape[0], _ptr(faces), faces.shape[0], _ptr(scratch), _ptr(raylen_dev)) == 0

    def texture_store(rgb, count, first, atlas_u8):
        assert 3 * (first + count) <= atlas_u8.numel()
        assert lib.hc_texture_store(_ptr(rgb), count, first, _ptr(atlas_u8)) == 0

    texel_rays.lib = lib
    return texel_rays, mesh_raylen, texture_store


def host_rays(host, vertices, normals, faces, P, raylen, first=0, count=None, rows=None):
    from nerfstudio_amd.texture import TexelAtlas

    atlas = TexelAtlas.for_faces(len(faces), P)
    count = atlas.width * atlas.height - first if count is None else count
    rows = count if rows is None else rows
    o, d, nr, fr = torch.full((rows, 3), -7.0), torch.full((rows, 3), -7.0), torch.full((rows,), -7.0), torch.full((rows,), -7.0)
    host[0](atlas.native(), T(vertices), T(normals), T(faces), torch.tensor([raylen], dtype=torch.float32), first, count, rows, o, d, nr, fr)
    return o.numpy(), d.numpy(), nr.numpy(), fr.numpy()


def check_rays(o, d, ref, what, extra_o=0.0, extra_d=0.0):
    eo = np.abs(o.astype(np.float64) - ref["origins"])
    ed = np.abs(d.astype(np.float64) - ref["directions"])
    print(f"{what}: origins max err {eo.max():.3e} (bound at it {ref['origin_bound'].flat[eo.argmax()] + extra_o:.3e}), "
          f"directions {ed.max():.3e} (bound {ref['direction_bound'].flat[ed.argmax()] + extra_d:.3e})")
    assert (eo <= ref["origin_bound"] + extra_o).all(), what
    assert (ed <= ref["direction_bound"] + extra_d).all(), what


# ---------------------------------------------------------------- texture.h on the host ------------------------------------------
@pytest.mark.parametrize("F,P", CASES)
def test_host_build_matches_float64_on_every_texel(host, F, P):
    vertices, normals, faces = tx.soup(F)
    raylen = float(np.float32(tx.raylen(vertices, faces)))
    o, d, nr, fr = host_rays(host, vertices, normals, faces, P, raylen)
    ref = tx.texel_rays(vertices, normals, faces, P, raylen)
    sw, sh, W, H = tx.layout(F, P)
    assert o.shape == (W * H, 3) and ref["blend_norm"].min() >= 0.1
    assert (ref["t"] == F - 1).sum() >= ((ref["t"] == F - 2).sum() if F > 1 else 1)  # the clamped texels belong to the last face
    check_rays(o, d, ref, f"host F={F} P={P}")
    assert (nr == 0).all() and (fr == np.float32(raylen)).all()
    o0, d0, _, fr0 = host_rays(host, vertices, normals, faces, P, 0.0)  # raylen_method="none"
    ref0 = tx.texel_rays(vertices, normals, faces, P, 0.0)
    check_rays(o0, d0, ref0, f"host F={F} P={P} raylen 0")
    assert np.array_equal(d0, d) and (fr0 == 0).all()


def test_a_zero_blend_gives_a_zero_direction_and_out_of_range_faces_are_clamped(host):
    vertices, normals, faces = tx.soup(7)
    normals = normals.copy()
    normals[faces[2]] = 0.0  # every corner of face 2
    o, d, _, _ = host_rays(host, vertices, normals, faces, 4, 0.5)
    ref = tx.texel_rays(vertices, normals, faces, 4, 0.5)
    zero = ref["blend_norm"] == 0
    assert zero.sum() >= 4 and (d[zero] == 0).all() and np.isfinite(d).all()
    check_rays(o, d, ref, "zero blend")
    assert (np.abs(o[zero].astype(np.float64) - ref["origins"][zero]) <= tx.C_BLEND * tx.U * 3).all()  # no offset along a zero direction
    wild = faces.copy()
    wild[1], wild[4, 2] = (-5, len(vertices), 2 ** 31 - 1), -2 ** 31
    o, d, _, _ = host_rays(host, vertices, normals, wild, 4, 0.5)
    check_rays(o, d, tx.texel_rays(vertices, normals, np.clip(wild, 0, len(vertices) - 1), 4, 0.5), "clamped faces")


@pytest.mark.parametrize("F,P", GOLDEN_CASES)
def test_host_build_matches_the_reference_fixture(host, g, F, P):
    k = f"m{F}_{P}_"
    vertices, normals, faces = g[k + "vertices"], g[k + "normals"], g[k + "faces"]
    mine = tx.soup(F)
    assert all(np.array_equal(a, b) for a, b in zip((vertices, normals, faces), mine))  # the fixture's meshes are soup(F)
    o, d, _, _ = host_rays(host, vertices, normals, faces, P, 0.0)  # the reference's arrays are those before the offset
    H, W = g[k + "origins"].shape[:2]
    assert (W, H) == tx.layout(F, P)[2:]
    ref = tx.texel_rays(vertices, normals, faces, P, 0.0)
    ref_as_fixture = dict(ref, origins=g[k + "origins"].reshape(-1, 3).astype(np.float64),
                          directions=g[k + "directions"].reshape(-1, 3).astype(np.float64))
    check_rays(o, d, ref_as_fixture, f"fixture F={F} P={P}", float(g[k + "ref_vs_f64_origins"]), float(g[k + "ref_vs_f64_directions"]))
    assert float(g[k + "ref_vs_f64_origins"]) < 1e-5 and float(g[k + "ref_vs_f64_directions"]) < 1e-5  # the restatement IS the reference's function


@pytest.mark.parametrize("F,P", ((37, 4), (127, 4), (3, 2)))
def test_host_build_is_clean_under_the_sanitizers(tmp_path, F, P):
    """a stand-alone program with the sanitizers' runtimes linked in statically: it runs in the environment it inherits, as it
    is, and nothing of it runs inside python"""
    exe = str(tmp_path / "texture_main")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(HOSTCHECK, "texture_main.cc"), os.path.join(HOSTCHECK, "texture_helpers.cc")], check=True)
    vertices, normals, faces = tx.soup(F)
    faces = faces.copy()
    faces[0, 0], faces[-1, 2] = -3, len(vertices) + 9  # clamped, never read past an end
    path = tmp_path / "mesh.bin"
    with open(path, "wb") as f:
        f.write(vertices.tobytes() + normals.tobytes() + faces.tobytes())
    sw, sh, W, H = tx.layout(F, P)
    run = subprocess.run([exe, str(path), str(len(vertices)), str(F), str(P), str(sw), str(sh)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    expected = np.float32(tx.raylen(vertices, faces))
    texels, raylen = re.fullmatch(r"texels (\d+) raylen (\S+)", run.stdout.strip()).groups()
    assert int(texels) == W * H and abs(float(raylen) - expected) <= np.spacing(expected)


# ---------------------------------------------------------------- the layout, the rule, the ray length --------------------------
@pytest.mark.parametrize("F,P", GOLDEN_CASES)
def test_texture_coordinates_match_the_fixture_and_texel_centres_map_into_their_triangle(g, F, P):
    from nerfstudio_amd.texture import TexelAtlas

    atlas = TexelAtlas.for_faces(F, P)
    assert (atlas.squares_w, atlas.squares_h, atlas.width, atlas.height) == tx.layout(F, P)
    tc = atlas.texture_coordinates()
    assert tuple(tc.shape) == (F, 3, 2) and tc.dtype == torch.float32
    ref = g[f"m{F}_{P}_texture_coordinates"]
    err = np.abs(tc.numpy().astype(np.float64) - ref).max()
    print(f"F={F} P={P}: texture coordinates vs the reference {err:.2e}")
    assert err <= 2.0 ** -24 + float(g[f"m{F}_{P}_ref_vs_f64_texture_coordinates"])  # one rounding of a value below 1, plus the reference's
    assert np.abs(tc.numpy() - tx.texture_coordinates(F, P)).max() <= 2.0 ** -25
    # every texel centre whose weights are all >= 0 lies inside its own triangle's texture coordinates, where it interpolates to itself
    t, w = tx.texel_sites(F, P)
    inside = (w >= 0).all(1)
    W, H = atlas.width, atlas.height
    centre = np.stack([(np.arange(W * H) % W + 0.5) / W, (np.arange(W * H) // W + 0.5) / H], 1)
    back = np.einsum("nc,ncd->nd", w, tx.texture_coordinates(F, P)[t])
    assert inside.sum() >= F * P * (P + 1) // 2 and np.abs(back[inside] - centre[inside]).max() < 1e-12
    assert np.abs(w.sum(1) - 1).max() < 1e-12


def test_atlas_sizes_and_refusals():
    from nerfstudio_amd.texture import TexelAtlas

    for F, P in ((1, 2), (2, 2), (7, 4), (37, 4), (200, 3), (5000, 4), (50000, 4), (50000, 10), (10 ** 6, 4)):
        a = TexelAtlas.for_faces(F, P)
        assert (a.squares_w, a.squares_h, a.width, a.height) == tx.layout(F, P) and 2 * a.squares_w * a.squares_h >= F
    assert (TexelAtlas.for_faces(50000, 4).width, TexelAtlas.for_faces(50000, 4).height) == (1113, 632)
    with pytest.raises(ValueError, match="at least 2"):
        TexelAtlas.for_faces(4, 1)
    with pytest.raises(ValueError, match="no texture"):
        TexelAtlas.for_faces(0, 4)


def test_store_rule(host):
    one = np.float32(1.0)
    half = np.float32(0.5) / np.float32(255)
    v = np.array([0.0, 1.0, half, np.nextafter(half, -one), np.nextafter(half, one), -0.3, 1.7, np.nan, np.inf, -np.inf, -0.0,
                  254.5 / 255, 0.999, 1e-30, 0.4 / 255, 0.6 / 255], dtype=np.float32)
    rgb = np.resize(v, (16, 3)).astype(np.float32)  # 48 values: every one above three times, at every byte phase
    expected = tx.levels(rgb)
    # the three values around 0.5 / 255 follow the fp32 product and sum of the rule (the sum of 0.49999997 and 0.5 is a tie
    # that rounds to 1): whatever tx.levels — numpy's fp32 — gives, 0 or 1; a clear 0.4 / 255 and 0.6 / 255 are 0 and 1
    flat = expected.reshape(-1)
    assert flat[:2].tolist() == [0, 255] and set(flat[2:5].tolist()) <= {0, 1} and flat[4] == 1
    assert flat[5:11].tolist() == [0, 255, 0, 255, 0, 0] and flat[12] == 255 and flat[13:16].tolist() == [0, 0, 1]
    for first in (0, 1, 2, 3):  # every alignment of the destination's first byte
        for count in (1, 2, 5, 16):
            image = torch.full((20, 3), 7, dtype=torch.uint8)
            host[2](T(rgb), count, first, image)
            assert np.array_equal(image.numpy()[first:first + count], expected[:count]), (first, count)
            assert (image.numpy()[:first] == 7).all() and (image.numpy()[first + count:] == 7).all()


@pytest.mark.parametrize("F,P", GOLDEN_CASES)
def test_raylen_matches_the_fixture(host, g, F, P):
    k = f"m{F}_{P}_"
    out = torch.zeros(1)
    host[1](T(g[k + "vertices"]), T(g[k + "faces"]), torch.zeros(8 * 1024, dtype=torch.uint8), out)
    ref = float(g[k + "raylen"])
    print(f"F={F}: raylen {float(out[0]):.9g}, the reference's {ref:.9g}")
    assert abs(float(out[0]) - ref) <= 16 * 2.0 ** -24 * ref  # fp32 pairwise summation of <= 128 terms on the reference's side
    exact = tx.raylen(g[k + "vertices"], g[k + "faces"])
    assert abs(float(out[0]) - exact) <= np.spacing(np.float32(exact))


@pytest.mark.parametrize("T_", (1, 255, 256, 257, 5000))
def test_raylen_is_the_rounded_float64_sum(host, T_):
    rs = np.random.RandomState(T_)
    vertices = rs.uniform(-1, 1, (max(3, T_ // 2), 3)).astype(np.float32)
    faces = rs.randint(0, len(vertices), (T_, 3)).astype(np.int32)
    out = torch.zeros(1)
    host[1](T(vertices), T(faces), torch.zeros(8 * 1024, dtype=torch.uint8), out)
    exact = tx.raylen(vertices, faces)
    assert abs(float(out[0]) - exact) <= 0.5 * np.spacing(np.float32(exact)) * (1 + 1e-6)


# ---------------------------------------------------------------- the Python layer ------------------------------------------------
class FakeModel(torch.nn.Module):
    """what eval_render.supported asks of a nerfacto model"""

    def __init__(self, **extra):
        super().__init__()
        self.config = types.SimpleNamespace(predict_normals=False, far_plane=1000.0, eval_num_rays_per_chunk=64)
        self.proposal_networks, self.field, self.proposal_sampler = torch.nn.ModuleList(), torch.nn.Identity(), torch.nn.Identity()
        for k, v in extra.items():
            setattr(self, k, v)


def fake_runner(model, n=64, fail_at=None):
    """an EvalRenderer over host buffers whose chunk colours every ray by its origin and records the bounds it ran with"""
    from nerfstudio_amd.eval_render import EvalRenderer

    r = EvalRenderer.__new__(EvalRenderer)
    r.model, r.chunk, r.normals = model, n, False
    r.step = types.SimpleNamespace(origins=torch.zeros(n, 3), directions=torch.zeros(n, 3), nears=torch.zeros(n),
                                   fars=torch.full((n,), 1000.0), rgb=torch.zeros(n, 3), acc=torch.zeros(n), depth_exp=torch.zeros(n),
                                   depth_med=[torch.zeros(n)], n_prop=0)
    r.ran, r.modes = [], []
    r._refresh_constants = lambda: r.modes.append(model.training)

    def run_chunk():
        if fail_at is not None and len(r.ran) == fail_at:
            raise RuntimeError("chunk failed")
        s = r.step
        r.ran.append((s.origins.clone(), s.directions.clone(), s.nears.clone(), s.fars.clone()))
        s.rgb.copy_(0.5 + s.origins)

    r._run_chunk = run_chunk
    return r


@pytest.fixture()
def injected(monkeypatch):
    from nerfstudio_amd import functional

    log = []
    rays, raylen, store = tx.restatement_launches(log)
    monkeypatch.setattr(functional, "texel_rays_launch", rays)
    monkeypatch.setattr(functional, "mesh_raylen_launch", raylen)
    monkeypatch.setattr(functional, "texture_store_launch", store)
    return log


def mesh_of(F, **kw):
    vertices, normals, faces = tx.soup(F, **kw)
    return types.SimpleNamespace(vertices=T(vertices), normals=T(normals), faces=T(faces))


def test_render_texture_chunks_in_order_and_restores_the_bounds(injected, monkeypatch):
    from nerfstudio_amd import eval_render, texture

    model = FakeModel().train()
    runner = fake_runner(model)
    monkeypatch.setattr(eval_render, "runner_for", lambda m, dev: runner if m is model and not m.training else None)
    mesh = mesh_of(37)
    rgb = torch.zeros(35 * 16, 3)
    image = texture.render_texture(model, mesh, 4, out_f32=rgb)
    assert tuple(image.shape) == (16, 35, 3) and image.dtype == torch.uint8 and model.training and runner.modes == [False]
    # 560 texels in chunks of 64: 8 full ones and 48, each one rays launch, one chunk, one store, in texel order
    firsts = list(range(0, 560, 64))
    assert injected == [("raylen", 37)] + [e for a in firsts for e in (("texel_rays", a, min(64, 560 - a), 64), ("store", a, min(64, 560 - a)))]
    raylen = np.float32(tx.raylen(mesh.vertices.numpy(), mesh.faces.numpy()))
    ref = tx.texel_rays(mesh.vertices.numpy(), mesh.normals.numpy(), mesh.faces.numpy(), 4, float(raylen))
    assert np.array_equal(rgb.numpy(), (np.float32(0.5) + ref["origins"].astype(np.float32)))
    assert np.array_equal(image.numpy().reshape(-1, 3), tx.levels(rgb.numpy()))
    for o, d, nr, fr in runner.ran:
        assert (nr == 0).all() and (fr == float(raylen)).all()
    last = runner.ran[-1]
    assert torch.equal(last[0][48:], last[0][47:48].expand(16, 3)) and torch.equal(last[1][48:], last[1][47:48].expand(16, 3))
    assert (runner.step.nears == 0).all() and (runner.step.fars == 1000.0).all()  # the next camera frame's planes
    injected.clear()
    texture.render_texture(model.eval(), mesh, 4, raylen_method="none")
    assert injected[0][0] == "texel_rays" and all((fr == 0).all() for *_, fr in runner.ran[9:]) and not model.training


def test_bounds_are_restored_after_a_failed_chunk(injected, monkeypatch):
    from nerfstudio_amd import eval_render, texture
    from nerfstudio_amd.cameras.rays import RayBundle

    model = FakeModel().eval()
    runner = fake_runner(model, fail_at=1)
    monkeypatch.setattr(eval_render, "runner_for", lambda m, dev: runner)
    with pytest.raises(RuntimeError, match="chunk failed"):
        texture.render_texture(model, mesh_of(37), 4)
    assert len(runner.ran) == 1 and (runner.ran[0][3] != 1000.0).all()
    assert (runner.step.nears == 0).all() and (runner.step.fars == 1000.0).all()
    # the same for render(bundle) with the bundle's own bounds; a bundle without them never touches the planes
    n = 100
    o, d = torch.rand(n, 3), torch.rand(n, 3)
    bundle = RayBundle(origins=o, directions=d, pixel_area=torch.ones(n, 1), nears=torch.full((n, 1), 0.25), fars=torch.rand(n, 1) + 1)
    runner = fake_runner(model, fail_at=1)
    with pytest.raises(RuntimeError, match="chunk failed"):
        runner.render(bundle)
    assert (runner.ran[0][2] == 0.25).all() and torch.equal(runner.ran[0][3], bundle.fars[:64, 0])
    assert (runner.step.nears == 0).all() and (runner.step.fars == 1000.0).all()
    runner = fake_runner(model)
    out = runner.render(bundle)
    assert torch.equal(out["rgb"], 0.5 + o) and len(runner.ran) == 2
    assert torch.equal(runner.ran[1][3][:36], bundle.fars[64:, 0]) and (runner.ran[1][3][36:] == bundle.fars[-1, 0]).all()  # padded with the last ray's
    assert (runner.step.nears == 0).all() and (runner.step.fars == 1000.0).all()
    for half in (dict(nears=bundle.nears), dict(fars=bundle.fars), {}):  # both or neither, as the collider decides
        runner = fake_runner(model)
        runner.render(RayBundle(origins=o, directions=d, pixel_area=torch.ones(n, 1), **half))
        assert all((nr == 0).all() and (fr == 1000.0).all() for _, _, nr, fr in runner.ran)


def test_what_is_refused_and_why(injected, monkeypatch, tmp_path):
    from nerfstudio_amd import eval_render, texture

    mesh = mesh_of(7)
    with pytest.raises(NotImplementedError, match="instant-ngp.*no per-ray near and far"):
        texture.render_texture(FakeModel(occupancy_grid=torch.nn.Identity()), mesh, 4)
    with pytest.raises(NotImplementedError, match="not a nerfacto model.*no torch fallback"):
        texture.render_texture(types.SimpleNamespace(config=types.SimpleNamespace()), mesh, 4)
    model = FakeModel().eval()
    model.config.predict_normals = True
    with pytest.raises(NotImplementedError, match="not a predict_normals model"):
        texture.render_texture(model, mesh, 4)
    model = FakeModel().eval()
    monkeypatch.setattr(eval_render, "runner_for", lambda m, dev: fake_runner(m))
    with pytest.raises(ValueError, match="Ray length method mean not supported"):
        texture.render_texture(model, mesh, 4, raylen_method="mean")
    with pytest.raises(ValueError, match="at least 2"):
        texture.render_texture(model, mesh, 1)
    bad = types.SimpleNamespace(vertices=mesh.vertices, normals=mesh.normals, faces=mesh.faces.clone())
    bad.faces[3, 1] = mesh.vertices.shape[0]
    with pytest.raises(ValueError, match=f"index vertices 0 .. {mesh.vertices.shape[0]}"):
        texture.render_texture(model, bad, 4)
    with pytest.raises(ValueError, match="vertex normals must be equal"):
        texture.render_texture(model, types.SimpleNamespace(vertices=mesh.vertices, normals=mesh.normals[:-1], faces=mesh.faces), 4)
    pipeline = types.SimpleNamespace(device="cpu", model=model)
    with pytest.raises(ValueError, match="Unwrap method planar not supported"):
        texture.export_textured_mesh(mesh, pipeline, tmp_path, 4, unwrap_method="planar")
    monkeypatch.setitem(sys.modules, "nerfstudio", None)  # the reference is not there
    with pytest.raises(ImportError, match='unwrap_method="custom"'):
        texture.export_textured_mesh(mesh, pipeline, tmp_path, 4)  # the default is the reference's: xatlas
    monkeypatch.setattr(eval_render, "runner_for", lambda m, dev: None)
    with pytest.raises(RuntimeError, match="no CPU fallback|switched off"):
        texture.render_texture(model, mesh, 4)


# ---------------------------------------------------------------- the files -------------------------------------------------------
def read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        (n,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()  # filter 0 on every row
    return raw[:, 1:].reshape(H, W, 3)


def read_obj(path):
    rows = {"v": [], "vt": [], "vn": [], "f": []}
    head = []
    for line in open(path, encoding="utf-8").read().splitlines():
        key, _, rest = line.partition(" ")
        if key in rows:
            rows[key].append(rest.split())
        else:
            head.append(line)
    order = [line.split(" ", 1)[0] for line in open(path, encoding="utf-8").read().splitlines()[3:]]
    assert order == ["v"] * len(rows["v"]) + ["vt"] * len(rows["vt"]) + ["vn"] * len(rows["vn"]) + ["f"] * len(rows["f"])
    f = np.array([[[int(i) for i in corner.split("/")] for corner in row] for row in rows["f"]]) if rows["f"] else np.zeros((0, 3, 3), int)
    return head, np.array(rows["v"], float), np.array(rows["vt"], float), np.array(rows["vn"], float), f


def check_files(out, vertices, normals, faces, P, image=None):
    from nerfstudio_amd import texture

    F = len(faces)
    head, v, vt, vn, f = read_obj(out / "mesh.obj")
    assert head == ["# Generated with nerfstudio", "mtllib material_0.mtl", "usemtl material_0"]
    assert np.array_equal(v.astype(np.float32), vertices) and np.array_equal(vn.astype(np.float32), normals)  # nine digits read back exactly
    tc = tx.texture_coordinates(F, P).reshape(-1, 2)
    assert vt.shape == (3 * F, 2) and np.abs(vt - np.stack([tc[:, 0], 1 - tc[:, 1]], 1)).max() < 1e-7
    assert f.shape == (F, 3, 3) and np.array_equal(f[:, :, 0], faces + 1) and np.array_equal(f[:, :, 2], faces + 1)
    assert np.array_equal(f[:, :, 1], 3 * np.arange(F)[:, None] + np.arange(1, 4)[None])
    assert open(out / "material_0.mtl", encoding="utf-8").read().splitlines() == list(texture.MTL_LINES)
    assert texture.MTL_LINES[-1] == "map_Kd material_0.png" and texture.MTL_LINES[1] == "newmtl material_0"
    png = read_png(out / "material_0.png")
    sw, sh, W, H = tx.layout(F, P)
    assert png.shape == (H, W, 3) and (image is None or np.array_equal(png, image))
    return png


def test_export_textured_mesh_writes_files_that_parse_back(injected, monkeypatch, tmp_path):
    from nerfstudio_amd import eval_render, texture

    model = FakeModel().eval()
    runner = fake_runner(model)
    monkeypatch.setattr(eval_render, "runner_for", lambda m, dev: runner)
    monkeypatch.setitem(sys.modules, "nerfstudio", None)
    mesh = mesh_of(37)
    texture.export_textured_mesh(mesh, types.SimpleNamespace(device="cpu", model=model), tmp_path / "out", 4, unwrap_method="custom")
    raylen = float(np.float32(tx.raylen(mesh.vertices.numpy(), mesh.faces.numpy())))
    ref = tx.texel_rays(mesh.vertices.numpy(), mesh.normals.numpy(), mesh.faces.numpy(), 4, raylen)
    image = tx.levels(np.float32(0.5) + ref["origins"].astype(np.float32)).reshape(16, 35, 3)
    check_files(tmp_path / "out", mesh.vertices.numpy(), mesh.normals.numpy(), mesh.faces.numpy(), 4, image)
    rs = np.random.RandomState(0)
    for shape in ((1, 1, 3), (3, 5, 3), (64, 33, 3)):
        img = rs.randint(0, 256, shape).astype(np.uint8)
        texture.write_png(tmp_path / "a.png", T(img))
        assert np.array_equal(read_png(tmp_path / "a.png"), img)
    with pytest.raises(ValueError, match="uint8"):
        texture.write_png(tmp_path / "b.png", np.zeros((2, 2, 3), np.float32))


def test_textured_tsdf_export_keeps_the_ply_and_adds_the_three_files(injected, monkeypatch, tmp_path):
    import mesh_reference as mr
    import tsdf_reference as tr
    from test_mesh_cpu import read_mesh_ply
    from test_tsdf_cpu import same_size_cameras, stub_render
    from nerfstudio_amd import eval_render, export

    gt = load_golden("tsdf")
    count, emit = mr.restatement_launches()
    monkeypatch.setattr(export.F, "tsdf_integrate_launch", tr.fake_launch())
    monkeypatch.setattr(export.F, "mesh_count_launch", count)
    monkeypatch.setattr(export.F, "mesh_emit_launch", emit)
    for name in ("nerfstudio", "xatlas", "pymeshlab", "mediapy", "PIL"):
        monkeypatch.setitem(sys.modules, name, None)  # none of them is there
    model = FakeModel().train()
    runner = fake_runner(model)
    monkeypatch.setattr(eval_render, "runner_for", lambda m, dev: runner)
    outputs = types.SimpleNamespace(cameras=same_size_cameras(gt, 3), scene_box=types.SimpleNamespace(aabb=torch.tensor([[-2.0, -2, -2], [2, 2, 2]])))
    pipeline = types.SimpleNamespace(device="cpu", model=model, datamanager=types.SimpleNamespace(
        train_dataset=types.SimpleNamespace(_dataparser_outputs=outputs)))
    plain = tmp_path / "plain"
    plain.mkdir()
    assert export.export_tsdf_mesh_on_device(pipeline, plain, resolution=[9, 8, 7], batch_size=2, render_fn=stub_render([])) is None
    mesh = export.export_textured_tsdf_mesh_on_device(pipeline, tmp_path, px_per_uv_triangle=3, resolution=[9, 8, 7], batch_size=2,
                                                      render_fn=stub_render([]))
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["material_0.mtl", "material_0.png", "mesh.obj", "tsdf_mesh.ply"]
    assert open(tmp_path / "tsdf_mesh.ply", "rb").read() == open(plain / "tsdf_mesh.ply", "rb").read()  # the PLY is export_tsdf_mesh's
    vertex, face = read_mesh_ply(tmp_path / "tsdf_mesh.ply")
    assert len(face) == mesh.faces.shape[0] > 0 and model.training
    check_files(tmp_path, mesh.vertices.numpy(), mesh.normals.numpy(), mesh.faces.numpy(), 3)
    assert np.array_equal(face["i"], mesh.faces.numpy())


def test_module_imports_nothing_of_nerfstudio():
    src = open(os.path.join(ROOT, "nerfstudio_amd", "texture.py")).read()
    assert not re.findall(r"^(?:import|from)\s+(?:nerfstudio|PIL|mediapy|xatlas)\b", src, re.M)  # the xatlas path imports lazily


# ---------------------------------------------------------------- the entry points ------------------------------------------------
def test_entry_points_are_declared_bound_and_launched_from_one_place(tmp_path):
    from nerfstudio_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(nsamd_[a-z0-9_]+)\s*\(", header))) == sorted(N._TEXTURE_SIGNATURES) == NAMES
    others = (set(N._SIGNATURES) | set(N._EXPORT_SIGNATURES) | set(N._RENDER_SIGNATURES) | set(N._POINTCLOUD_SIGNATURES)
              | set(N._MESH_SIGNATURES))
    assert not set(N._TEXTURE_SIGNATURES) & others
    cdll = C.CDLL(N.LIB_PATH)
    lib = N.load()
    for name in NAMES:
        assert hasattr(cdll, name) and callable(getattr(lib, name))
    vp, i64 = N.vp, N.i64
    assert N._TEXTURE_SIGNATURES == {"nsamd_texel_rays": [N.TexelAtlasPod, vp, vp, vp, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp],
                                     "nsamd_mesh_raylen": [vp, i64, vp, i64, vp, vp, vp],
                                     "nsamd_texture_store": [vp, i64, i64, vp, vp]}
    assert C.sizeof(N.TexelAtlasPod) == 16
    text = open(HEADER).read()
    assert int(re.search(r"#define NSAMD_RAYLEN_MAX_BLOCKS\s+(\d+)", text).group(1)) * 8 == N.RAYLEN_SCRATCH_BYTES
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "nsamd_texture.h"\n'
                   "int main(void) {\n"
                   "  nsamd_texel_atlas atlas = {37, 4, 5, 4};\n"
                   "  nsamd_texel_atlas flat = {37, 1, 5, 4};\n"
                   "  nsamd_texel_atlas small = {37, 4, 3, 3};\n"
                   "  nsamd_texel_atlas wide = {37, 2147483000, 5, 4};\n"
                   "  static double scratch[NSAMD_RAYLEN_SCRATCH_BYTES / 8];\n"
                   "  float x[8];\n"
                   "  if (sizeof(atlas) != 16 || sizeof(scratch) != 8192) return 9;\n"
                   "  if (nsamd_texel_rays(atlas, NULL, NULL, NULL, 4, NULL, 0, 0, 0, NULL, NULL, NULL, NULL, NULL) != NSAMD_OK) return 1;\n"
                   "  if (nsamd_texel_rays(atlas, NULL, NULL, NULL, 4, NULL, 0, 4, 4, NULL, NULL, NULL, NULL, NULL) != NSAMD_ERR_INVALID_ARG) return 2;\n"
                   "  if (nsamd_texel_rays(flat, x, x, NULL, 4, x, 0, 1, 1, x, x, x, x, NULL) != NSAMD_ERR_INVALID_ARG) return 3;\n"
                   "  if (nsamd_texel_rays(small, x, x, NULL, 4, x, 0, 1, 1, x, x, x, x, NULL) != NSAMD_ERR_INVALID_ARG) return 4;\n"
                   "  if (nsamd_texel_rays(wide, x, x, NULL, 4, x, 0, 1, 1, x, x, x, x, NULL) != NSAMD_ERR_UNSUPPORTED) return 5;\n"
                   "  if (nsamd_mesh_raylen(x, 2, NULL, 0, scratch, x, NULL) != NSAMD_ERR_INVALID_ARG) return 6;\n"
                   "  if (nsamd_texture_store(NULL, 0, 0, NULL, NULL) != NSAMD_OK) return 7;\n"
                   "  if (nsamd_texture_store(x, -1, 0, (uint8_t*)x, NULL) != NSAMD_ERR_INVALID_ARG) return 8;\n"
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
    assert " texture.hip" in makefile and " texture.h " in makefile and "nsamd_texture.h" in makefile
    assert "nsamd_tex" not in open(os.path.join(ROOT, "include", "nsamd_mesh.h")).read()  # that header keeps its two entry points


def test_entry_points_validate_before_they_launch(host):
    """No call here reaches a launch: every one fails a check or has nothing to do (the pointers are host memory). The host
    build answers the same."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    p = torch.zeros(4096, dtype=torch.int64).data_ptr()
    atlas = N.make_texel_atlas(37, 4, 5, 4)  # 35 x 16 = 560 texels

    def variants(rays, raylen, store, stream):
        def r(atlas=atlas, vertices=p, normals=p, faces=p, V=8, rl=p, first=0, count=4, rows=4, o=p, d=p, nr=p, fr=p):
            return rays(atlas, vertices, normals, faces, V, rl, first, count, rows, o, d, nr, fr, *stream)

        assert r(count=0, rows=0, vertices=None, o=None) == 0
        for bad in (dict(vertices=None), dict(normals=None), dict(faces=None), dict(rl=None), dict(o=None), dict(d=None), dict(nr=None),
                    dict(fr=None), dict(V=0), dict(first=-1), dict(count=0), dict(count=5), dict(first=557), dict(first=560, count=1, rows=1),
                    dict(count=561, rows=561), dict(atlas=N.make_texel_atlas(0, 4, 5, 4)), dict(atlas=N.make_texel_atlas(37, 1, 5, 4)),
                    dict(atlas=N.make_texel_atlas(37, 4, 0, 4)), dict(atlas=N.make_texel_atlas(37, 4, 6, 3))):
            assert r(**bad) == -1, bad
        assert r(atlas=N.make_texel_atlas(37, 2 ** 31 - 4, 5, 4)) == -2
        for bad in (dict(V=0), dict(T=0), dict(T=2 ** 31), dict(vertices=None), dict(faces=None), dict(scratch=None), dict(out=None)):
            a = dict(vertices=p, V=8, faces=p, T=4, scratch=p, out=p)
            a.update(bad)
            assert raylen(a["vertices"], a["V"], a["faces"], a["T"], a["scratch"], a["out"], *stream) == -1, bad
        assert store(None, 0, 0, None, *stream) == 0
        for bad in ((None, 1, 0, p), (p, 1, 0, None), (p, -1, 0, p), (p, 2 ** 31, 0, p), (p, 1, -1, p)):
            assert store(*bad, *stream) == -1, bad

    variants(lib.nsamd_texel_rays, lib.nsamd_mesh_raylen, lib.nsamd_texture_store, (None,))
    hl = host[0].lib
    variants(hl.hc_texel_rays, hl.hc_mesh_raylen, hl.hc_texture_store, ())
    with pytest.raises(RuntimeError, match="status -1"):
        N.check(lib.nsamd_mesh_raylen(p, 8, p, 0, p, p, None), "mesh_raylen")
