"""CPU tests of the mesh extraction (include/nsamd_mesh.h, nerfstudio_amd/export.py: TSDFVolume.get_mesh, write_mesh_ply,
export_tsdf_mesh_on_device): the generated triangle table against its generator and its own invariants, the float64
restatement (tests/mesh_reference.py) against the invariants of a closed surface, the arithmetic of nerfstudio_amd/csrc/mesh.h
compiled for the host (tests/hostcheck/mesh_helpers.cc) and looped as the kernels compose it, the same build under the address
and undefined-behaviour sanitizers as a stand-alone program, the Python layer over launches served by the restatement, and the ABI.

Bounds (mesh_reference.compare): faces, counts and colours exact; positions within 4 fp32 ulp of the largest coordinate
magnitude; normals within 1e-4 per component where the index-space gradient norm is at least 1e-2; vertices with
|t - 0.5| < 1e-5 are left out of the colour comparison — except those whose t is exactly 0.5 in fp32 and in float64, which
round alike in both (clamped white noise has a tenth of its vertices between a +1 and a -1 voxel) — and a test fails when
either exclusion exceeds 5 % of the vertices.

On the closedness of white noise. A surface that crosses the border of the volume is open there, so "every directed edge
occurs as often as its reverse" is asserted (a) on the raw (20,13,11) noise for every edge that does not lie in a boundary
face of the volume, and (b) for EVERY edge on the same noise inside a border of -1 voxels, which closes the surface."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_reference as mr

T = torch.from_numpy
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")
HEADER = os.path.join(ROOT, "include", "nsamd_mesh.h")
NAMES = ["nsamd_mesh_count", "nsamd_mesh_emit"]
ORIGIN, VOXEL = [0.5, -1.25, 2.0], [0.1, 0.2, 0.15]  # non-zero, anisotropic
SEEDS = (0, 1, 2)


# ---------------------------------------------------------------- the table ------------------------------------------------------
def test_generator_reproduces_the_committed_table():
    committed = open(os.path.join(ROOT, "nerfstudio_amd", "csrc", "mesh_table.h")).read()
    assert committed == mr.gen.header_text()
    numbers = [int(x) for x in re.findall(r"\b\d+(?=,)", committed.split("{", 1)[1])]
    assert np.array_equal(np.array(numbers, np.uint8).reshape(256, 16), mr.TABLE)


def test_table_cases_close_and_complement():
    table = mr.gen.triangle_table()
    assert sum(len(t) for t in table) == 820 and max(len(t) for t in table) == 5
    assert table[0] == [] and table[255] == []
    for case in range(256):
        loops = mr.gen.case_loops(case)  # asserts that every crossed edge is the head of one segment and the tail of one
        crossed = sorted(e for e in range(12) if ((case >> mr.gen.edge_corners(e)[0]) ^ (case >> mr.gen.edge_corners(e)[1])) & 1)
        assert sorted(e for loop in loops for e in loop) == crossed and all(3 <= len(loop) <= 7 for loop in loops)
        assert sorted({e for tri in table[case] for e in tri}) == crossed
        assert sorted({e for tri in table[255 - case] for e in tri}) == crossed  # the complement cuts the same edges
        assert len(table[case]) == sum(len(loop) - 2 for loop in loops)
        # inside one cell every directed edge of the triangles that is not a loop's own segment meets its reverse
        directed = [(t[i], t[(i + 1) % 3]) for t in table[case] for i in range(3)]
        segments = {(a, b) for a, b in mr.gen.case_segments(case)} | {(b, a) for a, b in mr.gen.case_segments(case)}
        inner = [d for d in directed if d not in segments]
        assert sorted(inner) == sorted((b, a) for a, b in inner)
    # winding: the single negative corner c is cut off by a triangle whose normal points away from it
    for c in range(8):
        (tri,) = table[1 << c]
        mid = [0.5 * (np.array(mr.gen.corner_xyz(mr.gen.edge_corners(e)[0])) + np.array(mr.gen.corner_xyz(mr.gen.edge_corners(e)[1])))
               for e in tri]
        normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
        assert normal @ (np.mean(mid, 0) - np.array(mr.gen.corner_xyz(c))) > 0


# ---------------------------------------------------------------- the restatement alone ------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """name -> (values, colors, restatement): computed once, never written to"""
    out = {}

    def add(name, values, origin=ORIGIN, voxel=VOXEL):
        colors = mr.noise_colors(len(out), values.shape)
        for a in (values, colors):
            a.setflags(write=False)
        out[name] = (values, colors, mr.extract(values, colors, origin, voxel), origin, voxel)

    for seed in SEEDS:
        add(f"noise{seed}", mr.noise_volume(seed))
        add(f"padded{seed}", np.pad(mr.noise_volume(seed), 1, constant_values=-1.0))
    add("sphere", mr.sphere_volume()[0], [0, 0, 0], [1, 1, 1])
    add("smooth", mr.smooth_volume(), [0, 0, 0], [1, 1, 1])
    for name, values in mr.degenerate_volumes().items():
        add(name, values)
    for shape in ((5, 3, 17), (4, 4, 16), (1, 1, 257), (2, 2, 2), (2, 130, 2)):
        add("x".join(map(str, shape)), np.random.default_rng(7).standard_normal(shape).astype(np.float32))
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_white_noise_meets_every_case_and_closes(refs, seed):
    values, _, ref, _, _ = refs[f"noise{seed}"]
    neg = mr.clamp32(values) < 0
    cases = sum(neg[dx:19 + dx, dy:12 + dy, dz:10 + dz].astype(int) << (dx + 2 * dy + 4 * dz)
                for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    assert len(np.unique(cases)) == 256
    V = len(ref["vertices"])
    assert ref["kept"].all() and V == len(np.unique(ref["faces"]))  # no exact zero: nothing dropped, no vertex unreferenced
    inner = mr.interior_faces_edges(ref, values.shape)
    print(f"noise {seed}: {len(inner)} of {3 * len(ref['faces'])} directed edges off the volume's border")
    assert 0.5 * 3 * len(ref["faces"]) < len(inner) < 3 * len(ref["faces"])
    assert mr.edges_balanced(inner, V)
    padded = refs[f"padded{seed}"][2]
    assert len(padded["faces"]) > len(ref["faces"]) and mr.directed_edge_balance(padded["faces"])


def test_sphere_is_a_closed_manifold_that_faces_outward(refs):
    _, _, ref, _, _ = refs["sphere"]
    centre, R = np.full(3, 7.5), 5.2
    assert mr.strictly_manifold(ref["faces"]) and mr.euler_characteristic(ref["faces"]) == 2
    volume = mr.signed_volume(ref["vertices"], ref["faces"])
    assert 0.95 < volume / (4 / 3 * np.pi * R ** 3) < 1.0  # positive: normals out of the surface; chords lie inside the ball
    radial = ref["vertices"] - centre
    assert (np.einsum("ij,ij->i", radial, ref["normals"]) > 0).all()
    h = 1.0
    error = float(np.abs(np.linalg.norm(radial, axis=1) - R).max())
    print(f"sphere: radius error {error:.4f}, bound {h * h / (2 * (R - 2 * h)):.4f}")
    assert error <= h * h / (2 * (R - 2 * h))
    p = ref["vertices"][ref["faces"]]
    face_normals = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", face_normals, p.mean(1) - centre) > 0).all()  # the winding agrees with the vertex normals


def test_smooth_volume_is_strictly_manifold(refs):
    _, _, ref, _, _ = refs["smooth"]
    assert len(ref["faces"]) > 1000 and mr.strictly_manifold(ref["faces"])


# ---------------------------------------------------------------- mesh.h on the host ---------------------------------------------
def _ptr(t):
    if t is None:
        return None
    assert t.is_contiguous()
    return t.data_ptr()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """(count, emit) with the arguments of functional.mesh_count_launch / mesh_emit_launch, served by the host build of mesh.h"""
    from nerfstudio_amd import _native as N

    out = str(tmp_path_factory.mktemp("hostcheck") / "libmeshcheck.so")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(HOSTCHECK, "mesh_helpers.cc")], check=True)
    lib = C.CDLL(out)
    for name, argtypes in N._MESH_SIGNATURES.items():
        getattr(lib, name.replace("nsamd_", "hc_")).argtypes = argtypes[:-1]  # no stream

    def count(vol, values, scratch, totals):
        assert scratch.numel() >= N.mesh_scratch_bytes(values.numel()) and scratch.data_ptr() % 8 == 0
        assert lib.hc_mesh_count(vol, _ptr(values), _ptr(scratch), _ptr(totals)) == 0

    def emit(vol, values, colors, scratch, vertices, normals, vertex_colors, faces):
        assert lib.hc_mesh_emit(vol, _ptr(values), _ptr(colors), _ptr(scratch), vertices.shape[0], faces.shape[0], _ptr(vertices),
                                _ptr(normals), _ptr(vertex_colors), _ptr(faces)) == 0

    count.lib = lib
    return count, emit


def volume_of(values, colors, origin, voxel):
    from nerfstudio_amd.export import TSDFVolume

    return TSDFVolume(T(values.copy()), torch.zeros(values.shape), T(colors.copy()), torch.tensor(origin), torch.tensor(voxel))


def mesh_arrays(mesh):
    return dict(vertices=mesh.vertices.cpu().numpy(), normals=mesh.normals.cpu().numpy(), colors=mesh.colors.cpu().numpy(),
                faces=mesh.faces.cpu().numpy())


NAMES_COMPARED = [f"noise{s}" for s in SEEDS] + [f"padded{s}" for s in SEEDS] + ["sphere", "smooth", "5x3x17", "4x4x16", "1x1x257",
                                                                                 "2x2x2", "2x130x2"]


@pytest.mark.parametrize("name", NAMES_COMPARED)
def test_host_build_matches_the_restatement(refs, host, name):
    values, colors, ref, origin, voxel = refs[name]
    got = mesh_arrays(volume_of(values, colors, origin, voxel).get_mesh(launch_fns=host))
    if name == "1x1x257":
        assert len(ref["vertices"]) == 0 and len(ref["faces"]) == 0  # a dimension below 2
    else:
        assert len(ref["faces"]) > 0
    mr.compare(got, ref, f"host {name}")


@pytest.mark.parametrize("name", sorted(mr.degenerate_volumes()))
def test_degenerate_triangles_are_exactly_those_the_predicate_names(refs, host, name):
    values, colors, ref, origin, voxel = refs[name]
    got = mesh_arrays(volume_of(values, colors, origin, voxel).get_mesh(launch_fns=host))
    mr.compare(got, ref, f"host {name}")
    # independently of t: on these volumes a snapped vertex sits exactly on a lattice point in float64 too, so the dropped
    # triangles are those with two equal float64 index positions
    pos = ref["index_positions"][ref["candidates"]]
    coincide = ((pos[:, 0] == pos[:, 1]).all(1) | (pos[:, 0] == pos[:, 2]).all(1) | (pos[:, 1] == pos[:, 2]).all(1))
    assert np.array_equal(~coincide, ref["kept"])
    expected_dropped = {"zero_corner": 8, "tiny_negative": 8, "zero_sea": 0, "zero_pair": 16}[name]
    assert int((~ref["kept"]).sum()) == expected_dropped
    tri = got["vertices"][got["faces"]]  # no emitted triangle has two bitwise-equal positions
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not (tri[:, a].view(np.uint32) == tri[:, b].view(np.uint32)).all(1).any()
    if name == "tiny_negative":
        assert ((ref["t32"] == 1) & (values[tuple((ref["owner"] + np.eye(3, dtype=int)[ref["axis"]]).T)] != 0)).any()  # t == 1, v1 != 0
    if name == "zero_corner":  # (its surface stays off the volume's border)
        assert mr.directed_edge_balance(ref["candidates"])  # closed before the rule; the slivers take their edges with them


@pytest.mark.parametrize("name", ["noise1", "zero_corner", "5x3x17"])
def test_host_build_is_clean_under_the_sanitizers(refs, tmp_path, name):
    """a stand-alone program with the sanitizers' runtimes linked in statically: it runs in the environment it inherits, as it
    is, and nothing of it runs inside python"""
    exe = str(tmp_path / "mesh_main")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HOSTCHECK, "mesh_main.cc"),
                    os.path.join(HOSTCHECK, "mesh_helpers.cc")], check=True)
    values, _, ref, _, _ = refs[name]
    path = tmp_path / "values.f32"
    values.tofile(path)
    run = subprocess.run([exe, str(path)] + [str(d) for d in values.shape], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.strip() == f"vertices {len(ref['vertices'])} triangles {len(ref['faces'])}"


# ---------------------------------------------------------------- the Python layer ------------------------------------------------
def read_mesh_ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    V = int(lines[2].split()[-1])
    assert lines[2].startswith("element vertex ")
    kinds = {"float": "<f4", "uchar": "u1"}
    props = lines[3:13]
    vertex = np.dtype([(ln.split()[2], kinds[ln.split()[1]]) for ln in props])
    assert lines[13].startswith("element face ") and lines[14:] == ["property list uchar int vertex_indices"]
    F = int(lines[13].split()[-1])
    face = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(body) == V * vertex.itemsize + F * face.itemsize
    return np.frombuffer(body[:V * vertex.itemsize], dtype=vertex), np.frombuffer(body[V * vertex.itemsize:], dtype=face)


def test_get_mesh_over_injected_launches_and_the_empty_mesh(refs):
    from nerfstudio_amd import export

    values, colors, ref, origin, voxel = refs["noise0"]
    mesh = volume_of(values, colors, origin, voxel).get_mesh(launch_fns=mr.restatement_launches())
    assert isinstance(mesh, export.Mesh) and [f for f in mesh.__dataclass_fields__] == ["vertices", "faces", "normals", "colors"]
    V, F = len(ref["vertices"]), len(ref["faces"])
    assert tuple(mesh.vertices.shape) == tuple(mesh.normals.shape) == tuple(mesh.colors.shape) == (V, 3) and tuple(mesh.faces.shape) == (F, 3)
    assert mesh.vertices.dtype == mesh.normals.dtype == mesh.colors.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert np.array_equal(mesh.faces.numpy(), ref["faces"]) and np.array_equal(mesh.colors.numpy(), ref["colors"])
    for fill in (1.0, -1.0):
        vol = export.TSDFVolume.from_aabb([[-1.0, -1, -1], [1, 1, 1]], [4, 3, 5])
        vol.values.fill_(fill)
        empty = vol.get_mesh(launch_fns=mr.restatement_launches())
        assert tuple(empty.vertices.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 3) and empty.faces.dtype == torch.int32
    assert export.TSDFVolume.from_aabb([[-1.0, -1, -1], [1, 1, 1]], [4, 3, 5]).get_mesh(mr.restatement_launches()).faces.shape[0] == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the native launches refuse host tensors
        volume_of(values, colors, origin, voxel).get_mesh()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        export.device_mesh(volume_of(values, colors, origin, voxel))


def test_write_mesh_ply_reads_back(refs, tmp_path):
    from nerfstudio_amd import export

    values, colors, ref, origin, voxel = refs["zero_corner"]
    mesh = volume_of(values, colors, origin, voxel).get_mesh(launch_fns=mr.restatement_launches())
    mesh.colors[0] = torch.tensor([0.0, 1.0, 0.999])
    mesh.colors[1] = torch.tensor([1.7, -0.2, float("nan")])
    mesh.colors[2] = T((np.array([1, 128, 254]) / 255).astype(np.float32))  # level boundaries
    export.write_mesh_ply(mesh, tmp_path / "a.ply")
    vertex, face = read_mesh_ply(tmp_path / "a.ply")
    assert vertex.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "alpha") and vertex.dtype.itemsize == 28
    assert np.array_equal(np.stack([vertex[k] for k in ("x", "y", "z")], 1), mesh.vertices.numpy())
    assert np.array_equal(np.stack([vertex[k] for k in ("nx", "ny", "nz")], 1), mesh.normals.numpy())
    rgb = np.stack([vertex[k] for k in ("red", "green", "blue")], 1)
    assert rgb[0].tolist() == [0, 255, 254] and rgb[1].tolist() == [255, 0, 0] and (vertex["alpha"] == 255).all()
    assert np.array_equal(rgb[2:], (mesh.colors[2:].numpy().astype(np.float64) * 255).astype(np.uint8))
    assert (face["n"] == 3).all() and np.array_equal(face["i"], mesh.faces.numpy()) and face.dtype.itemsize == 13
    empty = export.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3), torch.zeros(0, 3))
    export.write_mesh_ply(empty, str(tmp_path / "empty.ply"))
    vertex, face = read_mesh_ply(tmp_path / "empty.ply")
    assert len(vertex) == 0 and len(face) == 0


def test_export_on_device_meshes_refines_and_writes_without_the_reference(tmp_path, monkeypatch):
    import inspect

    import tsdf_reference as tr
    from test_tsdf_cpu import _Model, same_size_cameras, stub_render
    from conftest import load_golden
    from nerfstudio_amd import export

    g = load_golden("tsdf")
    count, emit = mr.restatement_launches()
    monkeypatch.setattr(export.F, "tsdf_integrate_launch", tr.fake_launch())
    monkeypatch.setattr(export.F, "mesh_count_launch", count)
    monkeypatch.setattr(export.F, "mesh_emit_launch", emit)
    monkeypatch.setitem(sys.modules, "nerfstudio.exporter", None)  # the reference is not there
    cams = same_size_cameras(g, 3)
    outputs = types.SimpleNamespace(cameras=cams, scene_box=types.SimpleNamespace(aabb=torch.tensor([[-2.0, -2, -2], [2, 2, 2]])))
    pipeline = types.SimpleNamespace(device="cpu", model=_Model().train(), datamanager=types.SimpleNamespace(
        train_dataset=types.SimpleNamespace(_dataparser_outputs=outputs)))
    volumes, calls = [], []

    def recording_mesh(volume):
        volumes.append(volume)
        return export.device_mesh(volume)

    export.export_tsdf_mesh_on_device(pipeline, tmp_path, resolution=[9, 8, 7], batch_size=2, render_fn=stub_render(calls),
                                      mesh_fn=recording_mesh, refine_mesh_using_initial_aabb_estimate=True, refinement_epsilon=0.25)
    assert len(volumes) == 2 and len(calls) == 6  # the refinement renders, fuses and meshes again
    first = mr.extract(volumes[0].values.numpy(), volumes[0].colors.numpy(), volumes[0].origin.numpy(), volumes[0].voxel_size.numpy())
    assert len(first["faces"]) > 0
    lo, hi = first["vertices"].min(0) - 0.25, first["vertices"].max(0) + 0.25
    assert np.allclose(volumes[1].origin.numpy(), lo, atol=1e-6)
    assert np.allclose(volumes[1].voxel_size.numpy(), (hi - lo) / np.array([9, 8, 7]), atol=1e-6)
    second = mr.extract(volumes[1].values.numpy(), volumes[1].colors.numpy(), volumes[1].origin.numpy(), volumes[1].voxel_size.numpy())
    vertex, face = read_mesh_ply(tmp_path / "tsdf_mesh.ply")
    assert len(vertex) == len(second["vertices"]) > 0 and np.array_equal(face["i"], second["faces"])
    assert np.array_equal(np.stack([vertex[k] for k in ("x", "y", "z")], 1), second["vertices"].astype(np.float32))
    # both defaults of the wrapper are the device's; mesh_fn=None / write_fn=None of export_tsdf_mesh still reach the reference
    export.export_tsdf_mesh_on_device(pipeline, tmp_path / "missing", resolution=4, render_fn=stub_render([]),
                                      write_fn=lambda mesh, filename: calls.append(filename))
    assert calls[-1] == str(tmp_path / "missing" / "tsdf_mesh.ply")
    with pytest.raises(ImportError, match="nerfstudio"):
        export.export_tsdf_mesh(pipeline, tmp_path, resolution=4, render_fn=stub_render([]), mesh_fn=None)
    with pytest.raises(ImportError, match="nerfstudio"):
        export.export_tsdf_mesh(pipeline, tmp_path, resolution=4, render_fn=stub_render([]), mesh_fn=export.device_mesh)
    params = inspect.signature(export.export_tsdf_mesh).parameters
    assert [params[k].default for k in ("render_fn", "mesh_fn", "write_fn")] == [None, None, None]
    assert export._reference_mesh is not export.device_mesh and export._reference_write is not export.write_mesh_ply


def test_module_imports_nothing_of_nerfstudio():
    src = open(os.path.join(ROOT, "nerfstudio_amd", "export.py")).read()
    assert not re.findall(r"^(?:import|from)\s+nerfstudio\b", src, re.M)  # at module level; the reference path imports it lazily


# ---------------------------------------------------------------- the entry points ------------------------------------------------
def test_entry_points_are_declared_bound_and_launched_from_one_place(tmp_path):
    from nerfstudio_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(nsamd_[a-z0-9_]+)\s*\(", header))) == sorted(N._MESH_SIGNATURES) == NAMES
    others = set(N._SIGNATURES) | set(N._EXPORT_SIGNATURES) | set(N._RENDER_SIGNATURES) | set(N._POINTCLOUD_SIGNATURES)
    assert not set(N._MESH_SIGNATURES) & others
    cdll = C.CDLL(N.LIB_PATH)
    lib = N.load()
    for name in NAMES:
        assert hasattr(cdll, name) and callable(getattr(lib, name))
    vp, i64 = N.vp, N.i64
    assert N._MESH_SIGNATURES == {"nsamd_mesh_count": [N.MeshVolume, vp, vp, vp, vp],
                                  "nsamd_mesh_emit": [N.MeshVolume, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp]}
    assert C.sizeof(N.MeshVolume) == 36
    assert N.MESH_BLOCK == int(re.search(r"#define NSAMD_MESH_BLOCK\s+(\d+)", open(HEADER).read()).group(1)) == 256
    for n in (0, 1, 256, 257, 513, 256 ** 3):
        assert N.mesh_scratch_bytes(n) == 16 + 8 * ((n + 255) // 256) + 4 * n
    assert N.mesh_scratch_bytes(256 ** 3) <= 4 * 256 ** 3 + 8 * 65536 + 16  # 4 bytes per voxel plus the per-workgroup words
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "nsamd_mesh.h"\n'
                   "int main(void) {\n"
                   "  nsamd_mesh_volume vol = {{0, 0, 0}, {1, 1, 1}, {4, 4, 16}};\n"
                   "  nsamd_mesh_volume big = {{0, 0, 0}, {1, 1, 1}, {2048, 2048, 512}};\n"
                   "  static int64_t words[(NSAMD_MESH_SCRATCH_BYTES(256) + 7) / 8];\n"
                   "  int64_t totals[2];\n"
                   "  if (sizeof(words) != 16 + 8 + 1024) return 9;\n"
                   "  if (NSAMD_MESH_SCRATCH_BYTES(257) != 16 + 16 + 1028) return 10;\n"
                   "  if (nsamd_mesh_count(vol, NULL, words, totals, NULL) != NSAMD_ERR_INVALID_ARG) return 1;\n"
                   "  if (nsamd_mesh_count(big, NULL, words, totals, NULL) != NSAMD_ERR_UNSUPPORTED) return 2;\n"
                   "  if (nsamd_mesh_emit(vol, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL) != NSAMD_OK) return 3;\n"
                   "  if (nsamd_mesh_emit(vol, NULL, NULL, NULL, 3 * 256 + 1, 0, NULL, NULL, NULL, NULL, NULL) != NSAMD_ERR_INVALID_ARG)"
                   " return 4;\n"
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
    assert " mesh.hip" in makefile and " mesh.h " in makefile and " mesh_table.h " in makefile and "nsamd_mesh.h" in makefile
    export_header = open(os.path.join(ROOT, "include", "nsamd_export.h")).read()
    assert "nsamd_mesh" not in export_header  # that header keeps its one entry point


def test_entry_points_validate_before_they_launch(host):
    """No call here reaches a launch: every one fails a check or has nothing to do (the pointers are host memory). The host
    build answers the same."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    p = torch.zeros(4096, dtype=torch.int64).data_ptr()
    vol = N.make_mesh_volume([0, 0, 0], [1, 1, 1], [4, 4, 16])

    def variants(count, emit, stream):
        def c(vol=vol, values=p, scratch=p, totals=p):
            return count(vol, values, scratch, totals, *stream)

        def e(vol=vol, values=p, colors=p, scratch=p, V=4, T=4, vertices=p, normals=p, vcolors=p, faces=p):
            return emit(vol, values, colors, scratch, V, T, vertices, normals, vcolors, faces, *stream)

        for bad in (dict(values=None), dict(scratch=None), dict(totals=None), dict(vol=N.make_mesh_volume([0, 0, 0], [1, 1, 1], [4, -1, 4])),
                    dict(vol=N.make_mesh_volume([0, 0, 0], [1, 0, 1], [4, 4, 4])),
                    dict(vol=N.make_mesh_volume([0, float("nan"), 0], [1, 1, 1], [4, 4, 4]))):
            assert c(**bad) == -1, bad
        assert c(vol=N.make_mesh_volume([0, 0, 0], [1, 1, 1], [2048, 2048, 512])) == -2  # 2^31 voxels
        assert c(vol=N.make_mesh_volume([0, 0, 0], [1, 1, 1], [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1])) == -2
        assert e(V=0, T=0, values=None, colors=None, scratch=None, vertices=None, faces=None) == 0
        for bad in (dict(V=-1), dict(T=-1), dict(V=3 * 256 + 1), dict(T=5 * 256 + 1), dict(values=None), dict(colors=None),
                    dict(scratch=None), dict(vertices=None), dict(normals=None), dict(vcolors=None), dict(faces=None),
                    dict(vol=N.make_mesh_volume([0, 0, 0], [1, 1, 1], [1, 1, 257]), V=1, T=0)):
            assert e(**bad) == -1, bad

    variants(lib.nsamd_mesh_count, lib.nsamd_mesh_emit, (None,))
    variants(host[0].lib.hc_mesh_count, host[0].lib.hc_mesh_emit, ())
    big = N.make_mesh_volume([0, 0, 0], [1, 1, 1], [1290, 1290, 1290])  # 2.1e9 voxels: V = 2^31 is within 3 n, not within int32
    assert lib.nsamd_mesh_emit(big, p, p, p, 2 ** 31, 4, p, p, p, p, None) == -2
    with pytest.raises(RuntimeError, match="status -2"):
        N.check(lib.nsamd_mesh_count(N.make_mesh_volume([0, 0, 0], [1, 1, 1], [2048, 2048, 512]), p, p, p, None), "mesh_count")
