"""GPU tests of nsamd_mesh_count / nsamd_mesh_emit (csrc/mesh.hip over csrc/mesh.h) and export.TSDFVolume.get_mesh against the
float64 restatement of tests/mesh_reference.py, under the bounds of mesh_reference.compare (tests/test_mesh_cpu.py states them):
faces, counts and colours exact, positions within 4 fp32 ulp of the largest coordinate magnitude, normals within 1e-4 where the
index-space gradient norm is at least 1e-2, at most 5 % of the vertices excluded. Every comparison prints its figures before
it asserts."""
import numpy as np
import pytest
import torch

import mesh_reference as mr
import tsdf_reference as tr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
ORIGIN, VOXEL = [0.5, -1.25, 2.0], [0.1, 0.2, 0.15]  # non-zero, anisotropic
POISON, GUARD = -77.0, 512


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    info = _native.device_info()
    assert info["wavefront_size"] == 64 and info["arch"].startswith("gfx950"), info
    return functional


def volume_of(values, colors, origin=ORIGIN, voxel=VOXEL):
    from nerfstudio_amd.export import TSDFVolume

    return TSDFVolume(T(values.copy()).cuda(), torch.zeros(values.shape, device="cuda"), T(colors.copy()).cuda(),
                      torch.tensor(origin), torch.tensor(voxel))


def mesh_arrays(mesh):
    return dict(vertices=mesh.vertices.cpu().numpy(), normals=mesh.normals.cpu().numpy(), colors=mesh.colors.cpu().numpy(),
                faces=mesh.faces.cpu().numpy())


def check(values, label, origin=ORIGIN, voxel=VOXEL, seed=0):
    colors = mr.noise_colors(seed, values.shape)
    ref = mr.extract(values, colors, origin, voxel)
    got = mesh_arrays(volume_of(values, colors, origin, voxel).get_mesh())
    mr.compare(got, ref, f"gpu {label}")
    return got, ref


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_white_noise_against_the_restatement(F, seed):
    got, ref = check(mr.noise_volume(seed), f"noise{seed}", seed=seed)
    assert len(ref["faces"]) > 7000


# 255, 256 and 257 voxels: one lane short of a workgroup, exactly one, one lane more (a dimension below 2: nothing to mesh);
# 513 voxels in three workgroups; (41,41,40): 263 workgroups, the scan of their sums takes a second sweep of its workgroup
@pytest.mark.parametrize("shape", [(5, 3, 17), (4, 4, 16), (1, 1, 257), (3, 9, 19), (41, 41, 40)])
def test_workgroup_and_scan_edges(F, shape):
    values = np.random.default_rng(7).standard_normal(shape).astype(np.float32)
    got, ref = check(values, "x".join(map(str, shape)))
    if shape == (1, 1, 257):
        assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)
    else:
        assert len(ref["faces"]) > 100
    if shape == (41, 41, 40):
        assert -(-values.size // 256) == 263


def test_surfaces_cross_every_face_of_the_volume(F):
    i, j, k = np.meshgrid(np.arange(9), np.arange(7), np.arange(6), indexing="ij")
    values = (((i + 2 * j + 3 * k) % 5) - 1.75).astype(np.float32) / 3
    got, ref = check(values, "stripes")
    dims = np.array(values.shape)
    for b in range(3):  # vertices owned by voxels of the first and of the last slab of every axis, on edges along the other axes
        for side in (0, dims[b] - 1):
            assert ((ref["owner"][:, b] == side) & (ref["axis"] != b)).sum() > 5, (b, side)
    referenced = np.unique(got["faces"])
    assert len(referenced) == len(ref["vertices"])  # the last slabs' vertices are used by the cells below them


def guarded(numel, dtype, fill):
    slab = torch.full((GUARD + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return slab, slab[GUARD:GUARD + numel]


def intact(slab, numel, fill):
    return bool((slab[:GUARD] == fill).all()) and bool((slab[GUARD + numel:] == fill).all())


@pytest.mark.parametrize("case", ["noise", "plus", "minus", "thin"])
def test_guard_rows_stay_intact_and_runs_repeat_bit_for_bit(F, case):
    from nerfstudio_amd import _native as N

    shape = (1, 1, 257) if case == "thin" else (5, 3, 17)
    values = {"noise": mr.noise_volume(3, shape), "thin": mr.noise_volume(3, shape), "plus": np.ones(shape, np.float32),
              "minus": -np.ones(shape, np.float32)}[case]
    colors = mr.noise_colors(3, shape)
    ref = mr.extract(values, colors, ORIGIN, VOXEL)
    V, Tn = len(ref["vertices"]), len(ref["faces"])
    assert (V > 0) == (case == "noise")
    vol = N.make_mesh_volume(ORIGIN, VOXEL, shape)
    v, c = T(values).cuda(), T(colors).cuda()
    nbytes = N.mesh_scratch_bytes(values.size)
    runs = []
    for _ in range(2):
        scratch_slab, scratch = guarded(nbytes, torch.uint8, 0xAB)
        totals_slab, totals = guarded(2, torch.int64, -5)
        F.mesh_count_launch(vol, v, scratch, totals)
        assert totals.tolist() == [V, Tn]
        slabs = [guarded(3 * V, torch.float32, POISON) for _ in range(3)] + [guarded(3 * Tn, torch.int32, -7)]
        outs = [s[1].view(s[1].numel() // 3, 3) for s in slabs]
        F.mesh_emit_launch(vol, v, c, scratch, *outs)
        torch.cuda.synchronize()
        assert intact(scratch_slab, nbytes, 0xAB) and intact(totals_slab, 2, -5)
        for (slab, _), fill, n in zip(slabs, (POISON, POISON, POISON, -7), (3 * V, 3 * V, 3 * V, 3 * Tn)):
            assert intact(slab, n, fill)
        runs.append([o.clone() for o in outs] + [scratch.clone()])
        if V > 1:  # totals that are not the count's: nothing is written
            wrong = [guarded(3 * (V - 1), torch.float32, POISON) for _ in range(3)] + [guarded(3 * Tn, torch.int32, -7)]
            F.mesh_emit_launch(vol, v, c, scratch, *[s[1].view(s[1].numel() // 3, 3) for s in wrong])
            torch.cuda.synchronize()
            assert all(bool((s[0] == fill).all()) for s, fill in zip(wrong, (POISON, POISON, POISON, -7)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    got = dict(vertices=runs[0][0].cpu().numpy(), normals=runs[0][1].cpu().numpy(), colors=runs[0][2].cpu().numpy(),
               faces=runs[0][3].cpu().numpy())
    mr.compare(got, ref, f"gpu guarded {case}")


def test_sphere_on_the_device_is_a_closed_manifold_that_faces_outward(F):
    values, centre = mr.sphere_volume()
    got, ref = check(values, "sphere", [0, 0, 0], [1, 1, 1])
    R = 5.2
    vertices, faces, normals = got["vertices"].astype(np.float64), got["faces"], got["normals"].astype(np.float64)
    assert mr.strictly_manifold(faces) and mr.euler_characteristic(faces) == 2
    assert 0.95 < mr.signed_volume(vertices, faces) / (4 / 3 * np.pi * R ** 3) < 1.0
    radial = vertices - centre
    assert (np.einsum("ij,ij->i", radial, normals) > 0).all()
    assert float(np.abs(np.linalg.norm(radial, axis=1) - R).max()) <= 1.0 / (2 * (R - 2.0))


@pytest.mark.parametrize("name", sorted(mr.degenerate_volumes()))
def test_degenerate_volumes(F, name):
    got, ref = check(mr.degenerate_volumes()[name], name)
    assert len(got["faces"]) == int(ref["kept"].sum()) < len(ref["candidates"]) or name == "zero_sea"
    tri = got["vertices"][got["faces"]]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not (tri[:, a].view(np.uint32) == tri[:, b].view(np.uint32)).all(1).any()


def test_fused_sphere_views_mesh_and_ply_round_trip(F, tmp_path):
    """four analytic depth views of a sphere fused by nsamd_tsdf_integrate, meshed on the device: the mesh of the volume the
    device holds equals the restatement of that volume, lies on the sphere, and survives the PLY writer"""
    from nerfstudio_amd.export import TSDFVolume, write_mesh_ply
    from test_mesh_cpu import read_mesh_ply

    H, W, R = 48, 64, 0.6
    positions = ((2.0, 0.3, 0.4), (-1.8, 0.9, 0.2), (0.2, -2.0, 0.6), (0.3, 0.4, 2.1))
    c2w = np.stack([tr.look_at(p) for p in positions])
    K = np.array([[[70.0, 0, 32.0], [0, 70.0, 24.0], [0, 0, 1]]] * len(positions))
    depth = np.stack([tr.sphere_depth(c2w[b], K[b], H, W, R) for b in range(len(positions))]).astype(np.float32)
    color = np.random.default_rng(5).uniform(0, 1, (len(positions), H, W, 3)).astype(np.float32)
    vol = TSDFVolume.from_aabb([[-1.0, -1, -1], [1, 1, 1]], [24, 20, 22], device="cuda")
    vol.integrate(T(c2w.astype(np.float32)).cuda(), T(K.astype(np.float32)).cuda(), T(depth).cuda(), T(color).cuda())
    mesh = vol.get_mesh()
    ref = mr.extract(vol.values.cpu().numpy(), vol.colors.cpu().numpy(), vol.origin.numpy(), vol.voxel_size.numpy())
    got = mesh_arrays(mesh)
    mr.compare(got, ref, "gpu fused sphere")
    assert len(ref["faces"]) > 500
    # the surface between observed free space and the sphere: vertices whose two voxels were both observed lie near radius R
    weights = vol.weights.cpu().numpy()
    upper = ref["owner"] + np.eye(3, dtype=np.int64)[ref["axis"]]
    seen = (weights[tuple(ref["owner"].T)] > 0) & (weights[tuple(upper.T)] > 0)
    radius = np.linalg.norm(got["vertices"].astype(np.float64), axis=1)
    print(f"fused sphere: {int(seen.sum())} of {len(seen)} vertices between observed voxels, radius {radius[seen].min():.3f} .. "
          f"{radius[seen].max():.3f}")
    # How far off the sphere such a vertex can lie: a voxel on a ray that grazes the sphere, s <= truncation behind the tangent
    # point, is sqrt(R^2 + s^2) - R outside the sphere and still reads as "behind the surface" for that view; the crossing is
    # then interpolated over at most one voxel.
    h, trunc = float(vol.voxel_size.max()), vol.truncation
    assert seen.sum() > 100 and np.abs(radius[seen] - R).max() <= np.sqrt(R * R + trunc * trunc) - R + h
    write_mesh_ply(mesh, tmp_path / "sphere.ply")
    vertex, face = read_mesh_ply(tmp_path / "sphere.ply")
    assert np.array_equal(np.stack([vertex[k] for k in ("x", "y", "z")], 1), got["vertices"])
    assert np.array_equal(np.stack([vertex[k] for k in ("nx", "ny", "nz")], 1), got["normals"])
    assert np.array_equal(face["i"], got["faces"]) and (vertex["alpha"] == 255).all()
    assert np.array_equal(np.stack([vertex[k] for k in ("red", "green", "blue")], 1),
                          (got["colors"].astype(np.float64) * 255).astype(np.uint8))
