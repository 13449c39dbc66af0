"""Numpy restatement of the mesh extraction of include/nsamd_mesh.h over the generated triangle table
(scripts/gen_mesh_table.py): this project's definition of the mesh, since skimage cannot be run where the tests run.
Positions, normals and colour indices in float64; the sign test and the snap predicate (fp32 t exactly 0 or 1) in fp32, so
they are exact. Used by tests/test_mesh_cpu.py and tests/test_gpu_mesh.py."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_mesh_table", os.path.join(ROOT, "scripts", "gen_mesh_table.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

TABLE = gen.table_bytes()  # [256, 16] uint8
EDGE_START = np.array([gen.corner_xyz(gen.edge_corners(e)[0]) for e in range(12)])  # [12, 3]
EDGE_AXIS = np.array([gen.edge_corners(e)[2] for e in range(12)])

POSITION_ULPS = 4  # of the largest coordinate magnitude (fp32)
NORMAL_ATOL = 1e-4  # per component, where the index-space gradient norm is >= GRADIENT_FLOOR
GRADIENT_FLOOR = 1e-2
TIE_BAND = 1e-5  # |t - 0.5| below it: the colour's rounding may go either way in fp32
EXCLUDED_CAP = 0.05


def clamp32(values):
    return np.clip(np.asarray(values, np.float32), np.float32(-1), np.float32(1))


def extract(values, colors, origin, voxel_size):
    """dict: vertices, index_positions, normals [V,3] float64; color_index [V,3] int64; colors [V,3] fp32; faces [T,3] int32;
    t32 [V] fp32; owner [V,3], axis [V]; gradient_norm [V] (index space, of the blended gradient); candidates [C,3] int32 (every
    triangle before the degenerate rule, same order) and kept [C] bool."""
    v = clamp32(values)
    dims = np.array(v.shape)
    origin = np.asarray(origin, np.float32).astype(np.float64)
    vs = np.asarray(voxel_size, np.float32).astype(np.float64)
    empty = dict(vertices=np.zeros((0, 3)), index_positions=np.zeros((0, 3)), normals=np.zeros((0, 3)),
                 color_index=np.zeros((0, 3), np.int64), colors=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32),
                 t32=np.zeros(0, np.float32), t64=np.zeros(0), owner=np.zeros((0, 3), np.int64), axis=np.zeros(0, np.int64),
                 gradient_norm=np.zeros(0), candidates=np.zeros((0, 3), np.int32), kept=np.zeros(0, bool))
    if (dims < 2).any():
        return empty
    neg = v < 0
    crossed = np.zeros((*dims, 3), bool)
    upper = np.zeros((*dims, 3), np.float32)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        crossed[(*lo, a)] = neg[tuple(lo)] != neg[tuple(hi)]
        upper[(*lo, a)] = v[tuple(hi)]
    vid = np.full(crossed.shape, -1, np.int64)
    vid[crossed] = np.arange(int(crossed.sum()))  # C order: voxel linear index, then axis
    owner = np.argwhere(crossed)  # [V, 4] in the same order
    axis, owner = owner[:, 3], owner[:, :3]
    V = len(axis)
    v0 = v[tuple(owner.T)]
    v1 = upper[crossed]
    with np.errstate(all="ignore"):
        t32 = (v0 / (v0 - v1)).astype(np.float32)
    t64 = v0.astype(np.float64) / (v0.astype(np.float64) - v1.astype(np.float64))
    step = np.zeros((V, 3))
    step[np.arange(V), axis] = 1.0
    index_positions = owner + step * t64[:, None]
    vertices = origin + index_positions * vs
    grad = np.stack(np.gradient(v.astype(np.float64)), axis=-1)  # central inside, one-sided on the border
    upper_owner = owner + step.astype(np.int64)
    g0, g1 = grad[tuple(owner.T)], grad[tuple(upper_owner.T)]
    blended_index = g0 * (1 - t64[:, None]) + g1 * t64[:, None]
    blended = blended_index / vs
    norm = np.linalg.norm(blended, axis=1)
    normals = np.where(norm[:, None] > 0, blended / np.where(norm > 0, norm, 1.0)[:, None], 0.0)
    color_index = np.clip(np.rint(index_positions).astype(np.int64), 0, dims - 1)
    vertex_colors = np.asarray(colors, np.float32)[tuple(color_index.T)] if V and colors is not None else empty["colors"]

    # the lattice corner a vertex snaps to (linear index), or -1 - its own id: never equal to another's
    strides = np.array([dims[1] * dims[2], dims[2], 1])
    lin = owner @ strides
    snap = np.where(t32 == 0, lin, np.where(t32 == 1, lin + strides[axis], -1 - np.arange(V)))

    cells = np.zeros(tuple(dims - 1), np.int64)
    for c in range(8):
        dx, dy, dz = gen.corner_xyz(c)
        cells |= neg[dx:dims[0] - 1 + dx, dy:dims[1] - 1 + dy, dz:dims[2] - 1 + dz].astype(np.int64) << c
    count = TABLE[:, 15].astype(np.int64)[cells]
    where = np.argwhere(count > 0)
    cases = cells[tuple(where.T)]
    keys, tris = [], []
    for k in range(5):
        m = count[tuple(where.T)] > k
        cell, case = where[m], cases[m]
        ids = []
        for j in range(3):
            e = TABLE[case, 3 * k + j].astype(np.int64)
            o = cell + EDGE_START[e]
            ids.append(vid[o[:, 0], o[:, 1], o[:, 2], EDGE_AXIS[e]])
        keys.append((cell @ strides) * 5 + k)
        tris.append(np.stack(ids, 1))
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    order = np.argsort(keys, kind="stable")
    candidates = tris[order]
    assert (candidates >= 0).all()
    s = snap[candidates]
    kept = ~((s[:, 0] == s[:, 1]) | (s[:, 0] == s[:, 2]) | (s[:, 1] == s[:, 2]))
    return dict(vertices=vertices, index_positions=index_positions, normals=normals, color_index=color_index,
                colors=vertex_colors, faces=candidates[kept].astype(np.int32), t32=t32, t64=t64, owner=owner, axis=axis,
                gradient_norm=np.linalg.norm(blended_index, axis=1), candidates=candidates.astype(np.int32), kept=kept)


def compare(got, ref, label=""):
    """got: dict of vertices, normals, colors [V,3] fp32 and faces [T,3] int32 from the code under test. Faces and counts exact;
    positions within POSITION_ULPS ulp of the largest coordinate magnitude; normals within NORMAL_ATOL where the gradient is at
    least GRADIENT_FLOOR; colours exact off the rounding ties. Fails when either exclusion exceeds EXCLUDED_CAP of the vertices.
    Prints its figures before it asserts."""
    V, T = len(ref["vertices"]), len(ref["faces"])
    assert got["vertices"].shape == (V, 3) and got["normals"].shape == (V, 3) and got["colors"].shape == (V, 3), label
    assert got["faces"].shape == (T, 3) and got["faces"].dtype == np.int32 and got["vertices"].dtype == np.float32, label
    assert np.array_equal(got["faces"], ref["faces"]), label
    if V == 0:
        return
    scale = float(np.abs(ref["vertices"]).max())
    tol = POSITION_ULPS * np.spacing(np.float32(scale)).astype(np.float64)
    dpos = float(np.abs(got["vertices"].astype(np.float64) - ref["vertices"]).max())
    steep = ref["gradient_norm"] >= GRADIENT_FLOOR
    dnrm = float(np.abs(got["normals"].astype(np.float64) - ref["normals"])[steep].max()) if steep.any() else 0.0
    # t exactly 0.5 in fp32 AND in float64 (v0 == -v1: every pair of clamped voxels, a tenth of the vertices of white noise) is no
    # tie to exclude: p + 0.5 is exact in both precisions and rounds to even in both
    off_tie = (np.abs(ref["t32"].astype(np.float64) - 0.5) >= TIE_BAND) | ((ref["t32"] == 0.5) & (ref["t64"] == 0.5))
    print(f"mesh {label}: V {V}, T {T}, position error {dpos:.3e} (bound {tol:.3e}), normal error {dnrm:.3e}, "
          f"flat {int((~steep).sum())}, ties {int((~off_tie).sum())}")
    assert (~steep).mean() <= EXCLUDED_CAP and (~off_tie).mean() <= EXCLUDED_CAP, label
    assert dpos <= tol, label
    assert dnrm <= NORMAL_ATOL, label
    assert np.array_equal(got["colors"][off_tie], ref["colors"][off_tie]), label
    flat = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
    assert (np.abs(flat[steep] - 1) <= 1e-5).all(), label


# ---- invariants ---------------------------------------------------------------------------------------------------------------
def directed_edge_balance(faces):
    """True when every directed edge occurs exactly as often as its reverse"""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1 if len(f) else 1
    fwd = np.sort(e[:, 0] * n + e[:, 1])
    bwd = np.sort(e[:, 1] * n + e[:, 0])
    return np.array_equal(fwd, bwd)


def interior_faces_edges(ref, dims):
    """[E, 2] directed edges of ref["faces"] that do not lie in a boundary face of the volume (both ends in the same one): a
    surface that crosses the volume's border is open THERE, and only there"""
    f = np.asarray(ref["faces"], np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    owner, axis = ref["owner"], ref["axis"]
    on = np.zeros((len(owner), 6), bool)  # vertex lies in boundary face (axis b, side)
    for b in range(3):
        off_axis = axis != b
        on[:, 2 * b] = off_axis & (owner[:, b] == 0)
        on[:, 2 * b + 1] = off_axis & (owner[:, b] == dims[b] - 1)
    return e[~(on[e[:, 0]] & on[e[:, 1]]).any(axis=1)]


def edges_balanced(e, n):
    return np.array_equal(np.sort(e[:, 0] * n + e[:, 1]), np.sort(e[:, 1] * n + e[:, 0]))


def strictly_manifold(faces):
    """every directed edge exactly once and its reverse exactly once: two triangles per edge, consistently wound"""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    keys = e[:, 0] * n + e[:, 1]
    return len(np.unique(keys)) == len(keys) and directed_edge_balance(faces)


def euler_characteristic(faces):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return len(np.unique(f)) - len(np.unique(e, axis=0)) + len(f)


def signed_volume(vertices, faces):
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- volumes ------------------------------------------------------------------------------------------------------------------
def noise_volume(seed, shape=(20, 13, 11)):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def noise_colors(seed, shape):
    return np.random.default_rng(1000 + seed).uniform(0, 1, (*shape, 3)).astype(np.float32)


def sphere_volume(n=16, radius=5.2, truncation=5.0, centre=None):
    """values > 0 outside (free space), < 0 inside, as a TSDF has them; index units"""
    c = np.full(3, (n - 1) / 2.0) if centre is None else np.asarray(centre, float)
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), -1)
    return np.clip((np.linalg.norm(g - c, axis=-1) - radius) / truncation, -1, 1).astype(np.float32), c


def smooth_volume(n=20, sigma=1.5, seed=1):
    """Gaussian-smoothed noise with a -1 border. With seed 1 (and 2, 3, 9, 10, 11) the restatement's mesh is strictly manifold;
    with seeds 0 and 4-8 one or two fan diagonals lie in a cube face and coincide with the neighbouring cell's (4 or 8 directed
    edges used twice in ~6500 triangles), which the mesh's definition allows."""
    x = np.random.default_rng(seed).standard_normal((n, n, n))
    r = int(4 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for a in range(3):
        x = np.apply_along_axis(lambda m: np.convolve(m, k, mode="same"), a, x)
    x = x / np.abs(x).max()
    x[0], x[-1], x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1] = -1, -1, -1, -1, -1, -1
    return x.astype(np.float32)


def degenerate_volumes():
    """hand-built volumes with exact zeros at corners, and one v1 = -1e-30 against v0 = 1 (fp32 t == 1)"""
    a = np.ones((4, 4, 4), np.float32)
    a[1:3, 1:3, 1:3] = -0.5
    a[1, 1, 1] = 0.0  # a zero (non-negative) corner surrounded by negatives on three sides
    a[2, 2, 1] = -0.0
    b = np.ones((3, 4, 5), np.float32)
    b[1:, 1:3, 1:4] = -1.0
    # the UPPER end of every crossed edge it is on (its lower neighbours are +1, its upper ones negative): v0 = 1 against
    # v1 = -1e-30 gives t == 1 in fp32. (As a LOWER end it would give t = 1e-30: not snapped, yet p + t rounds to p.)
    b[1, 1, 1] = np.float32(-1e-30)
    b[1, 2, 3] = 0.0
    c = np.zeros((3, 3, 3), np.float32)  # zeros everywhere but one negative voxel: all its vertices snap to its neighbours
    c[1, 1, 1] = -1.0
    d = -np.ones((3, 3, 4), np.float32)
    d[1, 1, 1] = 0.0
    d[1, 1, 2] = 0.0  # two zero corners next to each other in a negative volume: every vertex snaps onto one of them
    return {"zero_corner": a, "tiny_negative": b, "zero_sea": c, "zero_pair": d}


def restatement_launches():
    """(count, emit) with the arguments of functional.mesh_count_launch / mesh_emit_launch, on host tensors, served by the
    restatement cast to fp32: stand-ins for the native launches in the CPU tests of the Python layer."""
    import torch

    stash = {}

    def count(vol, values, scratch, totals):
        r = extract(values.numpy(), None, list(vol.origin), list(vol.voxel_size))
        stash[scratch.data_ptr()] = r
        totals[0], totals[1] = len(r["vertices"]), len(r["faces"])

    def emit(vol, values, colors, scratch, vertices, normals, vertex_colors, faces):
        r = stash.pop(scratch.data_ptr())
        assert tuple(vertices.shape) == (len(r["vertices"]), 3) and tuple(faces.shape) == (len(r["faces"]), 3)
        vertices.copy_(torch.from_numpy(r["vertices"].astype(np.float32)))
        normals.copy_(torch.from_numpy(r["normals"].astype(np.float32)))
        faces.copy_(torch.from_numpy(r["faces"]))
        if len(r["vertices"]):
            vertex_colors.copy_(colors[tuple(torch.from_numpy(r["color_index"]).T)])

    return count, emit
