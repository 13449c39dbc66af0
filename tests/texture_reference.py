"""Float64 restatement of the texture export (include/nsamd_texture.h) for tests/test_texture_cpu.py and
tests/test_gpu_texture.py: the closed form of the reference's per-UV-triangle unwrap (exporter/texture_utils.py:77-208) —
triangle and weights of a texel as exact ratios —, the texel's ray, the ray length, the 8-bit rule, the error bounds the tests
hold the fp32 arithmetic to, small meshes, and stand-ins for the three launches that serve CPU tensors from all of this.

BOUNDS (u = 2^-24, the unit roundoff of fp32; S_v = sum_i |w_i| |v_i| per component, in float64):
  blend      a component of v0 w0 + v1 w1 + v2 w2 in fp32: every term passes through at most FOUR roundings — its weight (one
             integer ratio), the product, two additions — so |error| <= ((1 + u)^4 - 1) S_v <= C_BLEND u S_v with C_BLEND = 5
             (4 plus the second-order terms).
  direction  d = b / |b| of a blend b with error e, |e_k| <= C_BLEND u S_n,k: d moves by (e_k - d_k (d . e)) / |b|, at most
             2 |e|_2 / |b| per component; the normalisation adds 3 u (squares and their sums, all positive) / 2 for the root,
             u for the root itself, u for the division: < 4 u |d_k| <= 4 u. So C_BLEND * 2 u |S_n|_2 / |b| + 4 u.
  origin     after o - (raylen / 2) d: the product's and the difference's roundings, u (raylen / 2) and u (S_v + raylen / 2),
             plus raylen / 2 times the direction's bound: (C_BLEND + 1) u (S_v + raylen) + (raylen / 2) * direction bound.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
C_BLEND = 5.0


# ---------------------------------------------------------------- the layout -----------------------------------------------------
def layout(F, P):
    """-> (sw, sh, W, H) of texture_utils.py:101-109"""
    nsq = math.ceil(F / 2)
    sw = math.ceil(math.sqrt(nsq))
    sh = math.ceil(nsq / sw)
    return sw, sh, sw * (P + 3), sh * P


def corner_offsets(P):
    """[2,3,2]: the texel offsets of the corners of the upper and of the lower triangle inside their square"""
    return np.array([[[0, 0], [P - 1, 0], [0, P - 1]], [[P + 2, P - 1], [3, P - 1], [P + 2, 0]]], dtype=np.int64)


def texture_coordinates(F, P):
    """[F,3,2] float64"""
    sw, sh, W, H = layout(F, P)
    t = np.arange(F)
    q = t // 2
    offs = corner_offsets(P)[t % 2]
    u = ((q % sw)[:, None] * (P + 3) + offs[..., 0] + 0.5) / W
    v = ((q // sw)[:, None] * P + offs[..., 1] + 0.5) / H
    return np.stack([u, v], -1)


def texel_sites(F, P, texels=None):
    """-> (t [n] int64, w [n,3] float64) of the given linear texel indices (all of them by default)"""
    sw, sh, W, H = layout(F, P)
    texels = np.arange(W * H) if texels is None else np.asarray(texels, dtype=np.int64)
    x, y = texels % W, texels // W
    su, sv = x // (P + 3), y // P
    uo, vo = x - su * (P + 3), y - sv * P
    lower = (uo + vo >= P + 1).astype(np.int64)
    t = np.minimum(2 * (sv * sw + su) + lower, F - 1)
    q = t // 2
    du, dv = x - (q % sw) * (P + 3), y - (q // sw) * P
    odd = t % 2 == 1
    n1 = np.where(odd, P + 2 - du, du)
    n2 = np.where(odd, P - 1 - dv, dv)
    w = np.stack([P - 1 - n1 - n2, n1, n2], -1).astype(np.float64) / (P - 1)
    return t, w


def texel_rays(vertices, normals, faces, P, raylen, texels=None):
    """float64 rays of the given texels (all by default) -> dict(origins, directions [n,3], origin_bound, direction_bound [n,3],
    blend_norm [n], t, w). raylen: the fp32 value the kernel reads, as a float."""
    v, n = np.asarray(vertices, np.float64), np.asarray(normals, np.float64)
    f = np.clip(np.asarray(faces, np.int64), 0, len(v) - 1)  # the kernel's clamp
    t, w = texel_sites(len(f), P, texels)
    tri = f[t]  # [n,3]
    o = np.einsum("nc,ncd->nd", w, v[tri])
    b = -np.einsum("nc,ncd->nd", w, n[tri])
    norm = np.linalg.norm(b, axis=1)
    d = b / np.maximum(norm, 1e-12)[:, None]
    h = 0.5 * float(raylen)
    S_v = np.einsum("nc,ncd->nd", np.abs(w), np.abs(v[tri]))
    S_n = np.einsum("nc,ncd->nd", np.abs(w), np.abs(n[tri]))
    with np.errstate(divide="ignore", invalid="ignore"):
        dir_bound = C_BLEND * 2 * U * np.linalg.norm(S_n, axis=1) / norm + 4 * U
    dir_bound = np.where(norm > 0, dir_bound, 0.0)[:, None] * np.ones((1, 3))  # the zero blend: exactly zero
    org_bound = (C_BLEND + 1) * U * (S_v + 2 * h) + h * dir_bound
    return dict(origins=o - h * d, directions=d, origin_bound=org_bound, direction_bound=dir_bound, blend_norm=norm, t=t, w=w)


def raylen(vertices, faces):
    """2 mean |v[f1] - v[f0]| in float64 (texture_utils.py:374-380)"""
    v = np.asarray(vertices, np.float64)
    f = np.clip(np.asarray(faces, np.int64), 0, len(v) - 1)
    return 2.0 * float(np.mean(np.linalg.norm(v[f[:, 1]] - v[f[:, 0]], axis=1)))


def levels(rgb):
    """the 8-bit rule, in fp32 as the header states it: floor(clamp(v, 0, 1) * 255 + 0.5), NaN -> 0"""
    v = np.asarray(rgb, np.float32)
    c = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))).astype(np.float32)
    return np.floor(c * np.float32(255) + np.float32(0.5)).astype(np.uint8)


# ---------------------------------------------------------------- meshes ---------------------------------------------------------
def soup(F, seed=0, V=None):
    """F random triangles over V random vertices in [-1, 1]^3 with smooth unit normals close to one direction, so that no blend
    — the extrapolated ones of the texels past the last face included — comes near zero. -> vertices, normals fp32, faces int32"""
    rs = np.random.RandomState(1000 + 7 * F + seed)
    V = max(3, (F + 1) // 2 + 2) if V is None else V
    vertices = rs.uniform(-1, 1, (V, 3)).astype(np.float32)
    faces = np.stack([rs.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    n = np.array([0.3, 0.5, 0.8]) + 0.2 * np.sin(3.0 * vertices.astype(np.float64) + 0.5)
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return vertices, normals, faces


def octahedron(subdivisions=2, radius=0.3):
    """a subdivided octahedron on the sphere of `radius`: 8 * 4^subdivisions faces, outward normals"""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(p, np.float64) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    normals = np.stack(v).astype(np.float32)
    return (radius * np.stack(v)).astype(np.float32), normals, np.array(f, np.int32)


# ---------------------------------------------------------------- stand-ins for the launches ------------------------------------
def restatement_launches(log=None):
    """(texel_rays_launch, mesh_raylen_launch, texture_store_launch) with the arguments of nerfstudio_amd.functional's, over CPU
    tensors, served by the functions above. log: a list that receives ("texel_rays", first, count, rows) / ("raylen", T) /
    ("store", first, count)."""
    log = [] if log is None else log

    def texel_rays_launch(atlas, vertices, normals, faces, raylen_dev, first, count, rows, origins, directions, nears, fars):
        log.append(("texel_rays", first, count, rows))
        assert (atlas.squares_w, atlas.squares_h) == layout(atlas.faces, atlas.px)[:2] and 1 <= count <= rows
        texels = first + np.minimum(np.arange(rows), count - 1)
        r = texel_rays(vertices.numpy(), normals.numpy(), faces.numpy(), atlas.px, float(raylen_dev[0]), texels)
        origins[:rows] = torch.from_numpy(r["origins"].astype(np.float32))
        directions[:rows] = torch.from_numpy(r["directions"].astype(np.float32))
        nears[:rows] = 0.0
        fars[:rows] = float(raylen_dev[0])

    def mesh_raylen_launch(vertices, faces, scratch, raylen_dev):
        log.append(("raylen", int(faces.shape[0])))
        raylen_dev[0] = raylen(vertices.numpy(), faces.numpy())

    def texture_store_launch(rgb, count, first, atlas_u8):
        log.append(("store", first, count))
        atlas_u8.view(-1, 3)[first:first + count] = torch.from_numpy(levels(rgb[:count].numpy()))

    return texel_rays_launch, mesh_raylen_launch, texture_store_launch
