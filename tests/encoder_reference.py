"""Float64 references of the kernels that turn a position or a direction into network inputs (csrc/common.h, hashgrid.hip,
density_mlp.hip's fused proposal forward), in plain numpy / torch, importable without a GPU, and the point sets the tests of
those kernels share (tests/test_encoder_reference_cpu.py, tests/test_gpu_encoders_float64.py).

The cells of a hash grid are discontinuous in the position, so every reference takes the fp32 inputs of the rounding-free part
exactly as the kernels define them (separately rounded numpy float32 operations; the library is built with -ffp-contract=off)
and does everything after that in float64:

* positions32      load_position: positions as given, or o + d * (t[s] + t[s+1]) / 2 per ray sample;
* contract32       contract_linf, as torch evaluates SceneContraction(order=inf): the L-inf norm of a row with a NaN is NaN;
* normalise32      normalise_position for NSAMD_XFORM_NONE / CONTRACT / AABB: the grid input and the selector;
* hash_features64  per level sx = fl(x * scale), floor / ceil corners, w = sx - floor(sx) (exact in fp32), the reference's
                   hash; the blend of the eight fp32 table values with the fp32 weights in float64 (u = 1 - w exactly), and
                   A, the same blend of |q_k|;
* density64        orc.density_mlp_fwd64 on the float64 features + the error bounds of `pre` and the density;
* nerf_rows64      s = fl(fl(2pi_f32 * x) * freq) in fp32, sin(float64(s)), sin(float64(fl(s + (pi/2)_f32))), the raw input;
* sh4_64           the sixteen polynomials of utils/spherical_harmonics.py in float64 on the fp32 components, and per
                   component the sum of the absolute values of its monomials.

The bounds themselves are derived in the docstring of tests/test_gpu_encoders_float64.py."""
import functools
import math

import numpy as np
import torch

from float64_check import E_EXP, U
from oracle import nerfacto_oracle as orc

F32 = np.float32
XFORM_NONE, XFORM_CONTRACT, XFORM_AABB = 0, 1, 2
TRANSFORMS = {"none": XFORM_NONE, "contract": XFORM_CONTRACT, "aabb": XFORM_AABB}
BOX = np.array([[-0.5, -1.0, 0.25], [1.5, 1.0, 2.25]], F32)  # the non-cubic box of tests/test_gpu_table_scatter.py
TWO_PI32 = F32(6.283185307179586)
HALF_PI32 = F32(1.5707963267948966)
HASH_ROUNDINGS = 9  # trilinear_blend: three lerp stages of fl(1 - w), two products and a sum (see the GPU tests' docstring)

# ---------------------------------------------------------------- the cases of the GPU tests --------------------------------------
# name -> (levels, hidden, min_res, max_res, log2_T): the four instantiations of density_field_fwd_kernel + the shipped proposal grid
FUSED_GRIDS = {"L5-H16": (5, 16, 16, 128, 12), "L8-H16": (8, 16, 16, 256, 12), "L5-H64": (5, 64, 16, 128, 12),
               "L8-H64": (8, 64, 16, 256, 12), "L5-H16-T17-shipped": (5, 16, 16, 256, 17)}
FUSED_M = (1, 63, 64, 255, 256, 257, 513)
FUSED_RAYS = ((1, 1), (3, 85), (257, 1), (5, 96))
# name -> (levels, min_res, max_res, log2_T): one grid per forward kernel of nsamd_hashgrid_encode_fwd (8 << log2_T < 2 MiB
# selects four levels per thread, else lane pairs: with the XCD level sweep when the level count is a multiple of 8)
HASH_GRIDS = {"four-levels-per-thread-L5-T12": (5, 16, 128, 12), "pair-sweep-even-and-odd-li-L16-T18": (16, 16, 2048, 18),
              "pair-no-sweep-L5-T18": (5, 16, 512, 18)}
HASH_M = (1, 2, 255, 256, 257)
HASH_RAYS = ((3, 85),)
SH_ROUNDINGS = np.array([1, 2, 2, 2, 3, 3, 4, 3, 4, 6, 4, 6, 6, 6, 5, 6], np.float64)  # counted in the GPU tests' docstring


def scalings32(levels, min_res, max_res):
    return orc.hash_level_scalings(levels, min_res, max_res).numpy().astype(F32)


@functools.lru_cache(maxsize=None)
def table32(levels, log2_T, seed=0):
    """[levels * 2^log2_T, 2] fp32 table values of either sign (do not modify: cached and shared)."""
    return (np.random.RandomState(1000 + 31 * levels + log2_T + seed).standard_normal((levels << log2_T, 2)) * 0.5).astype(F32)


def mlp_params(in_dim, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    W0 = torch.randn(hidden, in_dim, generator=g) / math.sqrt(in_dim)
    b0 = torch.randn(hidden, generator=g) * 0.1
    W1 = torch.randn(1, hidden, generator=g) / math.sqrt(hidden)
    b1 = torch.randn(1, generator=g) * 0.1
    return W0, b0, W1, b1


def contract_edges():
    """Raw points at the edges of the L-inf contraction: |x| = 1 exactly, just below 1, 3, 1e3, 1e30 on one axis (either sign),
    ties between two and three axes."""
    below = np.nextafter(F32(1), F32(0))
    rows = []
    for k, m in enumerate((1.0, below, 3.0, 1e3, 1e30)):
        for axis in range(3):
            v = np.array([0.25, -0.5, 0.125], F32) * F32(min(m, 3.0))
            v[axis] = F32(m) * (1 if (k + axis) % 2 == 0 else -1)
            rows.append(v)
    for m in (1.0, below, 3.0):
        rows += [np.array([m, m, 0.3], F32), np.array([-m, 0.2, m], F32), np.array([0.1, m, -m], F32), np.array([m, -m, m], F32)]
    return np.stack(rows).astype(F32)


def _unit_specials(min_res):
    """Grid inputs in [0, 1]: the box's corners, face points and points on lattice planes of the coarsest level."""
    rs = np.random.RandomState(7)
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], F32)
    faces = rs.uniform(0.1, 0.9, (6, 3)).astype(F32)
    for a in range(3):
        faces[2 * a, a], faces[2 * a + 1, a] = 0.0, 1.0
    lattice = (rs.randint(1, min_res, (12, 3)) / F32(min_res)).astype(F32)
    lattice[:6, 1] = rs.uniform(0.05, 0.95, 6).astype(F32)  # on one or two planes only
    lattice[:3, 2] = rs.uniform(0.05, 0.95, 3).astype(F32)
    return np.concatenate([corners[[0, 7, 3, 5]], faces, lattice, corners[[1, 2, 4, 6]]]).astype(F32)


def position_case(M, transform, min_res, seed):
    """{"positions": [M,3] fp32 raw points}: random points, and (from the second point on, as many as fit) points on lattice
    planes of the coarsest level, the box's corners and faces (selector 0 under CONTRACT / AABB; exact 0 and 1 under NONE) and,
    under CONTRACT, contract_edges()."""
    rs = np.random.RandomState(seed)
    unit = _unit_specials(min_res)
    if transform == XFORM_NONE:
        raw, special = rs.uniform(0, 1, (M, 3)).astype(F32), unit
    elif transform == XFORM_AABB:  # a share of the random points beyond the box
        raw = (rs.uniform(-0.1, 1.1, (M, 3)).astype(F32) * F32(2.0) + BOX[0]).astype(F32)
        special = (unit * F32(2.0) + BOX[0]).astype(F32)  # exact: the box's extent is 2 on every axis
    else:  # inside the unit cube (identity) and outside (contracted); (c + 2) / 4 is exact for the lattice planes' c = 4 k / res - 2
        raw = (rs.standard_normal((M, 3)) * 1.5).astype(F32)
        inner = unit[(np.abs(unit * 4 - 2) < 1).all(-1)] * F32(4.0) - F32(2.0)
        far = np.where(unit[:10] < 0.5, F32(-1e30), F32(1e30)).astype(F32) * np.array([1, 0.5, 0.25], F32)  # contracts to the faces
        special = np.concatenate([contract_edges(), inner, far]).astype(F32)
    k = min(len(special), M - 1)
    if k > 0:
        first = (seed * 5) % len(special)
        raw[1 : 1 + k] = np.roll(special, -first, axis=0)[:k]
    return {"positions": np.ascontiguousarray(raw)}


def ray_case(n, S, transform, seed):
    """{"origins", "directions": [n,3], "t_bins": [n,S+1]} fp32: samples that start inside the grid and, under CONTRACT / AABB,
    leave the unit cube / the box along the ray."""
    rs = np.random.RandomState(seed)
    d = rs.standard_normal((n, 3)).astype(F32)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    if transform == XFORM_NONE:
        o, far = rs.uniform(0.3, 0.7, (n, 3)).astype(F32), 0.29
    elif transform == XFORM_AABB:
        o, far = (rs.uniform(0.3, 0.7, (n, 3)).astype(F32) * F32(2.0) + BOX[0]).astype(F32), 1.5
    else:
        o, far = (rs.standard_normal((n, 3)) * 0.4).astype(F32), 8.0
    t = np.sort(rs.uniform(0.01, far, (n, S + 1)).astype(F32), axis=-1)
    if transform == XFORM_CONTRACT and n * S > 1:
        # the last ray ends beyond 2^24: 2 - 1 / mag rounds to 2, the point contracts onto the face, the selector is 0
        t[-1, -1] = 1e9
        if S > 1:
            t[-1, -2] = 1e8
    return {"origins": o, "directions": d, "t_bins": np.ascontiguousarray(t)}


def case_seed(*parts):
    s = 17
    for p in parts:
        s = (s * 1000003 + int(p)) % (2**31 - 1)
    return s


def fused_cases(mode, transform, min_res):
    """[(label, points dict, M)] of the fused proposal forward's tests for one point mode and transform."""
    if mode == "positions":
        return [(f"M={M}", position_case(M, transform, min_res, case_seed(M, transform, 1)), M) for M in FUSED_M]
    return [(f"rays={n}x{S}", ray_case(n, S, transform, case_seed(n, S, transform, 2)), n * S) for n, S in FUSED_RAYS]


def hash_cases(mode, transform, min_res):
    if mode == "positions":
        return [(f"M={M}", position_case(M, transform, min_res, case_seed(M, transform, 3)), M) for M in HASH_M]
    return [(f"rays={n}x{S}", ray_case(n, S, transform, case_seed(n, S, transform, 4)), n * S) for n, S in HASH_RAYS]


# ---------------------------------------------------------------- the rounding-free part, in fp32 ---------------------------------

def positions32(points):
    """load_position (csrc/common.h) in separately rounded fp32: [M,3]."""
    if points.get("positions") is not None:
        return np.ascontiguousarray(points["positions"], dtype=F32).reshape(-1, 3)
    o, d, t = (np.asarray(points[k], dtype=F32) for k in ("origins", "directions", "t_bins"))
    span = (t[:, :-1] + t[:, 1:]).astype(F32)                                   # starts + ends
    prod = (d[:, None, :] * span[:, :, None]).astype(F32)                       # d * span
    return np.ascontiguousarray((o[:, None, :] + (prod / F32(2.0)).astype(F32)).astype(F32).reshape(-1, 3))


def contract32(x32):
    """contract_linf in fp32: where(mag < 1, x, (2 - 1 / mag) * (x / mag)), mag the row's L-inf norm (NaN if the row has one)."""
    x = np.asarray(x32, dtype=F32)
    with np.errstate(all="ignore"):
        mag = np.max(np.abs(x), axis=-1, keepdims=True)  # (np.max propagates NaN, as torch's norm does)
        a = (F32(2.0) - (F32(1.0) / mag).astype(F32)).astype(F32)
        far = (a * (x / mag).astype(F32)).astype(F32)
    return np.where(mag < F32(1.0), x, far).astype(F32)


def normalise32(raw, transform, box=BOX):
    """normalise_position in fp32: (grid input [M,3], selector [M] of 1.0 / 0.0)."""
    x = np.asarray(raw, dtype=F32)
    if transform == XFORM_NONE:
        return x.copy(), np.ones(x.shape[0], F32)
    with np.errstate(all="ignore"):
        if transform == XFORM_CONTRACT:
            x = ((contract32(x) + F32(2.0)).astype(F32) / F32(4.0)).astype(F32)
        else:
            lo, hi = np.asarray(box, dtype=F32)
            x = ((x - lo).astype(F32) / (hi - lo).astype(F32)).astype(F32)
        sel = ((x > 0) & (x < 1)).all(-1).astype(F32)
        return (x * sel[:, None]).astype(F32), sel


# ---------------------------------------------------------------- float64 from there on -------------------------------------------

def hash_features64(x32, table, scalings, log2_T):
    """(enc64, A) [M, 2L] float64: the hash grid's features of the fp32 grid inputs x32 and the same blend of |q_k|."""
    x = np.asarray(x32, dtype=F32)
    tab = np.asarray(table, dtype=F32)
    T = 1 << log2_T
    enc, mag = [], []
    for lvl, scale in enumerate(np.asarray(scalings, dtype=F32)):
        sx = (x * scale).astype(F32)
        lo, hi = np.floor(sx), np.ceil(sx)
        w = (sx - lo).astype(F32).astype(np.float64)
        u = 1.0 - w
        lo_i, hi_i = lo.astype(np.int32), hi.astype(np.int32)

        def q(cx, cy, cz):
            idx = orc.hash_corner_index((hi_i if cx else lo_i)[:, 0], (hi_i if cy else lo_i)[:, 1], (hi_i if cz else lo_i)[:, 2],
                                        lvl, T)
            return tab[idx].astype(np.float64)

        for out, f in ((enc, lambda v: v), (mag, np.abs)):
            wx, wy, wz, ux, uy, uz = w[:, 0:1], w[:, 1:2], w[:, 2:3], u[:, 0:1], u[:, 1:2], u[:, 2:3]
            yc_zc = f(q(1, 1, 1)) * wx + f(q(0, 1, 1)) * ux
            yf_zc = f(q(1, 0, 1)) * wx + f(q(0, 0, 1)) * ux
            yf_zf = f(q(1, 0, 0)) * wx + f(q(0, 0, 0)) * ux
            yc_zf = f(q(1, 1, 0)) * wx + f(q(0, 1, 0)) * ux
            out.append((yc_zc * wy + yf_zc * uy) * wz + (yc_zf * wy + yf_zf * uy) * uz)
    return np.concatenate(enc, axis=-1), np.concatenate(mag, axis=-1)


def density64(enc64, enc_err, sel, mlp, avg):
    """orc.density_mlp_fwd64 on float64 features enc64 [M,IN] that the kernel holds to within enc_err [M,IN], selector sel [M],
    mlp = (W0, b0, W1, b1) fp32 tensors. Adds what the bounds need: dpre (|W1| . (|W0| @ enc_err) + IN u (a_abs @ |W1|) + H u
    pre_abs) and ddensity (density (dpre (1 + dpre) + E_EXP + 2u))."""
    W0, b0, W1, b1 = mlp
    r = orc.density_mlp_fwd64(torch.from_numpy(np.ascontiguousarray(enc64)), torch.from_numpy(np.asarray(sel, dtype=np.float64)),
                              W0, b0, W1, b1, avg)
    H, IN = W0.shape
    w1 = W1.double().abs().reshape(-1)
    dpre = (torch.from_numpy(np.ascontiguousarray(enc_err)) @ W0.double().abs().t()) @ w1 + IN * U * (r["a_abs"] @ w1) + H * U * r["pre_abs"]
    return dict(r, dpre=dpre, ddensity=r["density"] * (dpre * (1 + dpre) + E_EXP + 2 * U))


def nerf_rows64(x32, freqs32, include_input):
    """[M, 6 F (+3)] float64 rows of nsamd_nerf_encode for fp32 positions x32 [M,3] and fp32 frequencies [F]."""
    x = np.asarray(x32, dtype=F32)
    fr = np.asarray(freqs32, dtype=F32)
    with np.errstate(all="ignore"):
        s = ((TWO_PI32 * x).astype(F32)[:, :, None] * fr[None, None, :]).astype(F32).reshape(x.shape[0], -1)  # [M, d F + f]
        s2 = (s + HALF_PI32).astype(F32)
        cols = [np.sin(s.astype(np.float64)), np.sin(s2.astype(np.float64))]
    if include_input:
        cols.append(x.astype(np.float64))
    return np.concatenate(cols, axis=-1)


def sh4_64(d32):
    """(sh [M,16], mono_abs [M,16]) float64: utils/spherical_harmonics.py:24-93 on the fp32 components as given, and per component
    the sum of the absolute values of its monomials."""
    d = np.asarray(d32, dtype=F32).astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    one = np.ones_like(x)
    sh = [0.28209479177387814 * one, 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
          1.0925484305920792 * x * y, 1.0925484305920792 * y * z, 0.9461746957575601 * zz - 0.31539156525251999,
          1.0925484305920792 * x * z, 0.5462742152960396 * (xx - yy), 0.5900435899266435 * y * (3 * xx - yy),
          2.890611442640554 * x * y * z, 0.4570457994644658 * y * (5 * zz - 1), 0.3731763325901154 * z * (5 * zz - 3),
          0.4570457994644658 * x * (5 * zz - 1), 1.445305721320277 * z * (xx - yy), 0.5900435899266435 * x * (xx - 3 * yy)]
    mono = [0.28209479177387814 * one, 0.4886025119029199 * ay, 0.4886025119029199 * az, 0.4886025119029199 * ax,
            1.0925484305920792 * ax * ay, 1.0925484305920792 * ay * az, 0.9461746957575601 * zz + 0.31539156525251999,
            1.0925484305920792 * ax * az, 0.5462742152960396 * (xx + yy), 0.5900435899266435 * ay * (3 * xx + yy),
            2.890611442640554 * ax * ay * az, 0.4570457994644658 * ay * (5 * zz + 1), 0.3731763325901154 * az * (5 * zz + 3),
            0.4570457994644658 * ax * (5 * zz + 1), 1.445305721320277 * az * (xx + yy), 0.5900435899266435 * ax * (xx + 3 * yy)]
    return np.stack(sh, axis=-1), np.stack(mono, axis=-1)


# ---------------------------------------------------------------- inputs of the small encoders ------------------------------------

def nerf_inputs(M, seed):
    """[M,3] fp32: uniform in [-4, 4]; the last rows (as many as fit behind the first) hold exact 0 and -0, a denormal, 1e-20 and one
    row each with NaN, +Inf and -Inf."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-4, 4, (M, 3)).astype(F32)
    special = np.array([[0.0, -0.0, 1e-40], [1e-20, -1e-20, -1e-40], [np.nan, 0.5, -2.0], [1.0, np.inf, -0.25],
                        [-np.inf, 3.0, 0.0]], F32)
    k = min(len(special), M - 1)
    if k > 0:
        x[M - k :] = special[:k]
    return x


def sh_inputs(M, seed):
    """[M,3] fp32 unit vectors; the last rows hold the six axis directions, vectors within 1e-4 of an axis, the diagonals, non-unit
    input (the zero vector, lengths 1e-3 and 10) and a row with a NaN."""
    rs = np.random.RandomState(seed)
    d = rs.standard_normal((M, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    near = axes + 1e-4 * np.array([[0, 1, -0.5], [0.7, 0, 0.7], [-1, 0.3, 0], [0, -0.2, 1], [1, 0, -1], [0.5, 0.5, 0]])
    near /= np.linalg.norm(near, axis=-1, keepdims=True)
    diag = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, -1], [1, 1, 0], [0, -1, 1], [-1, 0, 1]], np.float64)
    diag /= np.linalg.norm(diag, axis=-1, keepdims=True)
    v = rs.standard_normal((2, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    special = np.concatenate([axes, near, diag, np.zeros((1, 3)), v[:1] * 1e-3, v[1:] * 10, [[0.6, np.nan, 0.8]]]).astype(F32)
    k = min(len(special), M - 1)
    if k > 0:
        d[M - k :] = special[:k]
    return d


def contract_inputs(M, seed):
    """[M,3] fp32: random normal x 3; the last rows hold contract_edges(), +-0, a denormal, 3e38 and rows with +Inf and NaN."""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((M, 3)) * 3).astype(F32)
    extra = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [1e-40, -1e-42, 0.0], [3e38, 1.0, -3e38], [-3e38, 3e38, 3e38],
                      [np.inf, 1.0, 2.0], [0.5, -np.inf, np.inf], [np.nan, 3.0, 0.5], [0.25, np.nan, 0.5], [np.nan, np.nan, np.nan]],
                     F32)
    special = np.concatenate([extra, contract_edges()])
    k = min(len(special), M - 1)
    if k > 0:
        x[M - k :] = special[:k]
    return x


def nerf_freqs(F, e):
    """2 ** torch.linspace(0, e, F): host-evaluated, so the fp32 values are the reference's (include/nsamd.h)."""
    return (2 ** torch.linspace(0.0, float(e), F)).numpy().astype(F32)
