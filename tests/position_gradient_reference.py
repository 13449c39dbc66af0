"""Float64 references, per-entry bounds and the shared cases of the hash grid's position, ray and scratch-free table gradients
(csrc/hashgrid.hip: position_gradient under hash_encode_bwd_pos_kernel and hash_encode_bwd_rays_kernel, hash_encode_bwd_table_kernel,
hash_encode_bwd_sliced_kernel). A helper module, importable without a GPU: tests/test_position_gradient_reference_cpu.py holds a
correct fp32 evaluation and twelve seeded defects to it, tests/test_gpu_hash_position_gradients.py holds the kernels to it.

The reference evaluates position_gradient's expression in float64 FROM THE KERNEL'S OWN fp32 BRANCH INPUTS: the raw position
(encoder_reference.positions32 = load_position), the grid input and the selector (normalise32 = normalise_position; the box is a
parameter here), the cell and its weights w = fl(scaled) - floor(fl(scaled)) (exact in fp32). The cell, `sel`, `mag < 1`, which
coordinates tie for the maximum and the sign of a coordinate are all decided on those fp32 values, by both sides alike, so no entry
is excluded from any check. u = 2^-24, gamma_k = k u / (1 - k u); every check goes through float64_check.check_entries
(x SAFE = 1 + 2^-6 for second-order terms, + TINY). Nothing below is fitted to a kernel; the counts are read off the code.

* Grid-coordinate gradient G (the loop over the levels). |G_fp32 - G64| <= gamma_D A per axis with D = 13 + L (x), 12 + L (y),
  11 + L (z) and A the float64 sum of the absolute terms scale |g| (two weights) |corner value|: the derivation and the
  definition of A are those of tests/test_kernel_helpers_cpu.py::test_position_gradient_from_the_kernel_helpers_vs_float64
  (1 - wz, g wz, 1 - wy, (g wz) wy, q7 - q6, their product, 3 additions of the four products, 2 into lx over the features, the
  product with the scale, L additions over the levels), restated here as grid_gradient64.
* Selector: x sel is exact (sel is 0 or 1). G, A and the error are multiplied by it; a masked point's bound is 0 (TINY) and
  check_dpositions also asserts its three entries == 0.
* NSAMD_XFORM_AABB: fl(hi - lo) and the division are two more roundings on every term: gamma_(D+2) A / (hi - lo), the extent in
  float64 from the fp32 corners.
* NSAMD_XFORM_CONTRACT: / 4 is exact (g = G / 4, e = gamma_D A / 4). contract_linf_bwd (common.h:207-225) is the identity for
  mag < 1. Otherwise out_i = g_i a inv + share_i sign_i g_mag with inv = 1 / mag, a = 2 - inv,
  g_mag = (sum_j g_j x_j inv) inv^2 - a (sum_j g_j x_j) inv^2, share_i = [|x_i| == mag] / cnt. To first order the incoming error
  e_j passes through the absolute values of the Jacobian's terms:
      E_i = e_i a inv + share_i (sum_j e_j |x_j|) (inv^3 + a inv^2)
  and the operation's own roundings are counted per term on |g_j| + e_j (the fp32 operand may be that large):
      k1 = 6 on T1_i = (|g_i| + e_i) a inv:  fl(1 / mag); a = fl(2 - inv) carries 2 roundings (relative 2 u: inv <= 1 <= a);
             fl(g a), fl(. inv); the final addition.
      k2 = 13 on T2_i = share_i (sum_j (|g_j| + e_j) |x_j|) (inv^3 + a inv^2). The longer chain is the second half of g_mag:
             fl(g x), 2 additions of the dot product (3), a (2), fl(a dot) (6), inv inv = 2 + 1, fl(. (inv inv)) (10), the
             subtraction (11), sign and tie are exact products, / cnt (12), the final addition (13); the first half has
             fl(1 / mag), fl(x inv), fl(g .), 2 additions (5), inv inv (3), the product (9), the subtraction (10), / cnt, the sum (12).
  bound_i = E_i + gamma_6 T1_i + gamma_13 T2_i. g_mag is a difference of two terms of similar size (the share of the maximal
  axis' own gradient in it is g_i x_i inv^2 (inv - a): nothing is left of it at mag = 1), which is why the bound is on the
  absolute terms and not on the result.
* Ray sums (hash_encode_bwd_rays_kernel). Lane l adds samples l, l + 64, ... in order, six butterfly steps follow: a term passes
  at most adds = ceil(S / 64) - 1 + 6 additions. d_origins: sum_s b_s + gamma_adds sum_s (|dpos64_s| + b_s) with b_s the sample's
  bound from above. d_directions: the weight is the float64 (t_s + t_(s+1)) / 2 of the fp32 edges; fl(t_s + t_(s+1)) and the
  product add two roundings (/ 2 is exact): sum_s b_s h_s + gamma_(adds+2) sum_s (|dpos64_s| + b_s) h_s.
* accumulate = 1: the kernel adds its value to the prior in one fp32 addition, so the result is fl32(prior + value written by the
  accumulate = 0 call) bit for bit (check_accumulate; tests/test_gpu_depth.py checks its accumulation the same way).
* Scratch-free table paths. Entry e receives n_e contributions c_j = corner_share = ((g bz) by) bx, three roundings each, summed
  in no fixed order on top of the prefill (global float atomics; or LDS sums from 0 and one addition to the prefill: the same
  count): |got - (prefill + ref64)| <= gamma_(n_e+3) (abs64 + |prefill|) + n_e 2^-126, with ref64, abs64 and n_e from
  orc.hashgrid_scatter64 on the points that contribute: a point whose two gradients of a level are both zero is skipped by the
  kernels, the cases zero whole rows of denc, so the skipped points are dropped from the reference's input. Entries nothing
  reaches keep the prefill's bits.

Inputs are finite (asserted). `census` counts the branches a case holds and the case builders assert them wherever a case has
room for its special points: points with mag < 1 and far outside (1e4), two- and three-way exact ties of |coordinate| with mixed
signs, mag == 1.0f exactly, a zero coordinate and a negative maximal coordinate on a contracted point, masked points, points
outside the box, and a point exactly on a grid line of a level (ceil == floor on an axis: that axis contributes exactly 0 there).
"""
import functools

import numpy as np
import torch

import encoder_reference as er
from float64_check import U, check_entries
from oracle import nerfacto_oracle as orc

F32 = np.float32
F64 = np.float64
XFORM_NONE, XFORM_CONTRACT, XFORM_AABB = er.XFORM_NONE, er.XFORM_CONTRACT, er.XFORM_AABB
TRANSFORMS = er.TRANSFORMS
BOX = np.array([[-0.5, -1.0, 0.25], [1.5, 2.0, 1.25]], F32)  # extents 2, 3, 1: the division by 3 rounds, no two axes alike
FLT_MIN = 2.0**-126

# name -> (levels, min_res, max_res, log2_T)
GRIDS = {"L5-T12": er.HASH_GRIDS["four-levels-per-thread-L5-T12"], "L16-T18": er.HASH_GRIDS["pair-sweep-even-and-odd-li-L16-T18"],
         "L8-T12": (8, 16, 256, 12)}
RAY_GRIDS = ("L5-T12", "L16-T18")
POS_M = (1, 255, 256, 257, 1000)           # kHashBlock = 256 threads per block
POS_RAY_S = 5                              # ray mode for the M it divides
RAY_S = (1, 48, 63, 64, 65, 130, 256)      # the edges of the 64-lane strided loop
RAY_N = (1, 3, 4, 5, 257)                  # four rays per workgroup
# the 16-level grid: every S with at least two ray counts, every ray count with at least three S (257 x 65 the largest);
# the 5-level grid: every pair
RAY_SHAPES = {"L16-T18": ((1, 1), (257, 1), (4, 1), (3, 48), (5, 48), (4, 63), (1, 63), (5, 64), (3, 64), (257, 65), (4, 65), (1, 65),
                          (5, 130), (3, 130), (1, 256), (4, 256), (5, 256)),
              "L5-T12": tuple((n, S) for S in RAY_S for n in RAY_N)}
TABLE_GRIDS = {"L5-T12-one-slice": (5, 16, 128, 12), "L5-T15-two-slices": (5, 16, 128, 15)}
TABLE_M = (8191, 8192)                     # direct atomics below 8192 points, the sliced kernel from there


def gamma(k):
    k = np.asarray(k, dtype=F64)
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------- the existing aggregate test's evaluation ------------------------
def _contract_bwd(x, gx, gy, gz):
    """contract_linf_bwd (common.h) vectorised, in the dtype of its arguments."""
    ax, ay, az = x[:, 0].abs(), x[:, 1].abs(), x[:, 2].abs()
    mag = torch.maximum(ax, torch.maximum(ay, az))
    a, inv = 2.0 - 1.0 / mag, 1.0 / mag
    g_a = gx * (x[:, 0] * inv) + gy * (x[:, 1] * inv) + gz * (x[:, 2] * inv)
    g_mag = g_a * (inv * inv) - a * (gx * x[:, 0] + gy * x[:, 1] + gz * x[:, 2]) * (inv * inv)
    t = [(v == mag).to(x.dtype) for v in (ax, ay, az)]
    cnt = t[0] + t[1] + t[2]
    out = [g * a * inv + g_mag * torch.sign(x[:, i]) * t[i] / cnt for i, g in enumerate((gx, gy, gz))]
    inside = mag < 1.0
    return [torch.where(inside, g, o) for g, o in zip((gx, gy, gz), out)]


def _position_grad(raw, table, scal, T, denc, dtype, transform=XFORM_CONTRACT, box=None):
    """dL/d(raw position) of the hash encoding as position_gradient (hashgrid.hip) writes it, evaluated in `dtype` from the
    fp32 cells, weights and table values. raw: [M,3] fp32 positions (of a ray's samples or explicit ones); transform / box: one of
    NSAMD_XFORM_NONE / CONTRACT / AABB and, for AABB, the [2,3] fp32 corners."""
    if transform == XFORM_NONE:
        x, sel = raw, torch.ones(raw.shape[0], dtype=torch.bool)
    else:
        x, sel = orc.normalise_positions(raw, transform == XFORM_CONTRACT, box)
    M, L = x.shape[0], len(scal)
    g = denc.view(M, L, 2).to(dtype)
    G = [torch.zeros(M, dtype=dtype) for _ in range(3)]
    for l, s in enumerate(scal):
        scaled = x * s
        lo, hi = torch.floor(scaled), torch.ceil(scaled)
        w = (scaled - lo).to(dtype)
        lo_i, hi_i = lo.numpy().astype(np.int32), hi.numpy().astype(np.int32)
        v = []
        for k in range(8):
            idx = orc.hash_corner_index((hi_i if k & 1 else lo_i)[:, 0], (hi_i if k & 2 else lo_i)[:, 1],
                                        (hi_i if k & 4 else lo_i)[:, 2], l, T)
            v.append(table[torch.from_numpy(idx)].to(dtype))
        wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
        ux, uy, uz = 1 - wx, 1 - wy, 1 - wz
        yc_zc, yf_zc = v[7] * wx + v[6] * ux, v[5] * wx + v[4] * ux
        yf_zf, yc_zf = v[1] * wx + v[0] * ux, v[3] * wx + v[2] * ux
        zc, zf = yc_zc * wy + yf_zc * uy, yc_zf * wy + yf_zf * uy
        gg = g[:, l]
        lz = (gg * (zc - zf)).sum(1)
        g_zc, g_zf = gg * wz, gg * uz
        ly = (g_zc * (yc_zc - yf_zc) + g_zf * (yc_zf - yf_zf)).sum(1)
        lx = (g_zc * wy * (v[7] - v[6]) + g_zc * uy * (v[5] - v[4]) + g_zf * uy * (v[1] - v[0]) + g_zf * wy * (v[3] - v[2])).sum(1)
        G[0], G[1], G[2] = G[0] + lx * s, G[1] + ly * s, G[2] + lz * s
    if transform == XFORM_CONTRACT:
        G = [gi * sel.to(dtype) / 4.0 for gi in G]
        return torch.stack(_contract_bwd(raw.to(dtype), *G), dim=1)
    G = [gi * sel.to(dtype) for gi in G]
    if transform == XFORM_AABB:
        ext = (box[1] - box[0]).to(dtype)
        G = [gi / ext[i] for i, gi in enumerate(G)]
    return torch.stack(G, dim=1)


# ---------------------------------------------------------------- float64 reference and bounds ------------------------------------
def grid_gradient64(x32, table, scal, log2_T, denc, variant=None):
    """(G, A) [M,3] float64: dL/d(grid input) of the fp32 grid inputs x32 for the feature gradient denc [M, 2L], and the same sum
    over the absolute values of its terms (as _position_gradient64 of tests/test_kernel_helpers_cpu.py defines it)."""
    x = np.asarray(x32, dtype=F32)
    tab = np.asarray(table, dtype=F32)
    M, L, T = x.shape[0], len(scal), 1 << log2_T
    g = np.asarray(denc, dtype=F32).reshape(M, L, 2).astype(F64)
    G, A = np.zeros((M, 3)), np.zeros((M, 3))
    for lvl, scale in enumerate(np.asarray(scal, dtype=F32)):
        sx = (x * scale).astype(F32)
        lo, hi = np.floor(sx), np.ceil(sx)
        w = (sx - lo).astype(F32).astype(F64)
        lo_i, hi_i = lo.astype(np.int32), hi.astype(np.int32)
        q = [tab[orc.hash_corner_index((hi_i if k & 1 else lo_i)[:, 0], (hi_i if k & 2 else lo_i)[:, 1],
                                       (hi_i if k & 4 else lo_i)[:, 2], lvl, T)].astype(F64) for k in range(8)]
        wx, wy, wz = (w[:, a, None] for a in range(3))
        ux, uy, uz = 1.0 - wx, 1.0 - wy, 1.0 - wz
        gf = g[:, lvl]
        yc_zc, yf_zc = q[7] * wx + q[6] * ux, q[5] * wx + q[4] * ux
        yf_zf, yc_zf = q[1] * wx + q[0] * ux, q[3] * wx + q[2] * ux
        zc, zf = yc_zc * wy + yf_zc * uy, yc_zf * wy + yf_zf * uy
        lz = gf * (zc - zf)
        ly = gf * (wz * (yc_zc - yf_zc) + uz * (yc_zf - yf_zf))
        lx = gf * (wz * wy * (q[7] - q[6]) + wz * uy * (q[5] - q[4]) + uz * uy * (q[1] - q[0]) + uz * wy * (q[3] - q[2]))
        s = 1.0 if (variant == "scale_dropped_on_level_1" and lvl == 1) else float(scale)
        G += s * np.stack([lx.sum(1), ly.sum(1), lz.sum(1)], axis=1)
        a = [np.abs(v) for v in q]
        az = (a[7] * wx + a[6] * ux) * wy + (a[5] * wx + a[4] * ux) * uy + (a[3] * wx + a[2] * ux) * wy + (a[1] * wx + a[0] * ux) * uy
        ay = wz * (a[7] * wx + a[6] * ux + a[5] * wx + a[4] * ux) + uz * (a[3] * wx + a[2] * ux + a[1] * wx + a[0] * ux)
        ax = wz * wy * (a[7] + a[6]) + wz * uy * (a[5] + a[4]) + uz * uy * (a[1] + a[0]) + uz * wy * (a[3] + a[2])
        ag = np.abs(gf)
        A += float(scale) * np.stack([(ag * ax).sum(1), (ag * ay).sum(1), (ag * az).sum(1)], axis=1)
    return G, A


def position_gradient64(raw32, sel, transform, box, G, A, L, variant=None):
    """(dpos64, bound) [M,3]: the selector, the affine map and the contraction Jacobian behind grid_gradient64."""
    D = np.array([13 + L, 12 + L, 11 + L], dtype=F64)
    s = np.ones_like(G[:, :1]) if variant == "selector_ignored" else np.asarray(sel, dtype=F64)[:, None]
    g, ab, e = G * s, A * s, gamma(D) * A * np.asarray(sel, dtype=F64)[:, None]
    if transform == XFORM_NONE:
        return g, e
    if transform == XFORM_AABB:
        lo, hi = np.asarray(box, dtype=F32).astype(F64)
        ext = hi - lo
        return g / (np.roll(ext, 1) if variant == "aabb_other_axis" else ext), gamma(D + 2) * ab / ext
    if variant != "quarter_dropped":
        g = g / 4.0
    e = e / 4.0
    x = np.asarray(raw32, dtype=F32).astype(F64)
    ax = np.abs(x)
    mag = ax.max(axis=1, keepdims=True)
    far = ~(mag < 1.0)
    with np.errstate(all="ignore"):
        inv = np.where(far, 1.0 / np.where(far, mag, 1.0), 0.0)
        a = 2.0 - inv
        tie = (ax == mag).astype(F64)
        share = tie / tie.sum(axis=1, keepdims=True)
        if variant == "tie_to_the_first_maximum":
            share = np.zeros_like(tie)
            share[np.arange(x.shape[0]), np.argmax(tie, axis=1)] = 1.0
        sign = np.sign(x)
        if variant == "sign_taken_as_plus":
            sign = (x != 0).astype(F64)
        g_a = (g * (x * inv)).sum(axis=1, keepdims=True)
        g_mag = g_a * (inv * inv) - a * (g * x).sum(axis=1, keepdims=True) * (inv * inv)
        out = g * a * inv + g_mag * sign * share
        gb = np.abs(g) + e
        weight = inv**3 + a * inv * inv
        T1 = gb * a * inv
        T2 = share * (gb * ax).sum(axis=1, keepdims=True) * weight
        E = e * a * inv + share * (e * ax).sum(axis=1, keepdims=True) * weight
        bound = E + gamma(6) * T1 + gamma(13) * T2
    return np.where(far, out, g), np.where(far, bound, e)


def ray_sums64(dpos, bpos, t_bins, variant=None):
    """d_origins / d_directions and their bounds, each [n,3], from the per-sample reference and bound [n S, 3]."""
    t = np.asarray(t_bins, dtype=F32).astype(F64)
    n, S = t.shape[0], t.shape[1] - 1
    p, b = dpos.reshape(n, S, 3).copy(), bpos.reshape(n, S, 3)
    if variant == "sample_64_dropped" and S > 64:
        p[:, 64] = 0.0
    half = ((t[:, :-1] + t[:, 1:]) / 2.0)[..., None]
    hw = t[:, :-1, None] if variant == "half_is_t_s" else half
    adds = -(-S // 64) - 1 + 6
    mag = np.abs(p) + b
    out = {"d_origins": p.sum(1), "d_directions": (p * hw).sum(1)}
    if variant == "credited_to_ray_r_plus_1":
        out = {k: np.roll(v, 1, axis=0) for k, v in out.items()}
    h = np.abs(half)
    bounds = {"d_origins": b.sum(1) + gamma(adds) * mag.sum(1),
              "d_directions": (b * h).sum(1) + gamma(adds + 2) * (mag * h).sum(1)}
    return out, bounds, {"d_origins": b.sum(1), "d_directions": (b * h).sum(1)}


class Case:
    """One call's inputs on the host: points (explicit or rays), transform and box, grid, table and denc [M, 2L]."""

    def __init__(self, name, grid, transform, points, denc_seed):
        self.name, self.grid_name, self.transform = name, grid, transform
        self.L, self.min_res, self.max_res, self.log2_T = (GRIDS.get(grid) or TABLE_GRIDS[grid])
        self.T = 1 << self.log2_T
        self.scal = er.scalings32(self.L, self.min_res, self.max_res)
        self.table = er.table32(self.L, self.log2_T)
        self.points = points
        self.box = BOX
        self.raw = er.positions32(points)
        self.M = self.raw.shape[0]
        self.rays = points.get("positions") is None
        self.n, self.S = (points["t_bins"].shape[0], points["t_bins"].shape[1] - 1) if self.rays else (0, 0)
        self.x, self.sel = er.normalise32(self.raw, transform, BOX)
        self.denc = denc_rows(self.M, self.L, denc_seed)
        for v in list(points.values()) + [self.raw, self.x, self.denc]:
            assert v is None or np.isfinite(v).all(), f"{name}: non-finite input"

    @functools.lru_cache(maxsize=None)
    def reference(self, variant=None):
        """{"dpos": (ref, bound)} and, in ray mode, "d_origins" / "d_directions": (ref, bound, the summed sample bounds)."""
        x = self.x
        if variant == "selector_ignored":
            # (a masked point's grid input is 0: one entry at all eight corners, gradient exactly 0 whatever `sel` multiplies.
            # The seeded defect therefore ignores the selector altogether: the unmasked grid input and no product with it.)
            with np.errstate(all="ignore"):
                lo, hi = self.box
                x = (((er.contract32(self.raw) + F32(2.0)).astype(F32) / F32(4.0)) if self.transform == XFORM_CONTRACT else
                     ((self.raw - lo).astype(F32) / (hi - lo).astype(F32))).astype(F32)
        G, A = grid_gradient64(x, self.table, self.scal, self.log2_T, self.denc, variant)
        dpos, b = position_gradient64(self.raw, self.sel, self.transform, self.box, G, A, self.L, variant)
        out = {"dpos": (dpos, b)}
        if self.rays:
            sums, bounds, sample = ray_sums64(dpos, b, self.points["t_bins"], variant)
            for k in sums:
                out[k] = (sums[k], bounds[k], sample[k])
        return out

    @functools.lru_cache(maxsize=None)
    def table_reference(self):
        """(ref64, abs64, n) [L T, 2] float64 of orc.hashgrid_scatter64 over the rows of denc that are not all zero."""
        live = (self.denc != 0).any(axis=1)
        per_level = (self.denc.reshape(self.M, self.L, 2) != 0).any(axis=2)
        assert bool((per_level == live[:, None]).all()), "a live row has a level with both gradients zero"
        r = orc.hashgrid_scatter64(torch.from_numpy(np.ascontiguousarray(self.x[live])), torch.from_numpy(np.ascontiguousarray(self.denc[live])),
                                   torch.from_numpy(self.scal), self.T)
        return tuple(v.numpy() for v in r)


def denc_rows(M, L, seed):
    """[M, 2L] fp32: magnitudes log-uniform over six decades, both signs, one row in eight all zero (from the third row on)."""
    rs = np.random.RandomState(seed)
    g = rs.choice([-1.0, 1.0], (M, 2 * L)) * 10.0 ** rs.uniform(-6, 0, (M, 2 * L))
    dead = rs.uniform(0, 1, M) < 0.125
    dead[:2] = False
    if M > 8:
        dead[5] = True
    g[dead] = 0.0
    return np.ascontiguousarray(g.astype(F32))


# ---------------------------------------------------------------- points ----------------------------------------------------------
CONTRACT_POINTS = np.array([
    [0.25, -0.5, 0.125],     # mag < 1: identity; (x + 2) / 4 = 9/16 on x: a grid line of level 0 (scale 16)
    [1e4, -3e3, 20.0],       # far outside: the grid input is within 2.5e-5 of the selector's edge
    [-7e3, 1e4, 1e4],        # ... with a two-way tie
    [3.0, -3.0, 0.5],        # two-way ties, mixed signs
    [-2.5, 1.0, 2.5],
    [0.75, 1.5, -1.5],
    [1.5, -1.5, 1.5],        # three-way ties, mixed signs
    [-4.0, -4.0, 4.0],
    [1.0, 0.3, -0.2],        # mag == 1.0f exactly
    [-1.0, 1.0, 0.5],        # ... and tied
    [0.0, 2.0, -0.7],        # a zero coordinate on a contracted point (sign 0)
    [0.0, 0.0, -3.0],
    [-5.0, 1.0, 2.0],        # the maximal coordinate negative
    [0.3, -1.0000001, 0.9],  # just beyond 1
    [1e9, 3.0, 2.0],         # 2 - 1 / mag rounds to 2: on the face, selector 0
    [2.0, -3e8, 1.0],
], F32)
AABB_POINTS = np.array([
    [0.625, 0.5, 0.75],      # inside; (x - lo) / 2 = 9/16: a grid line of level 0
    [-0.5, 0.0, 0.5],        # on the lo face: selector 0
    [1.5, 1.0, 1.0],         # on the hi face
    [1.6, 0.0, 0.5],         # outside on one axis
    [0.0, -1.5, 3.0],        # outside on two
    [0.0, 0.0, 0.75],        # a zero coordinate inside
    [0.5, 0.125, 1.2499999],
], F32)
NONE_POINTS = np.array([
    [0.5625, 0.3, 0.7],      # a grid line of level 0 on x
    [0.5, 0.25, 0.125],      # ... on all three axes
    [0.0, 0.4, 0.9],         # a zero coordinate
    [1.0, 1.0, 1.0],
    [0.0, 0.0, 0.0],
    [0.99999994, 0.3, 0.5],
], F32)
SPECIAL_POINTS = {XFORM_NONE: NONE_POINTS, XFORM_CONTRACT: CONTRACT_POINTS, XFORM_AABB: AABB_POINTS}


def _random_points(rs, M, transform):
    if transform == XFORM_NONE:
        return rs.uniform(0, 1, (M, 3)).astype(F32)
    if transform == XFORM_AABB:  # a share beyond the box
        return (rs.uniform(-0.1, 1.1, (M, 3)).astype(F32) * (BOX[1] - BOX[0]) + BOX[0]).astype(F32)
    return (rs.standard_normal((M, 3)) * 10.0 ** rs.uniform(-1, 1.5, (M, 1))).astype(F32)


def explicit_points(M, transform, seed):
    """{"positions": [M,3]}: the transform's special points first (as many as fit), random points behind them."""
    rs = np.random.RandomState(seed)
    raw = _random_points(rs, M, transform)
    special = SPECIAL_POINTS[transform]
    k = min(M, len(special))
    raw[:k] = np.roll(special, -(seed % len(special)), axis=0)[:k] if M < len(special) else special[:k]
    return {"positions": np.ascontiguousarray(raw)}


# (origin, direction) of the special rays; their bins below. Equal |direction| components keep the ties exact along the ray.
CONTRACT_RAYS = [((0.0, 0.0, 0.0), (1.0, -1.0, 1.0)),      # three-way ties, mixed signs; mag == 1 at the first sample
                 ((0.0, 0.0, 0.0), (-1.0, 0.25, 1.0)),      # two-way ties; the first maximum negative
                 ((0.0, 0.25, -0.5), (-1.0, 0.0, 0.0)),     # the maximal coordinate negative
                 ((0.0, 0.5, -0.25), (0.0, 1.0, 0.0)),      # a zero coordinate; the last sample beyond 2^24: selector 0
                 ((0.25, -0.5, 0.125), (0.0, 0.0, 1.0))]    # stays inside the unit cube, x on a grid line of level 0
AABB_RAYS = [((0.625, 0.5, 0.3), (0.0, 0.0, 1.0))]          # x on a grid line of level 0; leaves the box through z = 1.25
NONE_RAYS = [((0.5625, 0.3, 0.3), (0.0, 0.0, 1.0))]
SPECIAL_RAYS = {XFORM_NONE: NONE_RAYS, XFORM_CONTRACT: CONTRACT_RAYS, XFORM_AABB: AABB_RAYS}


def ray_points(n, S, transform, seed):
    """{"origins", "directions", "t_bins"}: the transform's special rays first (as many as fit), random rays behind them."""
    rs = np.random.RandomState(seed)
    d = rs.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    if transform == XFORM_NONE:
        o, far = rs.uniform(0.3, 0.7, (n, 3)).astype(F32), 0.29
    elif transform == XFORM_AABB:
        o, far = (rs.uniform(0.3, 0.7, (n, 3)).astype(F32) * (BOX[1] - BOX[0]) + BOX[0]).astype(F32), 1.2
    else:
        o, far = (rs.standard_normal((n, 3)) * 0.4).astype(F32), 8.0
    t = np.sort(rs.uniform(0.01, far, (n, S + 1)).astype(F32), axis=-1)
    special = SPECIAL_RAYS[transform]
    for r, (so, sd) in enumerate(special[:n]):
        o[r], d[r] = so, sd
        if transform == XFORM_CONTRACT and r < 4:
            # the first sample at (t0 + t1) / 2 = 1 exactly, the others log-uniform out to 1e4
            steps = np.sort(10.0 ** rs.uniform(-1, 4, S + 1)).astype(F32)
            t[r] = (F32(1.25) + steps).astype(F32)
            t[r, 0], t[r, 1] = 0.75, 1.25
            if r == 0 and S >= 3:
                t[r, -2], t[r, -1] = 1.1e4, 1.3e4  # the last sample at 1.2e4: the grid input 2e-5 below the selector's edge
            if r == 3 and S >= 3:
                t[r, -1] = 1e9
        elif transform == XFORM_CONTRACT:
            t[r] = np.sort(rs.uniform(0.01, 0.6, S + 1).astype(F32))
        elif transform == XFORM_AABB:
            t[r] = np.sort(rs.uniform(0.01, 1.6, S + 1).astype(F32))
    assert bool((np.diff(t, axis=1) >= 0).all())
    return {"origins": np.ascontiguousarray(o), "directions": np.ascontiguousarray(d), "t_bins": np.ascontiguousarray(t)}


def census(case):
    """{branch: number of points of the case that take it}."""
    raw, x, sel = case.raw.astype(F64), case.x, case.sel
    ax = np.abs(raw)
    mag = ax.max(axis=1)
    ties = (ax == mag[:, None]).sum(axis=1)
    live = sel == 1
    contracted = live & (mag >= 1) if case.transform == XFORM_CONTRACT else np.zeros_like(live)
    is_max = ax == mag[:, None]
    mixed = ((np.where(is_max, raw, 0) > 0).any(axis=1)) & ((np.where(is_max, raw, 0) < 0).any(axis=1))
    line = np.zeros(case.M, dtype=bool)
    for scale in case.scal:
        sx = (x * scale).astype(F32)
        line |= ((np.floor(sx) == np.ceil(sx)) & (x > 0)).any(axis=1) & live
    return {"inside": int((live & (mag < 1)).sum()), "far": int((contracted & (mag >= 5e3)).sum()),
            "tie2": int((contracted & (ties == 2) & mixed).sum()), "tie3": int((contracted & (ties == 3) & mixed).sum()),
            "mag_is_1": int((contracted & (mag == 1.0)).sum()), "zero_coordinate": int((contracted & (raw == 0).any(axis=1)).sum()),
            "negative_maximum": int((contracted & (ties == 1) & (np.where(is_max, raw, 0).sum(axis=1) < 0)).sum()),
            "masked": int((~live).sum()), "grid_line": int(line.sum()), "zero_rows": int((~(case.denc != 0).any(axis=1)).sum())}


REQUIRED = {XFORM_NONE: ("grid_line", "zero_rows"), XFORM_AABB: ("masked", "grid_line", "zero_rows"),
            XFORM_CONTRACT: ("inside", "far", "tie2", "tie3", "mag_is_1", "zero_coordinate", "negative_maximum", "masked", "grid_line",
                             "zero_rows")}


def _assert_branches(case):
    c = census(case)
    missing = [k for k in REQUIRED[case.transform] if c[k] == 0]
    assert not missing, f"{case.name}: no point takes {missing} ({c})"
    if case.transform == XFORM_AABB:
        assert c["masked"] < case.M  # points outside the box and points inside it


@functools.lru_cache(maxsize=None)
def position_case(grid, transform, M, mode="positions"):
    """The dpositions case of one grid, transform and M; mode "rays": M / POS_RAY_S rays of POS_RAY_S samples."""
    seed = er.case_seed(M, transform, len(grid), 71 if mode == "rays" else 70)
    if mode == "rays":
        assert M % POS_RAY_S == 0
        pts = ray_points(M // POS_RAY_S, POS_RAY_S, transform, seed)
    else:
        pts = explicit_points(M, transform, seed)
    case = Case(f"{grid}-{mode}-M{M}", grid, transform, pts, seed + 1)
    if M >= 255:  # room for every special point / ray
        _assert_branches(case)
    return case


@functools.lru_cache(maxsize=None)
def ray_case(grid, transform, n, S):
    seed = er.case_seed(n, S, transform, len(grid), 72)
    case = Case(f"{grid}-rays-{n}x{S}", grid, transform, ray_points(n, S, transform, seed), seed + 1)
    if n >= 5 and S >= 48:
        _assert_branches(case)
    return case


@functools.lru_cache(maxsize=None)
def table_case(grid, M, batch):
    """Scratch-free table cases under the contraction. batch "spread": explicit points; "identical": every ray the same
    (M rays of one sample for the odd M, M / 2 rays of two samples otherwise), so an entry receives thousands of contributions."""
    seed = er.case_seed(M, len(grid), 73 if batch == "spread" else 74)
    if batch == "spread":
        pts = explicit_points(M, XFORM_CONTRACT, seed)
    else:
        S = 2 if M % 2 == 0 else 1
        one = ray_points(6, S, XFORM_CONTRACT, seed)
        pts = {k: np.ascontiguousarray(np.repeat(v[5:6], M // S, axis=0)) for k, v in one.items()}
    case = Case(f"{grid}-table-{batch}-M{M}", grid, XFORM_CONTRACT, pts, seed + 1)
    if batch == "identical":
        assert float(case.table_reference()[2].max()) >= 2000
    return case


# ---------------------------------------------------------------- checks ----------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def check_dpositions(case, got, worst, variant=None):
    ref, bound = case.reference(variant)["dpos"]
    got = np.asarray(got, dtype=F32).reshape(case.M, 3)
    masked = case.sel == 0
    assert bool((got[masked] == 0).all()), f"{case.name}: a masked point's gradient is not exactly 0"
    return check_entries("dpos", got, ref, bound, worst)


def check_rays(case, d_origins, d_directions, worst, variant=None, extra=None):
    """extra: {"d_origins", "d_directions"} [n,3] added to the bounds (torch's own reduction on the module route)."""
    r = case.reference(variant)
    for name, got in (("d_origins", d_origins), ("d_directions", d_directions)):
        ref, bound, _ = r[name]
        check_entries(name, np.asarray(got, dtype=F32).reshape(case.n, 3), ref, bound + (extra[name] if extra else 0.0), worst)


def check_rays_against_dpositions(case, dpos, d_origins, d_directions, worst):
    """The two kernels against each other: the ray outputs within the sum of both bounds of dpositions reduced in float64."""
    r = case.reference()
    t = case.points["t_bins"].astype(F64)
    p = np.asarray(dpos, dtype=F32).astype(F64).reshape(case.n, case.S, 3)
    half = ((t[:, :-1] + t[:, 1:]) / 2.0)[..., None]
    for name, got, red in (("d_origins=sum dpos", d_origins, p.sum(1)), ("d_directions=sum dpos h", d_directions, (p * half).sum(1))):
        _, bound, sample = r[name.split("=")[0]]
        check_entries(name, np.asarray(got, dtype=F32).reshape(case.n, 3), red, bound + sample, worst)


def check_accumulate(name, prior, plain, got):
    """accumulate = 1 on `prior` against the accumulate = 0 result `plain`: fl32(prior + plain) bit for bit."""
    want = (np.asarray(prior, dtype=F32) + np.asarray(plain, dtype=F32)).astype(F32)
    assert np.array_equal(bits(want), bits(got)), f"{name}: accumulate = 1 is not fl32(prior + the accumulate = 0 result)"


def check_table(case, got, prefill, worst, name="dtable"):
    """got, prefill: [L T, 2] fp32 (prefill None: zeros)."""
    ref, ab, n = case.table_reference()
    got = np.asarray(got, dtype=F32).reshape(ref.shape)
    pre = np.zeros(ref.shape, F32) if prefill is None else np.asarray(prefill, dtype=F32).reshape(ref.shape)
    untouched = n == 0
    assert np.array_equal(bits(got)[untouched], bits(pre)[untouched]), f"{case.name}: an entry nothing reaches changed"
    bound = gamma(n + 3) * (ab + np.abs(pre.astype(F64))) + n * FLT_MIN
    return check_entries(name, got, pre.astype(F64) + ref, bound, worst)


def torch_reduction_allowance(case):
    """gamma_S on the absolute terms: what torch's own sums over a ray's samples may add on the module route."""
    dpos, b = case.reference()["dpos"]
    t = case.points["t_bins"].astype(F64)
    half = np.abs((t[:, :-1] + t[:, 1:]) / 2.0)[..., None]
    mag = (np.abs(dpos) + b).reshape(case.n, case.S, 3)
    return {"d_origins": gamma(case.S) * mag.sum(1), "d_directions": gamma(case.S) * (mag * half).sum(1)}
