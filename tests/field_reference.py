"""Float64 reference of the nerfacto main field's MLPs at the ABI of include/nsamd.h (nsamd_field_ray_terms, nsamd_field_mlp_fwd,
nsamd_field_mlp_bwd), the per-entry bounds and the case table that tests/test_field_reference_cpu.py (no GPU) and
tests/test_gpu_field_float64.py (csrc/field_mlp.hip) share.

The reference, all in float64 on the fp32 inputs (x = enc^T [M, 32]; point p takes direction / camera row p // dir_group):
    pre0 = x W0^T + b0      h1 = relu(pre0)      o = h1 W1^T + b1 [M, 16]      density = avg exp(o0) sel
    hin = [SH16((dir + 1) / 2) | o[1:16] | appearance row (camera table, constant row, or nothing)]       (63 or 31 columns)
    p0 = hin Wh0^T + bh0    ha = relu(p0)        p1 = ha Wh1^T + bh1    hb = relu(p1)    p2 = hb Wh2^T + bh2    rgb = sigmoid(p2)
    ray_terms[r] = bh0 + Wh0[:, SH | appearance] [SH16 | appearance row]  [R, 64]        ray_inputs[r] = [SH16 | appearance row]
Backward from ddensity [M] and drgb [M, 3]:
    g2 = drgb sg (1 - sg)        g_hb = (g2 Wh2) [p1 > 0]       g_ha = (g_hb Wh1) [p0 > 0]       g_hin = g_ha Wh0
    g_o = [ddensity avg sel exp(clamp(o0, -15, 15)) | g_hin[:, 16:31]]     (a point with sel == 0 keeps its rgb gradient)
    g_h1 = (g_o W1) [pre0 > 0]   denc = (g_h1 W0)^T [32, M]     dappearance[cam] = sum over the camera's points of g_hin[:, 31:63]
    dW = G^T X and db = sum G for the five layers (G, X) = (g2, hb), (g_hb, ha), (g_ha, hin), (g_o, h1), (g_h1, x).

BOUNDS, per entry, by running error analysis (u = 2^-24; nothing here is fitted to a kernel's output). e(v) bounds the
deviation of a correct fp32 evaluation's v from the float64 v:
  * a layer y = in W^T + b with K inputs: e(y) = (K + 2) u (|in| |W|^T + |b|) + e(in) |W|^T: K - 1 additions of K products in
    any order (an fmaf chain, an MFMA k-order, the ray terms added first or last), the bias, and the store;
  * ReLU: 1-Lipschitz, and the case generator leaves NO unit whose float64 pre-activation lies within 2 e(pre) of zero, so
    the mask is the reference's own on every point: e(relu) = e(pre) [pre > 0], masks carry no error, nothing is excluded;
  * exp: E_EXP (float64_check: 2 ulp of expf, checked by test_expf_budget). density: three factors and the argument's error:
    |density| (expm1(e(o0)) + E_EXP + 3 u). The backward's avg sel exp(clamp(o0)) ddensity: one product more, and the
    clamp is 1-Lipschitz;
  * sigmoid sg = 1 / (1 + exp(-p)): d sg / dp = sg (1 - sg); exp(-p) carries E_EXP, and exp(-p) / (1 + exp(-p)) = 1 - sg of
    it reaches sg; the add and the divide are one rounding each: e(sg) = sg (1 - sg) (e(p) + E_EXP) + 2 u sg;
  * its derivative s' = sg (1 - sg) from the fp32 sg: |1 - 2 sg| e(sg) through both factors, the rounding of 1 - sg and of the
    product (2 u s'), and the ABSOLUTE term u sg for the cancellation in 1 - sg: near sg = 1 the error of sg does not shrink
    with s', so a saturated channel (s' = 1e-13) is allowed what one rounding of sg near 1 moves it by, not 1e-13 u;
  * SH16: every component is a polynomial of degree <= 3 in (dir + 1) / 2 with at most three monomials: the three inputs
    carry u each (the addition of 1), the constants u each, and at most five multiplications / additions follow:
    e(sh) = SH_OPS u sh_abs with SH_OPS = 10 and sh_abs the component with every monomial taken absolute (0.946 zz - 0.315
    cancels: its bound is relative to 0.946 zz + 0.315, not to the difference);
  * a weight gradient dW[n, k] = sum_p G[p, n] X[p, k]: the operands' errors sum_p (e(G) |X| + |G| e(X)), plus
    (chain + 2) u sum_p |G| |X|, `chain` being the number of additions on the longest path to the entry — the launch geometry
    of field_mlp_bwd_impl restated in `field_chains`: the points one workgroup accumulates into a tile (128 per pass of its
    persistent loop), plus the partial rows the reduce sums (ceil(blocks / 16) + 16 + 1) or, without a workspace, the
    workgroup count (float atomics in any order). The four layers whose weight gradient runs on two-piece bf16 operands
    (field_mlp.hip, store_rows_pk / coop_dw_pk: every value is h + m up to 2^-17 of itself) get 2 x 2^-17 sum |G| |X| more,
    the representation error of both operands, and four piece products per point on the chain; their bias gradients (one
    operand, v_dot2c_f32_bf16) 2^-17 sum |G|, with three additions more on their chain (the folds across the lane groups and
    the two point halves). Head layer 0 stays on fp32 operands and does not get that term — also where the ray-terms backward
    forms its 15 geo columns and its bias on two-piece operands: the bound is kept at the tighter fp32 form there, and the
    kernel's worst ratio on those cases is 0.21 (profiles/field_float64_ratios.txt);
  * the appearance gradient of a camera: the sum of its points' e(g_hin) plus (chain + 2) u sum |g_ha| |Wh0| with the chain of
    the path taken (per-tile rows, per-point rows, or one atomic per point of the camera); a camera no point uses: bound 0.
`check_entries` multiplies every bound by 1 + 2^-6 for the second-order terms and the reference's own rounding.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

from float64_check import E_EXP, U, check_entries
from oracle import nerfacto_oracle as orc

SH_OPS = 10
TWO_PIECE = 2.0 ** -17        # |x - (h + m)| <= 2^-17 |x| (field_mlp.hip, "Round 6")
AMBIGUITY_MARGIN = 2.0        # a ReLU is decided when |pre| > 2 e(pre)
MAX_REDRAW_ROUNDS = 64
W_KEYS = ("base_W0", "base_b0", "base_W1", "base_b1", "head_W0", "head_b0", "head_W1", "head_b1", "head_W2", "head_b2")
GRAD_KEYS = tuple("d" + k for k in W_KEYS)
ORACLE_KEYS = ("field.mlp_base.model.1.layers.0.weight", "field.mlp_base.model.1.layers.0.bias",
               "field.mlp_base.model.1.layers.1.weight", "field.mlp_base.model.1.layers.1.bias",
               "field.mlp_head.layers.0.weight", "field.mlp_head.layers.0.bias", "field.mlp_head.layers.1.weight",
               "field.mlp_head.layers.1.bias", "field.mlp_head.layers.2.weight", "field.mlp_head.layers.2.bias")
AVG_INIT_DENSITY = 0.01

# ---- field_mlp.hip / field_reduce.h restated -------------------------------------------------------------------------------
NUM_CUS = 256                  # MI355X; the GPU test passes the device's own count
K_COOP_WAVES = 8               # backward: waves (16-point tiles) per workgroup pass
K_FWD_WAVES = 16
K_PARTIAL_STRIDE = 12544       # floats of one workgroup's weight-gradient partial row
K_REDUCE_GROUPS = 16
K_REDUCE_THREADS = 1024
K_APP_ROWS_MAX_IMAGES = 8192


def _ceil(a, b):
    return -(-a // b)


def bwd_blocks(M, cus=NUM_CUS):
    return min(cus, _ceil(_ceil(M, 16), K_COOP_WAVES))


def workspace_floats(kind, M, cus=NUM_CUS):
    """Floats of the backward workspace of a case: None (NULL), `full` (the header's 256 x 12544 + a row per point, which also
    holds a row per tile), `weights` (exactly the partial rows: no room for appearance rows)."""
    if kind == "null":
        return 0
    if kind == "weights":
        return bwd_blocks(M, cus) * K_PARTIAL_STRIDE
    assert kind == "full", kind
    return max(cus, NUM_CUS) * K_PARTIAL_STRIDE + 32 * M


Case = namedtuple("Case", "name M dir_group app ray_terms selector workspace num_images grad_app spread expect")


def expected_branch(c, cus=NUM_CUS):
    """The conditions of nsamd_field_mlp_fwd / field_mlp_bwd_impl restated -> 'fwd / bwd / weight gradients / appearance
    gradient': fwd, bwd in {plain, rayc}; weights in {partials, atomics}; appearance in {tile_rows, point_rows, atomics, none}."""
    M, dg = c.M, c.dir_group
    tiles, blocks = _ceil(M, 16), bwd_blocks(M, cus)
    ws = workspace_floats(c.workspace, M, cus)
    terms_apply = c.ray_terms and dg % 16 == 0 and M % dg == 0
    partials = ws > 0 and ws >= blocks * K_PARTIAL_STRIDE
    want_app = c.app == "cams" and c.grad_app
    rows_ok = partials and want_app and c.num_images <= K_APP_ROWS_MAX_IMAGES
    if rows_ok and dg % 16 == 0 and M % dg == 0 and ws >= blocks * K_PARTIAL_STRIDE + tiles * 32:
        app = "tile_rows"
    elif rows_ok and dg == 1 and ws >= blocks * K_PARTIAL_STRIDE + M * 32:
        app = "point_rows"
    else:
        app = "atomics" if want_app else "none"
    rayc = partials and terms_apply and (app == "tile_rows" or not want_app)
    return "/".join(("rayc" if terms_apply else "plain", "rayc" if rayc else "plain", "partials" if partials else "atomics", app))


def field_chains(c, cus=NUM_CUS):
    """Additions on the longest path to one entry of a weight / bias / appearance gradient (module docstring)."""
    M, dg = c.M, c.dir_group
    _, _, weights, app = expected_branch(c, cus).split("/")
    blocks = bwd_blocks(M, cus)
    iters = _ceil(_ceil(M, 16), blocks * K_COOP_WAVES)
    points = 16 * K_COOP_WAVES * iters  # (the 1 x 4 layers: two halves of 64 points and one addition: not longer)
    red = blocks if weights == "atomics" else _ceil(blocks, K_REDUCE_GROUPS) + K_REDUCE_GROUPS + 1
    rows_tail = 6 + K_REDUCE_GROUPS + 1  # wave butterfly, the 16 wave sums, the update
    if app == "tile_rows":
        app_chain = 4 + _ceil(M // dg, K_REDUCE_THREADS) * (dg // 16) + rows_tail
    elif app == "point_rows":
        app_chain = _ceil(M, K_REDUCE_THREADS) + rows_tail
    else:
        app_chain = None  # atomics: one per point of the camera at most (+ the tile butterfly): set per camera
    return {"f32": points + red, "pk": 4 * points + red, "bias": 3, "app": app_chain}


# ---- the case table --------------------------------------------------------------------------------------------------------

def _case(tag, M, dg=1, app="cams", rt=False, sel="values", ws="full", images=8, grad_app=True, spread=None, expect=None):
    name = f"{tag}-M{M}-g{dg}-{app}" + ("-rt" if rt else "") + ("" if sel == "values" else f"-sel_{sel}") + f"-ws_{ws}" + \
        ("" if images == 8 else f"-img{images}") + ("" if grad_app else "-noappgrad") + (f"-spread_{spread}" if spread else "")
    c = Case(name, M, dg, app, rt, sel, ws, images if app == "cams" else 0, grad_app, spread, expect)
    assert expected_branch(c) == expect, (name, expected_branch(c), expect)
    return c


_APP_GRAD = {"cams": "point_rows", "const": "none", "none": "none"}
# 16-point tile, 8-wave backward workgroup, 16-wave forward workgroup; per-point cameras with room for a row per point
TILE_EDGES = [_case("edge", M, expect="plain/plain/partials/point_rows") for M in (1, 15, 16, 17, 127, 128, 129, 255, 256, 257)]
APP_SOURCES = ([_case("app", 100, 1, a, expect="plain/plain/partials/" + _APP_GRAD[a]) for a in ("cams", "const", "none")]
               + [_case("app", 96, 16, a, rt=True, expect="rayc/rayc/partials/" + ("tile_rows" if a == "cams" else "none"))
                  for a in ("cams", "const", "none")])
DIR_GROUPS = ([_case("group", 36, 6, rt=True, expect="plain/plain/partials/atomics")]     # terms handed in, not applicable
              + [_case("group", 6 * g, g, rt=True, expect="rayc/rayc/partials/tile_rows") for g in (48, 80)]
              + [_case("group", 36, 6, expect="plain/plain/partials/atomics")]
              + [_case("group", 6 * g, g, expect="plain/plain/partials/tile_rows") for g in (16, 48, 80)])
FORWARD_VARIANTS = [_case("fwd", 100, sel="none", expect="plain/plain/partials/point_rows"),
                    _case("fwd", 100, sel="zeros", expect="plain/plain/partials/point_rows"),
                    _case("fwd", 96, 16, rt=True, sel="zeros", expect="rayc/rayc/partials/tile_rows")]
WORKSPACES = [
    _case("ws", 100, ws="null", expect="plain/plain/atomics/atomics"),
    _case("ws", 100, ws="weights", expect="plain/plain/partials/atomics"),
    _case("ws", 100, images=8193, expect="plain/plain/partials/atomics"),
    _case("ws", 100, grad_app=False, expect="plain/plain/partials/none"),
    _case("ws", 96, 16, ws="null", expect="plain/plain/atomics/atomics"),
    _case("ws", 96, 16, ws="weights", expect="plain/plain/partials/atomics"),
    _case("ws", 96, 16, images=8193, expect="plain/plain/partials/atomics"),
    _case("ws", 96, 16, grad_app=False, expect="plain/plain/partials/none"),
    _case("ws", 96, 16, rt=True, ws="null", expect="rayc/plain/atomics/atomics"),       # the backward's ray terms need the rows
    _case("ws", 96, 16, rt=True, ws="weights", expect="rayc/plain/partials/atomics"),
    _case("ws", 96, 16, rt=True, images=8193, expect="rayc/plain/partials/atomics"),
    _case("ws", 96, 16, rt=True, grad_app=False, expect="rayc/rayc/partials/none"),
]
SPREAD = [_case("spread", 200, spread="o0", expect="plain/plain/partials/point_rows"),
          _case("spread", 200, spread="p2", expect="plain/plain/partials/point_rows"),
          _case("spread", 208, 16, rt=True, spread="o0", expect="rayc/rayc/partials/tile_rows"),
          _case("spread", 208, 16, rt=True, spread="p2", expect="rayc/rayc/partials/tile_rows")]
# more tiles than 256 CUs x 16 waves forward and 256 x 8 backward: the second pass of a persistent workgroup
PERSISTENT = [_case("loop", 65553, expect="plain/plain/partials/point_rows"),
              _case("loop", 48 * 1366, 48, rt=True, expect="rayc/rayc/partials/tile_rows")]
SMALL_CASES = TILE_EDGES + APP_SOURCES + DIR_GROUPS + FORWARD_VARIANTS + WORKSPACES + SPREAD
CASES = SMALL_CASES + PERSISTENT
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RAY_TERM_CASES = [(R, a, keep) for R in (1, 15, 17, 65) for a in ("cams", "const", "none") for keep in (False, True)]
CARRIER_FEATURE, CARRIER_GEO = 5, 3   # spread cases: enc feature 5 -> base unit 0 -> (o0 | geo output 3 -> head units 0 -> p2)
SINGLE_CAMERA, UNUSED_CAMERA = 1, 2


# ---- inputs ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def base_params():
    """The ten MLP tensors of init_params(NerfactoCfg(), seed=0, table_std=0.3), fp32 numpy, in nsamd_field_mlp order."""
    p = orc.init_params(orc.NerfactoCfg(), seed=0, table_std=0.3)
    return tuple(p[k].numpy().copy() for k in ORACLE_KEYS)


def app_dim_of(app):
    return 0 if app == "none" else 32


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def draw_inputs(name, M, dir_group, app, selector="values", num_images=8, spread=None):
    """fp32 inputs of one call, seeded by `name`, WITHOUT undecided ReLUs (asserted; `rounds` = redraw rounds it took)."""
    rs = np.random.RandomState(_seed(name))
    P = {k: v.copy() for k, v in zip(W_KEYS, base_params())}
    ad = app_dim_of(app)
    if ad == 0:
        P["head_W0"] = np.ascontiguousarray(P["head_W0"][:, :31])
    R = _ceil(M, dir_group)
    enc = (0.3 * rs.standard_normal((32, M))).astype(np.float32)
    d = rs.standard_normal((R, 3))
    dirs = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    inp = {"M": M, "dir_group": dir_group, "directions": dirs, "camera_indices": None, "appearance_const": None,
           "appearance": None, "num_images": 0, "avg": AVG_INIT_DENSITY, "selector": None}
    if app == "cams":
        assert num_images >= 5
        inp["appearance"] = rs.standard_normal((num_images, 32)).astype(np.float32)
        inp["num_images"] = num_images
        pool = np.array([0, 3, 4] + ([num_images - 1] if num_images > 5 else []))
        cams = pool[rs.randint(0, len(pool), R)].astype(np.int64)
        cams[rs.randint(0, R)] = SINGLE_CAMERA      # one row (with dir_group 1: one POINT) uses it; nothing uses UNUSED_CAMERA
        inp["camera_indices"] = cams
    elif app == "const":
        inp["appearance_const"] = rs.standard_normal(32).astype(np.float32)
    if selector == "values":
        inp["selector"] = rs.uniform(0.5, 1.5, M).astype(np.float32)
    elif selector == "zeros":
        inp["selector"] = (rs.uniform(0, 1, M) > 0.3).astype(np.float32)
        inp["selector"][-1] = 0.0
    carriers = []
    if spread is not None:
        f, g, top = CARRIER_FEATURE, CARRIER_GEO, (40.0 if spread == "o0" else 60.0)
        carriers = [f]
        enc[f] = rs.permutation(np.linspace(0.01, top, M)).astype(np.float32)
        P["base_W0"][0] = 0.0
        P["base_W0"][0, f] = 1.0
        P["base_b0"][0] = 0.0
        if spread == "o0":       # o0 = enc[f] - 20 + the other units' small share: over [-20, 20]
            P["base_W1"][0, 0] = 1.0
            P["base_b1"][0] = -20.0
        else:                    # p2 = +-(relu(geo g) - 30) + the other units' share: over [-30, 30], both signs per channel
            P["base_W1"][g, 0] = 1.0
            P["head_W0"][0] = 0.0
            P["head_W0"][0, 16 + g - 1] = 1.0
            P["head_b0"][0] = 0.0
            P["head_W1"][0] = 0.0
            P["head_W1"][0, 0] = 1.0
            P["head_b1"][0] = 0.0
            P["head_W2"][:, 0] = (1.0, -1.0, 1.0)
            P["head_b2"][:] = (-30.0, 30.0, -30.0)
    inp.update(P)
    inp["enc"] = enc
    inp["ddensity"] = rs.standard_normal(M).astype(np.float32)
    inp["drgb"] = rs.standard_normal((M, 3)).astype(np.float32)
    free = np.array([k for k in range(32) if k not in carriers])
    for rounds in range(MAX_REDRAW_ROUNDS + 1):
        bad = np.flatnonzero(forward64(inp)["undecided"])
        if bad.size == 0:
            break
        assert rounds < MAX_REDRAW_ROUNDS, (name, bad.size)
        enc[np.ix_(free, bad)] = (0.3 * rs.standard_normal((free.size, bad.size))).astype(np.float32)
    inp["rounds"] = rounds
    assert not forward64(inp)["undecided"].any(), name
    return inp


def make_inputs(c):
    return draw_inputs(c.name, c.M, c.dir_group, c.app, c.selector, c.num_images or 8, c.spread)


# ---- the reference ---------------------------------------------------------------------------------------------------------

def sh16(d):
    """-> (SH16 of d [R, 3], every monomial taken absolute), float64."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    xx, yy, zz = x * x, y * y, z * z
    one = np.ones_like(x)
    c = [0.28209479177387814 * one, 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
         1.0925484305920792 * x * y, 1.0925484305920792 * y * z, 0.9461746957575601 * zz - 0.31539156525251999,
         1.0925484305920792 * x * z, 0.5462742152960396 * (xx - yy), 0.5900435899266435 * y * (3 * xx - yy),
         2.890611442640554 * x * y * z, 0.4570457994644658 * y * (5 * zz - 1), 0.3731763325901154 * z * (5 * zz - 3),
         0.4570457994644658 * x * (5 * zz - 1), 1.445305721320277 * z * (xx - yy), 0.5900435899266435 * x * (xx - 3 * yy)]
    a = [0.28209479177387814 * one, 0.4886025119029199 * ay, 0.4886025119029199 * az, 0.4886025119029199 * ax,
         1.0925484305920792 * ax * ay, 1.0925484305920792 * ay * az, 0.9461746957575601 * zz + 0.31539156525251999,
         1.0925484305920792 * ax * az, 0.5462742152960396 * (xx + yy), 0.5900435899266435 * ay * (3 * xx + yy),
         2.890611442640554 * ax * ay * az, 0.4570457994644658 * ay * (5 * zz + 1), 0.3731763325901154 * az * (5 * zz + 3),
         0.4570457994644658 * ax * (5 * zz + 1), 1.445305721320277 * az * (xx + yy), 0.5900435899266435 * ax * (xx + 3 * yy)]
    return np.stack(c, 1), np.stack(a, 1)


def _layer(x, e_x, W, b, K):
    """-> (x W^T + b, its bound)."""
    return x @ W.T + b, (K + 2) * U * (np.abs(x) @ np.abs(W).T + np.abs(b)) + e_x @ np.abs(W).T


def _f64(inp, k):
    return None if inp[k] is None else inp[k].astype(np.float64)


def ray_rows(inp):
    """Per ray: SH16 and its bound, the appearance row ([R, 32] or [R, 0])."""
    dirs = _f64(inp, "directions")
    sh, sh_abs = sh16((dirs + 1.0) / 2.0)
    R = dirs.shape[0]
    if inp["camera_indices"] is not None:
        app = _f64(inp, "appearance")[inp["camera_indices"]]
    elif inp["appearance_const"] is not None:
        app = np.broadcast_to(_f64(inp, "appearance_const"), (R, 32)).copy()
    else:
        app = np.zeros((R, 0))
    return sh, SH_OPS * U * sh_abs, app


def ray_terms64(inp):
    """nsamd_field_ray_terms -> dict(ray_terms [R, 64], ray_inputs [R, 16 + app_dim], e_ray_terms, e_ray_inputs)."""
    sh, e_sh, app = ray_rows(inp)
    W, b = _f64(inp, "head_W0"), _f64(inp, "head_b0")
    cols = np.r_[0:16, 31:31 + app.shape[1]]
    x, e_x = np.concatenate([sh, app], 1), np.concatenate([e_sh, np.zeros_like(app)], 1)
    t, e_t = _layer(x, e_x, W[:, cols], b, 48)
    return {"ray_terms": t, "e_ray_terms": e_t, "ray_inputs": x, "e_ray_inputs": e_x}


def forward64(inp):
    """-> dict of the float64 forward: density, rgb, their bounds e_density / e_rgb, every intermediate v with its bound e_v, and
    `undecided` [M]: the point owns a hidden unit with |pre| <= AMBIGUITY_MARGIN e(pre) (and e(pre) > 0: a pre-activation whose
    every term is exactly 0 is 0 in fp32 too)."""
    M, dg = inp["M"], inp["dir_group"]
    P = {k: _f64(inp, k) for k in W_KEYS}
    x = _f64(inp, "enc").T
    sel = np.ones(M) if inp["selector"] is None else _f64(inp, "selector")
    r = {"x": x, "sel": sel}
    r["pre0"], r["e_pre0"] = _layer(x, np.zeros_like(x), P["base_W0"], P["base_b0"], 32)
    r["h1"], r["e_h1"] = np.maximum(r["pre0"], 0), r["e_pre0"] * (r["pre0"] > 0)
    r["o"], r["e_o"] = _layer(r["h1"], r["e_h1"], P["base_W1"], P["base_b1"], 64)
    o0, e_o0 = r["o"][:, 0], r["e_o"][:, 0]
    r["density"] = inp["avg"] * np.exp(o0) * sel
    r["e_density"] = np.abs(r["density"]) * (np.expm1(e_o0) + E_EXP + 3 * U)
    sh, e_sh, app = ray_rows(inp)
    rp = np.arange(M) // dg
    r["rp"] = rp
    r["hin"] = np.concatenate([sh[rp], r["o"][:, 1:], app[rp]], 1)
    r["e_hin"] = np.concatenate([e_sh[rp], r["e_o"][:, 1:], np.zeros((M, app.shape[1]))], 1)
    r["p0"], r["e_p0"] = _layer(r["hin"], r["e_hin"], P["head_W0"], P["head_b0"], 64)
    r["ha"], r["e_ha"] = np.maximum(r["p0"], 0), r["e_p0"] * (r["p0"] > 0)
    r["p1"], r["e_p1"] = _layer(r["ha"], r["e_ha"], P["head_W1"], P["head_b1"], 64)
    r["hb"], r["e_hb"] = np.maximum(r["p1"], 0), r["e_p1"] * (r["p1"] > 0)
    r["p2"], r["e_p2"] = _layer(r["hb"], r["e_hb"], P["head_W2"], P["head_b2"], 64)
    p2 = r["p2"]
    r["rgb"] = sg = 1.0 / (1.0 + np.exp(-p2))
    r["sgd"] = sgd = 1.0 / ((1.0 + np.exp(-p2)) * (1.0 + np.exp(p2)))  # sg (1 - sg) without the cancellation
    r["e_rgb"] = sgd * (np.expm1(r["e_p2"]) + E_EXP) + 2 * U * sg
    und = np.zeros(M, bool)
    r["unit_bound_max"] = 0.0
    for k in ("pre0", "p0", "p1"):
        und |= ((np.abs(r[k]) <= AMBIGUITY_MARGIN * r["e_" + k]) & (r["e_" + k] > 0)).any(1)
        r["unit_bound_max"] = max(r["unit_bound_max"], float(r["e_" + k].max()))
    r["undecided"] = und
    return r


def _wgrad(out, name, G, e_G, X, e_X, chain, chain_b, two_piece):
    A = np.abs(G).T @ np.abs(X)
    Ab = np.abs(G).sum(0)
    tp = 2 * TWO_PIECE if two_piece else 0.0
    out["d" + name + "W"], out["d" + name + "b"] = G.T @ X, G.sum(0)
    out["e_d" + name + "W"] = e_G.T @ np.abs(X) + np.abs(G).T @ e_X + ((chain + 2) * U + tp) * A
    out["e_d" + name + "b"] = e_G.sum(0) + ((chain_b + 2) * U + tp / 2) * Ab
    out["abs_d" + name + "W"] = A


def backward64(inp, fw, chains, mutate=None):
    """-> denc [32, M], the ten parameter gradients d<key>, dappearance [num_images, 32] (cameras only), each with its bound
    e_<name>. `chains`: field_chains of the case. `mutate` (the CPU test's deliberately wrong evaluations): 'no_clamp' |
    'wrong_channel' | 'selector_ignored'."""
    M = inp["M"]
    P = {k: _f64(inp, k) for k in W_KEYS}
    dd, drgb = _f64(inp, "ddensity"), _f64(inp, "drgb")
    sg, sgd = fw["rgb"], fw["sgd"]
    e_sg = fw["e_rgb"]
    e_sgd = np.abs(1 - 2 * sg) * e_sg + 2 * U * sgd + U * sg
    if mutate == "wrong_channel":
        sgd = np.roll(sgd, 1, axis=1)
    g2 = drgb * sgd
    e_g2 = np.abs(drgb) * e_sgd + U * np.abs(g2)
    out = {}
    f32, pk, cb = chains["f32"], chains["pk"], chains["bias"]
    _wgrad(out, "head_2", g2, e_g2, fw["hb"], fw["e_hb"], pk, pk + cb, True)
    m1, m0, mb = fw["p1"] > 0, fw["p0"] > 0, fw["pre0"] > 0
    g_hb, e_g_hb = _layer(g2, e_g2, P["head_W2"].T, 0.0, 3)
    g_hb, e_g_hb = g_hb * m1, e_g_hb * m1
    _wgrad(out, "head_1", g_hb, e_g_hb, fw["ha"], fw["e_ha"], pk, pk + cb, True)
    g_ha, e_g_ha = _layer(g_hb, e_g_hb, P["head_W1"].T, 0.0, 64)
    g_ha, e_g_ha = g_ha * m0, e_g_ha * m0
    _wgrad(out, "head_0", g_ha, e_g_ha, fw["hin"], fw["e_hin"], f32, f32 + cb, False)
    g_hin, e_g_hin = _layer(g_ha, e_g_ha, P["head_W0"].T, 0.0, 64)
    o0, e_o0 = fw["o"][:, 0], fw["e_o"][:, 0]
    sel = np.ones(M) if mutate == "selector_ignored" else fw["sel"]
    arg = o0 if mutate == "no_clamp" else np.clip(o0, -15.0, 15.0)
    g_o0 = dd * sel * inp["avg"] * np.exp(arg)
    g_o = np.concatenate([g_o0[:, None], g_hin[:, 16:31]], 1)
    e_g_o = np.concatenate([(np.abs(g_o0) * (np.expm1(e_o0) + E_EXP + 4 * U))[:, None], e_g_hin[:, 16:31]], 1)
    _wgrad(out, "base_1", g_o, e_g_o, fw["h1"], fw["e_h1"], pk, pk + cb, True)
    g_h1, e_g_h1 = _layer(g_o, e_g_o, P["base_W1"].T, 0.0, 16)
    g_h1, e_g_h1 = g_h1 * mb, e_g_h1 * mb
    _wgrad(out, "base_0", g_h1, e_g_h1, fw["x"], np.zeros_like(fw["x"]), pk, pk + cb, True)
    denc, e_denc = _layer(g_h1, e_g_h1, P["base_W0"].T, 0.0, 64)
    out["denc"], out["e_denc"] = denc.T.copy(), e_denc.T.copy()
    for layer, key in (("head_2", "head_W2"), ("head_1", "head_W1"), ("head_0", "head_W0"), ("base_1", "base_W1"), ("base_0", "base_W0")):
        for a, b in (("W", key), ("b", key.replace("W", "b"))):
            for pre in ("d", "e_d"):
                out[pre + b] = out.pop(pre + layer + a)
        out["abs_d" + key] = out.pop("abs_d" + layer + "W")
    if inp["camera_indices"] is not None:
        cp = inp["camera_indices"][fw["rp"]]
        n, A_app = inp["num_images"], np.abs(g_ha) @ np.abs(P["head_W0"][:, 31:63])
        dapp, e_sum, a_sum = np.zeros((n, 32)), np.zeros((n, 32)), np.zeros((n, 32))
        np.add.at(dapp, cp, g_hin[:, 31:63])
        np.add.at(e_sum, cp, e_g_hin[:, 31:63])
        np.add.at(a_sum, cp, A_app)
        count = np.bincount(cp, minlength=n).astype(np.float64)[:, None]
        chain = (count + 4) if chains["app"] is None else chains["app"]
        out["dappearance"], out["e_dappearance"] = dapp, e_sum + (chain + 2) * U * a_sum
        out["camera_points"] = count[:, 0]
    for k in ("g2", "g_hb", "g_ha", "g_hin", "g_o", "g_h1"):
        out[k] = locals()[k]
    return out


def reference_of(c, inp, cus=NUM_CUS):
    fw = forward64(inp)
    r = dict(fw)
    r.update(backward64(inp, fw, field_chains(c, cus)))
    if c.ray_terms:
        r.update(ray_terms64(inp))
    return r


@functools.lru_cache(maxsize=4)
def _cached(name, cus):
    c = BY_NAME[name]
    inp = make_inputs(c)
    return inp, reference_of(c, inp, cus)


def case_data(name, cus=NUM_CUS):
    """(inputs, reference) of a case of the table, computed once per process for the most recent cases. Read-only."""
    return _cached(name, cus)


FORWARD_OUTPUTS = ("density", "rgb")
BACKWARD_OUTPUTS = ("denc",) + GRAD_KEYS + ("dappearance",)


def check(c, ref, got, worst):
    """Every entry of every output in `got` against the reference inside its bound (float64_check.check_entries: nothing
    excluded, a non-finite entry fails); the gradient of a camera no point uses must be exactly 0. -> worst ratios by output."""
    for k, g in got.items():
        g = np.asarray(g)
        assert g.shape == ref[k].shape, (c.name, k, g.shape, ref[k].shape)
        check_entries(k, g, ref[k], ref["e_" + k], worst)
    if "dappearance" in got:
        unused = ref["camera_points"] == 0
        assert unused[UNUSED_CAMERA] and not np.asarray(got["dappearance"])[unused].any(), \
            f"{c.name}: the gradient row of an unused camera is not exactly 0"
    return worst


# ---- the same graph under torch (float64: autograd against the reference; float32: a correct fp32 evaluation) ----------------

def torch_evaluate(inp, dtype):
    """density, rgb, denc, the ten parameter gradients and dappearance by torch autograd on the CPU in `dtype`, with the
    oracle's trunc_exp and sh_levels4."""
    M, dg = inp["M"], inp["dir_group"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    P = {k: t(inp[k]).requires_grad_(True) for k in W_KEYS}
    x = t(inp["enc"].T).requires_grad_(True)
    sel = torch.ones(M, dtype=dtype) if inp["selector"] is None else t(inp["selector"])
    rp = torch.arange(M) // dg
    h = torch.relu(x @ P["base_W0"].t() + P["base_b0"]) @ P["base_W1"].t() + P["base_b1"]
    density = inp["avg"] * orc.trunc_exp(h[:, 0]) * sel
    parts = [orc.sh_levels4((t(inp["directions"]) + 1.0) / 2.0)[rp], h[:, 1:]]
    table = None
    if inp["camera_indices"] is not None:
        table = t(inp["appearance"]).requires_grad_(True)
        parts.append(table[torch.from_numpy(inp["camera_indices"])[rp]])
    elif inp["appearance_const"] is not None:
        parts.append(t(inp["appearance_const"]).expand(M, 32))
    p0 = torch.cat(parts, -1) @ P["head_W0"].t() + P["head_b0"]
    p1 = torch.relu(p0) @ P["head_W1"].t() + P["head_b1"]
    rgb = torch.sigmoid(torch.relu(p1) @ P["head_W2"].t() + P["head_b2"])
    ((density * t(inp["ddensity"])).sum() + (rgb * t(inp["drgb"])).sum()).backward()
    out = {"density": density.detach().numpy(), "rgb": rgb.detach().numpy(), "denc": x.grad.t().contiguous().numpy()}
    out.update({"d" + k: P[k].grad.numpy() for k in W_KEYS})
    if table is not None:
        out["dappearance"] = table.grad.numpy()
    return out


def bf16_pieces(x):
    """The two-piece representation of field_mlp.hip's split_pair: h = bf16(x) (RNE), m = bf16(x - h), as float64."""
    def rne(v):
        b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
        return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    x32 = np.asarray(x, np.float32)
    h = rne(x32)
    return h.astype(np.float64), rne(x32 - h).astype(np.float64)


def launch_note(c):
    return f"{c.name} [{c.expect}]"

