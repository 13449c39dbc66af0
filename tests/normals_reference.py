"""Float64 restatements of the two normals kernels (nsamd_field_normals, nsamd_normals_composite) and the seeded inputs the
normals tests share. Not a test module.

`field_normals_f64` follows NerfactoField.get_density + Field.get_normals of the reference (fields/nerfacto_field.py:203-229,
fields/base_field.py:79-99) on ALREADY NORMALISED fp32 positions: per level `scaled = x * scalings[l]`, its floor and ceil are
formed in fp32 exactly as HashEncoding.pytorch_fwd forms them (field_components/encodings.py:417-458), so the restatement, the
reference and the kernel look at the same cells; everything behind that — the blend, its derivative in the offsets, the base
MLP, the data gradient of the density pre-activation, the normalisation — is float64. The gradient is taken in closed form:
`test_normals_kernel_cpu` checks it against torch.autograd.grad of `field_pre_torch64`, the same composition written in
differentiable float64 torch ops, and against the reference's own fixture.
"""
import numpy as np
import torch

from oracle import nerfacto_oracle as orc


def normalise_fp32(raw, contraction, aabb=None):
    """The field's position normalisation in fp32 torch ops (nerfacto_field.py:205-214) -> (positions * selector, selector)."""
    pos, sel = orc.normalise_positions(torch.as_tensor(raw, dtype=torch.float32).reshape(-1, 3), contraction,
                                       None if aabb is None else torch.as_tensor(aabb, dtype=torch.float32))
    return pos.detach().numpy(), sel.numpy()


def ray_positions_fp32(origins, directions, t_bins):
    """Sample midpoints of rays + bin edges as Frustums.get_positions forms them (cameras/rays.py:50-59), fp32 -> [n * S, 3]."""
    o, d, t = (torch.as_tensor(a, dtype=torch.float32) for a in (origins, directions, t_bins))
    return (o[:, None, :] + d[:, None, :] * ((t[:, :-1] + t[:, 1:]) / 2)[..., None]).reshape(-1, 3).numpy()


def _cells(pos32, scalings, table_size):
    """Per level: (corner table rows [8, M] — bit0 / bit1 / bit2 of the corner = x / y / z is the ceil corner —, offsets [M, 3]
    as float64, the fp32 scale). scaled / floor / ceil in fp32."""
    pos32 = np.ascontiguousarray(pos32, dtype=np.float32)
    out = []
    for lvl, sc in enumerate(np.asarray(scalings, dtype=np.float32)):
        scaled = pos32 * sc  # fp32
        lo, hi = np.floor(scaled), np.ceil(scaled)
        w = scaled.astype(np.float64) - lo.astype(np.float64)
        lo_i, hi_i = lo.astype(np.int32), hi.astype(np.int32)
        idx = np.stack([orc.hash_corner_index((hi_i if k & 1 else lo_i)[:, 0], (hi_i if k & 2 else lo_i)[:, 1],
                                              (hi_i if k & 4 else lo_i)[:, 2], lvl, table_size) for k in range(8)])
        out.append((idx, w, float(sc)))
    return out


def field_normals_f64(pos32, table, scalings, table_size, W0, b0, W1, b1):
    """-> dict: enc [M,32], z [M,64] (hidden pre-activation), geo [M,15], g [M,3] (gradient of the density pre-activation in the
    normalised position), normals [M,3] = -g / max(|g|, 1e-12); all float64."""
    table = np.asarray(table, dtype=np.float64)
    W0, b0, W1, b1 = (np.asarray(a, dtype=np.float64) for a in (W0, b0, W1, b1))
    M = np.asarray(pos32).reshape(-1, 3).shape[0]
    cells = _cells(np.asarray(pos32).reshape(-1, 3), scalings, table_size)
    enc = np.zeros((M, 2 * len(cells)))
    d_enc = np.zeros((M, 2 * len(cells), 3))  # d enc / d offset
    for lvl, (idx, w, _) in enumerate(cells):
        v = table[idx]  # [8, M, 2]
        wx, wy, wz = (w[:, a:a + 1] for a in range(3))
        ux, uy, uz = 1 - wx, 1 - wy, 1 - wz
        yc_zc, yf_zc = v[7] * wx + v[6] * ux, v[5] * wx + v[4] * ux  # x blends (encodings.py:446-449)
        yf_zf, yc_zf = v[1] * wx + v[0] * ux, v[3] * wx + v[2] * ux
        zc, zf = yc_zc * wy + yf_zc * uy, yc_zf * wy + yf_zf * uy  # y blends
        enc[:, 2 * lvl:2 * lvl + 2] = zc * wz + zf * uz
        d_enc[:, 2 * lvl:2 * lvl + 2, 2] = zc - zf
        d_enc[:, 2 * lvl:2 * lvl + 2, 1] = wz * (yc_zc - yf_zc) + uz * (yc_zf - yf_zf)
        d_enc[:, 2 * lvl:2 * lvl + 2, 0] = (wz * (wy * (v[7] - v[6]) + uy * (v[5] - v[4]))
                                           + uz * (wy * (v[3] - v[2]) + uy * (v[1] - v[0])))
    z = enc @ W0.T + b0
    h = np.maximum(z, 0.0)
    out16 = h @ W1.T + b1
    g_enc = (W1[0][None, :] * (z > 0)) @ W0  # [M, 32]
    scale = np.repeat(np.array([c[2] for c in cells]), 2)
    g = np.einsum("mk,mka->ma", g_enc * scale[None, :], d_enc)
    nrm = np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-12)
    return {"enc": enc, "z": z, "pre": out16[:, 0], "geo": out16[:, 1:], "g": g, "normals": -g / nrm}


def field_pre_torch64(pos64, pos32, table, scalings, table_size, W0, b0, W1, b1):
    """The density pre-activation [M] as differentiable float64 torch ops of `pos64` (a leaf holding the fp32 positions' values);
    the cells come from the fp32 positions, as in `field_normals_f64`."""
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    table = T(table)
    feats = []
    for idx, w32, sc in _cells(np.asarray(pos32).reshape(-1, 3), scalings, table_size):
        w = T(w32) + (pos64 - pos64.detach()) * sc  # the fp32 offset's value, slope scalings[l] (offset = scaled - floor)
        v = [table[torch.from_numpy(idx[k].astype(np.int64))] for k in range(8)]
        wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
        yc_zc, yf_zc = v[7] * wx + v[6] * (1 - wx), v[5] * wx + v[4] * (1 - wx)
        yf_zf, yc_zf = v[1] * wx + v[0] * (1 - wx), v[3] * wx + v[2] * (1 - wx)
        zc, zf = yc_zc * wy + yf_zc * (1 - wy), yc_zf * wy + yf_zf * (1 - wy)
        feats.append(zc * wz + zf * (1 - wz))
    h = torch.relu(torch.cat(feats, dim=-1) @ T(W0).t() + T(b0))
    return (h @ T(W1).t() + T(b1))[:, 0]


def pred_normals_f64(raw_pos32, geo, params):
    """The predicted-normals branch (nerfacto_field.py:287-295, field_heads.py:190-206) in float64 on fp32 raw positions and
    float64 geometry features -> (head pre-activation [M,3], pred_normals [M,3])."""
    P = lambda k: params[k].detach().numpy().astype(np.float64)  # noqa: E731
    # the phases are formed in fp32 as NeRFEncoding.pytorch_fwd forms them (encodings.py:148-166: at |x| ~ 1e9, a sample of the
    # reference's fixture, the fp32 phase IS the input); the sines and everything behind them are float64
    x = np.asarray(raw_pos32, dtype=np.float32).reshape(-1, 3)
    scaled = ((np.float32(2 * np.pi) * x)[..., None] * np.array([1.0, 2.0], np.float32)).reshape(x.shape[0], -1)
    phases = np.concatenate([scaled, scaled + np.float32(np.pi / 2)], axis=-1)
    assert phases.dtype == np.float32
    a = np.concatenate([np.sin(phases.astype(np.float64)), geo], axis=-1)
    for j in range(3):
        a = a @ P(f"field.mlp_pred_normals.layers.{j}.weight").T + P(f"field.mlp_pred_normals.layers.{j}.bias")
        if j < 2:
            a = np.maximum(a, 0.0)
    pre = a @ P("field.field_head_pred_normals.net.weight").T + P("field.field_head_pred_normals.net.bias")
    t = np.tanh(pre)
    return pre, t / np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-12)


def normals_composite_f64(weights, normals, pred_pre):
    """nsamd_normals_composite in float64: weights [n,S], per-sample [n,S,3] -> the two shaded images [n,3]."""
    w = np.asarray(weights, dtype=np.float64)[..., None]
    t = np.tanh(np.asarray(pred_pre, dtype=np.float64))
    pred = t / np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-12)
    out = []
    for n in (np.asarray(normals, dtype=np.float64), pred):
        s = (w * n).sum(axis=1)
        out.append((s / (np.linalg.norm(s, axis=-1, keepdims=True) + 1e-10) + 1.0) / 2.0)
    return out[0], out[1]


# ---- seeded field-level inputs ---------------------------------------------------------------------------------------------
def grid_cfg(log2_hashmap_size):
    c = orc.NerfactoCfg(main_grid=orc.HashGridCfg(16, 16, 2048, int(log2_hashmap_size)),
                        prop_grids=(orc.HashGridCfg(5, 16, 128, 8), orc.HashGridCfg(5, 16, 256, 8)), num_images=3)
    c.predict_normals = True
    return c


BASE_KEYS = tuple(f"field.mlp_base.model.1.layers.{j}.{w}" for j in range(2) for w in ("weight", "bias"))  # W0, b0, W1, b1
TABLE_KEY = "field.mlp_base.model.0.hash_table"
AABB = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))

# (M, rays, samples per ray) of the ray-mode form of each size: one 16-sample tile short by one, exact, over by one, one
# sample, and five 48-sample rays' worth plus 7 (more than one wavefront, more than one workgroup)
SIZES = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (1, 17), 5 * 48 + 7: (13, 19)}
TRANSFORMS = ("aabb", "contract", "contract_far")  # contract_far: origins scaled x 6 — most samples are contracted
LOG2 = {"aabb": 10, "contract": 12, "contract_far": 10}


SEED = 1  # (chosen on the CPU: with it the float64 reference keeps every case inside the exclusion cap, test_normals_kernel_cpu)


def case_inputs(M, transform, ray_mode, seed=SEED):
    """One case of the entry-by-entry test: dict with the raw fp32 positions [M,3] (and, ray mode, origins / directions / t_bins
    that produce them), the grid configuration and the parameters."""
    n, S = SIZES[M]
    rs = np.random.RandomState(1000 * seed + 7 * M + 3 * TRANSFORMS.index(transform) + int(ray_mode))
    cfg = grid_cfg(LOG2[transform])
    params = orc.init_params(cfg, seed=seed + 11, table_std=0.5)
    o = rs.uniform(-0.45, 0.45, (n, 3)).astype(np.float32)
    d = rs.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    if transform == "aabb":  # stay inside the box: a masked-out sample has no direction to compare
        t = np.sort(rs.uniform(0.0, 0.5, (n, S + 1)).astype(np.float32), axis=-1)
    else:
        t = np.sort(rs.uniform(0.05, 6.0, (n, S + 1)).astype(np.float32), axis=-1)
        if transform == "contract_far":
            o = (o * np.float32(6.0)).astype(np.float32)
    pos = ray_positions_fp32(o, d, t)
    case = {"M": M, "transform": transform, "ray_mode": ray_mode, "cfg": cfg, "params": params, "positions": pos}
    if ray_mode:
        case.update(origins=o, directions=d, t_bins=t)
    return case


def case_reference(case):
    """Float64 reference of a case + the samples the entry-by-entry comparison keeps: no hidden unit within 1e-5 of its ReLU
    kink (a flip changes the gradient by a finite amount) and |g| >= 1e-3 median |g|."""
    cfg, p = case["cfg"], case["params"]
    contraction = case["transform"] != "aabb"
    pos32, _ = normalise_fp32(case["positions"], contraction, None if contraction else AABB)
    ref = field_normals_f64(pos32, p[TABLE_KEY].numpy(), cfg.main_grid.scalings().numpy(), cfg.main_grid.table_size,
                            *(p[k].numpy() for k in BASE_KEYS))
    gn = np.linalg.norm(ref["g"], axis=-1)
    ref["keep"] = (np.abs(ref["z"]).min(axis=-1) >= 1e-5) & (gn >= 1e-3 * np.median(gn))
    ref["pos32"] = pos32
    return ref


def oracle_gradient_fp32(case):
    """The raw gradient as the fp32 oracle composition computes it on the CPU (oracle/nerfacto_oracle.py: the reference's
    arithmetic, torch autograd) -> [M,3] float32."""
    cfg, p = case["cfg"], case["params"]
    contraction = case["transform"] != "aabb"
    pos, _ = orc.normalise_positions(torch.from_numpy(case["positions"]), contraction, None if contraction else torch.tensor(AABB))
    pos = pos.detach().requires_grad_(True)
    enc = orc.hashgrid_encode(pos, p[TABLE_KEY], cfg.main_grid.scalings(), cfg.main_grid.table_size)
    pre = orc.mlp_forward(enc, p, "field.mlp_base.model.1.")[:, 0]
    return torch.autograd.grad(pre, pos, grad_outputs=torch.ones_like(pre))[0].numpy()


def relative_error(g, ref_g, keep):
    """Per-sample relative L2 error of a gradient against the float64 one, on the kept samples."""
    g, ref_g = np.asarray(g, dtype=np.float64)[keep], ref_g[keep]
    return np.linalg.norm(g - ref_g, axis=-1) / np.linalg.norm(ref_g, axis=-1)


ALL_CASES = [(M, tr, ray) for M in SIZES for tr in TRANSFORMS for ray in (True, False)]
