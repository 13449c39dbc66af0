"""Torch restatements of nsamd_normals_losses and nsamd_nerf_encode_bwd_rays and the seeded inputs their tests share. Not a test
module.

The three reference functions are restated verbatim in meaning — orientation_loss and pred_normal_loss of
model_components/losses.py:201-222, PredNormalsFieldHead's activation (field_components/field_heads.py: tanh, then
torch.nn.functional.normalize) — and the gradients come from autograd, exactly as the reference gets them: evaluated in float64
they are the yardstick, in fp32 they are the reference's own rounding, whose distance from float64 is the unit the kernels'
error is measured in (`MARGIN` of them, the rule of tests/test_depth_cpu.py; the unit is floored at one fp32 ulp).
"""
import numpy as np
import torch

from depth_reference import rel_err  # noqa: F401  (largest entrywise relative error; exact zeros must be exact zeros)

MARGIN = 4.0
ULP = 2.0 ** -23
CASES = ((7, 48), (5, 1), (9, 130))  # (rays, samples per ray) of the fixture; the GPU test adds (2, 4096)
OUTPUTS = ("orientation_per_ray", "pred_per_ray", "d_pred_pre", "d_directions")


# ---- the reference's three functions --------------------------------------------------------------------------------------
def orientation_loss(weights, normals, viewdirs):
    """losses.py:201-213: weights [*bs,S,1], normals [*bs,S,3], viewdirs [*bs,3] -> [*bs]: sum_s w min(0, n . (-v))^2, the
    minimum as torch.fmin takes it (a NaN product counts as 0)."""
    towards_camera = torch.sum(normals * (-viewdirs).unsqueeze(-2), dim=-1)
    back_facing = torch.fmin(towards_camera.new_zeros(()).expand_as(towards_camera), towards_camera)
    return torch.sum(weights.squeeze(-1) * back_facing.square(), dim=-1)


def pred_normal_loss(weights, normals, pred_normals):
    """losses.py:216-222: sum_s w (1 - n . p)."""
    agreement = torch.sum(normals * pred_normals, dim=-1)
    return torch.sum(weights.squeeze(-1) * (1.0 - agreement), dim=-1)


def pred_normals_head(pre):
    """PredNormalsFieldHead.forward on the head's linear output."""
    return torch.nn.functional.normalize(torch.tanh(pre), dim=-1)


def normals_losses_torch(weights, normals, pred_pre, directions, dtype=torch.float64, orientation_scale=1.0, pred_scale=1.0):
    """nsamd_normals_losses restated: weights [n,S], normals / pred_pre [n,S,3] (or [n*S,3]), directions [n,3] -> dict of numpy
    arrays in `dtype`: the two unscaled per-ray terms, d_pred_pre [n*S,3] = pred_scale * d sum(pred term) / d pred_pre and
    d_directions [n,3] = orientation_scale * d sum(orientation term) / d directions. Weights and normals are constants."""
    w = torch.as_tensor(np.asarray(weights)).to(dtype)
    n_rays, S = w.shape
    nr = torch.as_tensor(np.asarray(normals)).to(dtype).reshape(n_rays, S, 3)
    x = torch.as_tensor(np.asarray(pred_pre)).to(dtype).reshape(n_rays, S, 3).clone().requires_grad_(True)
    v = torch.as_tensor(np.asarray(directions)).to(dtype).reshape(n_rays, 3).clone().requires_grad_(True)
    orientation = orientation_loss(w[..., None], nr, v)
    pred = pred_normal_loss(w[..., None], nr, pred_normals_head(x))
    (d_x,) = torch.autograd.grad(pred.sum(), x)
    (d_v,) = torch.autograd.grad(orientation.sum(), v)
    return {"orientation_per_ray": orientation.detach().numpy(), "pred_per_ray": pred.detach().numpy(),
            "d_pred_pre": (d_x * pred_scale).reshape(-1, 3).numpy(), "d_directions": (d_v * orientation_scale).numpy()}


# ---- the frequency encoding and its ray gradient ------------------------------------------------------------------------------
def nerf_encode_torch(x, freqs, include_input=False):
    """NeRFEncoding.pytorch_fwd without covariances (encodings.py:148-189): [sin(s), sin(s + pi/2), x], s[d F + f] = 2 pi x_d f_f."""
    scaled = (2 * torch.pi * x)[..., None] * freqs
    scaled = scaled.reshape(*scaled.shape[:-2], -1)
    out = torch.sin(torch.cat([scaled, scaled + torch.pi / 2.0], dim=-1))
    return torch.cat([out, x], dim=-1) if include_input else out


def nerf_encode_bwd_rays_torch(origins, directions, t_bins, freqs, include_input, d_out, dtype=torch.float64):
    """nsamd_nerf_encode_bwd_rays restated: the encoding of the rays' sample midpoints (cameras/rays.py:50-59) under the upstream
    gradient `d_out` [n*S, 6 F (+3)], differentiated by autograd with respect to origins and directions -> two [n,3] arrays."""
    T = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    o, d = T(origins).clone().requires_grad_(True), T(directions).clone().requires_grad_(True)
    t = T(t_bins)
    pos = o[:, None, :] + d[:, None, :] * ((t[:, :-1] + t[:, 1:]) / 2)[..., None]
    enc = nerf_encode_torch(pos.reshape(-1, 3), T(freqs), include_input)
    g_o, g_d = torch.autograd.grad((enc * T(d_out)).sum(), (o, d))
    return g_o.numpy(), g_d.numpy()


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------
def case_inputs(n, S, seed=0):
    """Inputs of one (rays, samples) case with the planted edge cases: ray 0 has all-zero weights; the normals of ray 1 all face
    the camera (n . v < 0: orientation term and its gradient exactly 0); sample (min(2, n - 1), 0) is masked (normal exactly 0); the
    pre-activation of sample (n - 1, S - 1) is exactly (0, 0, 0). Pre-activations ~ 0.7 N(0, 1): |tanh| stays clear of 1, where
    1 - t^2 has no fp32 digits left in any implementation."""
    rs = np.random.RandomState(1000 * seed + 13 * n + S)
    unit = lambda a: (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)  # noqa: E731
    w = rs.uniform(0.0, 2.0 / max(S, 2), (n, S)).astype(np.float32)
    nr = unit(rs.standard_normal((n, S, 3)))
    x = (0.7 * rs.standard_normal((n, S, 3))).astype(np.float32)
    v = unit(rs.standard_normal((n, 3)))
    w[0] = 0.0
    towards = np.einsum("sc,c->s", nr[1].astype(np.float64), v[1].astype(np.float64)) > 0  # n . (-v) < 0: faces away -> flip
    nr[1][towards] = -nr[1][towards]
    nr[min(2, n - 1), 0] = 0.0
    x[n - 1, S - 1] = 0.0
    return {"weights": w, "normals": nr, "pred_pre": x, "directions": v}


def encode_case_inputs(n, S, stride, include_input, seed=0):
    """Rays, bin edges, the two frequencies of the field's position encoding and an upstream gradient whose rows are `stride`
    floats apart (the columns behind the encoding's hold other values, which the kernel must not read as gradient)."""
    rs = np.random.RandomState(2000 * seed + 17 * n + S + stride + int(include_input))
    o = rs.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    d = rs.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = np.sort(rs.uniform(0.05, 2.0, (n, S + 1)).astype(np.float32), axis=-1)
    width = 12 + (3 if include_input else 0)
    assert stride >= width
    rows = rs.standard_normal((n * S, stride)).astype(np.float32)
    return {"origins": o, "directions": d, "t_bins": t, "freqs": np.array([1.0, 2.0], np.float32), "rows": rows,
            "d_out": np.ascontiguousarray(rows[:, :width])}


def error_unit(fp32_value, f64_value):
    """The fp32 restatement's own distance from float64, floored at one fp32 ulp: the unit of the kernels' bound."""
    return max(rel_err(fp32_value, f64_value), ULP)


def check_against_float64(got, inp, orientation_scale=1.0, pred_scale=1.0, report=None):
    """Every output array of `got` (fp32) against float64 within MARGIN units of the fp32 restatement's own error."""
    f64 = normals_losses_torch(**inp, dtype=torch.float64, orientation_scale=orientation_scale, pred_scale=pred_scale)
    f32 = normals_losses_torch(**inp, dtype=torch.float32, orientation_scale=orientation_scale, pred_scale=pred_scale)
    ratios = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        assert got[k].shape == f64[k].shape, k
        unit = error_unit(f32[k], f64[k])
        ratios[k] = rel_err(got[k], f64[k]) / unit
        if report is not None:
            report(k, rel_err(got[k], f64[k]), unit, ratios[k])
    for k, r in ratios.items():
        assert r <= MARGIN, (k, r)
    return ratios
