"""CPU restatement of the PACKED-sample arithmetic of the instant-ngp path (BASELINE.json
configs[3]). TEST INFRASTRUCTURE ONLY.

The arithmetic lives in a third-party dependency that is absent from /root/reference: **nerfacc == 0.5.2**
(pyproject.toml:34). This module restates the published semantics of the three nerfacc functions the reference calls
after sampling — `pack_info`, `render_weight_from_density`, `accumulate_along_rays` (call sites:
models/instant_ngp.py:192-198, model_components/renderers.py:93-102, 310-314, 369-377) — and
`render_visibility_from_density` (inside `OccGridEstimator.sampling`, called at ray_samplers.py:481-493). Anchors: for
rays with equally many samples the packed results must equal the reference's dense path (`RaySamples.get_weights`,
the dense branches of the renderers), which IS pinned (tests/golden/render.npz, samplers.npz); that is what
tests/test_oracle_vs_golden.py::test_packed_* check. The occupancy-grid marcher (`occgrid_march`, further down) restates
the marching of the instant-ngp paper on nerfacc's grid layout, not nerfacc's `traverse_grids` step for step: its sample
placement cannot be pinned in this container (nerfacc is not installable, the reference's only test of it is the opt-in
tests/utils/test_aabb_intersection.py) — **parity of config 3's sample positions stays unpinned** until it can."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor


def pack_info(ray_indices: Tensor, num_rays: int) -> Tensor:
    """nerfacc.pack_info: `[num_rays, 2]` (start, count) of each ray's contiguous run in the packed arrays; samples of a
    ray are contiguous and rays appear in increasing order (what the sampler produces)."""
    counts = torch.bincount(ray_indices, minlength=num_rays)
    starts = torch.cumsum(counts, 0) - counts
    return torch.stack([starts, counts], dim=-1)


def _exclusive_segment_cumsum(x: Tensor, ray_indices: Tensor, num_rays: int) -> Tensor:
    """Exclusive running sum restarting at every ray (packed analogue of rays.py:141-144). Accumulated in double and
    rounded per element, like torch's CPU cumsum does for each row of the dense path (the global scan minus the ray's
    base would cancel catastrophically in fp32)."""
    xd = x.double()
    excl = torch.cumsum(xd, 0) - xd
    info = pack_info(ray_indices, num_rays)
    first = info[:, 0].clamp(max=max(x.shape[0] - 1, 0))
    base = torch.where(info[:, 1] > 0, excl[first], torch.zeros(num_rays, dtype=torch.float64))
    return (excl - base[ray_indices]).to(x.dtype)


def render_weight_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, ray_indices: Tensor,
                               num_rays: int) -> Tuple[Tensor, Tensor, Tensor]:
    """nerfacc.render_weight_from_density: alpha = 1 - exp(-sigma dt), T = exp(-exclusive sum of sigma dt along the
    ray), w = T alpha. Returns (weights, transmittance, alphas), all `[n_samples]`. Same formulas as the dense
    `RaySamples.get_weights` (cameras/rays.py:129-152) without its nan_to_num."""
    sd = sigmas * (t_ends - t_starts)
    alphas = 1.0 - torch.exp(-sd)
    trans = torch.exp(-_exclusive_segment_cumsum(sd, ray_indices, num_rays))
    return trans * alphas, trans, alphas


def render_visibility_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, ray_indices: Tensor, num_rays: int,
                                   early_stop_eps: float = 1e-4, alpha_thre: float = 0.0) -> Tensor:
    """nerfacc.render_visibility_from_density: a sample is kept while the transmittance in front of it is at least
    `early_stop_eps` and its own alpha reaches `alpha_thre`."""
    _, trans, alphas = render_weight_from_density(t_starts, t_ends, sigmas, ray_indices, num_rays)
    return (trans >= early_stop_eps) & (alphas >= alpha_thre)


def accumulate_along_rays(weights: Tensor, values: Optional[Tensor], ray_indices: Tensor, num_rays: int) -> Tensor:
    """nerfacc.accumulate_along_rays: per-ray sum of w (values None -> `[num_rays, 1]`) or of w * values (`[num_rays, D]`)."""
    src = weights[:, None] if values is None else weights[:, None] * values
    out = torch.zeros((num_rays, src.shape[-1]), dtype=src.dtype)
    return out.index_add(0, ray_indices, src)


def composite_packed(rgb: Tensor, weights: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, num_rays: int,
                     background: str = "black", training: bool = True):
    """The packed branches of RGBRenderer / AccumulationRenderer / DepthRenderer("expected") as NGPModel.get_outputs
    uses them (models/instant_ngp.py:199-215; renderers.py:93-119, 310-317, 365-383). "last_sample" is not defined for
    packed samples (renderers.py:95-96)."""
    if background == "last_sample":
        raise NotImplementedError("Background color 'last_sample' not implemented for packed samples.")
    if not training:
        rgb = torch.nan_to_num(rgb)
    comp = accumulate_along_rays(weights, rgb, ray_indices, num_rays)
    acc = accumulate_along_rays(weights, None, ray_indices, num_rays)
    if background == "white":
        comp = comp + 1.0 * (1.0 - acc)
    elif background == "black":
        comp = comp + 0.0 * (1.0 - acc)
    elif background != "random":
        raise ValueError(background)
    if not training:
        comp = comp.clamp(0.0, 1.0)
    steps = (t_starts + t_ends) / 2
    depth = accumulate_along_rays(weights, steps[:, None], ray_indices, num_rays) / (acc + 1e-10)
    depth = torch.clip(depth, steps.min(), steps.max())
    return comp, acc, depth


# ---------------------------------------------------------------------------------------------------------------------
# Occupancy-grid marching and bookkeeping (nerfacc.OccGridEstimator) — PARITY UNPINNED (module docstring): nerfacc's
# traverse_grids walks the cells with a DDA and re-anchors its steps at cell boundaries; what is restated here is the
# marching of the instant-ngp paper (arXiv:2201.05989, appendix E.1) on nerfacc's multi-level grid layout, as the product
# kernel (csrc/packed.hip) implements it: a fixed lattice t0 + k dt per ray, a step kept when the cell (finest level
# containing its midpoint) is occupied. The GPU tests pin the kernel to this restatement bit-exactly; nothing pins either to
# nerfacc's exact sample positions.
# ---------------------------------------------------------------------------------------------------------------------
def _ray_box(o, d, lo, hi):
    """Slab test in fp32 (numpy), rays [N,3] -> (hit [N] bool, t0 [N], t1 [N])."""
    import numpy as np

    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (np.float32(1.0) / d).astype(np.float32)
        ta = ((lo - o) * inv).astype(np.float32)
        tb = ((hi - o) * inv).astype(np.float32)
    swap = ta > tb
    ta, tb = np.where(swap, tb, ta), np.where(swap, ta, tb)
    nan = np.isnan(ta) | np.isnan(tb)
    outside = nan & ((o < lo) | (o > hi))
    ta = np.where(nan, -np.float32(3.4028234663852886e38), ta)
    tb = np.where(nan, np.float32(3.4028234663852886e38), tb)
    t0 = np.maximum.reduce([np.full(len(o), -3.4028234663852886e38, np.float32), ta[:, 0], ta[:, 1], ta[:, 2]])
    t1 = np.minimum.reduce([np.full(len(o), 3.4028234663852886e38, np.float32), tb[:, 0], tb[:, 1], tb[:, 2]])
    return (~outside.any(axis=1)) & (t0 <= t1), t0.astype(np.float32), t1.astype(np.float32)


def occgrid_march(origins, directions, binaries, roi_aabb, step_size, near_plane=0.0, far_plane=1e10, t_min=None, t_max=None,
                  cone_angle=0.0, jitter=None, max_steps=1 << 20):
    """-> (ray_indices int64 [n], t_starts fp32 [n], t_ends fp32 [n]); binaries [levels, R, R, R] bool, roi_aabb [6].
    All arithmetic in fp32 with the kernel's operation order (one ray at a time would be the same; vectorised over rays,
    sequential over steps)."""
    import numpy as np

    f = np.float32
    o = np.asarray(origins, f).reshape(-1, 3)
    d = np.asarray(directions, f).reshape(-1, 3)
    B = np.asarray(binaries).astype(bool)
    L, R = B.shape[0], B.shape[1]
    aabb = np.asarray(roi_aabb, f).reshape(6)
    centre = ((aabb[:3] + aabb[3:]) * f(0.5)).astype(f)
    half = ((aabb[3:] - aabb[:3]) * f(0.5)).astype(f)
    outer = f(1 << (L - 1))
    hit, ta, tb = _ray_box(o, d, (centre - half * outer).astype(f), (centre + half * outer).astype(f))
    n = len(o)
    t_lo = np.full(n, near_plane, f) if t_min is None else np.maximum(f(near_plane), np.asarray(t_min, f).reshape(-1))
    t_hi = np.full(n, min(far_plane, 3.4028234663852886e38), f) if t_max is None else np.minimum(f(min(far_plane, 3.4028234663852886e38)), np.asarray(t_max, f).reshape(-1))
    t = np.maximum(t_lo, ta).astype(f)
    t_end = np.minimum(t_hi, tb).astype(f)
    if jitter is not None:
        t = (t + np.asarray(jitter, f).reshape(-1) * f(step_size)).astype(f)
    alive = hit.copy()
    rows = [[] for _ in range(n)]
    step, cone = f(step_size), f(cone_angle)
    for _ in range(max_steps):
        alive &= t < t_end
        if not alive.any():
            break
        dt = np.minimum(np.maximum((t * cone).astype(f), step), f(1e10)).astype(f)
        mid = (t + (dt * f(0.5)).astype(f)).astype(f)
        p = (o + (d * mid[:, None]).astype(f)).astype(f)
        m = np.max((np.abs(p - centre) / half).astype(f), axis=1)
        level = np.zeros(n, np.int64)
        scale = np.ones(n, f)
        for _l in range(L - 1):
            grow = (level < L - 1) & (m > scale)
            scale = np.where(grow, scale * f(2.0), scale).astype(f)
            level = np.where(grow, level + 1, level)
        inside = m <= scale
        lo_l = (centre[None] - (half[None] * scale[:, None]).astype(f)).astype(f)
        u = (((p - lo_l).astype(f) / ((f(2.0) * half[None]).astype(f) * scale[:, None]).astype(f)).astype(f) * f(R)).astype(f)
        c = np.clip(np.floor(u).astype(np.int64), 0, R - 1)
        occ = B[level, c[:, 0], c[:, 1], c[:, 2]]
        keep = alive & inside & occ
        for r in np.nonzero(keep)[0]:
            rows[r].append((t[r], f(t[r] + dt[r])))
        t = np.where(alive, (t + dt).astype(f), t)
    idx = np.concatenate([np.full(len(r), i, np.int64) for i, r in enumerate(rows)]) if n else np.zeros(0, np.int64)
    flat = [x for r in rows for x in r]
    ts = np.array([x[0] for x in flat], f)
    te = np.array([x[1] for x in flat], f)
    return idx, ts, te


def occgrid_thresholds(occs, occ_thre: float = 0.01):
    """nerfacc OccGridEstimator._update tail: binaries = occs > min(mean of the cells evaluated so far, occ_thre)."""
    import numpy as np

    occs = np.asarray(occs, np.float32)
    seen = occs >= 0
    # the mean in double (the product's kernel and its torch path both sum in double), the threshold rounded to fp32 once
    mean = float(occs[seen].astype(np.float64).mean()) if seen.any() else 0.0
    thre = np.float32(min(mean, float(np.float32(occ_thre))))
    return occs > thre


# ---------------------------------------------------------------------------------------------------------------------
# float64 references of the packed kernels (csrc/packed.hip), per ray over `packed_info` segments: what
# tests/test_gpu_packed_float64.py holds the kernels to entry by entry. The inputs are the kernels' fp32 inputs; the two
# products the kernels form in fp32 before anything else (delta = fl32(te - ts), dd = fl32(delta * sigma)) are taken in
# fp32 here too, as the dense references of oracle/nerfacto_oracle.py take theirs; everything after them is float64.
# Rays are grouped by length (next power of two) and evaluated as rows of a dense float64 matrix padded with zeros, so no
# sum ever runs across a ray boundary (a global scan minus the ray's base would cancel, in any precision, next to a ray
# of optical depth 1e30).
# ---------------------------------------------------------------------------------------------------------------------
def _f64(x):
    import numpy as np

    return x.detach().cpu().double().numpy() if isinstance(x, Tensor) else np.asarray(x, dtype=np.float64)


def _f32(x):
    import numpy as np

    return x.detach().cpu().float().numpy() if isinstance(x, Tensor) else np.asarray(x, dtype=np.float32)


def _info(packed_info):
    import numpy as np

    info = packed_info.detach().cpu().numpy() if isinstance(packed_info, Tensor) else np.asarray(packed_info)
    return info.astype(np.int64).reshape(-1, 2)


def packed_ray_indices(packed_info):
    """int64 `[n]`: the ray of every packed sample."""
    import numpy as np

    info = _info(packed_info)
    return np.repeat(np.arange(len(info), dtype=np.int64), info[:, 1])


def _buckets(packed_info):
    """Rays of similar length together: yields (rays `[rows]`, flat `[rows, width]` int64 sample indices, valid `[rows,
    width]` bool)."""
    import numpy as np

    info = _info(packed_info)
    cnt = info[:, 1]
    width = np.where(cnt > 0, 2 ** np.ceil(np.log2(np.maximum(cnt, 1))).astype(np.int64), 0)
    for wd in np.unique(width[width > 0]):
        rays = np.flatnonzero(width == wd)
        col = np.arange(wd, dtype=np.int64)[None, :]
        valid = col < cnt[rays, None]
        yield rays, np.where(valid, info[rays, 0:1] + col, 0), valid


def _excl_prefix(x):
    import numpy as np

    return np.concatenate([np.zeros_like(x[:, :1]), np.cumsum(x[:, :-1], axis=1)], axis=1)


def _excl_suffix(x):
    return _excl_prefix(x[:, ::-1])[:, ::-1]


def _rowwise(packed_info, n, ins, fn, outs):
    """Evaluates fn(valid, *rows of `ins`) -> dict of rows per bucket of rays (the padding holds zeros); scatters the entries
    named in `outs` to `[n]`."""
    import numpy as np

    res = {k: np.zeros(n, np.float64) for k in outs}
    for _, flat, valid in _buckets(packed_info):
        rows = [np.where(valid, a[flat], 0.0) for a in ins]
        with np.errstate(all="ignore"):
            r = fn(valid, *rows)
        for k in outs:
            res[k][flat[valid]] = r[k][valid]
    return res


def segment_exclusive_suffix64(x, packed_info):
    """Float64 `[n]`: sum of x over the LATER samples of the same ray."""
    import numpy as np

    x = np.asarray(x, np.float64)
    return _rowwise(packed_info, len(x), [x], lambda valid, v: dict(s=_excl_suffix(v)), ("s",))["s"]


def _fl32_products(t_starts, t_ends, sigmas):
    import numpy as np

    ts, te, sg = _f32(t_starts), _f32(t_ends), _f32(sigmas)
    with np.errstate(all="ignore"):
        delta = (te - ts).astype(np.float32)
        dd = (sg * delta).astype(np.float32)
    return delta.astype(np.float64), dd.astype(np.float64)


def _weights_rows(valid, dd):
    import numpy as np

    X = _excl_prefix(dd)
    T, e = np.exp(-X), np.exp(-dd)
    alpha = 1.0 - e
    return dict(X=X, X_abs=_excl_prefix(np.abs(dd)), T=T, e=e, alpha=alpha, w=alpha * T)


def packed_weights64(t_starts, t_ends, sigmas, packed_info):
    """Float64 `render_weight_from_density` over packed segments. Returns float64 `[n]` arrays: delta = fl32(te - ts),
    dd = fl32(delta * sigma) (the kernels' own fp32 products), X = the exclusive prefix sum of dd along the ray, X_abs =
    the same sum of |dd|, T = exp(-X), e = exp(-dd), alpha = 1 - e, w = alpha T."""
    delta, dd = _fl32_products(t_starts, t_ends, sigmas)
    r = _rowwise(packed_info, len(dd), [dd], _weights_rows, ("X", "X_abs", "T", "e", "alpha", "w"))
    return dict(r, delta=delta, dd=dd)


def packed_weights_bwd64(t_starts, t_ends, sigmas, packed_info, dweights):
    """Float64 gradient of the packed weights with respect to sigma for the upstream gradient `dweights`:
    dsigma_j = delta_j (g_j T_j e_j - sum_{i>j} g_i w_i). Returns packed_weights64's arrays plus g, dsigmas, suf (the
    exclusive suffix sum of g w along the ray) and suf_abs (of |g w|)."""
    import numpy as np

    delta, dd = _fl32_products(t_starts, t_ends, sigmas)
    g = _f64(dweights)

    def rows(valid, dd_, g_, delta_):
        r = _weights_rows(valid, dd_)
        gw = np.where(valid, g_ * r["w"], 0.0)  # (behind a NaN sample the padding's own weight is NaN)
        r["suf"], r["suf_abs"] = _excl_suffix(gw), _excl_suffix(np.abs(gw))
        r["dsigmas"] = delta_ * (g_ * r["T"] * r["e"] - r["suf"])
        return r

    r = _rowwise(packed_info, len(dd), [dd, g, delta], rows,
                 ("X", "X_abs", "T", "e", "alpha", "w", "suf", "suf_abs", "dsigmas"))
    return dict(r, delta=delta, dd=dd, g=g)


def packed_visibility64(t_starts, t_ends, sigmas, packed_info, early_stop_eps, alpha_thre):
    """Float64 `render_visibility_from_density`: keep = T >= fl32(early_stop_eps) and alpha >= fl32(alpha_thre), with the
    margins m_T = T - eps and m_alpha = alpha - thre of every sample (and packed_weights64's arrays)."""
    import numpy as np

    r = packed_weights64(t_starts, t_ends, sigmas, packed_info)
    eps, thre = float(np.float32(early_stop_eps)), float(np.float32(alpha_thre))
    m_T, m_alpha = r["T"] - eps, r["alpha"] - thre
    return dict(r, keep=(m_T >= 0) & (m_alpha >= 0), m_T=m_T, m_alpha=m_alpha)


def _per_ray_sum(x, packed_info):
    """Float64 per-ray sums of `[n]` or `[n, D]`."""
    import numpy as np

    info = _info(packed_info)
    x = np.asarray(x, np.float64)
    out = np.zeros((len(info),) + x.shape[1:], np.float64)
    for rays, flat, valid in _buckets(packed_info):
        v = x[flat]
        v = np.where(valid.reshape(valid.shape + (1,) * (x.ndim - 1)), v, 0.0)
        out[rays] = v.sum(axis=1)
    return out


def packed_composite64(rgb, weights, t_starts, t_ends, packed_info, background_mode=0, bg_color=None, eval_mode=False):
    """Float64 packed compositing (csrc/packed.hip, nsamd_packed_composite_fwd): rgb = sum w c [+ bg (1 - acc)], acc =
    sum w, depth = sum w fl32(fl32(ts + te) / 2) / (acc + 1e-10). eval_mode: nan_to_num on the samples' colours, the result
    clamped to [0, 1]. Returns rgb `[N,3]`, acc, depth `[N]`, the abs sums rgb_abs / acc_abs / depth_abs of the terms, and
    dsum (the depth's numerator)."""
    import numpy as np

    c, w = _f64(rgb).reshape(-1, 3), _f64(weights)
    if eval_mode:
        c = np.nan_to_num(c, nan=0.0, posinf=float(np.finfo(np.float32).max), neginf=float(np.finfo(np.float32).min))
    with np.errstate(all="ignore"):
        wc = w[:, None] * c
        comp, comp_abs = _per_ray_sum(wc, packed_info), _per_ray_sum(np.abs(wc), packed_info)
        acc, acc_abs = _per_ray_sum(w, packed_info), _per_ray_sum(np.abs(w), packed_info)
        out = dict(acc=acc, acc_abs=acc_abs, sum_wc=comp, rgb_abs=comp_abs)
        if background_mode == 1:
            bg = np.asarray([float(np.float32(v)) for v in bg_color], np.float64)
            comp = comp + bg[None, :] * (1.0 - acc)[:, None]
        if eval_mode:
            comp = np.clip(comp, 0.0, 1.0)
        out["rgb"] = comp
        if t_starts is not None:
            mid = ((_f32(t_starts) + _f32(t_ends)).astype(np.float32) / np.float32(2.0)).astype(np.float64)
            out["dsum"], out["depth_abs"] = _per_ray_sum(w * mid, packed_info), _per_ray_sum(np.abs(w * mid), packed_info)
            out["depth"] = out["dsum"] / (acc + float(np.float32(1e-10)))
    return out


def packed_composite_bwd64(rgb, weights, packed_info, background_mode, bg_color, g_rgb, g_accumulation=None):
    """Float64 gradients of (rgb, accumulation) of the training composite: d_rgb_s = w_s g_rgb[ray],
    d_w_s = g_rgb . c_s [+ g_acc[ray]] [- g_rgb . bg]. Returns d_rgb `[n,3]`, d_weights `[n]`, dw_abs = sum |terms|."""
    import numpy as np

    c, w, g = _f64(rgb).reshape(-1, 3), _f64(weights), _f64(g_rgb).reshape(-1, 3)
    ri = packed_ray_indices(packed_info)
    gs = g[ri]
    with np.errstate(all="ignore"):
        dw, dw_abs = (gs * c).sum(-1), np.abs(gs * c).sum(-1)
        if g_accumulation is not None:
            ga = _f64(g_accumulation)[ri]
            dw, dw_abs = dw + ga, dw_abs + np.abs(ga)
        if background_mode == 1:
            bg = np.asarray([float(np.float32(v)) for v in bg_color], np.float64)
            dw, dw_abs = dw - (gs * bg).sum(-1), dw_abs + np.abs(gs * bg).sum(-1)
        return dict(d_rgb=w[:, None] * gs, d_weights=dw, dw_abs=dw_abs)


def prefix_by_forward_sum(dd):
    """The transmittance in front of every sample of ONE ray as the forward kernel forms it: expf(-(float) X) with X the
    exclusive forward prefix sum in double. (Restated in numpy: float64 sums, one fp32 cast.)"""
    import numpy as np

    dd = np.asarray(dd, np.float64)
    X = np.concatenate([[0.0], np.cumsum(dd[:-1])])
    with np.errstate(all="ignore"):
        return np.exp(-X.astype(np.float32).astype(np.float64))


def prefix_by_total_minus_suffix(dd):
    """The same transmittance as `total - inclusive suffix` in double: what a backward scan without a per-ray row is
    tempted to use. Equal to the forward prefix only while total * 2^-53 is small against fp32 rounding of X; Inf - Inf
    is NaN."""
    import numpy as np

    dd = np.asarray(dd, np.float64)
    with np.errstate(all="ignore"):
        total = np.cumsum(dd)[-1] if len(dd) else 0.0
        suffix = np.cumsum(dd[::-1])[::-1]
        return np.exp(-(total - suffix).astype(np.float32).astype(np.float64))
