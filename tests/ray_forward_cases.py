"""Inputs, per-entry bounds and defect models of tests/test_gpu_ray_forward.py (the sampler and compositing forward kernels
against float64), shared with tests/test_ray_forward_reference_cpu.py, which shows on the CPU that these inputs and bounds
reject a numpy model of each defect the GPU test is meant to see. The derivation of every bound is in the docstring of
test_gpu_ray_forward.py; nothing here is fitted to a kernel's output."""
import math

import numpy as np
import torch

from float64_check import D53, E_EXP, SAFE, TINY, U
from oracle import nerfacto_oracle as orc

F32 = np.float32
RAYS_PER_BLOCK = 4         # ray_bodies.h: kRaysPerBlock
CLIP_PARTIALS_PER_TRIP = 256  # render.hip: depth_clip_kernel re-reduces the partials 256 at a time
BG_COLOR = (0.25, 0.5, 0.75)


def n_add(S):
    """Additions of a wave sum over S samples: ceil(S / 64) per lane, then 6 shuffle steps."""
    return math.ceil(S / 64) + 6


def _fin(x):
    return torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)


# ---------------------------------------------------------------- RaySamples.get_weights --------------------------------

WEIGHT_S = [1, 64, 65, 129, 257, 1024]
WEIGHT_NAN_ROW, WEIGHT_INF_ROW = 5, 6


def weights_case(S):
    """t_bins [11, S+1], density [11, S]: row 0 density exactly 0; row 1 opaque early (optical depth to 1e6: transmittance
    through the denormals to 0); rows 2 / 3 an optical thickness of 2 / 0.25 per sample (the transmittance crosses the denormal
    range inside tile 0 / over tiles 5 and 6, every tile's carry matters); row 4 thin (alpha = 1 - exp(-dd) cancels); row 5 one
    NaN density, row 6 one +Inf; the rest random over four decades. All densities >= 0: every sum is sign-coherent."""
    n = 11
    g = torch.Generator().manual_seed(100 + S)
    _, t = orc.piecewise_bins(torch.full((n, 1), 0.05), torch.full((n, 1), 1000.0), S, torch.rand(n, 1, generator=g))
    t = t.contiguous()
    dens = torch.rand(n, S, generator=g) * 10.0 ** (torch.rand(n, S, generator=g) * 4 - 3)
    delta = t[:, 1:] - t[:, :-1]
    dens[0] = 0.0
    dens[1] = torch.logspace(-2, 4, S) if S > 1 else 1e4
    dens[2] = 2.0 / delta[2]
    dens[3] = 0.25 / delta[3]
    dens[4] = 1e-3
    dens[WEIGHT_NAN_ROW, S // 2] = float("nan")
    dens[WEIGHT_INF_ROW, (2 * S) // 3] = float("inf")
    plain = torch.ones(n, dtype=torch.bool)
    plain[WEIGHT_NAN_ROW] = plain[WEIGHT_INF_ROW] = False
    return t, dens, plain


def weights_fwd_bound(r):
    """Per-entry bound of w = fl(fl(1 - expf(-dd)) * expf(-fl32(X))) from orc.weights64's quantities."""
    S = r["dd"].shape[-1]
    dd, X, Xabs, E, e, alpha, w = (_fin(r[k]) for k in ("dd", "X", "Xabs", "E", "e", "alpha", "w"))
    dX = 2 * U * Xabs + U * X.abs() + S * D53 * Xabs
    dT = E * (torch.expm1(dX) + E_EXP)
    de = e * (torch.expm1(2 * U * dd.abs()) + E_EXP)
    dalpha = de + U * alpha.abs()
    return dalpha * E + alpha.abs() * dT + U * w.abs()


def weights_tile_carry_dropped(t, dens):
    """Defect model: the running optical depth restarts at every 64-sample tile."""
    r = orc.weights64(t, dens)
    dd = r["dd"]
    S = dd.shape[-1]
    X = torch.zeros_like(dd)
    for s0 in range(0, S, 64):
        tile = dd[:, s0:s0 + 64]
        X[:, s0:s0 + 64] = torch.cumsum(tile, -1) - tile
    return r["alpha"] * torch.exp(-X)


# ---------------------------------------------------------------- compositing -------------------------------------------

COMPOSITE_S = [1, 63, 64, 65, 129, 200]
COMPOSITE_RAYS = 1029  # 258 workgroups (two trips of the clip pass's loop over the partials), one live wave in the last


def median_rows(S):
    """{ray: (weight row, expected index)}: running sums that reach 0.5 at sample 0, 63, 64, 65 and S - 1 (two entries of 0.3:
    the second one needs the first one's carry when they lie in different tiles), exactly (0.25 + 0.25: side="left" takes
    that sample, `>` would not), and never (clamped to S - 1)."""
    rows = {}
    ray = 40
    for k in sorted({0, 63, 64, 65, S - 1}):
        if k >= S:
            continue
        w = np.zeros(S, F32)
        w[0] = 0.3
        w[k] += 0.3
        rows[ray] = (w, k)
        ray += 9
    if S >= 4:
        k = min(70, S - 2)
        w = np.zeros(S, F32)
        w[1] = 0.25
        w[k] = 0.25
        rows[ray] = (w, k)
        ray += 9
    rows[ray] = (np.full(S, 0.4 / S, F32), S - 1)
    return rows


def composite_case(S, n=COMPOSITE_RAYS, seed=None):
    """rgb [n, S, 3], weights [n, S], t_bins [n, S+1], target, bg_rays [n, 3] and the ray sets of the test. The weights come
    from random densities (sum <= 1). Ray 0 holds the global maximum midpoint and the LAST ray the global minimum; every 61st
    ray from 7 on has all weights zero (raw depth 0: clipped up to lo), every 61st from 11 on has its weights scaled by 1e-14
    (raw depth = num / (acc + 1e-10) far below lo without being 0); median_rows(S) are written over rays 40, 49, ..."""
    g = torch.Generator().manual_seed(200 + S if seed is None else seed)
    near = 0.5 + torch.rand(n, 1, generator=g)
    far = 5.0 + torch.rand(n, 1, generator=g) * 20
    steps = torch.sort(torch.rand(n, S + 1, generator=g), -1).values
    t = (near + (far - near) * steps).contiguous()
    t[0, -1] = 100.0
    t[-1] = torch.linspace(0.01, 0.3, S + 1)
    dens = torch.rand(n, S, generator=g) * 10.0 ** (torch.rand(n, S, generator=g) * 3 - 2)
    zero = torch.arange(n)[7::61]
    faint = torch.arange(n)[11::61]
    dens[zero] = 0.0  # (through the densities, so that nsamd_render_train has these rays too)
    w = orc.weights_from_density(t, dens).contiguous()
    assert bool((w[zero] == 0).all())
    w[faint] *= 1e-14
    med = {}
    if n >= 200:
        for ray, (row, k) in median_rows(S).items():
            w[ray] = torch.from_numpy(row)
            med[ray] = k
    rgb = torch.rand(n, S, 3, generator=g)
    target = torch.rand(n, 3, generator=g)
    bg_rays = torch.rand(n, 3, generator=g)
    return dict(rgb=rgb, w=w, t=t, dens=dens, target=target, bg_rays=bg_rays, zero=zero, faint=faint, median=med)


def eval_colours(rgb):
    """A copy of rgb [n, S, 3] with NaN, +Inf, -Inf and values outside [0, 1], one special value per ray (so that no fp32 sum of
    FLT_MAX-sized terms overflows where float64 does not), the last sample (the background under last_sample) among them."""
    c = rgb.clone()
    n, S, _ = c.shape
    # (S = 1: the only sample is the background too, w FLT_MAX + FLT_MAX (1 - w) may round to Inf in fp32 alone: 1e30 there)
    big = float("inf") if S > 1 else 1e30
    specials = [float("nan"), big, -big, 7.5, -3.25, 1e30]
    for i, v in enumerate(specials):
        c[20 + i::97, (i * 5) % S, i % 3] = v      # somewhere in the row
        c[60 + i::97, S - 1, (i + 1) % 3] = v      # the last sample
    return c


def clamp_bound(raw, b, lo=0.0, hi=1.0):
    """clamp is monotonic: a value within b of `raw` clamps to within this of clamp(raw) (<= b; 0 when raw is far outside)."""
    b = b * SAFE + TINY
    c = raw.clamp(lo, hi)
    return torch.maximum(((raw + b).clamp(lo, hi) - c).abs(), ((raw - b).clamp(lo, hi) - c).abs())


def composite_bounds(c, S, background, eval_mode, bg_rays=None, grad_scale=1.0):
    """Per-entry bounds of composite_fwd_body's outputs from orc.composite64's quantities (docstring of the GPU test)."""
    na = n_add(S)
    b = {}
    d_acc = na * U * c["acc_abs"]
    b["acc"] = d_acc
    d_rem = d_acc + U * c["rem"].abs()
    if "rgb" in c:
        raw = (na + 1) * U * c["rgb_sum_abs"]
        if background in (1, 2):
            term = c["bg"] * c["rem"][:, None]
            raw = raw + c["bg"].abs() * d_rem[:, None] + U * term.abs() + U * c["rgb_raw"].abs()
        b["rgb"] = clamp_bound(c["rgb_raw"], raw) if eval_mode else raw
        if "pred" in c:
            bp = b["rgb"]
            if background == 3:
                bgr = bg_rays.double()
                bp = bp + bgr.abs() * d_rem[:, None] + U * (bgr * c["rem"][:, None]).abs() + U * c["pred"].abs()
            dd = bp + U * c["diff"].abs()
            b["sq_err"] = (2 * c["diff"].abs() * dd + dd * dd).sum(-1) + 3 * U * c["sq_err"]
            b["d_rgb_out"] = 2 * float(F32(grad_scale)) * dd + U * c["d_rgb_out"].abs()
    if "depth_raw" in c:
        den = c["acc"] + orc.DEPTH_EPS
        d_num = (na + 2) * U * c["num_abs"]
        d_den = d_acc + U * den.abs()
        b["depth_raw"] = d_num / den.abs() + c["num"].abs() * d_den / (den * den) + U * c["depth_raw"].abs()
        b["depth"] = b["depth_raw"] + U * abs(float(c["lo"]))
    return b


def block_minmax(t):
    """Per-workgroup (4 rays) min / max of the fp32 sample midpoints: what composite_fwd_body leaves in the workspace."""
    mid = ((t[:, :-1] + t[:, 1:]) / 2).numpy()
    n = mid.shape[0]
    blocks = -(-n // RAYS_PER_BLOCK)
    lo = np.array([mid[4 * b:4 * b + 4].min() for b in range(blocks)], F32)
    hi = np.array([mid[4 * b:4 * b + 4].max() for b in range(blocks)], F32)
    return lo, hi


def global_minmax(t, defect=None):
    """The clip range (ws[0], ws[1]); defect models: "last_block" (the last workgroup's partial left out), "first_trip"
    (partials beyond index 255 left out), "idle_zero" (the tail workgroup's idle waves contribute 0 instead of +-inf)."""
    lo, hi = block_minmax(t)
    if defect == "last_block":
        lo, hi = lo[:-1], hi[:-1]
    elif defect == "first_trip":
        lo, hi = lo[:CLIP_PARTIALS_PER_TRIP], hi[:CLIP_PARTIALS_PER_TRIP]
    elif defect == "idle_zero" and t.shape[0] % RAYS_PER_BLOCK:
        lo, hi = np.append(lo, F32(0)), np.append(hi, F32(0))
    return F32(lo.min()), F32(hi.max())


def median_index_np(w, carry=True, strict=False):
    """searchsorted(cumsum(w), 0.5, side="left") clamped, on fp32 rows, with a left-to-right float64 accumulator rounded to fp32
    per output. Defect models: carry=False restarts the running sum at every 64-sample tile; strict=True compares with `>`."""
    w = np.asarray(w, F32)
    n, S = w.shape
    cum = np.zeros((n, S), F32)
    for s0 in range(0, S, 64):
        base = 0.0 if (not carry or s0 == 0) else acc[:, -1:]
        acc = np.cumsum(w[:, s0:s0 + 64].astype(np.float64), -1) + base
        cum[:, s0:s0 + 64] = acc.astype(F32)
    hit = (cum > F32(0.5)) if strict else (cum >= F32(0.5))
    idx = np.where(hit.any(-1), hit.argmax(-1), S)
    return np.minimum(idx, S - 1).astype(np.int64)


# ---------------------------------------------------------------- compositing backward ----------------------------------

BWD_S = [1, 64, 65, 200]
BWD_RAYS = 37
BWD_ZERO = (0, 9, 18, 36)  # all-zero-weight rays; rays 0 and 36 hold the global max / min midpoint (at S = 1 a ray's raw depth
                           # IS its midpoint: with weight those two would sit on the clip bounds)


def composite_bwd_case(S, seed=None):
    c = composite_case(S, BWD_RAYS, 300 + S if seed is None else seed)
    g = torch.Generator().manual_seed(310 + S)
    c["w"][list(BWD_ZERO)] = 0.0
    c["zero"] = torch.tensor(BWD_ZERO)
    c["d_out"] = torch.randn(BWD_RAYS, 3, generator=g)
    c["d_acc"] = torch.randn(BWD_RAYS, generator=g)
    c["d_depth"] = torch.randn(BWD_RAYS, generator=g)
    c["d_add"] = torch.randn(BWD_RAYS, S, generator=g) * 0.1
    return c


def composite_bwd_bounds(r, w, S, background, d_out):
    """(bound of d_rgb, bound of d_weights) from the extended orc.composite_bwd64's quantities."""
    na = n_add(S)
    w = w.double()
    wabs = w.abs().sum(-1)
    b_rgb = U * r["d_rgb"].abs()
    if background == 1 and d_out is not None:
        rem = (1 - w.sum(-1)).abs()
        drem = na * U * wabs + U * rem + U * (rem + w[:, -1].abs())
        b_rgb[:, -1, :] += d_out.double().abs() * drem[:, None]
    b_w = 12 * U * r["dw_abs"]
    if "g_den" in r:
        den, num = r["den"], r["num"]
        d_den = na * U * wabs + U * den.abs()
        d_num = (na + 2) * U * r["num_abs"]
        d_gnum = r["g_num"].abs() * (d_den / den.abs() + U)
        d_gden = r["gd"].abs() * (d_num / (den * den) + 2 * num.abs() * d_den / den.abs() ** 3) + 4 * U * r["g_den"].abs()
        b_w = b_w + d_gden[:, None] + r["mid"].abs() * d_gnum[:, None] + U * (r["g_num"][:, None] * r["mid"]).abs()
    return b_rgb, b_w


def clip_ambiguous(c, S):
    """Rays whose float64 raw depth lies within its bound of lo or hi: the clip mask may fall on either side."""
    b = composite_bounds(c, S, 0, False)["depth_raw"] * SAFE + TINY
    raw = c["depth_raw"]
    return ((raw - c["lo"]).abs() <= b) | ((raw - c["hi"]).abs() <= b)


# ---------------------------------------------------------------- PDF resampling ----------------------------------------

PDF_PAIRS = [(1, 1), (2, 5), (63, 7), (64, 127), (65, 128), (256, 200), (319, 48), (320, 48), (321, 300), (384, 96),
             (1024, 4096)]
PDF_JITTERS = ["none", "ray", "edge"]
PDF_PATTERNS = ["zero", "one", "runs"]
ORIGINAL_PAIRS = [(64, 128), (320, 200), (1024, 1024), (1024, 4096)]
PDF_RAYS = 9  # two full workgroups and one ray


def pdf_case(S_prev, S, jitter="ray", uniform=False, pattern=None, seed=None, far=1000.0):
    """s_bins_prev [9, S_prev+1], weights [9, S_prev] (from random densities over the previous level's edges), nears, fars [9, 1]
    and the jitter draws (None / [9, 1] / [9, S+1]). pattern (with histogram_padding = 0): "zero" all weights zero (the eps
    padding), "one" zero except one bin, "runs" runs of zero bins between live ones (c1 == c0: the nan_to_num(.., 0) result)."""
    n = PDF_RAYS
    g = torch.Generator().manual_seed(1000 * S_prev + S if seed is None else seed)
    nears = torch.full((n, 1), 2.0 if uniform else 0.05)
    fars = torch.full((n, 1), 6.0 if uniform else far)
    s0, t0 = orc.piecewise_bins(nears, fars, S_prev, torch.rand(n, 1, generator=g), uniform)
    s0, t0 = s0.contiguous(), t0.contiguous()
    dens = torch.exp(torch.randn(n, S_prev, generator=g) * 2)
    w = orc.weights_from_density(t0, dens).contiguous()
    if pattern == "zero":
        w.zero_()
    elif pattern == "one":
        w.zero_()
        w[torch.arange(n), (torch.arange(n) * 11) % S_prev] = 0.7
    elif pattern == "runs":
        w = torch.rand(n, S_prev, generator=g)
        w[:, (torch.arange(S_prev) // 5) % 3 != 0] = 0.0
    jit = {"none": None, "ray": torch.rand(n, 1, generator=g), "edge": torch.rand(n, S + 1, generator=g)}[jitter]
    if pattern and jit is not None:
        jit[0, -1] = 1.0 - 2.0**-24  # the largest draw: ray 0's last u reaches the end of the cdf (c1 == c0, t = 0 / 0 -> 0)
    return dict(s0=s0, t0=t0, dens=dens, w=w, nears=nears, fars=fars, jitter=jit, hist_pad=0.0 if pattern else 0.01)


def pdf_resample_np(s_prev, w, S, jitter, hist_pad=0.01, eps=1e-5, defect=None):
    """orc.pdf_resample's spacing-domain edges and indices restated in numpy fp32 with both cumsums as LEFT-TO-RIGHT float64
    loops rounded to fp32 per output (np.cumsum is sequential): where this agrees with the oracle on a seed, no index of that
    seed hangs on a double-rounding tie. Defect models: "edges320" reads the previous edges from 320 on as zero, "u127" takes
    the draws of the new edges from 128 on from u_base[127]."""
    s_prev, w = s_prev.numpy().astype(F32), w.numpy().astype(F32)
    n, S_prev = w.shape
    nb = S + 1
    with np.errstate(all="ignore"):
        w = w + F32(hist_pad)
        run = np.cumsum(w.astype(np.float64), -1)[:, -1:].astype(F32)
        pad = np.maximum(F32(eps) - run, F32(0))
        w = w + pad / F32(S_prev)
        wsum = run + pad
        pdf = w / wsum
        cdf = np.minimum(F32(1), np.cumsum(pdf.astype(np.float64), -1).astype(F32))
        cdf = np.concatenate([np.zeros((n, 1), F32), cdf], -1)
        u_base = torch.linspace(0.0, 1.0 - (1.0 / nb), steps=nb).numpy()
        if defect == "u127":
            u_base = u_base.copy()
            u_base[128:] = u_base[127]
        if jitter is not None:
            u = u_base[None, :] + jitter.numpy().astype(F32) / F32(nb)
        else:
            u = np.broadcast_to((u_base + F32(1.0 / (2 * nb)))[None, :], (n, nb))
        u = np.ascontiguousarray(u, F32)
        inds = np.stack([np.searchsorted(cdf[r], u[r], side="right") for r in range(n)])
        below, above = np.clip(inds - 1, 0, S_prev), np.clip(inds, 0, S_prev)
        c0, c1 = np.take_along_axis(cdf, below, -1), np.take_along_axis(cdf, above, -1)
        bprev = s_prev.copy()
        if defect == "edges320":
            bprev[:, 320:] = 0
        b0, b1 = np.take_along_axis(bprev, below, -1), np.take_along_axis(bprev, above, -1)
        tt = (u - c0) / (c1 - c0)
        tt = np.clip(np.nan_to_num(tt, nan=0.0, posinf=np.finfo(F32).max, neginf=np.finfo(F32).min), 0, 1).astype(F32)
        s = b0 + tt * (b1 - b0)
    return s.astype(F32), inds.astype(np.int64)


# ---------------------------------------------------------------- MSE, distance scale -----------------------------------

MSE_N = [1, 255, 256, 257, 16384, 16385, 40000]
MSE_BLOCK_SPAN = 16384  # render.hip: at most 64 workgroups of 256 threads


def mse_loss_bound(n, sum_sq):
    """(ceil(n / 16384) per-thread additions + 6 wave steps + 4 wave partials + 64 atomics) u of the sum of squares."""
    return (math.ceil(n / MSE_BLOCK_SPAN) + 6 + 4 + 64) * U * sum_sq


def distance_case():
    n, S = 37, 48
    g = torch.Generator().manual_seed(77)
    t = torch.sort(torch.rand(n, S + 1, generator=g) * 2.5, -1).values.contiguous()  # midpoints on both sides of 1
    return t, torch.randn(n, S, generator=g), torch.randn(n, S, 3, generator=g)
