"""CPU: the float64 references of the packed kernels (oracle/packed_oracle.py: packed_weights64, packed_weights_bwd64,
packed_visibility64, packed_composite64, packed_composite_bwd64), which tests/test_gpu_packed_float64.py holds the kernels
to entry by entry, pinned to torch autograd through the oracle's own render_weight_from_density / composite_packed
evaluated in float64 on the same fp32 products; the share of threshold-ambiguous samples of the committed visibility seeds,
from the reference alone; and a numpy restatement in fp32 of the kernels' arithmetic with the two candidate formulas for the
transmittance of the backward (forward exclusive prefix; total minus inclusive suffix): the first stays within the per-entry
bounds the GPU tests use (which must not be vacuous: the fp32 evaluation does round), the second leaves them once
total * 2^-53 is visible in fp32 — the reason for the one-dense-sample cases."""
import numpy as np
import pytest
import torch

from oracle import packed_oracle as po
from test_gpu_packed_float64 import (AMBIGUOUS_CAP, BIG, SAFE, TINY, VIS_CASES, backward_bound, composite_inputs, crossing_case,
                                     dense_sample_case, edge_values_case, forward_bounds, geometry_counts, info_from_counts,
                                     samples_case, upstream, visibility_ambiguous, visibility_inputs)

CPU_GEOMETRIES = ["edges", "n1", "n3", "n4", "n5", "n1023", "n1025", "empty", "zero"]


def _close(name, a, b, scale, rel=1e-12):
    a, b, scale = (np.asarray(x, np.float64).reshape(-1) for x in (a, b, scale))
    err = np.abs(a - b)
    assert bool((err <= rel * scale + 1e-300).all()), f"{name}: {float((err / (scale + 1e-300)).max()):.2e}"


def _autograd_weights(dd, g):
    """Per ray: float64 autograd through po.render_weight_from_density on sigma = dd, dt = 1 (so sigma * dt IS the product)."""
    d64 = torch.from_numpy(dd).clone().requires_grad_(True)
    n = len(dd)
    w, T, alpha = po.render_weight_from_density(torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64), d64,
                                                torch.zeros(n, dtype=torch.int64), 1)
    (w * torch.from_numpy(g)).sum().backward()
    return w.detach().numpy(), T.detach().numpy(), alpha.detach().numpy(), d64.grad.numpy()


@pytest.mark.parametrize("geometry", CPU_GEOMETRIES)
def test_packed_weights64_is_autograd(geometry):
    counts = geometry_counts(geometry)
    info = info_from_counts(counts)
    ts, te, sig = samples_case(counts, 11 + len(counts))
    g = upstream(len(ts), 3 + len(counts), "random")
    r = po.packed_weights_bwd64(ts, te, sig, info, g)
    f = po.packed_weights64(ts, te, sig, info)
    assert all(np.array_equal(f[k], r[k]) for k in f)
    assert np.array_equal(r["delta"], (te - ts).astype(np.float32).astype(np.float64))
    assert np.array_equal(r["dd"], ((te - ts).astype(np.float32) * sig).astype(np.float32).astype(np.float64))
    for s0, c in info:
        if c == 0:
            continue
        sl = slice(s0, s0 + c)
        w, T, alpha, grad = _autograd_weights(r["dd"][sl], r["g"][sl])
        _close("w", r["w"][sl], w, np.abs(w))
        _close("T", r["T"][sl], T, T * (1 + r["X"][sl]))
        _close("alpha", r["alpha"][sl], alpha, np.abs(alpha))
        own = np.abs(r["g"][sl]) * r["T"][sl] * r["e"][sl]
        _close("dsigmas", r["dsigmas"][sl], grad * r["delta"][sl], np.abs(r["delta"][sl]) * (own + r["suf_abs"][sl]) * (1 + r["X"][sl]))
        assert bool((r["suf_abs"][sl] >= np.abs(r["suf"][sl])).all()) and r["X"][sl][0] == 0 and r["suf"][sl][-1] == 0


@pytest.mark.parametrize("geometry", CPU_GEOMETRIES)
@pytest.mark.parametrize("bg_mode", [0, 1])
def test_packed_composite64_is_autograd(geometry, bg_mode):
    counts = geometry_counts(geometry)
    info = info_from_counts(counts)
    nr = len(counts)
    ts, te, w, rgb, g_rgb, g_acc = composite_inputs(counts, 60 + nr, "random")
    ri = torch.from_numpy(po.packed_ray_indices(info))
    white = (1.0, 1.0, 1.0)
    c = po.packed_composite64(rgb, w, ts, te, info, bg_mode, white)
    mid = torch.from_numpy(((ts + te).astype(np.float32) / np.float32(2.0)).astype(np.float64))
    w64 = torch.from_numpy(w).double().requires_grad_(True)
    c64 = torch.from_numpy(rgb).double().requires_grad_(True)
    name = "white" if bg_mode else "random"
    if len(ts):
        comp, acc, dep = po.composite_packed(c64, w64, mid, mid, ri, nr, background=name, training=True)
        _close("rgb", c["rgb"], comp.detach().numpy(), c["rgb_abs"] + 1)
        _close("acc", c["acc"], acc.detach().numpy(), c["acc_abs"])
        den = c["acc"] + 1e-10
        _close("depth", np.clip(c["depth"], float(mid.min()), float(mid.max())), dep.detach().numpy(),
               c["depth_abs"] / den + 1e-5 * c["depth_abs"] / den**2)  # (1e-10f is not 1e-10: 1.3e-18 apart)
        ((comp * torch.from_numpy(g_rgb).double()).sum() + (acc[:, 0] * torch.from_numpy(g_acc).double()).sum()).backward()
        cb = po.packed_composite_bwd64(rgb, w, info, bg_mode, white, g_rgb, g_acc)
        _close("d_rgb", cb["d_rgb"], c64.grad.numpy(), np.abs(cb["d_rgb"]))
        _close("d_weights", cb["d_weights"], w64.grad.numpy(), cb["dw_abs"])
        assert bool((cb["dw_abs"] >= np.abs(cb["d_weights"])).all())
        # without the accumulation's gradient the term is absent
        cb0 = po.packed_composite_bwd64(rgb, w, info, bg_mode, white, g_rgb, None)
        _close("d_weights", cb["d_weights"] - cb0["d_weights"], g_acc.astype(np.float64)[ri.numpy()], cb["dw_abs"])
        # eval mode: nan_to_num on the colours, clamp
        bad = rgb.copy()
        bad[::11] = np.nan
        ev = po.packed_composite64(bad, w, None, None, info, bg_mode, white, eval_mode=True)
        ev_r = po.composite_packed(torch.from_numpy(bad).double(), w64.detach(), mid, mid, ri, nr, background=name, training=False)[0]
        _close("eval rgb", ev["rgb"], ev_r.numpy(), ev["rgb_abs"] + 1)
    empty = counts == 0
    assert np.all(c["acc"][empty] == 0) and np.all(c["depth"][empty] == 0) and np.all(c["rgb"][empty] == float(bg_mode))


@pytest.mark.parametrize("geometry,eps,thre", VIS_CASES)
def test_visibility_seeds_are_rarely_ambiguous(geometry, eps, thre):
    """The cap of tests/test_gpu_packed_float64.py on threshold-ambiguous samples, from the float64 reference alone."""
    counts, ts, te, sig = visibility_inputs(geometry)
    info = info_from_counts(counts)
    v = po.packed_visibility64(ts, te, sig, info, eps, thre)
    amb = visibility_ambiguous(v, info, np.float32(eps), np.float32(thre))
    assert len(ts) == 0 or amb.mean() <= AMBIGUOUS_CAP, int(amb.sum())
    # the mask is the oracle's own fp32 scan wherever it is not ambiguous
    if len(ts):
        ri = torch.from_numpy(po.packed_ray_indices(info))
        keep32 = po.render_visibility_from_density(torch.from_numpy(ts), torch.from_numpy(te), torch.from_numpy(sig), ri,
                                                   len(counts), eps, thre).numpy()
        assert np.array_equal(keep32[~amb], v["keep"][~amb])
    assert np.array_equal(v["keep"], (v["T"] >= float(np.float32(eps))) & (v["alpha"] >= float(np.float32(thre))))


@pytest.mark.parametrize("eps", [1e-4, 1e-2])
def test_visibility_crossings_have_a_factor_two_to_spare(eps):
    counts, ts, te, sig, cross = crossing_case(eps)
    info = info_from_counts(counts)
    v = po.packed_visibility64(ts, te, sig, info, eps, 0.0)
    assert not visibility_ambiguous(v, info, np.float32(eps), np.float32(0.0)).any()
    for k, (s0, c) in enumerate(info):
        last = c - 1 if cross[k] is None else cross[k]
        T = v["T"][s0:s0 + c]
        assert np.array_equal(v["keep"][s0:s0 + c], np.arange(c) <= last)
        assert T[:last + 1].min() >= 2 * eps and (last == c - 1 or T[last + 1:].max() <= eps / 2)


# ---------------------------------------------------------------- the kernels' arithmetic restated in fp32 ------------------

def _fp32_ray(dd, delta, g, formula):
    """One ray of nsamd_packed_weights_fwd / _bwd in numpy: fp32 operations, the scans in double, the transmittance by
    `formula` (po.prefix_by_forward_sum: what the forward kernel does; po.prefix_by_total_minus_suffix)."""
    f = np.float32
    with np.errstate(all="ignore"):
        dd, delta, g = dd.astype(f), delta.astype(f), g.astype(f)
        T_fwd = po.prefix_by_forward_sum(dd.astype(np.float64)).astype(f)
        e = np.exp(-dd).astype(f)
        alpha = (f(1.0) - e).astype(f)
        w = (T_fwd * alpha).astype(f)
        T = formula(dd.astype(np.float64)).astype(f)
        gw = (g * (alpha * T).astype(f)).astype(f).astype(np.float64)
        suf = np.concatenate([np.cumsum(gw[::-1])[::-1][1:], [0.0]]).astype(f)
        ds = (delta * (((g * T).astype(f) * e).astype(f) - suf).astype(f)).astype(f)
    return w, T_fwd, ds


def _fp32_case(counts, ts, te, sig, g, formula):
    info = info_from_counts(counts)
    r = po.packed_weights_bwd64(ts, te, sig, info, g)
    w, T, ds = (np.zeros(len(ts), np.float32) for _ in range(3))
    for s0, c in info:
        if c:
            sl = slice(s0, s0 + c)
            w[sl], T[sl], ds[sl] = _fp32_ray(r["dd"][sl], r["delta"][sl], g[sl], formula)
    return r, info, w, T, ds


def _ratio(got, ref, bound):
    fin = np.isfinite(ref)
    err = np.abs(got.astype(np.float64) - ref)[fin]
    assert np.isfinite(got[fin]).all()
    return err / (bound[fin] * SAFE + TINY)


@pytest.mark.parametrize("case", ["lognormal", "edge values", "dense"])
def test_fp32_forward_prefix_is_within_the_gpu_bounds(case):
    if case == "lognormal":
        counts = geometry_counts("edges")
        ts, te, sig = samples_case(counts, 11 + len(counts))
    elif case == "edge values":
        counts, ts, te, sig = edge_values_case(31)
    else:
        counts, ts, te, sig = dense_sample_case(41)
    for kind in ("random", "positive"):
        g = upstream(len(ts), 42, kind)
        r, info, w, T, ds = _fp32_case(counts, ts, te, sig, g, po.prefix_by_forward_sum)
        f = forward_bounds(r, info)
        for name, got, ref, b in (("T", T, r["T"], f["dT"]), ("w", w, r["w"], f["dw"]), ("dsigma", ds, r["dsigmas"], backward_bound(r, info))):
            q = _ratio(got, ref, b)
            assert q.max() <= 1.0, f"{case} {kind} {name}: {q.max():.2f}x the bound"
            assert q.max() > 1e-3, f"{case} {kind} {name}: the comparison is vacuous ({q.max():.1e})"


def test_total_minus_suffix_loses_the_transmittance_in_front_of_a_dense_sample():
    """40 samples of dd in [0.001, 0.02], one of optical thickness `big` at position 30: the relative error of T for the samples
    IN FRONT of it. The forward prefix never feels the dense sample; total minus suffix carries total * 2^-53 as an absolute
    error of the exponent: invisible at 1e6, 2e-7 at 1e9, beyond every fp32 bound from 1e10 on, and NaN for +Inf."""
    rs = np.random.RandomState(0)
    dd = rs.uniform(0.001, 0.02, 40)
    exact = np.exp(-np.concatenate([[0.0], np.cumsum(dd[:-1])]))[:30]
    worst = {}
    for big in (1e2, 1e6, 1e9, 1e10, 1e12, 1e15, 1e30):
        d = dd.copy()
        d[30] = big
        fwd = np.abs(po.prefix_by_forward_sum(d)[:30] / exact - 1).max()
        tms = np.abs(po.prefix_by_total_minus_suffix(d)[:30] / exact - 1).max()
        worst[big] = tms
        assert fwd <= 2.0**-24 * 1.01, (big, fwd)  # the cast of X (< 0.5) alone
    assert worst[1e2] <= 2e-7 and worst[1e6] <= 2e-7
    assert worst[1e10] > 1e-6 and worst[1e12] > 1e-4 and worst[1e15] > 0.1 and worst[1e30] > 0.1
    d = dd.copy()
    d[30] = np.inf
    assert np.isfinite(po.prefix_by_forward_sum(d)[:31]).all() and np.isnan(po.prefix_by_total_minus_suffix(d)[:31]).all()
    # through the whole backward, against the GPU tests' bound: which magnitudes of the dense-sample case each formula passes
    counts, ts, te, sig = dense_sample_case(41)
    g = upstream(len(ts), 42, "positive")
    passes = {}
    for formula in (po.prefix_by_forward_sum, po.prefix_by_total_minus_suffix):
        r, info, _, _, ds = _fp32_case(counts, ts, te, sig, g, formula)
        q = _ratio(ds, r["dsigmas"], backward_bound(r, info))
        ends = np.cumsum([info[4 * k:4 * k + 4, 1].sum() for k in range(len(BIG))])
        passes[formula.__name__] = [bool(part.max() <= 1.0) for part in np.split(q, ends[:-1])]
    assert all(passes["prefix_by_forward_sum"])
    tms = dict(zip(BIG, passes["prefix_by_total_minus_suffix"]))
    assert all(tms[b] for b in (1e2, 1e4, 1e6)) and not any(tms[b] for b in (1e10, 1e12, 1e20, 1e30)), tms
