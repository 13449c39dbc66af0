"""CPU: the float64 references of the sampler and compositing forward kernels (orc.weights64, composite64, the extended
composite_bwd64, mse64, distance_scale64), which tests/test_gpu_ray_forward.py holds the kernels to entry by entry, pinned to
float64 torch autograd or to the plain torch expression; the seeds of the exact (integer) comparisons shown free of
double-rounding ties; and, for every defect the GPU test is meant to see, a numpy model of the defect REJECTED by the GPU
test's own bound at the GPU test's own inputs (tests/ray_forward_cases.py) — the inputs can see the defect."""
import numpy as np
import pytest
import torch

import ray_forward_cases as rc
from float64_check import SAFE, TINY
from oracle import nerfacto_oracle as orc
from oracle import vanilla_oracle as vo
from test_gpu_proposal_backward import _weights_case


def _worst(model, ref, bound):
    """max |model - ref| / bound as check_entries takes it (a NaN or Inf mismatch counts as rejected)."""
    model, ref, bound = (x.double().reshape(-1) for x in (model, ref, bound))
    fin = torch.isfinite(ref) & torch.isfinite(bound)
    if not bool(torch.isfinite(model[fin]).all()):
        return float("inf")
    return float(((model - ref)[fin].abs() / (bound[fin] * SAFE + TINY)).max())


def _same(a, b, rel=1e-14, scale=None):
    a, b = a.double(), b.double()
    s = b.abs() if scale is None else scale
    assert bool(((a - b).abs() <= rel * s + 1e-300).all()), float(((a - b).abs() / (s + 1e-300)).max())


# ---------------------------------------------------------------- the references -----------------------------------------

@pytest.mark.parametrize("S", [1, 48, 257])
def test_weights64_is_the_oracle_in_float64_and_weights_bwd64_is_unchanged(S):
    t, dens, dw = _weights_case(203, S, S)
    r = orc.weights64(t, dens)
    ref = orc.weights_from_density(t.double(), dens.double())
    ok = torch.isfinite(r["w_raw"])
    assert torch.equal(r["w"][ok], ref[ok])
    assert bool((r["w"][torch.isnan(r["w_raw"])] == 0).all()) and bool(torch.isfinite(r["w"]).all())
    b = orc.weights_bwd64(t, dens, dw)
    for k in ("X", "dd", "alpha", "E", "e", "delta"):
        assert torch.equal(torch.nan_to_num(r[k]), torch.nan_to_num(b[k])), k
    fin = torch.isfinite(r["Xabs"])
    assert bool((r["Xabs"][fin] >= r["X"][fin].abs() * (1 - 1e-15)).all())
    # weights_bwd64 itself: autograd's result bit for bit, as before the forward half was shared
    d64 = dens.double().requires_grad_(True)
    (orc.weights_from_density(t.double(), d64) * dw.double()).sum().backward()
    ok = ~torch.isnan(b["ddensity"])
    assert torch.equal(d64.grad[ok], b["ddensity"][ok])


@pytest.mark.parametrize("background", [0, 1, 2, 3])
@pytest.mark.parametrize("eval_mode", [False, True])
def test_composite64_is_the_oracle_in_float64(background, eval_mode):
    S = 65
    c = rc.composite_case(S, 41, seed=background)
    rgb = rc.eval_colours(c["rgb"]) if eval_mode else c["rgb"]
    w, t = c["w"], c["t"]
    r = orc.composite64(rgb, w, t, background, rc.BG_COLOR, c["bg_rays"], eval_mode, c["target"], 0.125)
    name = {0: "random", 1: "last_sample", 2: "black", 3: "random"}[background]
    # (float64 copies: +-Inf go to float64's limits in torch.nan_to_num, so the fp32 limits are applied here as the kernel does)
    c64 = torch.nan_to_num(rgb.double(), nan=0.0, posinf=orc.FLT_MAX, neginf=-orc.FLT_MAX) if eval_mode else rgb.double()
    comp = orc.composite_rgb(c64, w.double(), name, training=True)
    if background == 2:
        comp = comp + torch.tensor(rc.BG_COLOR, dtype=torch.float64) * (1 - w.double().sum(-1, keepdim=True))
    if eval_mode:
        comp = comp.clamp(0.0, 1.0)
    _same(r["rgb"], comp, scale=r["rgb_sum_abs"] + r["bg"].abs() + 1)
    _same(r["acc"], orc.accumulation(w.double())[:, 0])
    assert bool((r["acc_abs"] >= r["acc"].abs()).all()) and bool((r["num_abs"] >= r["num"].abs() * (1 - 1e-15)).all())
    # expected depth: the plain expression in float64 with the clip range of the fp32 midpoints
    mid32 = (t[:, :-1] + t[:, 1:]) / 2
    assert float(r["lo"]) == float(mid32.min()) and float(r["hi"]) == float(mid32.max())
    mid = (t.double()[:, :-1] + t.double()[:, 1:]) / 2
    raw = (w.double() * mid).sum(-1) / (w.double().sum(-1) + float(np.float32(1e-10)))
    _same(r["depth_raw"], raw)
    _same(r["depth"], torch.clip(raw, mid32.min().double(), mid32.max().double()))
    # the loss: MSELoss's per-ray terms and gradient by autograd
    p = r["rgb"].clone().requires_grad_(True)
    pred = p + c["bg_rays"].double() * (1 - r["acc"])[:, None] if background == 3 else p
    se = ((pred - c["target"].double()) ** 2).sum(-1)
    _same(r["sq_err"], se.detach())
    (se.sum() * 0.125).backward()
    _same(r["d_rgb_out"], p.grad, scale=p.grad.abs() + 1e-300)
    # and the fp32 oracle within the GPU test's bounds (torch sums pairwise: S more roundings at most)
    b = rc.composite_bounds(r, S, background, eval_mode, c["bg_rays"], 0.125)
    if not eval_mode:
        got = orc.composite_rgb(rgb, w, name, training=True)
        if background == 2:
            got = got + torch.tensor(rc.BG_COLOR) * (1 - w.sum(-1, keepdim=True))
        assert _worst(got, r["rgb"], b["rgb"] + S * rc.U * r["rgb_sum_abs"]) <= 1
        assert _worst(orc.depth_expected(w, t)[:, 0], r["depth"], b["depth"] + S * rc.U * r["num_abs"] / (r["acc"] + 1e-10)) <= 1


@pytest.mark.parametrize("background", [0, 1, 2])
@pytest.mark.parametrize("S", [1, 65])
def test_extended_composite_bwd64_is_autograd(background, S):
    c = rc.composite_bwd_case(S)
    rgb, w, t = c["rgb"], c["w"], c["t"]
    old = orc.composite_bwd64(rgb, w, c["d_out"], background, rc.BG_COLOR, None, c["d_add"])
    again = orc.composite_bwd64(rgb, w, c["d_out"], background, rc.BG_COLOR, None, c["d_add"], None, None, None)
    assert all(torch.equal(old[k], again[k]) for k in old) and set(old) == {"d_rgb", "d_rgb_abs", "d_weights", "dw_abs"}
    r = orc.composite_bwd64(rgb, w, c["d_out"], background, rc.BG_COLOR, None, c["d_add"], c["d_acc"], c["d_depth"], t)
    r64, w64 = rgb.double().requires_grad_(True), w.double().requires_grad_(True)
    acc = w64.sum(-1)
    comp = (w64[..., None] * r64).sum(-2)
    if background == 1:
        comp = comp + r64[:, -1, :] * (1 - acc)[:, None]
    elif background == 2:
        comp = comp + torch.tensor(rc.BG_COLOR, dtype=torch.float64) * (1 - acc)[:, None]
    mid32 = (t[:, :-1] + t[:, 1:]) / 2
    mid = (t.double()[:, :-1] + t.double()[:, 1:]) / 2
    depth = torch.clip((w64 * mid).sum(-1) / (acc + float(np.float32(1e-10))), mid32.min().double(), mid32.max().double())
    ((comp * c["d_out"].double()).sum() + (w64 * c["d_add"].double()).sum() + (acc * c["d_acc"].double()).sum()
     + (depth * c["d_depth"].double()).sum()).backward()
    _same(r["d_weights"], w64.grad, scale=r["dw_abs"])
    _same(r["d_rgb"], r64.grad, scale=r["d_rgb_abs"] + 1e-300)
    assert bool((r["dw_abs"] >= r["d_weights"].abs() * (1 - 1e-15)).all())
    assert not bool(r["depth_mask"][c["zero"]].any()) and bool(r["depth_mask"].any())
    # a depth exactly on a bound passes its gradient (inclusive), as torch.clip's backward does
    one = orc.composite_bwd64(torch.zeros(1, 1, 3), torch.ones(1, 1), None, 0, None, None, None, None, torch.ones(1),
                              torch.tensor([[1.0, 3.0]]))
    assert float(one["depth_raw"]) < 2.0 and not bool(one["depth_mask"])  # 2 / (1 + 1e-10) is below lo = hi = 2
    two = orc.composite_bwd64(torch.zeros(2, 1, 3), torch.tensor([[1.0], [0.0]]), None, 0, None, None, None, None, torch.ones(2),
                              torch.tensor([[0.0, 0.0], [1.0, 3.0]]))
    assert float(two["depth_raw"][0]) == 0.0 == float(two["lo"]) and bool(two["depth_mask"][0])


def test_mse64_and_distance_scale64_are_the_torch_expressions():
    g = torch.Generator().manual_seed(1)
    p, t = torch.rand(1000, generator=g), torch.rand(1000, generator=g)
    r = orc.mse64(p, t, 1.0 / 3000)
    p64 = p.double().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(p64, t.double(), reduction="sum")
    (loss * float(np.float32(1.0 / 3000))).backward()
    _same(r["loss_sum"], loss.detach())
    _same(r["dpred"], p64.grad, scale=p64.grad.abs() + 1e-300)
    tb, dd, dr = rc.distance_case()
    mids = (tb[:, :-1] + tb[:, 1:]) / 2
    assert float(mids.min()) < 1 < float(mids.max())
    d64, r64 = dd.double().requires_grad_(True), dr.double().requires_grad_(True)
    sd, sr = orc.scale_gradients_by_distance_squared(d64, r64, tb.double())
    (sd.sum() * 1 + (sr * 2).sum()).backward()
    gd, gr = orc.distance_scale64(tb, torch.ones_like(dd), torch.full_like(dr, 2.0))
    _same(gd, d64.grad)
    _same(gr, r64.grad)
    assert orc.distance_scale64(tb, None, None) == (None, None)


# ---------------------------------------------------------------- the seeds of the exact comparisons --------------------

def _pdf_cases():
    for sp, s in rc.PDF_PAIRS:
        for j in rc.PDF_JITTERS:
            yield sp, s, j, False, None
    yield 321, 300, "ray", True, None
    for p in rc.PDF_PATTERNS:
        for j in rc.PDF_JITTERS:
            yield 96, 48, j, False, p
    for sp, s in rc.ORIGINAL_PAIRS:
        yield sp, s, "edge", True, None


@pytest.mark.parametrize("S_prev,S,jitter,uniform,pattern", list(_pdf_cases()))
def test_pdf_seeds_have_no_double_rounding_tie(S_prev, S, jitter, uniform, pattern):
    """The oracle's indices and edges do not change when its cumsums are recomputed by a left-to-right float64 loop in numpy."""
    c = rc.pdf_case(S_prev, S, jitter, uniform, pattern)
    so, _, io = orc.pdf_resample(c["s0"], c["w"], S, c["jitter"], c["nears"], c["fars"], histogram_padding=c["hist_pad"],
                                 uniform=uniform)
    s, i = rc.pdf_resample_np(c["s0"], c["w"], S, c["jitter"], c["hist_pad"])
    assert np.array_equal(i, io.numpy()) and np.array_equal(s, so.numpy())
    if pattern and jitter != "none":
        assert int((io == S_prev + 1).sum()) > 0  # u at or beyond the last cdf entry: c1 == c0, t = nan_to_num(0 / 0) = 0


@pytest.mark.parametrize("S", rc.COMPOSITE_S)
def test_median_seeds_have_no_double_rounding_tie(S):
    c = rc.composite_case(S)
    _, idx = orc.depth_median(c["w"], c["t"])
    assert np.array_equal(rc.median_index_np(c["w"].numpy()), idx[:, 0].numpy())
    for ray, k in c["median"].items():
        assert int(idx[ray]) == k, (ray, k)
    hit = int((idx[:, 0] < S - 1).sum())
    assert S == 1 or 0 < hit < rc.COMPOSITE_RAYS  # random rows on both sides: found inside the row, and clamped



@pytest.mark.parametrize("S", rc.BWD_S)
def test_clip_mask_is_unambiguous_on_the_backward_inputs(S):
    c = rc.composite_bwd_case(S)
    r = orc.composite64(None, c["w"], c["t"], 0)
    amb = rc.clip_ambiguous(r, S)
    assert int(amb.sum()) <= 0.02 * rc.BWD_RAYS, int(amb.sum())
    assert not bool(amb[c["zero"]].any()) and bool((r["depth_raw"][c["zero"]] == 0).all())


# ---------------------------------------------------------------- defect models ------------------------------------------

@pytest.mark.parametrize("S", [65, 129, 257, 1024])
def test_defect_transmittance_tile_carry_dropped(S):
    t, dens, plain = rc.weights_case(S)
    r = orc.weights64(t, dens)
    bound = rc.weights_fwd_bound(r)
    assert _worst(rc.weights_tile_carry_dropped(t, dens)[plain], r["w"][plain], bound[plain]) > 1e3
    # (and the bound is not so tight that fp32 torch misses it: the same formulas, torch's exp)
    assert _worst(orc.weights_from_density(t, dens)[plain], r["w"][plain], bound[plain]) <= 1


@pytest.mark.parametrize("S", [129, 200])
def test_defect_median_tile_carry_dropped(S):
    """(At S = 65 the only sample of the second tile is S - 1, the clamped result: the carry cannot show there.)"""
    c = rc.composite_case(S)
    _, idx = orc.depth_median(c["w"], c["t"])
    bad = rc.median_index_np(c["w"].numpy(), carry=False)
    rows = [ray for ray, k in c["median"].items() if 64 <= k < S - 1]
    assert rows and all(bad[ray] != int(idx[ray]) for ray in rows)


@pytest.mark.parametrize("S", [63, 64, 65, 129, 200])
def test_defect_median_strict_comparison(S):
    c = rc.composite_case(S)
    _, idx = orc.depth_median(c["w"], c["t"])
    bad = rc.median_index_np(c["w"].numpy(), strict=True)
    assert np.flatnonzero(bad != idx[:, 0].numpy()).size >= 1


@pytest.mark.parametrize("defect", ["last_block", "first_trip", "idle_zero"])
@pytest.mark.parametrize("S", rc.COMPOSITE_S)
def test_defect_clip_range(S, defect):
    """The GPU test asserts ws[0] == lo and ws[1] == hi exactly and the all-zero-weight rays' depth == lo: each model moves lo."""
    c = rc.composite_case(S)
    r = orc.composite64(None, c["w"], c["t"], 0)
    lo, hi = rc.global_minmax(c["t"])
    assert float(lo) == float(r["lo"]) and float(hi) == float(r["hi"])
    assert float(lo) == float(rc.block_minmax(c["t"])[0][-1]) and float(hi) == float(rc.block_minmax(c["t"])[1][0])
    lo_d, hi_d = rc.global_minmax(c["t"], defect)
    assert float(lo_d) != float(lo)
    assert len(c["zero"]) >= 16 and bool((r["depth"][c["zero"]] == r["lo"]).all())
    # the faint rays are clipped too, without being zero
    assert bool(((r["depth_raw"][c["faint"]] > 0) & (r["depth_raw"][c["faint"]] < r["lo"])).all())
    blocks = {int(z) // rc.RAYS_PER_BLOCK for z in c["zero"]}
    assert min(blocks) < 64 and max(blocks) >= rc.CLIP_PARTIALS_PER_TRIP - 64


@pytest.mark.parametrize("S_prev,S", [(321, 300), (384, 96), (1024, 4096)])
def test_defect_previous_edges_from_320_read_as_zero(S_prev, S):
    for j in rc.PDF_JITTERS:
        c = rc.pdf_case(S_prev, S, j)
        s, _ = rc.pdf_resample_np(c["s0"], c["w"], S, c["jitter"], c["hist_pad"])
        bad, _ = rc.pdf_resample_np(c["s0"], c["w"], S, c["jitter"], c["hist_pad"], defect="edges320")
        assert not np.array_equal(s, bad)


@pytest.mark.parametrize("S_prev,S", [(65, 128), (256, 200), (321, 300), (1024, 4096)])
def test_defect_new_edge_draws_from_128_taken_from_127(S_prev, S):
    for j in rc.PDF_JITTERS:
        c = rc.pdf_case(S_prev, S, j)
        s, i = rc.pdf_resample_np(c["s0"], c["w"], S, c["jitter"], c["hist_pad"])
        bad, ib = rc.pdf_resample_np(c["s0"], c["w"], S, c["jitter"], c["hist_pad"], defect="u127")
        assert not np.array_equal(s[:, 128:], bad[:, 128:]) and np.array_equal(s[:, :128], bad[:, :128])


@pytest.mark.parametrize("S", rc.BWD_S)
def test_defect_rem_missing_from_the_last_sample(S):
    c = rc.composite_bwd_case(S)
    r = orc.composite_bwd64(c["rgb"], c["w"], c["d_out"], 1, None, None, None)
    b_rgb, _ = rc.composite_bwd_bounds(r, c["w"], S, 1, c["d_out"])
    bad = c["d_out"].double()[:, None, :] * c["w"].double()[..., None]
    assert _worst(bad, r["d_rgb"], b_rgb) > 1e3


@pytest.mark.parametrize("S", rc.BWD_S)
def test_defect_g_den_missing_from_d_weights(S):
    c = rc.composite_bwd_case(S)
    for d_out in (None, c["d_out"]):
        r = orc.composite_bwd64(c["rgb"], c["w"], d_out, 2, rc.BG_COLOR, None, None, c["d_acc"], c["d_depth"], c["t"])
        _, b_w = rc.composite_bwd_bounds(r, c["w"], S, 2, d_out)
        assert _worst(r["d_weights"] - r["g_den"][:, None], r["d_weights"], b_w) > 1e3
        assert _worst(r["d_weights"] - r["g_num"][:, None] * r["mid"], r["d_weights"], b_w) > 1e3


def test_original_edges_oracle_is_sorted():
    c = rc.pdf_case(64, 128, "edge", True)
    s, t = vo.pdf_resample_with_original(c["s0"], c["w"], c["nears"], c["fars"], 128, c["jitter"])
    assert s.shape == (rc.PDF_RAYS, 64 + 128 + 2) and bool((s[:, 1:] >= s[:, :-1]).all())
