"""CPU: the float64 references of the proposal backward chain and the per-ray losses (orc.weights_bwd64,
composite_bwd64, interlevel_bwd64, distortion_bwd64, density_mlp_fwd64 / density_mlp_bwd64), which
tests/test_gpu_proposal_backward.py holds the kernels to entry by entry, pinned to torch autograd through the oracle's own
functions evaluated in float64; and the fp32 autograd evaluation of the same functions within the per-entry bounds the GPU
tests use (which must not be vacuous: the fp32 evaluation does round)."""
import pytest
import torch

from oracle import nerfacto_oracle as orc
from test_gpu_proposal_backward import (U, _interlevel_case, _mlp_inputs, _mlp_params, _weights_case, interlevel_bounds,
                                        relu_ambiguous, weights_bound)


def _close(a, b, scale, rel=1e-14):
    a, b = a.double(), b.double()
    nan = torch.isnan(b)
    assert torch.equal(torch.isnan(a), nan)
    fin = torch.isfinite(b)
    assert torch.equal(a[~fin & ~nan], b[~fin & ~nan])
    err = (a - b)[fin].abs()
    assert bool((err <= rel * scale[fin] + 1e-300).all()), float((err / (scale[fin] + 1e-300)).max())


def _within(name, got, ref, bound):
    fin = torch.isfinite(ref) & torch.isfinite(bound)
    err = (got.double() - ref)[fin].abs()
    b = bound[fin] * (1 + 2.0**-6) + 2.0**-140
    assert bool((err <= b).all()), f"{name}: {float((err / b).max()):.2f}x the bound"
    assert float(err.max()) > 0, name  # the fp32 evaluation does round: the comparison above is not vacuous
    return float((err / b).max())


@pytest.mark.parametrize("S", [1, 48, 257])
def test_weights_bwd64_is_autograd(S):
    n = 203
    t, dens, dw = _weights_case(n, S, S)
    r = orc.weights_bwd64(t, dens, dw)
    d64 = dens.double().requires_grad_(True)
    (orc.weights_from_density(t.double(), d64) * dw.double()).sum().backward()
    assert torch.equal(torch.isnan(d64.grad), torch.isnan(r["ddensity"]))
    ok = ~torch.isnan(r["ddensity"])
    assert torch.equal(d64.grad[ok], r["ddensity"][ok])  # the same operations in the same order: bit for bit
    # fp32 autograd (the same formulas, fp32 throughout, torch's exp) within the kernels' bound, on the finite rows
    rows = torch.isfinite(r["ddensity"]).all(-1) & torch.isfinite(dens).all(-1) & (dens >= 0).all(-1)
    d32 = dens[rows].clone().requires_grad_(True)
    (orc.weights_from_density(t[rows], d32) * dw[rows]).sum().backward()
    rr = {k: v[rows] for k, v in r.items()}
    _within("ddensity", d32.grad, rr["ddensity"], weights_bound(rr))


@pytest.mark.parametrize("background", [0, 1, 2, 3])
def test_composite_bwd64_is_autograd(background):
    n, S = 61, 48
    g = torch.Generator().manual_seed(background)
    rgb = torch.rand(n, S, 3, generator=g)
    w = torch.rand(n, S, generator=g) / S
    d_out = torch.randn(n, 3, generator=g)
    bg_rays = torch.rand(n, 3, generator=g)
    dwa = torch.randn(n, S, generator=g) * 1e-3
    c = orc.composite_bwd64(rgb, w, d_out, background, (0.25, 0.5, 0.75), bg_rays, dwa)
    r64, w64 = rgb.double().requires_grad_(True), w.double().requires_grad_(True)
    name = {0: "random", 1: "last_sample", 2: "white", 3: "random"}[background]
    comp = orc.composite_rgb(r64, w64, name, training=True)
    if background == 2:  # a constant colour other than white: the same formula
        comp = (w64[..., None] * r64).sum(-2) + torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64) * (1 - w64.sum(-1, keepdim=True))
    if background == 3:  # the loss blend of "random" (renderers.py:194-196)
        comp = comp + bg_rays.double() * (1 - w64.sum(-1, keepdim=True))
    ((comp * d_out.double()).sum() + (w64 * dwa.double()).sum()).backward()
    _close(c["d_rgb"], r64.grad, c["d_rgb_abs"])
    _close(c["d_weights"], w64.grad, c["dw_abs"])
    assert bool((c["dw_abs"] >= c["d_weights"].abs()).all()) and bool((c["d_rgb_abs"] >= c["d_rgb"].abs()).all())


@pytest.mark.parametrize("Sf,Sp", [(48, 96), (63, 65), (65, 63), (1, 1)])
def test_interlevel_bwd64_is_autograd(Sf, Sp):
    n = 203
    c, w, cp, wp = _interlevel_case(n, Sf, Sp, Sf + Sp)
    r = orc.interlevel_bwd64(c, w, cp, wp)
    # the cover ranges are _outer_bound's: its outer, from the same searchsorted on the same fp32 edges
    assert torch.equal(orc._outer_bound(c, cp, wp.double()), r["outer"])
    # per-ray loss and dwp against autograd of the oracle's lossfun_outer term (per ray: sum, not mean)
    wp64 = wp.double().requires_grad_(True)
    outer = orc._outer_bound(c, cp, wp64)
    loss = (torch.clip(w.double() - outer, min=0) ** 2 / (w.double() + orc.LOSS_EPS)).sum(-1)
    loss.sum().backward()
    _close(r["loss"], loss.detach(), loss.detach().abs() + 1e-300)
    _close(r["dwp"], wp64.grad, r["cover_abs"] + r["rr"].abs().sum(-1, keepdim=True))  # (autograd: reversed prefix sums)
    # the mean over rays and samples is orc.interlevel_loss
    il = orc.interlevel_loss([wp.double(), w.double()], [cp, c])
    assert abs(float(il) - float(r["loss"].sum()) / (n * Sf)) <= 1e-14 * abs(float(il))
    # fp32 autograd within the kernels' bound (its prefix sums are fp32 cumsums: the same rounding as cy)
    wp32 = wp.clone().requires_grad_(True)
    o32 = orc._outer_bound(c, cp, wp32)
    l32 = (torch.clip(w - o32, min=0) ** 2 / (w + orc.LOSS_EPS)).sum(-1)
    l32.sum().backward()
    unsorted = torch.zeros(n, dtype=torch.float64)
    b_loss, b_dwp = interlevel_bounds(r, Sf, 1.0, unsorted + 1)
    _within("loss", l32.detach(), r["loss"], b_loss + Sf * U * r["loss"])  # (torch sums the row in fp32 pairwise)
    # (autograd's fp32 dwp is a reversed fp32 prefix sum over the whole row, not the kernel's cover sum of double prefix
    # sums: its own order adds Sp u of the row's total |rr|)
    _within("dwp", wp32.grad, r["dwp"], b_dwp + (Sf + Sp) * U * r["rr"].abs().sum(-1, keepdim=True))


def test_interlevel_unsorted_row_is_autograd():
    """On an unsorted row a fine interval can have lo > hi: autograd's d outer / d wp_k = [k <= hi] - [k < lo] is then
    MINUS the range (hi, lo), and so is the reference's."""
    c, w, cp, wp = _interlevel_case(7, 48, 96, 5)
    r = orc.interlevel_bwd64(c, w, cp, wp)
    assert bool((r["lo"][3] > r["hi"][3]).any())
    wp64 = wp.double().requires_grad_(True)
    (torch.clip(w.double() - orc._outer_bound(c, cp, wp64), min=0) ** 2 / (w.double() + orc.LOSS_EPS)).sum().backward()
    _close(r["dwp"], wp64.grad, r["cover_abs"] + r["rr"].abs().sum(-1, keepdim=True))


@pytest.mark.parametrize("S", [1, 48, 65])
def test_distortion_bwd64_is_autograd(S):
    n = 61
    g = torch.Generator().manual_seed(S)
    s = torch.sort(torch.rand(n, S + 1, generator=g), -1).values
    w = torch.rand(n, S, generator=g) * 2 / S
    r = orc.distortion_bwd64(s, w)
    w64 = w.double().requires_grad_(True)
    loss = orc.distortion_loss(w64, s.double()) * n
    loss.backward()
    _close(r["loss"].sum(), loss.detach(), r["loss"].abs().sum())
    _close(r["dw"], w64.grad, 2 * r["inner_abs"] + w.double() * r["delta"] + 1e-300)
    assert bool((r["inner_abs"] >= r["inner"].abs()).all())


@pytest.mark.parametrize("IN,H", [(10, 16), (16, 64)])
@pytest.mark.parametrize("coherent", [False, True])
def test_density_mlp64_is_autograd(IN, H, coherent):
    M = 3001
    W0, b0, W1, b1 = _mlp_params(IN, H, IN + H, coherent)
    enc, _, gd, sel = _mlp_inputs(IN, M, 9, coherent)
    prm = {"l.layers.0.weight": W0, "l.layers.0.bias": b0, "l.layers.1.weight": W1, "l.layers.1.bias": b1}
    avg = 0.01
    f = orc.density_mlp_fwd64(enc, sel, W0, b0, W1, b1, avg)
    p64 = {k: v.double().requires_grad_(True) for k, v in prm.items()}
    x64 = enc.double().requires_grad_(True)
    pre = orc.mlp_forward(x64, p64, "l.")[:, 0]
    dens = avg * orc.trunc_exp(pre) * sel.double()
    _close(f["pre"], pre.detach(), f["pre_abs"])
    _close(f["density"], dens.detach(), f["density"].abs())
    # backward: the helper takes `pre` as given, as autograd's trunc_exp saves it
    (dens * gd.double()).sum().backward()
    r = orc.density_mlp_bwd64(enc, sel, pre.detach(), gd, W0, b0, W1, b1, avg)
    _close(r["denc"], x64.grad, r["denc_abs"])
    for k, key in (("dW0", "l.layers.0.weight"), ("db0", "l.layers.0.bias"), ("dW1", "l.layers.1.weight"),
                   ("db1", "l.layers.1.bias")):
        _close(r[k].reshape(-1), p64[key].grad.reshape(-1), r[k + "_abs"].reshape(-1))
    # pre beyond the clamp: the gradient stops growing at +-15 (activations.py:39-42)
    pre_c = torch.tensor([-40.0, -15.0, 0.0, 15.0, 40.0])
    rc = orc.density_mlp_bwd64(enc[:5], None, pre_c, torch.ones(5), W0, b0, W1, b1, 1.0)
    assert torch.equal(rc["g_pre"], torch.exp(torch.tensor([-15.0, -15.0, 0.0, 15.0, 15.0], dtype=torch.float64)))
    # fp32 autograd within the kernels' per-point bounds (denc: the sums over points are torch's, not the kernel's)
    amb = relu_ambiguous(r["a"], r["a_abs"], IN)
    assert int(amb.sum()) <= 2
    keep = ~amb
    p32 = {k: v.clone().requires_grad_(True) for k, v in prm.items()}
    x32 = enc[keep].clone().requires_grad_(True)
    pre32 = orc.mlp_forward(x32, p32, "l.")[:, 0]
    dens32 = avg * orc.trunc_exp(pre32) * sel[keep]
    dpre = IN * U * (f["a_abs"][keep] @ W1.double().abs().reshape(-1)) + H * U * f["pre_abs"][keep]
    _within("pre", pre32.detach(), f["pre"][keep], dpre)
    _within("density", dens32.detach(), f["density"][keep], f["density"][keep] * (dpre * (1 + dpre) + 4 * U + 2 * U))
    (dens32 * gd[keep]).sum().backward()
    rk = orc.density_mlp_bwd64(enc[keep], sel[keep], pre32.detach(), gd[keep], W0, b0, W1, b1, avg)
    _within("denc", x32.grad, rk["denc"], (H + 8) * U * rk["denc_abs"])
