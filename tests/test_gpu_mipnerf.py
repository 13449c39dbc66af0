"""mip-NeRF on the MI355X kernels: nsamd_ipe_encode entry by entry against the float64 restatement of
tests/mipnerf_reference.py, MipNerfModel against the fixture the REFERENCE's modules wrote (tests/golden/mipnerf.npz,
tests/golden/make_golden_mipnerf.py), the ray-mode field against the explicit-mode field, and a short training loop.

Bounds. Encoding: per entry, mipnerf_reference.measure — |got - f64| / (damp64 2^-23 (2 pi freq (|o_d| + |d_d| t_mean) + 2) + 2^-23)
— within MARGIN = 4 x max(k_ref, 1) of float64 (mipnerf_reference.bound_f64) and MARGIN + 1 of the reference's own fp32 rows (read as
written, 4 max(k_ref, 1) + 1, or by the triangle inequality 4 max(k_ref, 1) + k_ref, whichever is smaller: bound_ref), k_ref the
reference's own figure on the inputs of the very case (recorded in the fixture):

    n1_s1 0.661   n3_s5 1.170   n33_s17 1.695 (the fixture case)   n4_s64 1.751   n2_s65 1.723   n5_s128 1.883   n2_s193 1.946
    n1_s63 1.477  n5_s13 1.454  n3_s19 1.617

Model outputs, loss and gradients, against the reference's fp32 fixture: per entry the larger of the vanilla-NeRF test's tolerance
for that output (tests/test_gpu_vanilla.py:140-163) and 4 x the reference's recorded fp32 distance from its own float64 run
(`<mode>_<output>_dist`: weights 3e-8 .. 2.2e-7, rgb 8e-8 .. 1.5e-7, depth <= 3.1e-7, loss 9.5e-9). Which of the two is the larger
differs by entry: on small weights 4 x the distance is (atol 2e-7 + 5e-4 |w| is below 7e-7 for w < 1e-3), on rgb, accumulation and
depth the vanilla tolerance is. Entries that are exactly zero in float64 must be zero.
"""
import numpy as np
import pytest
import torch

import mipnerf_reference as mr
from oracle import vanilla_oracle as van

pytestmark = pytest.mark.gpu
T = torch.from_numpy
NAN = float("nan")


def launch(case, name, include_input, mode):
    """nsamd_ipe_encode through the one launch helper on a NaN-filled buffer with a guard row behind it, twice -> rows."""
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import functional as F

    n, S = case["t_bins"].shape[0], case["t_bins"].shape[1] - 1
    M = n * S
    freqs = T(mr.frequencies(name)).cuda()
    width = 6 * freqs.shape[0] + (3 if include_input else 0)
    if mode == "ray":
        keep = [T(case[k]).cuda() for k in ("origins", "directions", "t_bins", "pixel_area")]
        pts, area, var = N.make_points(origins=keep[0], directions=keep[1], t_bins=keep[2], samples_per_ray=S), keep[3], None
    else:
        keep = [T(a).cuda() for a in mr.gaussians32(case)]
        pts, area, var = N.make_points(positions=keep[0]), None, keep[1]
    outs = []
    for _ in range(2):
        buf = torch.full((M + 1, width), NAN, device="cuda")
        F.ipe_encode_launch(pts, M, area, var, freqs, include_input, buf[:M])
        torch.cuda.synchronize()
        assert torch.isnan(buf[M]).all(), "the guard row behind the output was written"
        outs.append(buf[:M].cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), "two launches differ"
    return outs[0].reshape(n, S, width)


@pytest.mark.parametrize("n,S", mr.GPU_CASES)
def test_ipe_encode_entry_by_entry_against_float64(golden, n, S):
    g = golden("mipnerf")
    case = mr.make_case(n, S)
    k = float(g[mr.case_key(n, S)])
    for name in mr.ENCODINGS:
        freqs = mr.frequencies(name)
        for include_input in (True, False):
            for mode in ("ray", "explicit"):
                explicit = None
                if mode == "explicit":
                    mean32, var32 = mr.gaussians32(case)
                    explicit = (mean32.reshape(n, S, 3), var32.reshape(n, S, 3))
                rows = launch(case, name, include_input, mode)
                rows64, scale = mr.encode_f64(case, freqs, include_input, explicit=explicit)
                worst = mr.measure(rows, rows64, scale)
                print(f"ipe_encode n={n} S={S} {name} include_input={include_input} {mode}: measure {worst:.3f}, "
                      f"reference {float(g[mr.case_key(n, S)]):.3f}, bound {mr.bound_f64(k):.3f}")
                assert worst <= mr.bound_f64(k)
                if (n, S) == mr.FIXTURE_CASE and include_input and mode == "ray":  # the reference's own fp32 rows
                    ref = g[f"ref_enc_{name}"]
                    r = slice(0, ref.shape[0])
                    np.testing.assert_array_equal(g[f"freqs_{name}"], freqs)
                    far = (np.abs(rows[r].astype(np.float64) - ref) / scale[r]).max()
                    print(f"  ... against the reference's fp32 rows: {far:.3f}, bound {mr.bound_ref(k):.3f}")
                    assert far <= mr.bound_ref(k)


def test_ipe_encode_on_the_references_own_gaussians_and_through_the_encoding(golden):
    """Explicit mode as NeRFEncoding.forward(x, covs) reaches it: the reference's fp32 means and covariances -> its rows."""
    from nerfstudio_amd.field_components.encodings import NeRFEncoding

    g = golden("mipnerf")
    n, S = mr.FIXTURE_CASE
    case = mr.make_case(n, S)
    k = float(g[mr.case_key(n, S)])
    enc = NeRFEncoding(3, 16, 0.0, 16.0, True)
    mean, cov = T(g["ref_mean"]).cuda(), T(g["ref_cov"]).cuda()
    out = enc(mean, covs=cov)
    assert out.shape == (n, S, 99)
    rows64, scale = mr.encode_f64(case, g["freqs_f16"], True, explicit=(g["ref_mean"], mr.diagonal(g["ref_cov"])))
    assert mr.measure(out.cpu().numpy(), rows64, scale) <= mr.bound_f64(k)
    far = (np.abs(out.cpu().numpy().astype(np.float64) - g["ref_enc_f16"]) / scale).max()
    print(f"explicit mode on the reference's Gaussians against the reference's fp32 rows: {far:.3f}, bound {mr.bound_ref(k):.3f}")
    assert far <= mr.bound_ref(k)
    # inputs that carry gradient take the same arithmetic through torch: within the same bound, and a gradient
    mg = mean.clone().requires_grad_(True)
    out_g = enc(mg, covs=cov)
    assert mr.measure(out_g.detach().cpu().numpy(), rows64, scale) <= mr.bound_f64(k)
    out_g[..., :96].sum().backward()
    assert torch.isfinite(mg.grad).all() and float(mg.grad.abs().sum()) > 0


def _model(params, **cfg):
    from nerfstudio_amd.mipnerf import MipNerfModel, MipNerfModelConfig

    model = MipNerfModel(MipNerfModelConfig(**cfg)).cuda()
    assert set(model.state_dict()) == set(params)
    model.load_state_dict({k: v.detach() for k, v in params.items()})
    return model


def _params(g):
    params = van.init_field_params(van.VanillaCfg(pos_frequencies=16, pos_max_exp=16.0), 95, "field.")
    np.testing.assert_allclose(np.array([float(v.double().sum()) for v in params.values()]), g["param_checksum"], rtol=1e-12)
    return params


def _bundle(g):
    from nerfstudio_amd.cameras.rays import RayBundle

    n = g["m_origins"].shape[0]
    return RayBundle(origins=T(g["m_origins"]).cuda(), directions=T(g["m_directions"]).cuda(), pixel_area=T(g["m_pixel_area"]).cuda(),
                     nears=torch.full((n, 1), 2.0).cuda(), fars=torch.full((n, 1), 6.0).cuda())


# the vanilla-NeRF test's tolerance per output (tests/test_gpu_vanilla.py:140-153): (rtol, atol)
VANILLA_TOL = {"weights_coarse": (5e-4, 2e-7), "weights_fine": (2e-3, 1e-6), "rgb_coarse": (0, 1e-5), "rgb_fine": (0, 1e-5),
               "accumulation_coarse": (0, 5e-6), "accumulation_fine": (0, 5e-6), "depth_coarse": (2e-5, 0), "depth_fine": (2e-5, 0)}


def check_output(got, g, key, name):
    ref = g[key]
    got = got.reshape(ref.shape)
    rtol, atol = VANILLA_TOL[name]
    bound = np.maximum(atol + rtol * np.abs(ref), mr.MARGIN * float(g[key + "_dist"]))
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{key}: largest error {err.max():.3e}, smallest bound {bound.min():.3e}, reference's distance from float64 "
          f"{float(g[key + '_dist']):.3e}")
    assert (err <= bound).all(), key
    zero = np.unpackbits(g[key + "_zero64"])[:ref.size].astype(bool).reshape(ref.shape)
    assert not got[zero].any(), key


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_mipnerf_model_matches_the_reference_fixture(golden, mode):
    g = golden("mipnerf")
    params = _params(g)
    model = _model(params, num_coarse_samples=64, num_importance_samples=128)
    training = mode == "train"
    model.train(training)
    jit = (T(g["j0"]).cuda(), T(g["j1"]).cuda()) if training else None
    with torch.set_grad_enabled(training):
        out = model.get_outputs(_bundle(g), jitters=jit)
    for name in VANILLA_TOL:
        got = out[name].detach().cpu().numpy()
        check_output(got[..., 0] if name.startswith("weights") else got, g, f"{mode}_{name}", name)
    if not training:
        return
    loss_dict = model.get_loss_dict(out, {"image": T(g["m_target"]).cuda()})
    assert list(loss_dict) == ["rgb_loss_coarse", "rgb_loss_fine"]
    loss = sum(loss_dict.values())
    ref_loss = float(g["train_loss"])
    assert abs(float(loss.detach()) - ref_loss) <= max(2e-5 * abs(ref_loss), mr.MARGIN * float(g["train_loss_dist"]))
    loss.backward()
    grads = dict(model.named_parameters())
    for name in params:
        gr = grads[name].grad.reshape(-1).cpu()
        ref_vals, stat = g[f"train_gval_{name}"], g[f"train_gstat_{name}"]
        atol = max(3e-2 * max(float(np.abs(ref_vals).max()), float(stat[0]) / np.sqrt(gr.numel())) + 1e-12,
                   mr.MARGIN * float(g[f"train_gdist_{name}"]))
        np.testing.assert_allclose(gr[T(g[f"train_gidx_{name}"])].numpy(), ref_vals, rtol=0, atol=atol, err_msg=name)
        norm_tol = max(2e-3 * float(stat[0]), mr.MARGIN * abs(float(stat[0]) - float(g[f"train_gnorm64_{name}"])))
        assert abs(float(gr.double().norm()) - float(stat[0])) <= norm_tol, name


def test_ray_mode_field_equals_the_explicit_mode_field(golden):
    """The same samples with and without their pack: rays + bin edges into the kernel, or get_gaussian_blob's means and
    covariances (fp32 torch ops) into explicit mode. The encodings differ within the encoding bound — both are fp32 evaluations
    of the same float64 rows, each within bound_f64 of them — and the densities as two fp32 evaluations of the reference's field do:
    the vanilla test's weights tolerance, on the density (rtol 2e-3; atol 1e-6 of the largest)."""
    from nerfstudio_amd.cameras.rays import RayBundle, samples_from_bins
    from nerfstudio_amd.field_components.field_heads import FieldHeadNames

    g = golden("mipnerf")
    n, S = mr.FIXTURE_CASE
    case = mr.make_case(n, S)
    k = float(g[mr.case_key(n, S)])
    model = _model(_params(g), num_coarse_samples=16, num_importance_samples=16).eval()
    rb = RayBundle(origins=T(case["origins"]).cuda(), directions=T(case["directions"]).cuda(),
                   pixel_area=T(case["pixel_area"]).cuda()[:, None])
    tb = T(case["t_bins"]).cuda()
    packed = samples_from_bins(rb, tb, tb, None)
    loose = packed[0:n]
    assert packed.pack is not None and loose.pack is None
    field, enc = model.field, model.field.position_encoding
    with torch.no_grad():
        rows_ray = enc.ray_forward(field_point_spec(packed), packed.frustums.pixel_area[..., 0, 0]).cpu().numpy()
        blob = loose.frustums.get_gaussian_blob()
        rows_exp = enc(blob.mean, covs=blob.cov).cpu().numpy()
        out_ray, out_exp = field.forward(packed), field.forward(loose)
    rows64, scale = mr.encode_f64(case, mr.frequencies("f16"), True)
    # either route is an fp32 evaluation of the same float64 rows (the explicit one composed as the reference composes it: the
    # Gaussians in fp32 torch ops, then the encoding), so each gets bound_f64 and the two are at most twice that apart
    far_ray, far_exp = mr.measure(rows_ray, rows64, scale), mr.measure(rows_exp, rows64, scale)
    apart = (np.abs(rows_ray.astype(np.float64).reshape(scale.shape) - rows_exp.reshape(scale.shape)) / scale).max()
    print(f"ray mode {far_ray:.3f}, explicit mode {far_exp:.3f} against float64 (bound {mr.bound_f64(k):.3f}); apart {apart:.3f}")
    assert far_ray <= mr.bound_f64(k) and far_exp <= mr.bound_f64(k) and apart <= 2 * mr.bound_f64(k)
    d_ray, d_exp = (o[FieldHeadNames.DENSITY].cpu().numpy() for o in (out_ray, out_exp))
    assert d_ray.shape == (n, S, 1)
    np.testing.assert_allclose(d_exp, d_ray, rtol=2e-3, atol=1e-6 * float(np.abs(d_ray).max()))
    np.testing.assert_allclose(out_exp[FieldHeadNames.RGB].cpu().numpy(), out_ray[FieldHeadNames.RGB].cpu().numpy(), rtol=0, atol=1e-5)


def field_point_spec(samples):
    from nerfstudio_amd.fields.base_field import point_spec

    spec, _ = point_spec(samples)
    assert spec.ray_mode
    return spec


def test_mipnerf_trains():
    """30 RAdam steps (the method config's optimiser) on one batch: both losses end below their first values, every parameter
    gradient is finite and not all zero."""
    from nerfstudio_amd.cameras.rays import RayBundle
    from nerfstudio_amd.mipnerf import MipNerfModel, MipNerfModelConfig

    torch.manual_seed(0)
    model = MipNerfModel(MipNerfModelConfig(num_coarse_samples=16, num_importance_samples=16)).cuda().train()
    n = 256
    o = torch.zeros(n, 3).cuda()
    o[:, 2] = 4.0
    d = torch.nn.functional.normalize(torch.randn(n, 3) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1).cuda()
    area = torch.full((n, 1), 8.1e-7).cuda()
    target = torch.rand(n, 3).cuda() * 0.5
    opt = torch.optim.RAdam(model.get_param_groups()["fields"], lr=5e-4, eps=1e-8)
    first = None
    for _ in range(30):
        out = model(RayBundle(origins=o, directions=d, pixel_area=area))
        losses = model.get_loss_dict(out, {"image": target})
        first = {k: float(v.detach()) for k, v in losses.items()} if first is None else first
        opt.zero_grad()
        sum(losses.values()).backward()
        for name, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and bool(p.grad.any()), name
        opt.step()
    last = {k: float(v.detach()) for k, v in losses.items()}
    print("mip-NeRF losses, first and after 30 steps:", first, last)
    assert last["rgb_loss_coarse"] < first["rgb_loss_coarse"] and last["rgb_loss_fine"] < first["rgb_loss_fine"]
