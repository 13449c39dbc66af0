"""CPU tests of mip-NeRF's integrated positional encoding: the float64 restatement (tests/mipnerf_reference.py), the per-sample
arithmetic of nerfstudio_amd/csrc/ipe.h compiled for the host (tests/hostcheck/ipe_helpers.cc), every layer above the kernel —
functional.ipe_encode, NeRFEncoding, NeRFField(use_integrated_encoding=True), MipNerfModel — with functional.ipe_encode_launch
replaced by the fp32 cast of the float64 restatement, and the entry point's argument checks.

Fixture: tests/golden/mipnerf.npz, written by the reference's own modules (tests/golden/make_golden_mipnerf.py).

Bounds. `k_ref_n<n>_s<S>` in the fixture is the REFERENCE's largest value of mipnerf_reference.measure — per entry,
|fp32 - f64| / (damp64 2^-23 (2 pi freq (|o_d| + |d_d| t_mean) + 2) + 2^-23) — on the inputs of that one case, over the three
encodings (16 frequencies at exponents 0 .. 16, 4 at 0 .. 4, 1), measured when the fixture was written:

    n1_s1 0.661   n3_s5 1.170   n33_s17 1.695 (the fixture case)   n4_s64 1.751   n2_s65 1.723   n5_s128 1.883   n2_s193 1.946
    n1_s63 1.477  n5_s13 1.454  n3_s19 1.617

An independent fp32 evaluation gets MARGIN = 4 x max(k_ref, 1) against float64 (another libm's expf / sinf and another operation
order: mipnerf_reference.bound_f64), and MARGIN + 1 against the reference's own fp32 arrays — read as written,
4 max(k_ref, 1) + 1, or by the triangle inequality 4 max(k_ref, 1) + k_ref, whichever is smaller (mipnerf_reference.bound_ref:
7.78 on the fixture case). Entries that are exactly zero in float64 must be exactly zero.
"""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import mipnerf_reference as mr

T = torch.from_numpy
F32P = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
CASE_KEYS = ("origins", "directions", "t_bins", "pixel_area")


def fixture_case(g):
    return {k: g[k] for k in CASE_KEYS}


def k_bound(g, n, S):
    """The recorded figure of the reference on this case: mr.bound_f64 / mr.bound_ref turn it into the two bounds."""
    return float(g[mr.case_key(n, S)])


def check_rows(got, case, freqs, include_input, k, ref=None, explicit=None):
    """fp32 rows against float64 within bound_f64(k), and against the reference's fp32 rows within bound_ref(k)."""
    rows64, scale = mr.encode_f64(case, freqs, include_input, explicit=explicit)
    worst = mr.measure(got, rows64, scale)
    assert worst <= mr.bound_f64(k), (worst, mr.bound_f64(k))
    if ref is not None:
        assert (np.abs(np.asarray(got, np.float64).reshape(scale.shape) - ref.reshape(scale.shape)) / scale).max() <= mr.bound_ref(k)
    return worst


# ---------------------------------------------------------------- 1. the fixture ---------------------------------------------
def test_fixture_regenerates_and_holds_the_edge_rows_and_every_bound():
    g = load_golden("mipnerf")
    n, S = mr.FIXTURE_CASE
    again = mr.make_case(n, S)
    for k in CASE_KEYS:
        assert g[k].dtype == np.float32
        np.testing.assert_array_equal(again[k], g[k])
    assert g["t_bins"].shape == (33, 18) and g["ref_enc_f16"].shape == (33, 17, 99) and g["ref_cov"].shape == (33, 17, 3, 3)
    assert g["ref_enc_f4"].shape == (mr.EDGE_RAYS, 17, 27) and g["ref_enc_f1"].shape == (mr.EDGE_RAYS, 17, 9)
    norms = np.linalg.norm(g["directions"].astype(np.float64), axis=-1)
    assert abs(norms[1] - 0.5) < 1e-6 and abs(norms[2] - 2.0) < 1e-6 and np.abs(np.delete(norms, (1, 2)) - 1).max() < 1e-6
    tb = g["t_bins"]
    assert tb[0, -1] == tb[0, -2] and (np.diff(tb, axis=-1)[1:] > 0).all() and (tb[:, :-1] + tb[:, 1:]).min() > 0
    assert g["pixel_area"].min() < 8.1e-7 / 2 and g["pixel_area"].max() > 8.1e-7 * 2  # spread around a pinhole's
    keys = sorted(mr.case_key(*c) for c in mr.GPU_CASES)
    assert mr.FIXTURE_CASE in mr.GPU_CASES and sorted(k for k in g if k.startswith("k_ref_")) == keys
    assert all(0.1 < float(g[k]) < 4.0 for k in keys)  # the reference is a few ulp of its inputs from float64, no more
    for name in mr.ENCODINGS:
        np.testing.assert_array_equal(g[f"freqs_{name}"], mr.frequencies(name))


# ---------------------------------------------------------------- 2. the float64 restatement ---------------------------------
def cov_tolerance(case):
    """What fp32 may differ from float64 in a covariance entry var_along d_i d_j + var_across (delta_ij - d_i d_j / |d|^2): each
    product and each of the two variances is a handful of roundings of quantities without cancellation (h << c), the difference
    delta_ij - d_i d_j / |d|^2 cancels, so its error is an ulp of its TERMS: 16 ulp of the sum of the absolute terms."""
    mean, cov, t_mean = mr.gaussians(case)
    d = case["directions"].astype(np.float64)
    dd = np.abs(d[:, :, None] * d[:, None, :])
    mag = (d**2).sum(-1)[:, None, None]
    tb = case["t_bins"].astype(np.float64)
    c, h = (tb[:, :-1] + tb[:, 1:]) / 2, (tb[:, 1:] - tb[:, :-1]) / 2
    q = 3 * c**2 + h**2
    va = h**2 / 3 + (4 / 15) * h**4 * (12 * c**2 + h**2) / q**2
    vx = (case["pixel_area"].astype(np.float64) / np.pi)[:, None] * (c**2 / 4 + (5 / 12) * h**2 + (4 / 15) * h**4 / q)
    terms = va[..., None, None] * dd[:, None] + vx[..., None, None] * (np.eye(3) + dd / mag)[:, None]
    reach = np.abs(case["origins"].astype(np.float64))[:, None, :] + np.abs(d)[:, None, :] * t_mean[..., None]
    return mean, cov, 16 * mr.ULP * terms, 4 * mr.ULP * reach


def test_float64_gaussians_match_the_reference_and_this_package():
    from nerfstudio_amd.cameras.rays import Frustums

    g = load_golden("mipnerf")
    case = fixture_case(g)
    mean, cov, cov_tol, mean_tol = cov_tolerance(case)
    assert (np.abs(g["ref_cov"] - cov) <= cov_tol).all() and (np.abs(g["ref_mean"] - mean) <= mean_tol).all()
    # un-normalised directions: the along-ray part scales with |d|^2, the across-ray part does not (rays 1 and 2 against 3)
    assert np.abs(np.swapaxes(cov, -1, -2) - cov).max() == 0 and (np.diagonal(cov, axis1=-2, axis2=-1) >= 0).all()
    assert 0 < np.abs(cov[0, -1]).max() < 1e-4 < np.abs(cov[0, -2]).max()  # the zero-width bin: only the across-ray disc is left
    n, S = mr.FIXTURE_CASE
    tb = T(case["t_bins"])
    fr = Frustums(origins=T(case["origins"])[:, None].expand(n, S, 3), directions=T(case["directions"])[:, None].expand(n, S, 3),
                  starts=tb[:, :-1, None], ends=tb[:, 1:, None], pixel_area=T(case["pixel_area"])[:, None, None].expand(n, S, 1))
    blob = fr.get_gaussian_blob()
    assert blob.mean.shape == (n, S, 3) and blob.cov.shape == (n, S, 3, 3)
    assert (np.abs(blob.cov.numpy() - cov) <= cov_tol).all() and (np.abs(blob.mean.numpy() - mean) <= mean_tol).all()
    # the fp32 evaluation of the restatement itself
    mean32, cov32, _ = mr.gaussians(case, np.float32)
    assert cov32.dtype == np.float32 and (np.abs(cov32 - cov) <= cov_tol).all() and (np.abs(mean32 - mean) <= mean_tol).all()


@pytest.mark.parametrize("name", list(mr.ENCODINGS))
def test_float64_restatement_in_fp32_is_within_the_bound_of_the_reference(name):
    g = load_golden("mipnerf")
    case = fixture_case(g)
    k = k_bound(g, *mr.FIXTURE_CASE)
    freqs = g[f"freqs_{name}"]
    mean32, cov32, _ = mr.gaussians(case, np.float32)
    rows32, _ = mr.ipe(mean32, mr.diagonal(cov32), freqs, True, np.float32)
    assert rows32.dtype == np.float32
    rows64, scale = mr.encode_f64(case, freqs, True)
    ref = g[f"ref_enc_{name}"]
    r = slice(0, ref.shape[0])
    assert (np.abs(rows32[r].astype(np.float64) - ref) / scale[r]).max() <= mr.bound_ref(k)
    assert mr.measure(rows32, rows64, scale) <= mr.bound_f64(k)
    assert mr.measure(ref, rows64[r], scale[r]) <= float(g[mr.case_key(*mr.FIXTURE_CASE)])  # the reference within its own figure
    # the layout: [sin | sin(. + pi / 2) | mean], k = axis * F + f; without the input the same rows minus the last three columns
    F = freqs.shape[0]
    assert rows64.shape[-1] == 6 * F + 3
    np.testing.assert_array_equal(mr.ipe(*mr.gaussians(case)[:1], mr.diagonal(mr.gaussians(case)[1]), freqs, False)[0], rows64[..., :-3])
    m = mr.gaussians(case)[0]
    np.testing.assert_array_equal(rows64[..., -3:], m)
    var = mr.diagonal(mr.gaussians(case)[1])
    f = F - 1
    want = np.exp(-0.5 * var[..., 1] * float(freqs[f]) ** 2) * np.sin(2 * np.pi * m[..., 1] * float(freqs[f]) + np.pi / 2)
    np.testing.assert_allclose(rows64[..., 3 * F + 1 * F + f], want, rtol=0, atol=1e-9)


# ---------------------------------------------------------------- 3. ipe.h on the host ---------------------------------------
@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libipecheck.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "ipe_helpers.cc")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.hc_ipe_rays.argtypes = [F32P, F32P, F32P, F32P, C.c_int64, C.c_int, F32P, C.c_int, C.c_int, F32P, F32P, F32P]
    lib.hc_ipe_explicit.argtypes = [F32P, F32P, C.c_int64, F32P, C.c_int, C.c_int, F32P]
    return lib


def host_rays(hc, case, freqs, include_input):
    n, S = case["t_bins"].shape[0], case["t_bins"].shape[1] - 1
    F = freqs.shape[0]
    out = np.full((n, S, 6 * F + (3 if include_input else 0)), np.nan, np.float32)
    means, variances = np.empty((n * S, 3), np.float32), np.empty((n * S, 3), np.float32)
    assert hc.hc_ipe_rays(case["origins"], case["directions"], case["t_bins"], case["pixel_area"], n, S, np.ascontiguousarray(freqs),
                          F, int(include_input), out, means, variances) == 0
    return out, means, variances


def host_explicit(hc, means, variances, freqs, include_input):
    F = freqs.shape[0]
    out = np.full((means.shape[0], 6 * F + (3 if include_input else 0)), np.nan, np.float32)
    assert hc.hc_ipe_explicit(means, variances, means.shape[0], np.ascontiguousarray(freqs), F, int(include_input), out) == 0
    return out


@pytest.mark.parametrize("name", list(mr.ENCODINGS))
def test_header_arithmetic_reproduces_the_reference_and_float64(hc, name):
    g = load_golden("mipnerf")
    case = fixture_case(g)
    k = k_bound(g, *mr.FIXTURE_CASE)
    freqs, ref = g[f"freqs_{name}"], g[f"ref_enc_{name}"]
    rows, means, variances = host_rays(hc, case, freqs, True)
    r = slice(0, ref.shape[0])
    part = {kk: v[r] for kk, v in case.items()}  # the rays the fixture holds this encoding for
    worst = check_rows(rows, case, freqs, True, k)
    check_rows(rows[r], part, freqs, True, k, ref=ref)
    print(f"ipe.h on the host, {name}, ray mode: measure {worst:.3f} (reference {float(g[mr.case_key(*mr.FIXTURE_CASE)]):.3f})")
    # without the input: the same bits minus the last three columns
    np.testing.assert_array_equal(host_rays(hc, case, freqs, False)[0], rows[..., :-3])
    # the Gaussians the rows were formed from, against float64 and the reference
    mean64, cov64, cov_tol, mean_tol = cov_tolerance(case)
    diag_tol = mr.diagonal(cov_tol).reshape(-1, 3)
    assert (np.abs(variances - mr.diagonal(cov64).reshape(-1, 3)) <= diag_tol).all()
    assert (np.abs(means - mean64.reshape(-1, 3)) <= mean_tol.reshape(-1, 3)).all()
    # explicit mode on the reference's own fp32 Gaussians
    ref_mean, ref_var = g["ref_mean"].reshape(-1, 3), np.ascontiguousarray(mr.diagonal(g["ref_cov"]).reshape(-1, 3))
    rows_e = host_explicit(hc, ref_mean, ref_var, freqs, True).reshape(rows.shape)
    check_rows(rows_e, case, freqs, True, k, explicit=(g["ref_mean"], mr.diagonal(g["ref_cov"])))
    check_rows(rows_e[r], part, freqs, True, k, ref=ref, explicit=(g["ref_mean"][r], mr.diagonal(g["ref_cov"])[r]))
    # explicit mode on the Gaussians ray mode formed: the same bits
    np.testing.assert_array_equal(host_explicit(hc, means, variances, freqs, True).reshape(rows.shape), rows)


def test_header_arithmetic_on_the_edge_rows_and_where_the_damping_is_zero(hc):
    g = load_golden("mipnerf")
    case = fixture_case(g)
    k = k_bound(g, *mr.FIXTURE_CASE)
    freqs = g["freqs_f16"]
    rows, means, variances = host_rays(hc, case, freqs, True)
    rows64, scale = mr.encode_f64(case, freqs, True)
    for ray in (1, 2):  # directions of length 0.5 and 2
        assert mr.measure(rows[ray], rows64[ray], scale[ray]) <= mr.bound_f64(k)
        assert (np.abs(rows[ray].astype(np.float64) - g["ref_enc_f16"][ray]) / scale[ray]).max() <= mr.bound_ref(k)
    # an un-normalised direction is not the normalised one: ray 2's along-ray variance is 4 x what a unit direction would give
    unit = dict(case, directions=(case["directions"] / np.linalg.norm(case["directions"], axis=-1, keepdims=True)).astype(np.float32))
    assert np.median(host_rays(hc, unit, freqs, True)[2][17 * 2:17 * 3] / variances[17 * 2:17 * 3]) < 0.3
    # the zero-width bin: finite, var_along == 0, the row within the bound
    last = variances.reshape(33, 17, 3)[0, -1]
    assert np.isfinite(rows[0, -1]).all() and (last >= 0).all() and last.max() < 1e-4
    assert mr.measure(rows[0, -1], rows64[0, -1], scale[0, -1]) <= mr.bound_f64(k)
    # where the damping factor underflows in fp32 (exp(-x), x > 104) the entry is exactly zero — its sine is never evaluated —
    # in the reference's rows too; these are a good part of mip-NeRF's rows
    _, cov64, _ = mr.gaussians(case)
    x = 0.5 * (mr.diagonal(cov64)[..., None] * freqs.astype(np.float64) ** 2).reshape(33, 17, 48)
    gone = np.concatenate([x > 104.5, x > 104.5], axis=-1)
    print(f"entries damped to exactly zero: {gone.mean():.3f} of the fixture's 96 encoded columns")
    assert gone.mean() > 0.1 and not rows[..., :96][gone].any() and not g["ref_enc_f16"][..., :96][gone].any()
    # a Gaussian wider than every wavelength: the whole encoding is exactly zero, the appended mean is the mean
    wide_mean = np.array([[0.3, -1.7, 2.9]], np.float32)
    wide = host_explicit(hc, wide_mean, np.full((1, 3), 1.0e3, np.float32), freqs, True)
    np.testing.assert_array_equal(wide[0, :96], np.zeros(96, np.float32))
    np.testing.assert_array_equal(wide[0, 96:], wide_mean[0])
    assert hc.hc_ipe_explicit(wide_mean, wide_mean, 1, np.ones(65, np.float32), 65, 1, np.empty((1, 393), np.float32)) == -2


# ---------------------------------------------------------------- 4. the layers above the kernel -----------------------------
@pytest.fixture
def fake_kernel(monkeypatch):
    """functional.ipe_encode_launch -> the fp32 cast of the float64 restatement, on CPU tensors; -> the calls it saw."""
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import functional as F

    calls = []
    monkeypatch.setattr(N, "require_cuda", lambda *a: None)
    monkeypatch.setattr(N, "make_points", lambda positions=None, origins=None, directions=None, t_bins=None, samples_per_ray=0:
                        types.SimpleNamespace(_tensors={"positions": positions, "origins": origins, "directions": directions,
                                                        "t_bins": t_bins}, samples_per_ray=samples_per_ray))
    monkeypatch.setattr(F, "ipe_encode_launch", mr.fake_ipe_launch(calls))
    return calls


def test_nerf_encoding_with_covariances_reproduces_the_fixture(fake_kernel):
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.field_components.encodings import NeRFEncoding

    g = load_golden("mipnerf")
    case = fixture_case(g)
    k = k_bound(g, *mr.FIXTURE_CASE)
    enc = NeRFEncoding(3, 16, 0.0, 16.0, True)
    mean, cov = T(g["ref_mean"]), T(g["ref_cov"])
    out = enc(mean, covs=cov)
    assert out.shape == (33, 17, 99) and out.dtype == torch.float32  # batch shape preserved
    explicit = (g["ref_mean"], mr.diagonal(g["ref_cov"]))
    check_rows(out.numpy(), case, g["freqs_f16"], True, k, ref=g["ref_enc_f16"], explicit=explicit)
    assert fake_kernel[-1] == {"mode": "explicit", "M": 33 * 17, "F": 16, "include_input": True, "pixel_area": None}
    assert NeRFEncoding(3, 4, 0.0, 4.0, False)(mean[:2], covs=cov[:2]).shape == (2, 17, 24)
    # inputs that carry gradient take the same arithmetic through torch: same values, and a gradient; no launch
    seen = len(fake_kernel)
    mg_ = mean.clone().requires_grad_(True)
    out_g = enc(mg_, covs=cov)
    assert len(fake_kernel) == seen and out_g.requires_grad
    check_rows(out_g.detach().numpy(), case, g["freqs_f16"], True, k, ref=g["ref_enc_f16"], explicit=explicit)
    out_g[..., :96].sum().backward()
    assert mg_.grad.shape == mean.shape and np.isfinite(mg_.grad.numpy()).all() and mg_.grad.abs().sum() > 0
    cg = cov.clone().requires_grad_(True)
    enc(mean, covs=cg).sum().backward()
    assert len(fake_kernel) == seen and cg.grad.abs().sum() > 0
    with torch.no_grad():  # ... unless no graph is being recorded
        enc(mg_, covs=cov)
    assert len(fake_kernel) == seen + 1
    # covs=None is what it was: the plain encoding's kernel (not this one)
    monkey_calls = []
    plain = F.nerf_encode
    try:
        F.nerf_encode = lambda spec, *a: monkey_calls.append(a) or torch.zeros(spec.num_points, 99)
        assert enc(mean).shape == (33, 17, 99) and monkey_calls == [(16, 0.0, 16.0, True)] and len(fake_kernel) == seen + 1
    finally:
        F.nerf_encode = plain
    # the functional refuses gradient, as nerf_encode does, and a mode without its array
    for spec, area, var in ((F.PointSpec(positions=mg_.reshape(-1, 3)), None, T(explicit[1]).reshape(-1, 3)),
                            (F.PointSpec(positions=mean.reshape(-1, 3)), None, cg[..., 0].reshape(-1, 3)),
                            (F.PointSpec(origins=T(case["origins"]).requires_grad_(True), directions=T(case["directions"]),
                                         t_bins=T(case["t_bins"])), T(case["pixel_area"]), None)):
        with pytest.raises(RuntimeError, match="no backward"):
            F.ipe_encode(spec, area, var, 16, 0.0, 16.0, True)
    with pytest.raises(ValueError, match="pixel_area with rays"):
        F.ipe_encode(F.PointSpec(positions=mean.reshape(-1, 3)), T(case["pixel_area"]), None, 16, 0.0, 16.0)
    with pytest.raises(ValueError, match="one pixel area per ray"):
        F.ipe_encode(F.PointSpec(origins=T(case["origins"]), directions=T(case["directions"]), t_bins=T(case["t_bins"])),
                     T(case["pixel_area"])[:5], None, 16, 0.0, 16.0)
    assert len(fake_kernel) == seen + 1
    # ray mode through the functional: the fixture's rows
    rows = F.ipe_encode(F.PointSpec(origins=T(case["origins"]), directions=T(case["directions"]), t_bins=T(case["t_bins"])),
                        T(case["pixel_area"])[:, None], None, 16, 0.0, 16.0, True)
    check_rows(rows.numpy(), case, g["freqs_f16"], True, k, ref=g["ref_enc_f16"])
    assert fake_kernel[-1]["mode"] == "ray" and rows.shape == (33 * 17, 99)


def mip_field():
    from nerfstudio_amd.field_components.encodings import NeRFEncoding
    from nerfstudio_amd.fields.vanilla_nerf_field import NeRFField

    return NeRFField(position_encoding=NeRFEncoding(3, 16, 0.0, 16.0, True), direction_encoding=NeRFEncoding(3, 4, 0.0, 4.0, True),
                     use_integrated_encoding=True)


def package_samples(case):
    from nerfstudio_amd.cameras.rays import RayBundle, samples_from_bins

    rb = RayBundle(origins=T(case["origins"]), directions=T(case["directions"]), pixel_area=T(case["pixel_area"])[:, None])
    tb = T(case["t_bins"])
    return samples_from_bins(rb, tb, tb, None)


def test_nerf_field_with_integrated_encoding_takes_ray_mode_or_explicit_mode(fake_kernel, monkeypatch):
    import cpu_kernels
    from nerfstudio_amd.field_components.encodings import Identity
    from nerfstudio_amd.field_components.field_heads import FieldHeadNames
    from nerfstudio_amd.fields.vanilla_nerf_field import NeRFField

    g = load_golden("mipnerf")
    case = fixture_case(g)
    torch.manual_seed(0)
    field = mip_field()
    assert field.use_integrated_encoding and field.spatial_distortion is None
    assert sorted("field." + k for k in field.state_dict()) == list(g["param_names"])  # the reference's state-dict names
    assert field.mlp_base.layers[0].weight.shape == (256, 99)
    samples = package_samples(case)
    with cpu_kernels.installed(monkeypatch), torch.no_grad():
        density, features = field.get_density(samples)
        assert fake_kernel[-1]["mode"] == "ray" and fake_kernel[-1]["M"] == 33 * 17 and fake_kernel[-1]["include_input"]
        np.testing.assert_array_equal(fake_kernel[-1]["pixel_area"].numpy(), case["pixel_area"])
        assert density.shape == (33, 17, 1) and features.shape == (33, 17, 256)
        # materialised frustums (any batch operation drops the pack; the reference's own containers never had one)
        loose = samples[0:33]
        assert loose.pack is None
        density_e, _ = field.get_density(loose)
        assert fake_kernel[-1]["mode"] == "explicit" and fake_kernel[-1]["M"] == 33 * 17 and fake_kernel[-1]["pixel_area"] is None
        # the two routes differ by the fp32 rounding of get_gaussian_blob's means and covariances, through an 8-layer MLP: two
        # fp32 evaluations of one field, the vanilla test's weights tolerance on the density (tests/test_gpu_mipnerf.py)
        np.testing.assert_allclose(density_e.numpy(), density.numpy(), rtol=2e-3, atol=1e-6 * float(density.abs().max()))
        out = field.forward(samples)
        assert set(out) == {FieldHeadNames.RGB, FieldHeadNames.DENSITY} and out[FieldHeadNames.RGB].shape == (33, 17, 3)
        # frustums with offsets raise, as in the reference (rays.py:81-82), on either route
        seen = len(fake_kernel)
        for s in (package_samples(case), package_samples(case)[0:33]):
            s.frustums.set_offsets(torch.zeros(33, 17, 3))
            with pytest.raises(NotImplementedError):
                field.get_density(s)
        assert len(fake_kernel) == seen
    with pytest.raises(NotImplementedError, match="spatial_distortion"):
        NeRFField(use_integrated_encoding=True, spatial_distortion=object())
    with pytest.raises(NotImplementedError, match="NeRFEncoding only"):
        NeRFField(position_encoding=Identity(in_dim=3), use_integrated_encoding=True)
    assert not NeRFField().use_integrated_encoding


def test_mipnerf_model_structure_and_loss_coefficients(fake_kernel, monkeypatch):
    import cpu_kernels
    from nerfstudio_amd.cameras.rays import RayBundle
    from nerfstudio_amd.mipnerf import MipNerfModel, MipNerfModelConfig
    from nerfstudio_amd.model_components.ray_samplers import PDFSampler, UniformSampler
    from oracle import vanilla_oracle as van

    g = load_golden("mipnerf")
    cfg = MipNerfModelConfig()
    assert (cfg.num_coarse_samples, cfg.num_importance_samples, cfg.near_plane, cfg.far_plane) == (128, 128, 2.0, 6.0)
    assert cfg.loss_coefficients == {"rgb_loss_coarse": 0.1, "rgb_loss_fine": 1.0} and cfg.background_color == "white"
    model = MipNerfModel(MipNerfModelConfig(num_coarse_samples=64, num_importance_samples=128))
    assert [n for n, _ in model.named_children()] == ["field", "sampler_uniform", "sampler_pdf", "renderer_rgb",
                                                      "renderer_accumulation", "renderer_depth", "rgb_loss", "collider"]
    assert sorted(model.state_dict()) == list(g["param_names"])  # ONE field, the reference's names
    assert type(model.sampler_uniform) is UniformSampler and type(model.sampler_pdf) is PDFSampler
    assert model.sampler_pdf.include_original is False and model.sampler_pdf.num_samples == 128
    assert model.field.use_integrated_encoding and model.field.position_encoding.get_out_dim() == 99
    assert model.field.direction_encoding.get_out_dim() == 27
    groups = model.get_param_groups()
    assert set(groups) == {"fields"} and len(groups["fields"]) == 24 and groups["fields"][0] is next(model.field.parameters())
    for declined in ({"use_gradient_scaling": True}, {"enable_temporal_distortion": True}):
        with pytest.raises(NotImplementedError, match="not built"):
            MipNerfModel(MipNerfModelConfig(**declined))
    # the loss coefficients scale the two MSE terms (models/mipnerf.py:157-160)
    rs = np.random.RandomState(5)
    outputs = {f"{k}_{p}": T(rs.uniform(0, 1, (12, d)).astype(np.float32)) for k, d in (("rgb", 3), ("accumulation", 1))
               for p in ("coarse", "fine")}
    image = T(rs.uniform(0, 1, (12, 3)).astype(np.float32))
    losses = model.get_loss_dict(outputs, {"image": image})
    assert list(losses) == ["rgb_loss_coarse", "rgb_loss_fine"]
    assert float(losses["rgb_loss_coarse"]) == pytest.approx(0.1 * float(((image - outputs["rgb_coarse"]) ** 2).mean()), rel=1e-6)
    assert float(losses["rgb_loss_fine"]) == pytest.approx(float(((image - outputs["rgb_fine"]) ** 2).mean()), rel=1e-6)
    # end to end on the CPU stand-ins: the reference's fixture, train mode with the recorded jitters (the GPU test holds the
    # per-output bounds; here the wiring: which field, which sampler, which samples feed which pass)
    params = van.init_field_params(van.VanillaCfg(pos_frequencies=16, pos_max_exp=16.0), 95, "field.")
    np.testing.assert_allclose(np.array([float(v.double().sum()) for v in params.values()]), g["param_checksum"], rtol=1e-12)
    model.load_state_dict(params)
    model.train()
    rb = RayBundle(origins=T(g["m_origins"]), directions=T(g["m_directions"]), pixel_area=T(g["m_pixel_area"]))
    with cpu_kernels.installed(monkeypatch):
        out = model(rb, jitters=(T(g["j0"]), T(g["j1"])))
        loss = sum(model.get_loss_dict(out, {"image": T(g["m_target"])}).values())
    assert [c["mode"] for c in fake_kernel] == ["ray", "ray"] and [c["M"] for c in fake_kernel] == [12 * 64, 12 * 128]
    np.testing.assert_allclose(out["weights_coarse"][..., 0].detach().numpy(), g["train_weights_coarse"], rtol=5e-4, atol=2e-7)
    np.testing.assert_allclose(out["rgb_fine"].detach().numpy(), g["train_rgb_fine"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(out["depth_fine"].detach().numpy(), g["train_depth_fine"], rtol=2e-5)
    np.testing.assert_allclose(float(loss.detach()), float(g["train_loss"]), rtol=2e-5)


# ---------------------------------------------------------------- 5. the entry point -----------------------------------------
def test_ipe_entry_point_is_declared_exported_and_bound():
    from nerfstudio_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsamd.h")).read(), flags=re.S)
    assert len(re.findall(r"\bnsamd_ipe_encode\s*\(", header)) == 1
    assert hasattr(C.CDLL(N.LIB_PATH), "nsamd_ipe_encode")
    assert N._SIGNATURES["nsamd_ipe_encode"] == [N.Points, N.i64, N.vp, N.vp, N.vp, N.i32, N.i32, N.vp, N.vp]
    assert len(N._SIGNATURES) == len(set(re.findall(r"\b(nsamd_[a-z0-9_]+)\s*\(", header))) == 79


def test_ipe_entry_point_validates_before_it_launches():
    """No call here reaches a launch: every one fails a check or has M == 0 (the pointers are host memory)."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    a = torch.zeros(64)
    rays = dict(origins=a, directions=a, t_bins=a, samples_per_ray=4)

    def call(M=8, F=16, pts=None, area=a, var=None, freqs=a, out=a, **over):
        pts = N.make_points(**dict(rays, **over)) if pts is None else pts
        return lib.nsamd_ipe_encode(pts, M, N.ptr(area), N.ptr(var), N.ptr(freqs), F, 1, N.ptr(out), None)

    explicit = N.make_points(positions=a)
    assert call(M=0) == 0 and call(M=0, pts=explicit, area=None, var=a) == 0      # M == 0: nothing launched
    assert call(M=-1) == -1 and call(M=-1, pts=explicit, var=a) == -1
    for k in ("origins", "directions", "t_bins"):                                 # an incomplete ray description
        assert call(**{k: None}) == -1 and call(M=0, **{k: None}) == -1
    assert call(samples_per_ray=0) == -1 and call(samples_per_ray=-4) == -1
    assert call(M=10) == -1 and call(M=10, samples_per_ray=5, F=0) == N.ERR_UNSUPPORTED  # M a multiple of S, or not
    for F in (0, -1, 65):                                                         # frequencies beyond the kernel's table
        assert call(F=F) == N.ERR_UNSUPPORTED and call(M=0, F=F) == N.ERR_UNSUPPORTED
    assert call(M=0, F=64) == 0 and call(M=0, F=1) == 0
    assert call(freqs=None) == -1 and call(out=None) == -1                        # null pointers
    assert call(area=None) == -1 and call(area=None, var=a) == -1                 # ray mode without its pixel areas
    assert call(pts=explicit, var=None) == -1                                     # explicit mode without its variances
    # two at once: the points first, then the frequency count, then the empty launch, then the pointers
    assert call(M=-1, F=0) == -1 and call(M=10, F=0) == -1
    assert call(F=0, out=None) == N.ERR_UNSUPPORTED and call(F=65, area=None) == N.ERR_UNSUPPORTED
    assert call(M=0, out=None, freqs=None, area=None) == 0
