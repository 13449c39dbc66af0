"""CPU tests of the training side of `predict_normals` on the explicit kernel schedule: the torch restatements of
nsamd_normals_losses and nsamd_nerf_encode_bwd_rays (tests/normals_loss_reference.py) against the reference's own fixture
(tests/golden/normals_losses.npz, written by tests/golden/make_golden_normals_losses.py) and against finite differences; the
per-sample arithmetic of nerfstudio_amd/csrc/normals_loss.h compiled for the host (tests/hostcheck/normals_loss_helpers.cc); the
rendered loss terms of the model-level fixture (tests/golden/normals.npz); which models FusedTrainStep takes; and the two entry
points' argument checks, which answer before anything is launched.

Bounds. fp32 against fp32 (restatement against fixture): the gradients are the same autograd formulas element by element — bit
for bit; a per-ray term is a sum of S fp32 summands whose order torch may choose: (S + 8) 2^-24 sum |summands|. fp32 against
float64: MARGIN = 4 times the fp32 restatement's own distance from float64 on the same inputs, per output array, that distance
floored at one fp32 ulp (the rule of tests/test_depth_cpu.py); entries that are exactly zero in float64 must be exactly zero.
"""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import normals_loss_reference as nl

F32P = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
T = torch.from_numpy


def fixture_case(g, i):
    return ({k: g[f"c{i}_{k}"] for k in ("weights", "normals", "pred_pre", "directions")},
            {k: g[f"c{i}_{k}"] for k in nl.OUTPUTS})


# ---------------------------------------------------------------- the restatement against the reference's fixture -------------
def test_fixture_holds_the_cases_with_their_planted_entries():
    g = load_golden("normals_losses")
    assert [tuple(c) for c in g["cases"]] == list(nl.CASES)
    for i, (n, S) in enumerate(nl.CASES):
        inp, ref = fixture_case(g, i)
        again = nl.case_inputs(n, S)
        assert all(np.array_equal(inp[k], again[k]) for k in inp)  # the generator's inputs are the shared seeded ones
        assert inp["weights"].shape == (n, S) and ref["d_pred_pre"].shape == (n * S, 3)
        assert not inp["weights"][0].any() and ref["orientation_per_ray"][0] == 0 and ref["pred_per_ray"][0] == 0
        assert ref["orientation_per_ray"][1] == 0 and not ref["d_directions"][1].any()  # every normal faces the camera
        assert not inp["normals"][min(2, n - 1), 0].any() and not inp["pred_pre"][n - 1, S - 1].any()
        assert np.abs(ref["d_pred_pre"]).max() > 0 and np.abs(ref["d_directions"]).max() > 0


@pytest.mark.parametrize("i", range(len(nl.CASES)))
def test_fp32_restatement_equals_the_fixture(i):
    inp, ref = fixture_case(load_golden("normals_losses"), i)
    got = nl.normals_losses_torch(**inp, dtype=torch.float32)
    assert np.array_equal(got["d_pred_pre"], ref["d_pred_pre"])
    assert np.array_equal(got["d_directions"], ref["d_directions"])
    n, S = inp["weights"].shape
    f64 = nl.normals_losses_torch(**inp, dtype=torch.float64)
    w = inp["weights"].astype(np.float64)
    nr, v = inp["normals"].astype(np.float64), inp["directions"].astype(np.float64)
    p = nl.pred_normals_head(T(inp["pred_pre"]).double()).numpy()
    summands = {"orientation_per_ray": w * np.minimum(0.0, -(nr * v[:, None, :]).sum(-1)) ** 2,
                "pred_per_ray": w * (1.0 - (nr * p).sum(-1))}
    for k, terms in summands.items():
        np.testing.assert_allclose(terms.sum(-1), f64[k], rtol=1e-12, atol=1e-15)  # (the summands are the restatement's)
        bound = (S + 8) * 2.0 ** -24 * np.abs(terms).sum(-1)
        assert (np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64)) <= bound).all(), k
        assert (np.abs(ref[k].astype(np.float64) - f64[k]) <= bound).all(), k


def test_float64_autograd_equals_finite_differences():
    inp = nl.case_inputs(3, 4, seed=5)
    inp["pred_pre"][2, 3] = (0.3, -0.2, 0.1)  # (the planted exact zero sits on normalize's clamp: not differentiable there)
    f64 = nl.normals_losses_torch(**inp, dtype=torch.float64)
    h = 1e-6

    def total(x, v, which):
        out = nl.normals_losses_torch(inp["weights"], inp["normals"], x, v, dtype=torch.float64)
        return out[which].sum()

    x0, v0 = inp["pred_pre"].astype(np.float64).reshape(-1, 3), inp["directions"].astype(np.float64)
    for idx in np.ndindex(*x0.shape):
        e = np.zeros_like(x0)
        e[idx] = h
        fd = (total(x0 + e, v0, "pred_per_ray") - total(x0 - e, v0, "pred_per_ray")) / (2 * h)
        assert fd == pytest.approx(f64["d_pred_pre"][idx], rel=1e-6, abs=1e-9)
    for idx in np.ndindex(*v0.shape):
        e = np.zeros_like(v0)
        e[idx] = h
        fd = (total(x0, v0 + e, "orientation_per_ray") - total(x0, v0 - e, "orientation_per_ray")) / (2 * h)
        assert fd == pytest.approx(f64["d_directions"][idx], rel=1e-6, abs=1e-9)


def test_encoding_ray_gradient_restatement_against_finite_differences():
    inp = nl.encode_case_inputs(3, 5, 15, True, seed=3)
    args = (inp["t_bins"], inp["freqs"], True, inp["d_out"])
    g_o, g_d = nl.nerf_encode_bwd_rays_torch(inp["origins"], inp["directions"], *args)

    def total(o, d):
        t = T(inp["t_bins"]).double()
        pos = o[:, None, :] + d[:, None, :] * ((t[:, :-1] + t[:, 1:]) / 2)[..., None]
        return float((nl.nerf_encode_torch(pos.reshape(-1, 3), T(inp["freqs"]).double(), True) * T(inp["d_out"]).double()).sum())

    o0, d0, h = T(inp["origins"]).double(), T(inp["directions"]).double(), 1e-6
    for idx in np.ndindex(3, 3):
        e = torch.zeros_like(o0)
        e[idx] = h
        assert (total(o0 + e, d0) - total(o0 - e, d0)) / (2 * h) == pytest.approx(g_o[idx], rel=1e-6, abs=1e-8)
        assert (total(o0, d0 + e) - total(o0, d0 - e)) / (2 * h) == pytest.approx(g_d[idx], rel=1e-6, abs=1e-8)
    # the encoding itself: [sin(s), sin(s + pi/2), x], s[d F + f] = 2 pi x_d freqs[f]
    x = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float64)
    enc = nl.nerf_encode_torch(x, torch.tensor([1.0, 2.0], dtype=torch.float64), True)[0].numpy()
    s = 2 * np.pi * np.array([0.1, 0.2, -0.2, -0.4, 0.3, 0.6])
    np.testing.assert_allclose(enc, np.concatenate([np.sin(s), np.cos(s), [0.1, -0.2, 0.3]]), atol=1e-12)


# ---------------------------------------------------------------- normals_loss.h on the host ------------------------------------
@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libnormalslosscheck.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "normals_loss_helpers.cc")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.hc_normals_losses.argtypes = [F32P, F32P, F32P, F32P, C.c_int64, C.c_int, C.c_float, C.c_float, F32P, F32P, F32P, F32P]
    return lib


@pytest.mark.parametrize("n,S", nl.CASES)
def test_header_arithmetic_on_the_host_against_float64(hc, n, S):
    inp = nl.case_inputs(n, S)
    os_, ps = 1e-4 / n, 1e-3 / n
    got = {"orientation_per_ray": np.empty(n, np.float32), "pred_per_ray": np.empty(n, np.float32),
           "d_pred_pre": np.empty((n * S, 3), np.float32), "d_directions": np.empty((n, 3), np.float32)}
    assert hc.hc_normals_losses(inp["weights"], np.ascontiguousarray(inp["normals"].reshape(-1, 3)),
                                np.ascontiguousarray(inp["pred_pre"].reshape(-1, 3)), inp["directions"], n, S, os_, ps,
                                got["orientation_per_ray"], got["pred_per_ray"], got["d_pred_pre"], got["d_directions"]) == 0
    nl.check_against_float64(got, inp, os_, ps)
    # the planted entries: exact zeros, and the clamped normalisation's gradient -w n / 1e-12 (times 1 - tanh(0)^2 = 1)
    assert got["orientation_per_ray"][1] == 0 and not got["d_directions"][1].any() and not got["d_pred_pre"][:S].any()
    w, nr = inp["weights"][n - 1, S - 1], inp["normals"][n - 1, S - 1]
    np.testing.assert_allclose(got["d_pred_pre"][-1], -(np.float32(ps) * w * nr) / np.float32(1e-12), rtol=1e-6)


# ---------------------------------------------------------------- the model-level fixture --------------------------------------
def test_restatement_reproduces_the_rendered_terms_of_the_model_fixture():
    g = load_golden("normals")
    w, nr, p, v = (T(g[k]) for k in ("m_train_w", "m_train_normals_samples", "m_train_pred_normals_samples", "m_directions"))
    S = w.shape[1]
    for got, key, terms in ((nl.orientation_loss(w[..., None], nr, v), "m_rendered_orientation",
                             w * torch.clamp(-(nr * v[:, None, :]).sum(-1), max=0.0) ** 2),
                            (nl.pred_normal_loss(w[..., None], nr, p), "m_rendered_pred_normal", w * (1.0 - (nr * p).sum(-1)))):
        bound = (S + 8) * 2.0 ** -24 * terms.abs().sum(-1).numpy()
        assert (np.abs(got.numpy().astype(np.float64) - g[key].astype(np.float64)) <= bound).all(), key
    n = w.shape[0]
    assert 1e-4 * float(T(g["m_rendered_orientation"]).sum()) / n == pytest.approx(float(g["m_loss_orientation"]), rel=1e-5)
    assert 1e-3 * float(T(g["m_rendered_pred_normal"]).sum()) / n == pytest.approx(float(g["m_loss_pred_normal"]), rel=1e-5)


# ---------------------------------------------------------------- which models the fused step takes ---------------------------
def test_supported_table():
    from nerfstudio_amd import eval_render
    from nerfstudio_amd.depth_nerfacto import DepthNerfactoModelConfig
    from nerfstudio_amd.fused_step import FusedTrainStep
    from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig
    from nerfstudio_amd.pipeline import unsupported_model_reason
    from nerfstudio_amd.trainer import HipTrainer
    from test_fused_step_cpu import small_model

    m = lambda cfg: SimpleNamespace(config=cfg)  # noqa: E731
    args = [{"hidden_dim": 16, "log2_hashmap_size": 7, "num_levels": 5, "max_res": r, "use_linear": False} for r in (32, 64)]
    box = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])

    def build(**kw):
        return NerfactoModel(NerfactoModelConfig(log2_hashmap_size=8, proposal_net_args_list=args, **kw), box, 7).train()

    # the option AND the field's modules: supported, with the two loss keys behind the others
    model = build(predict_normals=True)
    fs = FusedTrainStep(model)
    assert model.field.use_pred_normals and fs.supported() is None
    assert fs.loss_keys() == ("rgb_loss", "interlevel_loss", "distortion_loss", "orientation_loss", "pred_normal_loss")
    assert FusedTrainStep(build()).loss_keys() == ("rgb_loss", "interlevel_loss", "distortion_loss")
    depth = FusedTrainStep(m(DepthNerfactoModelConfig()))
    assert depth.supported() is None and depth.loss_keys()[-1] == "depth_loss" and len(depth.loss_keys()) == 4
    # gradient scaling together with normals: declined with a reason that names both
    reason = FusedTrainStep(build(predict_normals=True, use_gradient_scaling=True)).supported()
    assert "predict_normals" in reason and "use_gradient_scaling" in reason
    assert FusedTrainStep(build(use_gradient_scaling=True)).supported() is None
    # ---- the pinned answers ----
    assert "predict_normals" in FusedTrainStep(m(NerfactoModelConfig(predict_normals=True))).supported()
    flipped = small_model()  # only the config flag: its field has no normals modules
    flipped.config.predict_normals = True
    flipped.config.fused_train_step = True
    assert not flipped.field.use_pred_normals
    assert FusedTrainStep(flipped).loss_keys() == ("rgb_loss", "interlevel_loss", "distortion_loss")  # no stage, no keys
    with pytest.raises(NotImplementedError, match="predict_normals"):
        flipped._fused_step()
    assert unsupported_model_reason(m(NerfactoModelConfig(predict_normals=True))) == "predict_normals"
    assert unsupported_model_reason(model) == "predict_normals"  # captured iterations keep declining
    assert eval_render.supported(model) == "predict_normals" and eval_render.supported(model, normals=True) is None
    with pytest.raises(NotImplementedError, match="module path"):
        HipTrainer(m(DepthNerfactoModelConfig()), None, None, None)


def test_eval_and_training_share_one_layer_list():
    from nerfstudio_amd import eval_render
    from nerfstudio_amd.fields.nerfacto_field import NerfactoField

    fld = NerfactoField(torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_images=3, log2_hashmap_size=8, use_pred_normals=True)
    layers = eval_render.pred_normals_layers(fld)
    assert [tuple(W.shape) for W, _, _ in layers] == [(64, 27), (64, 64), (64, 64), (3, 64)]
    assert [act for _, _, act in layers] == [1, 1, 0, 0]
    assert layers[0][0] is fld.mlp_pred_normals.layers[0].weight and layers[3][1] is fld.field_head_pred_normals.net.bias


# ---------------------------------------------------------------- the entry points' argument checks ----------------------------
OK, INVALID, UNSUPPORTED = 0, -1, -2


def test_normals_losses_validates_before_it_launches():
    from nerfstudio_amd import _native as N

    lib = N.load()
    one = 8  # a non-null address: no case below reaches a launch

    def call(weights=one, normals=one, pred_pre=one, directions=one, n=4, S=48, o_out=one, p_out=one, d_pre=one, d_dir=one):
        return lib.nsamd_normals_losses(weights, normals, pred_pre, directions, n, S, 1.0, 1.0, o_out, p_out, d_pre, d_dir, 0, None)

    assert call(n=0) == OK and call(n=0, weights=None, normals=None) == OK
    assert call(n=-1) == INVALID
    for S in (0, -3, 4097):
        assert call(S=S) == UNSUPPORTED and call(S=S, n=0) == UNSUPPORTED
    assert call(n=-1, S=4097) == INVALID  # the precedence
    assert call(n=1 << 34) == UNSUPPORTED  # more workgroups than a launch grid holds
    assert call(weights=None) == INVALID and call(normals=None) == INVALID
    assert call(pred_pre=None) == INVALID and call(directions=None) == INVALID
    assert call(o_out=None, p_out=None, d_pre=None, d_dir=None) == OK  # nothing wanted: nothing launched
    assert call(o_out=None, p_out=None, d_pre=None, d_dir=None, weights=None) == OK


def test_nerf_encode_bwd_rays_validates_before_it_launches():
    from nerfstudio_amd import _native as N

    lib = N.load()
    one = 8

    def call(M=96, S=48, positions=None, origins=one, dirs=one, t_bins=one, freqs=one, F=2, inc=0, d_out=one, stride=12, d_o=one,
             d_d=one):
        pts = N.Points()
        pts.positions, pts.origins, pts.directions, pts.t_bins, pts.samples_per_ray = positions, origins, dirs, t_bins, S
        return lib.nsamd_nerf_encode_bwd_rays(pts, M, freqs, F, inc, d_out, stride, d_o, d_d, 0, None)

    assert call(M=0) == OK
    assert call(M=-1) == INVALID and call(M=100) == INVALID and call(S=0) == INVALID  # check_points
    assert call(origins=None) == INVALID and call(dirs=None) == INVALID and call(t_bins=None) == INVALID
    assert call(positions=one) == INVALID  # ray mode only
    assert call(F=0) == INVALID and call(F=65) == INVALID
    assert call(stride=11) == INVALID and call(inc=1, stride=14) == INVALID and call(inc=1, stride=15, M=0) == OK
    assert call(freqs=None) == INVALID and call(d_out=None) == INVALID and call(d_o=None) == INVALID and call(d_d=None) == INVALID
