"""MI355X: training a `predict_normals` model on the explicit kernel schedule.

(a) nsamd_normals_losses and (b) nsamd_nerf_encode_bwd_rays against the float64 restatements of tests/normals_loss_reference.py,
every output entry, within MARGIN = 4 units of the fp32 restatement's own distance from float64 on the same inputs (the rule of
tests/test_depth_cpu.py; the unit is floored at one fp32 ulp, exact zeros must be exact zeros); (c) functional.normals_losses
under autograd against the reference's fixture; (d) the model of tests/test_normals.py::test_model_normals_golden_gpu built with
`fused_train_step=True` against the reference's own losses and gradients, with that test's tolerances; (e) fused against module
path on one model with the camera optimiser on; (f) repeatability, and a plain model untouched by the stage.

The ratios and distances the tests print are kept in profiles/normals_loss_float64_ratios.txt and profiles/normals_fused_step.txt.
"""
import numpy as np
import pytest
import torch

from oracle import nerfacto_oracle as orc

import normals_loss_reference as nl
import normals_reference as nref
from conftest import load_golden
from test_normals import FIELD_GRADS, _check_losses, _np, _rel, _rendered_normals_close

pytestmark = pytest.mark.gpu
T = torch.from_numpy
GPU_CASES = nl.CASES + ((2, 4096),)  # the largest S: the lane-chunk loop's last trip


def dev(a):
    return T(np.ascontiguousarray(a)).cuda()


def run_losses(inp, orientation_scale, pred_scale, want=nl.OUTPUTS, d_dir_prior=None):
    from nerfstudio_amd import functional as F

    n, S = inp["weights"].shape
    new = lambda *shape: torch.full(shape, float("nan"), device="cuda")  # noqa: E731  (an entry left out stays NaN)
    bufs = {"orientation_per_ray": new(n), "pred_per_ray": new(n), "d_pred_pre": new(n * S, 3),
            "d_directions": new(n, 3) if d_dir_prior is None else dev(d_dir_prior)}
    out = {k: (bufs[k] if k in want else None) for k in nl.OUTPUTS}
    F.normals_losses_launch(dev(inp["weights"]), dev(inp["normals"].reshape(-1, 3)),
                            dev(inp["pred_pre"].reshape(-1, 3)) if ("pred_per_ray" in want or "d_pred_pre" in want) else None,
                            dev(inp["directions"]) if ("orientation_per_ray" in want or "d_directions" in want) else None,
                            orientation_scale, pred_scale, out["orientation_per_ray"], out["pred_per_ray"], out["d_pred_pre"],
                            out["d_directions"], accumulate_directions=d_dir_prior is not None)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


# ---------------------------------------------------------------- (a) the loss kernel ----------------------------------------------
@pytest.mark.parametrize("n,S", GPU_CASES)
def test_normals_losses_against_float64(n, S):
    inp = nl.case_inputs(n, S)
    os_, ps = 1e-4 / n, 1e-3 / n
    got = run_losses(inp, os_, ps)

    def report(k, err, unit, ratio):
        print(f"normals_losses n={n} S={S} {k}: error {err:.3e}, fp32 restatement {unit:.3e}, ratio {ratio:.2f}")

    nl.check_against_float64(got, inp, os_, ps, report=report)
    assert got["orientation_per_ray"][1] == 0 and not got["d_directions"][1].any()  # every normal of ray 1 faces the camera
    assert not got["d_pred_pre"][:S].any() and got["pred_per_ray"][0] == 0  # ray 0 carries no weight
    # two runs: the same bits
    again = run_losses(inp, os_, ps)
    assert all(np.array_equal(got[k], again[k]) for k in nl.OUTPUTS)
    # the accumulate flag: prior + alone, bit for bit; the other outputs unchanged
    prior = np.random.RandomState(n + S).standard_normal((n, 3)).astype(np.float32)
    acc = run_losses(inp, os_, ps, d_dir_prior=prior)
    assert np.array_equal(acc["d_directions"], prior + got["d_directions"])
    assert all(np.array_equal(acc[k], got[k]) for k in nl.OUTPUTS[:3])
    # every nullable output: each one alone gives its own bits
    for k in nl.OUTPUTS:
        alone = run_losses(inp, os_, ps, want=(k,))
        assert np.array_equal(alone[k], got[k]) and all(alone[j] is None for j in nl.OUTPUTS if j != k)


def test_normals_losses_no_rays_and_too_many_samples():
    from nerfstudio_amd import _native as N

    lib = N.load()
    buf = torch.full((4097 * 3,), 7.0, device="cuda")
    p = N.ptr(buf)
    assert lib.nsamd_normals_losses(p, p, p, p, 0, 48, 1.0, 1.0, p, p, p, p, 0, N.stream()) == 0
    assert lib.nsamd_normals_losses(p, p, p, p, 1, 4097, 1.0, 1.0, p, p, p, p, 0, N.stream()) == N.ERR_UNSUPPORTED
    assert lib.nsamd_normals_losses(p, p, p, p, 1, 0, 1.0, 1.0, p, p, p, p, 0, N.stream()) == N.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())  # nothing was launched


# ---------------------------------------------------------------- (b) the encoding's ray gradient -----------------------------------
@pytest.mark.parametrize("n,S", [(5, 1), (7, 48), (3, 64), (3, 65), (2, 130)])  # S > 64: the lane-strided loop's later trips
@pytest.mark.parametrize("include_input", [0, 1])
@pytest.mark.parametrize("padded", [False, True])  # rows 12 (15 with the input) floats apart, or the 27 of the MLP's input rows
def test_nerf_encode_bwd_rays_against_float64(n, S, include_input, padded):
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import functional as F

    stride = 27 if padded else 12 + 3 * include_input
    inp = nl.encode_case_inputs(n, S, stride, bool(include_input))
    o, d, t, freqs, rows = (dev(inp[k]) for k in ("origins", "directions", "t_bins", "freqs", "rows"))
    pts = N.make_points(None, o, d, t, S)
    args = (inp["origins"], inp["directions"], inp["t_bins"], inp["freqs"], bool(include_input), inp["d_out"])
    f64 = nl.nerf_encode_bwd_rays_torch(*args, dtype=torch.float64)
    f32 = nl.nerf_encode_bwd_rays_torch(*args, dtype=torch.float32)
    prior = np.random.RandomState(S).standard_normal((2, n, 3)).astype(np.float32)
    alone = None
    for accumulate in (0, 1):
        g_o, g_d = (dev(prior[0]), dev(prior[1])) if accumulate else (torch.full((n, 3), float("nan"), device="cuda"),
                                                                      torch.full((n, 3), float("nan"), device="cuda"))
        F.nerf_encode_bwd_rays_launch(pts, n * S, freqs, bool(include_input), rows, stride, g_o, g_d, accumulate=bool(accumulate))
        torch.cuda.synchronize()
        got = (g_o.cpu().numpy(), g_d.cpu().numpy())
        if not accumulate:
            alone = got
            for name, a, b64, b32 in zip(("d_origins", "d_directions"), got, f64, f32):
                unit = nl.error_unit(b32, b64)
                err = nl.rel_err(a, b64)
                print(f"nerf_encode_bwd_rays n={n} S={S} include_input={include_input} stride={stride} {name}: error {err:.3e}, "
                      f"fp32 restatement {unit:.3e}, ratio {err / unit:.2f}")
                assert err <= nl.MARGIN * unit, name
        else:
            assert np.array_equal(got[0], prior[0] + alone[0]) and np.array_equal(got[1], prior[1] + alone[1])


# ---------------------------------------------------------------- (c) under autograd ------------------------------------------------
@pytest.mark.parametrize("i", range(len(nl.CASES)))
def test_functional_normals_losses_under_autograd(i):
    from nerfstudio_amd import functional as F

    g = load_golden("normals_losses")
    inp = {k: g[f"c{i}_{k}"] for k in ("weights", "normals", "pred_pre", "directions")}
    ref = {k: g[f"c{i}_{k}"] for k in nl.OUTPUTS}
    n, S = inp["weights"].shape
    x = dev(inp["pred_pre"]).requires_grad_(True)
    v = dev(inp["directions"]).requires_grad_(True)
    orientation, pred = F.normals_losses(dev(inp["weights"])[..., None], dev(inp["normals"]), x, v)
    assert orientation.shape == (n,) and pred.shape == (n,)
    (orientation.sum() + pred.sum()).backward()
    got = {"orientation_per_ray": orientation.detach().cpu().numpy(), "pred_per_ray": pred.detach().cpu().numpy(),
           "d_pred_pre": x.grad.reshape(-1, 3).cpu().numpy(), "d_directions": v.grad.cpu().numpy()}
    assert x.grad.shape == x.shape
    nl.check_against_float64(got, inp)
    f64 = nl.normals_losses_torch(**inp, dtype=torch.float64)
    f32 = nl.normals_losses_torch(**inp, dtype=torch.float32)
    for k in nl.OUTPUTS:  # ... and MARGIN + 1 of them from the reference's own fp32 arrays (the triangle inequality)
        assert nl.rel_err(got[k], ref[k]) <= (nl.MARGIN + 1) * max(nl.error_unit(ref[k], f64[k]), nl.error_unit(f32[k], f64[k])), k
    # upstream gradients other than ones scale the rays' rows
    x.grad, v.grad = None, None
    orientation, pred = F.normals_losses(dev(inp["weights"]), dev(inp["normals"]), x, v)
    up = torch.arange(1, n + 1, device="cuda", dtype=torch.float32)
    ((orientation * up).sum() + (pred * 2 * up).sum()).backward()
    np.testing.assert_allclose(v.grad.cpu().numpy(), got["d_directions"] * np.arange(1, n + 1)[:, None], rtol=1e-6)
    np.testing.assert_allclose(x.grad.reshape(n, S, 3).cpu().numpy(),
                               got["d_pred_pre"].reshape(n, S, 3) * (2.0 * np.arange(1, n + 1))[:, None, None], rtol=1e-6)


# ---------------------------------------------------------------- the models ---------------------------------------------------------
def oracle_cfg(num_images, main_log2=10):
    c = orc.NerfactoCfg(main_grid=orc.HashGridCfg(16, 16, 2048, main_log2),
                        prop_grids=(orc.HashGridCfg(5, 16, 128, 8), orc.HashGridCfg(5, 16, 256, 8)), num_images=int(num_images))
    c.predict_normals = True
    return c


def build_model(cfg, params, predict_normals=True, fused=True, camera="off", **kw):
    """The model of tests/test_normals.py::test_model_normals_golden_gpu (the oracle's parameters loaded into NerfactoModel)."""
    from nerfstudio_amd.cameras.camera_optimizers import CameraOptimizerConfig
    from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig

    mc = NerfactoModelConfig(
        log2_hashmap_size=cfg.main_grid.log2_hashmap_size, predict_normals=predict_normals, fused_train_step=fused,
        camera_optimizer=CameraOptimizerConfig(mode=camera),
        proposal_net_args_list=[{"hidden_dim": cfg.prop_hidden_dim, "log2_hashmap_size": gr.log2_hashmap_size,
                                 "num_levels": gr.num_levels, "max_res": gr.max_res, "use_linear": False} for gr in cfg.prop_grids],
        average_init_density=cfg.average_init_density, appearance_embed_dim=cfg.appearance_embed_dim, **kw)
    model = NerfactoModel(mc, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), cfg.num_images)
    sd = {k: v.detach().clone() for k, v in params.items()}
    for i in range(2):
        sd[f"proposal_networks.{i}.mlp_base.0.hash_table"] = sd[f"proposal_networks.{i}.encoding.hash_table"]
    if not predict_normals:
        sd = {k: v for k, v in sd.items() if "pred_normals" not in k}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    return model.cuda().train()


def bundle(o, d, cams):
    from nerfstudio_amd.cameras.rays import RayBundle

    n = o.shape[0]
    return RayBundle(origins=dev(o), directions=dev(d), pixel_area=torch.full((n, 1), 1e-6).cuda(), camera_indices=dev(cams)[:, None])


def iteration(model, o, d, cams, target, jit):
    """One training iteration through the Model API -> (outputs, losses); the gradients are in `param.grad`."""
    model.zero_grad()
    out = model(bundle(o, d, cams), jitters=jit)
    batch = {"image": dev(target)}
    losses = model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return out, losses


def golden_model_inputs():
    g = load_golden("normals")
    cfg = oracle_cfg(g["m_num_images"])
    params = orc.init_params(cfg, seed=int(g["m_seed"]), table_std=float(g["m_table_std"]))
    rays = (g["m_origins"], g["m_directions"], g["m_cams"], g["m_target"], [dev(g[f"m_j{i}"]) for i in range(3)])
    return g, cfg, params, rays


NORMALS_KEYS = {"rgb_loss", "interlevel_loss", "distortion_loss", "orientation_loss", "pred_normal_loss"}


# ---------------------------------------------------------------- (d) the reference's own gradients -------------------------------
def test_fused_step_reproduces_the_references_losses_and_gradients():
    g, cfg, params, rays = golden_model_inputs()
    model = build_model(cfg, params)
    out, losses = iteration(model, *rays)
    assert "fused_step" in out and model._fused.runner.normals is not None
    assert set(losses) == NORMALS_KEYS
    _check_losses(losses, g, normals_rtol=1e-2)
    n = g["m_origins"].shape[0]
    assert out["normals"].shape == (n, 3) and out["pred_normals"].shape == (n, 3)
    np.testing.assert_allclose(_np(out["rgb"]), g["m_train_rgb"], atol=1e-4, err_msg="rgb")
    _rendered_normals_close(out["normals"], g["m_train_normals"], "train")
    np.testing.assert_allclose(_np(out["pred_normals"]), g["m_train_pred_normals"], atol=2e-3)
    assert out["rendered_orientation_loss"].shape == (n,) and out["rendered_pred_normal_loss"].shape == (n,)
    named = dict(model.named_parameters())
    for name, key in FIELD_GRADS:
        print(f"fused step against the reference, {name}: relative L2 {_rel(named[name].grad, g['m_' + key]):.3e}")
    for name, key in FIELD_GRADS:
        assert _rel(named[name].grad, g["m_" + key]) < 2e-2, name
    assert _rel(model.proposal_networks[0].encoding.hash_table.grad, g["m_prop0_dtable"]) < 2e-2


def test_without_its_loss_the_stage_adds_nothing():
    _, cfg, params, rays = golden_model_inputs()
    silent = build_model(cfg, params, pred_normal_loss_mult=0.0)
    plain = build_model(cfg, params, predict_normals=False)
    _, losses = iteration(silent, *rays)
    _, plain_losses = iteration(plain, *rays)
    assert float(losses["pred_normal_loss"]) == 0.0 and set(plain_losses) == NORMALS_KEYS - {"orientation_loss", "pred_normal_loss"}
    assert plain._fused.runner.normals is None
    for name, p in silent.named_parameters():
        if "pred_normals" in name:
            assert p.grad is not None and not p.grad.any(), name  # exactly zero
    table = "field.mlp_base.model.0.hash_table"
    got, want = dict(silent.named_parameters()), dict(plain.named_parameters())
    assert torch.equal(got[table].grad, want[table].grad)
    for name, p in want.items():  # ... and touches nothing else
        if p.grad is not None:
            assert torch.equal(got[name].grad, p.grad), name
    for k in plain_losses:
        assert torch.equal(losses[k], plain_losses[k]), k


# ---------------------------------------------------------------- (e) fused against module path, camera optimiser on --------------
PN_NAMES = [f"field.mlp_pred_normals.layers.{j}.{k}" for j in range(3) for k in ("weight", "bias")] + \
    ["field.field_head_pred_normals.net.weight", "field.field_head_pred_normals.net.bias"]
POSE = "camera_optimizer.pose_adjustment"


def hash_features_f64(pos64, pos32, table64, scalings, table_size):
    """HashEncoding.pytorch_fwd as differentiable float64 torch ops of the normalised positions `pos64` and of the table; the
    cells come from the fp32 positions, as in normals_reference.field_pre_torch64 -> [M, 2 L]."""
    feats = []
    for idx, w32, sc in nref._cells(np.asarray(pos32).reshape(-1, 3), scalings, table_size):
        w = T(w32) + (pos64 - pos64.detach()) * sc  # the fp32 offset's value, slope scalings[l]
        v = [table64[T(idx[k].astype(np.int64))] for k in range(8)]
        wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
        yc_zc, yf_zc = v[7] * wx + v[6] * (1 - wx), v[5] * wx + v[4] * (1 - wx)
        yf_zf, yc_zf = v[1] * wx + v[0] * (1 - wx), v[3] * wx + v[2] * (1 - wx)
        zc, zf = yc_zc * wy + yf_zc * (1 - wy), yc_zf * wy + yf_zf * (1 - wy)
        feats.append(zc * wz + zf * (1 - wz))
    return torch.cat(feats, dim=-1)


def normals_chain_f64(model, runner, cfg):
    """The share of every gradient that comes from the two normals losses, in float64 on the kernels' own activations (the
    runner's fp32 buffers: the 27-wide input rows, the weights, the analytic normals, the hash features, the corrected rays and
    the final bins): the predicted-normals MLP and its head, the base MLP, the main table, the rays (hash grid + frequency
    encoding + the orientation loss's view directions) and, through the exponential map, the pose corrections."""
    from nerfstudio_amd.cameras.lie_groups import exp_map_SO3xR3

    nb, mc = runner.normals, model.config
    n, S = runner.weights[-1].shape
    c64 = lambda t: t.detach().double().cpu()  # noqa: E731
    named = dict(model.named_parameters())
    w, nrm = c64(runner.weights[-1]), c64(nb["n_smp"]).view(n, S, 3)
    out = {}
    # predicted-normals branch: parameters and the input rows' gradient
    x = c64(nb["in"]).requires_grad_(True)
    p = [c64(named[k]).requires_grad_(True) for k in PN_NAMES]
    h = torch.relu(x @ p[0].t() + p[1])
    h = torch.relu(h @ p[2].t() + p[3])
    h = h @ p[4].t() + p[5]
    pre = (h @ p[6].t() + p[7]).view(n, S, 3)
    loss = mc.pred_normal_loss_mult * nl.pred_normal_loss(w[..., None], nrm, nl.pred_normals_head(pre)).mean()
    *g_pn, d_in = torch.autograd.grad(loss, p + [x])
    out.update(zip(PN_NAMES, g_pn))
    # base MLP on the geometry-feature columns
    enc = c64(runner.f_enc).t().contiguous().requires_grad_(True)
    base = [c64(named[k]).requires_grad_(True) for k in nref.BASE_KEYS]
    out16 = torch.relu(enc @ base[0].t() + base[1]) @ base[2].t() + base[3]
    *g_base, d_enc = torch.autograd.grad((out16[:, 1:] * d_in[:, 12:]).sum(), base + [enc])
    out.update(zip(nref.BASE_KEYS, g_base))
    # hash grid: the table's share and the rays'
    o32, d32, t32 = (a.detach().cpu().numpy() for a in (runner.origins, runner.directions, runner.t_bins[-1]))
    o, d = T(o32).double().requires_grad_(True), T(d32).double().requires_grad_(True)
    t = T(t32).double()
    raw = (o[:, None, :] + d[:, None, :] * ((t[:, :-1] + t[:, 1:]) / 2)[..., None]).reshape(-1, 3)
    pos, _ = orc.normalise_positions(raw, True)
    pos32, _ = nref.normalise_fp32(nref.ray_positions_fp32(o32, d32, t32), True)
    table = c64(named[nref.TABLE_KEY]).requires_grad_(True)
    feats = hash_features_f64(pos, pos32, table, cfg.main_grid.scalings().numpy(), cfg.main_grid.table_size)
    out[nref.TABLE_KEY], h_o, h_d = torch.autograd.grad((feats * d_enc).sum(), (table, o, d))
    # frequency encoding of the raw positions, and the orientation loss's view directions
    e_o, e_d = nl.nerf_encode_bwd_rays_torch(o32, d32, t32, nb["freqs"].cpu().numpy(), False, d_in[:, :12].numpy())
    l_d = nl.normals_losses_torch(w.numpy(), nrm.numpy(), pre.detach().numpy(), d32, orientation_scale=mc.orientation_loss_mult / n)
    out["d_origins"] = h_o + T(e_o)
    out["d_directions"] = h_d + T(e_d) + T(l_d["d_directions"])
    # the pose corrections: origins + t(c), R(c) raw directions
    pose = c64(named[POSE]).requires_grad_(True)
    cams = runner.camera_indices.cpu()
    c = exp_map_SO3xR3(pose[cams])
    ro, rd = c64(runner.raw_origins), c64(runner.raw_directions)
    co, cd = ro + c[:, :3, 3], torch.bmm(c[:, :3, :3], rd[..., None]).squeeze(-1)
    (out[POSE],) = torch.autograd.grad((co * out["d_origins"]).sum() + (cd * out["d_directions"]).sum(), pose)
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("camera_kernels", [True, False])  # nsamd_camera_backward, or the pose share through torch's autograd
def test_fused_step_against_module_path_with_camera_optimiser(camera_kernels, monkeypatch):
    from nerfstudio_amd import functional as F

    monkeypatch.setenv("NSAMD_CAMERA_KERNELS", "1" if camera_kernels else "0")
    n = 65
    cfg = oracle_cfg(5, main_log2=12)
    params = orc.init_params(cfg, seed=3, table_std=0.5)
    o, d, cams, target = (a.numpy() for a in orc.synthetic_rays(n, cfg.num_images, seed=4))
    rs = np.random.RandomState(5)
    jit = [dev(rs.uniform(0, 1, (n, 1)).astype(np.float32)) for _ in range(3)]
    model = build_model(cfg, params, camera="SO3xR3")
    with torch.no_grad():
        model.camera_optimizer.pose_adjustment.copy_(dev(rs.normal(0, 1e-2, (cfg.num_images, 6)).astype(np.float32)))
    grads = lambda: {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}  # noqa: E731

    # ---- the whole iteration on both paths ----
    results = {}
    for path in ("fused", "module"):
        model.config.fused_train_step = path == "fused"
        out, losses = iteration(model, o, d, cams, target, jit)
        assert ("fused_step" in out) == (path == "fused")
        results[path] = ({k: float(v) for k, v in losses.items()}, grads())
    (lf, gf), (lm, gm) = results["fused"], results["module"]
    r = model._fused.runner
    assert r.cam_kernels == camera_kernels
    assert set(lf) == set(lm) == NORMALS_KEYS | {"camera_opt_regularizer"}
    for k in lm:  # the same sampler kernels, the same cells
        assert lf[k] == pytest.approx(lm[k], rel=1e-5), k
    assert set(gf) == set(gm) and POSE in gf
    for k in gm:
        print(f"fused against module path, {k}: relative L2 {_rel(gf[k], gm[k]):.3e}")

    # ---- the normals losses' share alone: the fused chain (the runner's buffers still hold the fused iteration) ... ----
    for p in model.parameters():
        p.grad.zero_()
    r.normals_backward()
    nb = r.normals
    pose = model.camera_optimizer.pose_adjustment
    F.camera_backward_launch(pose, F.CAMERA_MODES["SO3xR3"], r.raw_directions, r.camera_indices, [nb["d_origins"]],
                             [nb["d_directions"]], 0.0, 0.0, pose.grad, None)
    torch.cuda.synchronize()
    share_f = grads()
    share_f.update(d_origins=nb["d_origins"].cpu().numpy(), d_directions=nb["d_directions"].cpu().numpy())
    # ... and autograd's, on the module path: only the two terms are back-propagated
    model.config.fused_train_step = False
    model.zero_grad()
    rb = bundle(o, d, cams)
    out = model(rb, jitters=jit)
    batch = {"image": dev(target)}
    losses = model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch))
    terms = losses["orientation_loss"] + losses["pred_normal_loss"]
    ray_o, ray_d = torch.autograd.grad(terms, [rb.origins, rb.directions], retain_graph=True)  # (the corrected rays)
    terms.backward()
    torch.cuda.synchronize()
    share_m = grads()
    share_m.update(d_origins=ray_o.cpu().numpy(), d_directions=ray_d.cpu().numpy())

    # ---- both against float64 on the kernels' own activations: fused <= 4 x module path, every gradient the chain reaches ----
    f64 = normals_chain_f64(model, r, cfg)
    assert set(f64) == set(PN_NAMES) | set(nref.BASE_KEYS) | {nref.TABLE_KEY, POSE, "d_origins", "d_directions"}
    worst = {}
    for k, ref in f64.items():
        assert np.abs(ref).max() > 0, k
        df, dm = _rel(share_f[k], ref), _rel(share_m[k], ref)
        print(f"normals chain against float64, {k}: fused {df:.3e}, module path {dm:.3e}")
        worst[k] = (df, dm)
    for k, (df, dm) in worst.items():
        assert df <= 4.0 * max(dm, nl.ULP), k
    # the chain reaches nothing else
    for k, g in share_f.items():
        assert k in f64 or not g.any(), k

    # ---- the share arrives in the whole iteration's pose gradient: the two paths agree to well inside the share's size, so a
    # ---- missing, doubled or sign-flipped share (a distance of at least the share) cannot pass
    size = float(np.linalg.norm(f64[POSE]) / np.linalg.norm(gm[POSE]))
    print(f"normals share of the pose gradient: {size:.3e} of its norm; fused against module path {_rel(gf[POSE], gm[POSE]):.3e}")
    assert _rel(gf[POSE], gm[POSE]) <= size / 10.0


# ---------------------------------------------------------------- (f) repeatability; a plain model is untouched ----------------------
def test_two_identical_iterations_give_identical_bits():
    _, cfg, params, rays = golden_model_inputs()
    model = build_model(cfg, params)
    runs = []
    for _ in range(2):
        out, losses = iteration(model, *rays)
        runs.append(({k: v.detach().clone() for k, v in losses.items()}, {k: p.grad.clone() for k, p in model.named_parameters()},
                     {k: out[k].clone() for k in ("normals", "pred_normals", "rendered_orientation_loss", "rendered_pred_normal_loss")}))
    for a, b in zip(runs[0], runs[1]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_plain_model_runner_is_the_stage_disabled():
    from nerfstudio_amd.train_step import NerfactoTrainStep

    g, cfg, params, (o, d, cams, target, jit) = golden_model_inputs()
    grads = []
    for predict_normals in (False, True):
        model = build_model(cfg, params, predict_normals=predict_normals, fused=False)
        r = NerfactoTrainStep(model, o.shape[0], "cuda")
        if predict_normals:
            assert r.normals is not None
            r.normals = None  # the stage disabled: what is left is the schedule as it was
        else:
            assert r.normals is None and not any("normals" in k for k in vars(r) if k not in ("normals", "_normals_fresh"))
        r.set_batch(dev(o), dev(d), dev(cams), dev(target))
        for lvl, j in enumerate(jit):
            r.jitter[lvl].copy_(j.reshape(-1))
        model.zero_grad()
        r.prepare_grads(True)
        r.forward_backward(True, draw_jitter=False)
        torch.cuda.synchronize()
        assert set(r.loss_dict()) == {"rgb_loss", "interlevel_loss", "distortion_loss"} and "normals" not in r.outputs()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if "pred_normals" not in k})
    assert grads[0].keys() == grads[1].keys()
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
