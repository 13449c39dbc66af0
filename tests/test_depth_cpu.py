"""CPU tests of depth supervision (depth-nerfacto): the per-sample arithmetic of nerfstudio_amd/csrc/depth_loss.h compiled for the
host (tests/hostcheck/depth_helpers.cc), and every layer above the kernel — functional.depth_loss, model_components.losses,
DepthNerfactoModel, the plugin's subclass of the reference's model, discovery, pickle / yaml, the trainer seam's reason and the
entry point's validation — with nsamd_depth_loss replaced by the float64 restatement cast to fp32 (tests/depth_reference.py).

Fixture: tests/golden/depth_losses.npz, written by the reference's own losses.py (tests/golden/make_golden_depth.py).

Bounds. `e_ref_<ds|urf>_n<rays>_<euc|z>` in the fixture (depth_reference.case_key) is the REFERENCE's fp32 distance from float64
on the inputs of that one case — largest entrywise relative error of [per-ray values, weight gradients, predicted-depth gradient,
scalar loss], floored at one fp32 ulp — measured when the fixture was written; every test takes the bound of the case it checks.
On the fixture case (33 rays, z-depth / Euclidean):

    ds   [3.95e-07, 5.19e-06, floor, floor] / [1.73e-07, 7.25e-06, floor, floor]
    urf  [5.93e-06, 1.94e-05, 2.91e-07, 3.66e-07] / [5.98e-06, 1.18e-05, floor, 2.19e-07]

An independent fp32 evaluation gets that budget times MARGIN = 4 (another libm's expf / logf and another summation order) against
float64, and by the triangle inequality MARGIN + 1 against the reference's own fp32 arrays. Entries that are exactly zero in
float64 (masked rays, samples outside both URF intervals) must be exactly zero (depth_reference.rel_err).
"""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import depth_reference as dr

MARGIN = 4.0
F32P = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
NAMES = {dr.DS_NERF: "ds", dr.URF: "urf"}
COMBOS = [(lt, euc) for lt in (dr.DS_NERF, dr.URF) for euc in (True, False)]


def fixture_inputs(g):
    k = len(g["counts"])
    return {"t_bins": [g[f"t_bins_{i}"] for i in range(k)], "weights": [g[f"weights_{i}"] for i in range(k)],
            "termination_depth": g["termination_depth"], "directions_norm": g["directions_norm"],
            "predicted_depth": g["predicted_depth"], "sigma": g["sigma"]}


def fixture_reference(g, lt, euc):
    key = f"{NAMES[lt]}_{'euc' if euc else 'z'}"
    k = len(g["counts"])
    return {"loss": g[f"{key}_loss"], "d_weights": [g[f"{key}_d_weights_{i}"] for i in range(k)],
            "d_predicted": g.get(f"{key}_d_predicted")}


def f64_of(inp, lt, euc):
    return dr.depth_loss_f64(inp["t_bins"], inp["weights"], inp["termination_depth"], inp["directions_norm"],
                             inp["predicted_depth"], inp["sigma"], euc, lt)


def case_bounds(g, inp, lt, euc):
    """The reference's own fp32 error on the inputs of this case: [per_ray, d_weights, d_predicted, loss]."""
    return g[dr.case_key(lt, inp["termination_depth"].shape[0], euc)]


def check(got, inp, lt, euc, g, ref=None):
    """got: dict(loss, d_weights, d_predicted[, per_ray]) in fp32 -> asserts the bounds of the module docstring."""
    e = case_bounds(g, inp, lt, euc)
    f64 = f64_of(inp, lt, euc)
    if got.get("per_ray") is not None:
        assert dr.rel_err(got["per_ray"], f64["per_ray"]) <= MARGIN * e[0]
    for a, b in zip(got["d_weights"], f64["d_weights"]):
        assert dr.rel_err(a, b) <= MARGIN * e[1]
    assert dr.rel_err(got["loss"], f64["loss"]) <= MARGIN * e[3]
    if lt == dr.URF:
        assert dr.rel_err(got["d_predicted"], f64["d_predicted"]) <= MARGIN * e[2]
    if ref is not None:
        for a, b in zip(got["d_weights"], ref["d_weights"]):
            assert dr.rel_err(a, b) <= (MARGIN + 1) * e[1]
        assert dr.rel_err(got["loss"], ref["loss"]) <= (MARGIN + 1) * e[3]
        if lt == dr.URF:
            assert dr.rel_err(got["d_predicted"], ref["d_predicted"]) <= (MARGIN + 1) * e[2]


# ---------------------------------------------------------------- fixture and float64 ---------------------------------
def test_fixture_holds_the_cases_and_its_bounds():
    g = load_golden("depth_losses")
    inp = fixture_inputs(g)
    assert tuple(g["counts"]) == dr.FIXTURE_COUNTS and inp["termination_depth"].shape == (dr.FIXTURE_RAYS,)
    again = dr.make_inputs(dr.FIXTURE_RAYS, dr.FIXTURE_COUNTS, seed=100)  # the generator's inputs are reproducible
    for k in ("termination_depth", "directions_norm", "predicted_depth"):
        np.testing.assert_array_equal(again[k], inp[k])
    np.testing.assert_array_equal(again["weights"][0], inp["weights"][0])
    td = inp["termination_depth"]
    assert (td[0::7] == 0).all() and (td > 0).sum() > 20 and not inp["weights"][1][-1].any() and td[-1] > 0
    assert td[1] * 1.1 + dr.SIGMA < inp["t_bins"][0].min() and td[2] - dr.SIGMA > inp["t_bins"][0].max()
    for tb in inp["t_bins"]:
        for tgt in (td, (td * inp["directions_norm"]).astype(np.float32)):
            assert dr.boundary_clearance(tb, tgt, dr.SIGMA).min() >= 1e-5
    keys = [dr.case_key(lt, n, euc) for lt in NAMES for n in (dr.FIXTURE_RAYS,) + dr.GPU_RAYS for euc in (True, False)]
    assert sorted(k for k in g if k.startswith("e_ref_") and not k.endswith("_measured")) == sorted(keys)
    for k in keys:  # one bound per case, each the measured figure floored at one fp32 ulp
        np.testing.assert_array_equal(g[k], np.maximum(g[k + "_measured"], 2.0 ** -23))
        assert g[k].shape == (4,) and (g[k] <= 1e-4).all()
        assert (g[k + "_measured"][2] == 0) == k.startswith("e_ref_ds")  # DS_NERF has no predicted-depth gradient


@pytest.mark.parametrize("lt,euc", COMBOS)
def test_float64_restatement_matches_autograd_and_the_reference(lt, euc):
    g = load_golden("depth_losses")
    inp = fixture_inputs(g)
    f64 = f64_of(inp, lt, euc)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    ws = [t(w).requires_grad_(True) for w in inp["weights"]]
    pred = t(inp["predicted_depth"]).requires_grad_(True)
    loss = dr.depth_loss_torch([t(b) for b in inp["t_bins"]], ws, t(inp["termination_depth"]), t(inp["directions_norm"]), pred,
                               float(inp["sigma"]), euc, lt)
    loss.backward()
    assert abs(loss.item() - f64["loss"]) <= 1e-12 * abs(f64["loss"])
    for w, d in zip(ws, f64["d_weights"]):
        np.testing.assert_allclose(w.grad.numpy(), d, rtol=1e-11, atol=0)
    if lt == dr.URF:
        np.testing.assert_allclose(pred.grad.numpy(), f64["d_predicted"], rtol=1e-11, atol=0)
    # the reference's fp32 arrays lie within their own recorded error of it
    ref, e = fixture_reference(g, lt, euc), case_bounds(g, inp, lt, euc)
    assert max(dr.rel_err(a, b) for a, b in zip(ref["d_weights"], f64["d_weights"])) <= e[1]
    assert dr.rel_err(ref["loss"], f64["loss"]) <= e[3]
    last = f64["d_weights"][0][-1]  # the ray without weight: order 1e7 per unit of exp * len, finite
    if lt == dr.DS_NERF:
        assert np.isfinite(last).all() and np.abs(last).max() * dr.FIXTURE_RAYS * 3 > 1e3
    assert not f64["per_ray"][:, 0].any() and not f64["d_weights"][0][0].any()


# ---------------------------------------------------------------- (a) depth_loss.h on the host ---------------------------
@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libdepthcheck.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "depth_helpers.cc")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.hc_depth_level.argtypes = [F32P, F32P, C.c_int, C.c_int64, F32P, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_float,
                                   F32P, F32P, C.c_void_p]
    return lib


def host_eval(hc, inp, lt, euc):
    n, levels = inp["termination_depth"].shape[0], len(inp["weights"])
    scale = np.float32(1.0 / (n * levels))
    per_ray, dws, dpred = np.zeros((levels, n), np.float32), [], np.zeros(n, np.float32)
    dn, pred = np.ascontiguousarray(inp["directions_norm"]), np.ascontiguousarray(inp["predicted_depth"])
    for lvl in range(levels):
        w = np.ascontiguousarray(inp["weights"][lvl])
        dw, dp, row = np.empty_like(w), np.zeros(n, np.float32), np.empty(n, np.float32)
        assert hc.hc_depth_level(np.ascontiguousarray(inp["t_bins"][lvl]), w, w.shape[1], n, inp["termination_depth"],
                                 None if euc else dn.ctypes.data, pred.ctypes.data, float(inp["sigma"]), lt, scale, row, dw,
                                 dp.ctypes.data) == 0
        per_ray[lvl] = row
        dws.append(dw)
        dpred = dpred + dp  # one equal summand per level, as the kernel adds them
    loss = np.float32(per_ray.astype(np.float64).sum() * float(scale))
    return {"per_ray": per_ray, "d_weights": dws, "d_predicted": dpred, "loss": loss}


@pytest.mark.parametrize("lt,euc", COMBOS)
def test_header_arithmetic_reproduces_the_reference_and_float64(hc, lt, euc):
    g = load_golden("depth_losses")
    inp = fixture_inputs(g)
    got = host_eval(hc, inp, lt, euc)
    check(got, inp, lt, euc, g, ref=fixture_reference(g, lt, euc))
    masked = inp["termination_depth"] == 0
    assert not got["per_ray"][:, masked].any() and not got["d_weights"][0][masked].any()
    assert np.isfinite(got["d_weights"][0]).all()


@pytest.mark.parametrize("n", dr.GPU_RAYS)
def test_header_arithmetic_at_the_gpu_parity_shapes(hc, n):
    g = load_golden("depth_losses")
    inp = dr.make_inputs(n, dr.GPU_COUNTS, seed=n)
    for lt in (dr.DS_NERF, dr.URF):
        check(host_eval(hc, inp, lt, False), inp, lt, False, g)
    assert hc.hc_depth_level(inp["t_bins"][0], inp["weights"][0], 1, n, inp["termination_depth"], None, None, 0.1, 3, 1.0,
                             np.empty(n, np.float32), np.empty((n, 1), np.float32), None) == -2


# ---------------------------------------------------------------- (b) the layers above the kernel ------------------------
class _Lib:
    def __init__(self, real, fake):
        self._real, self.nsamd_depth_loss = real, fake.nsamd_depth_loss

    def __getattr__(self, name):
        return getattr(self._real, name)


@pytest.fixture
def fake_kernel(monkeypatch):
    from nerfstudio_amd import _native as N

    fake = dr.FakeDepthLib()
    lib = _Lib(N.load(), fake)
    monkeypatch.setattr(N, "load", lambda: lib)
    monkeypatch.setattr(N, "require_cuda", lambda *a: None)
    monkeypatch.setattr(N, "stream", lambda: 0)
    return fake


def torch_inputs(inp):
    ws = [torch.from_numpy(w.copy()).requires_grad_(True) for w in inp["weights"]]
    pred = torch.from_numpy(inp["predicted_depth"].copy())[:, None].requires_grad_(True)
    return (ws, [torch.from_numpy(b) for b in inp["t_bins"]], torch.from_numpy(inp["termination_depth"])[:, None], pred,
            torch.tensor([float(inp["sigma"])]), torch.from_numpy(inp["directions_norm"])[:, None])


@pytest.mark.parametrize("lt,euc", COMBOS)
def test_functional_depth_loss_reproduces_the_reference(fake_kernel, lt, euc):
    from nerfstudio_amd import functional as F

    g = load_golden("depth_losses")
    inp = fixture_inputs(g)
    ws, bins, td, pred, sigma, dn = torch_inputs(inp)
    loss = F.depth_loss(ws, bins, td, pred, sigma, dn, euc, lt)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (2.0 * loss).backward()  # an upstream gradient other than 1
    got = {"loss": loss.item(), "d_weights": [w.grad.numpy() / 2 for w in ws],
           "d_predicted": None if pred.grad is None else pred.grad[:, 0].numpy() / 2}
    check(got, inp, lt, euc, g, ref=fixture_reference(g, lt, euc))
    call = fake_kernel.calls[-1]
    assert call["levels"] == 3 and call["accumulate"] == 0 and call["grads"] == [True] * 3
    assert call["scale"] == pytest.approx(1.0 / (3 * dr.FIXTURE_RAYS), rel=1e-7)
    assert (lt == dr.URF) == (pred.grad is not None) and (pred.grad is None or pred.grad.shape == pred.shape)
    # levels whose weights take no gradient get no buffer (the proposal levels of a step that does not update them)
    ws2 = [w.detach() for w in ws[:2]] + [ws[2].detach().requires_grad_(True)]
    F.depth_loss(ws2, bins, td, pred.detach(), sigma, dn, euc, lt).backward()
    assert fake_kernel.calls[-1]["grads"] == [False, False, True]
    np.testing.assert_array_equal(ws2[2].grad.numpy(), ws[2].grad.numpy() / 2)


def test_functional_depth_loss_rejects_what_the_kernel_does_not_cover(fake_kernel):
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.model_components.losses import DepthLossType

    inp = fixture_inputs(load_golden("depth_losses"))
    ws, bins, td, pred, sigma, dn = torch_inputs(inp)
    with pytest.raises(NotImplementedError, match="not implemented"):
        F.depth_loss(ws, bins, td, pred, sigma, dn, False, DepthLossType.SPARSENERF_RANKING)
    with pytest.raises(ValueError, match="predicted_depth"):
        F.depth_loss(ws, bins, td, None, sigma, dn, False, 2)
    with pytest.raises(ValueError, match="directions_norm"):
        F.depth_loss(ws, bins, td, pred, sigma, None, False, 1)
    assert not fake_kernel.calls
    assert [t.value for t in DepthLossType] == [1, 2, 3] and [t.name for t in DepthLossType] == ["DS_NERF", "URF",
                                                                                                  "SPARSENERF_RANKING"]


def package_samples(inp, device="cpu"):
    from nerfstudio_amd.cameras.rays import RayBundle, samples_from_bins

    n = inp["termination_depth"].shape[0]
    rb = RayBundle(origins=torch.zeros(n, 3, device=device), directions=torch.ones(n, 3, device=device),
                   pixel_area=torch.ones(n, 1, device=device))
    bins = [torch.from_numpy(b).to(device) for b in inp["t_bins"]]
    return [samples_from_bins(rb, b, b, None) for b in bins]


@pytest.mark.parametrize("lt,euc", COMBOS)
def test_losses_depth_loss_has_the_reference_signature_per_level(fake_kernel, lt, euc):
    from nerfstudio_amd.model_components import losses as L

    g = load_golden("depth_losses")
    inp = fixture_inputs(g)
    ws, _, td, pred, sigma, dn = torch_inputs(inp)
    samples = package_samples(inp)
    total = 0.0
    for w, rs in zip(ws, samples):  # the loop of models/depth_nerfacto.py:94-104
        total = total + L.depth_loss(weights=w[..., None], ray_samples=rs, termination_depth=td, predicted_depth=pred, sigma=sigma,
                                     directions_norm=dn, is_euclidean=euc, depth_loss_type=L.DepthLossType(lt)) / len(ws)
    total.backward()
    got = {"loss": total.item(), "d_weights": [w.grad.numpy() for w in ws],
           "d_predicted": None if pred.grad is None else pred.grad[:, 0].numpy()}
    check(got, inp, lt, euc, g, ref=fixture_reference(g, lt, euc))
    assert [c["levels"] for c in fake_kernel.calls] == [1, 1, 1]


def test_depth_ranking_loss_is_the_reference_formula():
    from nerfstudio_amd.model_components.losses import depth_ranking_loss

    rs = np.random.RandomState(3)
    for n in (40, 41):
        rendered = torch.from_numpy(rs.uniform(1, 3, (n, 1)).astype(np.float32)).requires_grad_(True)
        gt = torch.from_numpy(rs.uniform(1, 3, (n, 1)).astype(np.float32))
        got = depth_ranking_loss(rendered, gt)
        r, t = rendered.detach().numpy()[: n - n % 2, 0].astype(np.float64), gt.numpy()[: n - n % 2, 0].astype(np.float64)
        out = r[::2] - r[1::2] + 1e-4
        differ = np.sign(t[::2] - t[1::2]) != np.sign(out)
        assert differ.any() and float(got) == pytest.approx(np.abs(out[differ]).mean(), rel=1e-5)
        got.backward()
        assert rendered.grad.abs().sum() > 0


def _small_config(cls, **over):
    args = [{"hidden_dim": 16, "log2_hashmap_size": 8, "num_levels": 5, "max_res": r, "use_linear": False} for r in (128, 256)]
    return cls(log2_hashmap_size=10, proposal_net_args_list=args, **over)


def model_outputs(inp, samples):
    ws, _, td, pred, sigma, dn = torch_inputs(inp)
    n = td.shape[0]
    rgb = torch.full((n, 3), 0.25, requires_grad=True)
    return ws, pred, {"rgb": rgb, "accumulation": torch.ones(n, 1), "expected_depth": pred, "depth": pred.detach() * 1.01,
                      "weights_list": [w[..., None] for w in ws], "ray_samples_list": samples, "directions_norm": dn}


@pytest.mark.parametrize("lt,euc", COMBOS)
def test_depth_nerfacto_model_reports_the_reference_loss_entries(fake_kernel, monkeypatch, lt, euc):
    import cpu_kernels
    from nerfstudio_amd.depth_nerfacto import DepthNerfactoModel, DepthNerfactoModelConfig
    from nerfstudio_amd.model_components.losses import DepthLossType

    g = load_golden("depth_losses")
    inp = fixture_inputs(g)
    cfg = _small_config(DepthNerfactoModelConfig, depth_loss_type=DepthLossType(lt), is_euclidean_depth=euc,
                        depth_sigma=float(inp["sigma"]))
    assert (cfg.depth_loss_mult, cfg.should_decay_sigma, cfg.starting_depth_sigma, cfg.sigma_decay_rate) == (1e-3, False, 0.2, 0.99985)
    assert DepthNerfactoModelConfig().depth_sigma == 0.01 and DepthNerfactoModelConfig().depth_loss_type is DepthLossType.DS_NERF
    assert not DepthNerfactoModelConfig().is_euclidean_depth
    model = DepthNerfactoModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4).train()
    ws, pred, out = model_outputs(inp, package_samples(inp))
    batch = {"image": torch.full((dr.FIXTURE_RAYS, 3), 0.5), "depth_image": torch.from_numpy(inp["termination_depth"])[:, None]}
    with cpu_kernels.installed(monkeypatch):
        metrics = model.get_metrics_dict(out, batch)
        losses = model.get_loss_dict(out, batch, metrics)
    assert {"rgb_loss", "interlevel_loss", "distortion_loss", "depth_loss"} == set(losses) and "depth_ranking" not in metrics
    assert float(losses["depth_loss"]) == pytest.approx(1e-3 * float(metrics["depth_loss"]), rel=1e-6)
    ws_grads = torch.autograd.grad(metrics["depth_loss"], ws + ([pred] if lt == dr.URF else []))
    got = {"loss": metrics["depth_loss"].item(), "d_weights": [x.numpy() for x in ws_grads[:3]],
           "d_predicted": ws_grads[3][:, 0].numpy() if lt == dr.URF else None}
    check(got, inp, lt, euc, g, ref=fixture_reference(g, lt, euc))
    assert fake_kernel.calls[-1]["levels"] == 3  # every level in ONE launch
    # eval mode: no depth terms; image metrics: depth_mse over the supervised pixels
    model.eval()
    with cpu_kernels.installed(monkeypatch):
        assert "depth_loss" not in model.get_metrics_dict(out, batch)
    m, _ = model.get_image_metrics_and_images(out, batch)
    gt = batch["depth_image"] if euc else batch["depth_image"] * out["directions_norm"]
    keep = gt > 0
    assert m["depth_mse"] == pytest.approx(float(((out["depth"][keep] - gt[keep]) ** 2).mean()), rel=1e-6)


def test_depth_nerfacto_model_sigma_decay_outputs_and_ranking(fake_kernel, monkeypatch):
    import cpu_kernels
    from nerfstudio_amd.cameras.rays import RayBundle
    from nerfstudio_amd.depth_nerfacto import DepthNerfactoModel, DepthNerfactoModelConfig
    from nerfstudio_amd.model_components.losses import DepthLossType
    from nerfstudio_amd.nerfacto import NerfactoModel

    box = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    model = DepthNerfactoModel(_small_config(DepthNerfactoModelConfig, should_decay_sigma=True, sigma_decay_rate=0.5), box, 4)
    assert float(model.depth_sigma) == pytest.approx(0.2)
    sig = [float(model._get_sigma()) for _ in range(6)]
    assert sig[:4] == pytest.approx([0.1, 0.05, 0.025, 0.0125]) and sig[4:] == pytest.approx([0.01, 0.01])  # floor: depth_sigma
    fixed = DepthNerfactoModel(_small_config(DepthNerfactoModelConfig), box, 4)
    assert float(fixed._get_sigma()) == pytest.approx(0.01) and float(fixed._get_sigma()) == pytest.approx(0.01)
    # directions_norm travels from the bundle's metadata into the outputs (models/depth_nerfacto.py:74-78)
    dn = torch.full((5, 1), 1.05)
    monkeypatch.setattr(NerfactoModel, "get_outputs", lambda self, rb, jitters=None: {"rgb": None})
    rb = RayBundle(origins=torch.zeros(5, 3), directions=torch.ones(5, 3), pixel_area=torch.ones(5, 1), metadata={"directions_norm": dn})
    assert torch.equal(fixed.get_outputs(rb)["directions_norm"], dn)
    assert "directions_norm" not in fixed.get_outputs(RayBundle(origins=torch.zeros(5, 3), directions=torch.ones(5, 3),
                                                                pixel_area=torch.ones(5, 1)))
    monkeypatch.undo()
    # the ranking loss: `depth_ranking` in both dictionaries, ramped over the first 2000 steps (:118-123)
    inp = fixture_inputs(load_golden("depth_losses"))
    rank = DepthNerfactoModel(_small_config(DepthNerfactoModelConfig, depth_loss_type=DepthLossType.SPARSENERF_RANKING), box, 4).train()
    rank.step = 500
    _, pred, out = model_outputs(inp, package_samples(inp))
    out["expected_depth"] = pred.flip(0)  # out of order against the ground truth: some pairs rank the other way round
    batch = {"image": torch.full((dr.FIXTURE_RAYS, 3), 0.5), "depth_image": torch.from_numpy(inp["termination_depth"])[:, None]}
    with cpu_kernels.installed(monkeypatch):
        metrics = rank.get_metrics_dict(out, batch)
        losses = rank.get_loss_dict(out, batch, metrics)
    assert "depth_loss" not in losses and float(metrics["depth_ranking"]) > 0
    assert float(losses["depth_ranking"]) == pytest.approx(1e-3 * 0.05 * float(metrics["depth_ranking"]), rel=1e-6)


# ---------------------------------------------------------------- the plugin under the reference's model code -------------
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refdrive  # noqa: E402

needs_reference = pytest.mark.skipif(not refdrive.available(), reason="the reference checkout is not on this machine")


@needs_reference
@pytest.mark.parametrize("lt,euc", COMBOS)
def test_plugin_subclass_of_the_reference_depth_model_reproduces_the_reference(fake_kernel, monkeypatch, lt, euc):
    refdrive.install()
    import cpu_kernels
    from nerfstudio.data.scene_box import SceneBox
    from nerfstudio.model_components import losses as ref_losses
    from nerfstudio.models.depth_nerfacto import DepthNerfactoModel as RefDepthModel

    from nerfstudio_amd import plugin

    g = load_golden("depth_losses")
    inp = fixture_inputs(g)
    cfg_cls, model_cls = plugin._depth_model_classes()
    assert issubclass(model_cls, RefDepthModel) and issubclass(model_cls, plugin._model_classes()[1])
    cfg = _small_config(cfg_cls, depth_loss_type=ref_losses.DepthLossType(lt), is_euclidean_depth=euc, depth_sigma=float(inp["sigma"]))
    model = model_cls(config=cfg, scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]])), num_train_data=4,
                      metadata={}).train()
    assert type(model.field).__module__.startswith("nerfstudio_amd") and float(model.depth_sigma) == pytest.approx(float(inp["sigma"]))
    ws, pred, out = model_outputs(inp, package_samples(inp))
    batch = {"image": torch.full((dr.FIXTURE_RAYS, 3), 0.5), "depth_image": torch.from_numpy(inp["termination_depth"])[:, None]}
    with cpu_kernels.installed(monkeypatch):
        metrics = model.get_metrics_dict(out, batch)
        losses = model.get_loss_dict(out, batch, metrics)
        # the reference's own get_metrics_dict (torch ops, per level) on the same outputs
        ref_metrics = RefDepthModel.get_metrics_dict(model, out, batch)
    assert {"rgb_loss", "interlevel_loss", "distortion_loss", "depth_loss"} <= set(losses)
    assert float(losses["depth_loss"]) == pytest.approx(1e-3 * float(metrics["depth_loss"]), rel=1e-6)
    e = case_bounds(g, inp, lt, euc)
    assert dr.rel_err(metrics["depth_loss"].item(), ref_metrics["depth_loss"].item()) <= (MARGIN + 1) * e[3]
    wrt = ws + ([pred] if lt == dr.URF else [])
    mine, theirs = torch.autograd.grad(metrics["depth_loss"], wrt), torch.autograd.grad(ref_metrics["depth_loss"], wrt)
    for a, b in zip(mine[:3], theirs[:3]):
        assert dr.rel_err(a.numpy(), b.numpy()) <= (MARGIN + 1) * e[1]
    if lt == dr.URF:
        assert dr.rel_err(mine[3].numpy(), theirs[3].numpy()) <= (MARGIN + 1) * e[2]
    got = {"loss": metrics["depth_loss"].item(), "d_weights": [x.numpy() for x in mine[:3]],
           "d_predicted": mine[3][:, 0].numpy() if lt == dr.URF else None}
    check(got, inp, lt, euc, g, ref=fixture_reference(g, lt, euc))


@needs_reference
def test_depth_method_is_discovered_through_the_environment_and_survives_pickle_and_yaml(monkeypatch):
    refdrive.install()
    import pickle

    import tomli
    import yaml
    from nerfstudio.models.depth_nerfacto import DepthNerfactoModel as RefDepthModel
    from nerfstudio.plugins import registry
    from nerfstudio.plugins.types import MethodSpecification

    from nerfstudio_amd import plugin

    class _NoEntryPoints:
        names = set()

    monkeypatch.setattr(registry, "entry_points", lambda group: _NoEntryPoints())
    monkeypatch.setenv("NERFSTUDIO_METHOD_CONFIGS", "depth-nerfacto-hip=nerfstudio_amd.plugin:depth_nerfacto_hip")
    methods, descriptions = registry.discover_methods()
    assert set(methods) == {"depth-nerfacto-hip"} and "depth" in descriptions["depth-nerfacto-hip"]
    spec = plugin.depth_nerfacto_hip()
    assert isinstance(spec, MethodSpecification)
    cfg = methods["depth-nerfacto-hip"]
    assert cfg.method_name == "depth-nerfacto-hip" and cfg.mixed_precision is False
    assert issubclass(cfg.pipeline.model._target, RefDepthModel) and cfg.pipeline.model.implementation == "hip"
    assert cfg.pipeline.model.depth_loss_mult == 1e-3 and cfg.pipeline.model.eval_num_rays_per_chunk == 1 << 15
    assert set(cfg.optimizers) == {"proposal_networks", "fields", "camera_opt"} and cfg.optimizers["fields"]["scheduler"] is None
    # not an entry point: pyproject.toml declares the two methods it declared before
    declared = tomli.load(open(os.path.join(ROOT, "pyproject.toml"), "rb"))["project"]["entry-points"]["nerfstudio.method_configs"]
    assert set(declared) == {"nerfacto-hip", "instant-ngp-hip"}
    model_cfg = spec.config.pipeline.model
    again = pickle.loads(pickle.dumps(model_cfg))
    assert type(again) is type(model_cfg) and again._target is model_cfg._target and again.depth_loss_type == model_cfg.depth_loss_type
    loaded = yaml.load(yaml.dump(model_cfg), Loader=yaml.Loader)
    assert type(loaded) is type(model_cfg) and loaded._target is model_cfg._target and loaded.depth_sigma == model_cfg.depth_sigma


# ---------------------------------------------------------------- (d) what is declined where -----------------------------
def test_unsupported_model_reason_names_depth_supervision():
    from nerfstudio_amd.depth_nerfacto import DepthNerfactoModelConfig
    from nerfstudio_amd.fused_step import FusedTrainStep
    from nerfstudio_amd.model_components.losses import DepthLossType
    from nerfstudio_amd.nerfacto import NerfactoModelConfig
    from nerfstudio_amd.pipeline import unsupported_model_reason
    from nerfstudio_amd.trainer import HipTrainer

    m = lambda cfg: types.SimpleNamespace(config=cfg)  # noqa: E731
    assert unsupported_model_reason(m(DepthNerfactoModelConfig())) == "depth supervision"
    assert unsupported_model_reason(m(DepthNerfactoModelConfig(depth_loss_type=DepthLossType.URF))) == "depth supervision"
    assert unsupported_model_reason(m(DepthNerfactoModelConfig(predict_normals=True))) == "predict_normals"
    assert unsupported_model_reason(m(NerfactoModelConfig())) is None
    assert unsupported_model_reason(m(NerfactoModelConfig(predict_normals=True))) == "predict_normals"
    assert unsupported_model_reason(m(NerfactoModelConfig(use_gradient_scaling=True, use_single_jitter=False))) is None
    with pytest.raises(NotImplementedError, match="module path"):
        HipTrainer(m(DepthNerfactoModelConfig()), None, None, None)
    # the explicit schedule behind the Model API: DS_NERF yes, the others stay on the module path
    assert FusedTrainStep(m(DepthNerfactoModelConfig())).supported() is None
    assert FusedTrainStep(m(DepthNerfactoModelConfig())).loss_keys()[-1] == "depth_loss"
    assert FusedTrainStep(m(NerfactoModelConfig())).loss_keys() == ("rgb_loss", "interlevel_loss", "distortion_loss")
    assert "URF" in FusedTrainStep(m(DepthNerfactoModelConfig(depth_loss_type=DepthLossType.URF))).supported()
    assert "SPARSENERF_RANKING" in FusedTrainStep(m(DepthNerfactoModelConfig(depth_loss_type=DepthLossType.SPARSENERF_RANKING))).supported()


def test_set_depth_target_declines_everything_but_ds_nerf():
    from nerfstudio_amd.train_step import NerfactoTrainStep

    step = object.__new__(NerfactoTrainStep)
    step.depth, step._depth_buffers = None, None
    for kind in (2, 3):
        with pytest.raises(NotImplementedError, match="module path"):
            step.set_depth_target(torch.ones(4), torch.ones(4), loss_type=kind)
    with pytest.raises(ValueError, match="directions_norm"):
        step.set_depth_target(torch.ones(4), None)
    step.set_depth_target(None)
    assert step.depth is None


# ---------------------------------------------------------------- (e) the entry point validates before launching ----------
def test_depth_entry_point_validates_before_launching():
    from nerfstudio_amd import _native as N

    lib = N.load()
    one = (C.c_void_p * 1)(None)
    nine = (C.c_void_p * 9)(*([None] * 9))

    def call(levels, S, n, loss_type=1, arrays=one):
        counts = (C.c_int32 * len(S))(*S)
        return lib.nsamd_depth_loss(levels, arrays, arrays, counts, n, None, None, None, 0.01, loss_type, 1.0, 0, None, None, None,
                                    None)

    assert call(1, [8], 0) == 0                                  # n = 0 is a no-op
    assert call(1, [8], 5) == -1                                 # null buffers: invalid argument, nothing launched
    assert call(1, [8], -1) == -1 and call(0, [8], 5) == -1
    assert lib.nsamd_depth_loss(1, None, None, None, 5, None, None, None, 0.01, 1, 1.0, 0, None, None, None, None) == -1
    for t in (0, 3, 4, -1):                                      # loss types the kernel does not cover
        assert call(1, [8], 5, loss_type=t) == N.ERR_UNSUPPORTED and call(1, [8], 0, loss_type=t) == N.ERR_UNSUPPORTED
    for s in (0, -3, 4097):                                      # sample counts outside what the launch covers
        assert call(1, [s], 5) == N.ERR_UNSUPPORTED
    assert call(1, [4096], 0) == 0 and call(1, [1], 0) == 0
    assert call(9, [8] * 9, 5, arrays=nine) == N.ERR_UNSUPPORTED  # more levels than the launch covers
    assert call(8, [8] * 8, 0, arrays=nine) == 0
