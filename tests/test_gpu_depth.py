"""GPU tests of nsamd_depth_loss (csrc/losses.hip over csrc/depth_loss.h), functional.depth_loss and the depth launch of the
explicit schedule (train_step.NerfactoTrainStep.set_depth_target).

Float64 parity: entry by entry against tests/depth_reference.depth_loss_f64 at the smallest shapes at which the kernel can go
wrong — S in {1, 48, 63, 64, 65, 96, 256} as the seven levels of ONE launch (below, at and above the 64 lanes of the wave that
owns a ray), n in {1, 65, 257} (one wave of a workgroup of four, a partial last workgroup, many workgroups), masked rays, a ray
without weight, a target in front of the first sample and one behind the last. The bound per quantity is the reference's own
fp32 distance from float64 on the inputs of the very case under test (`e_ref_<type>_n<rays>_<convention>` of
tests/golden/depth_losses.npz, see tests/test_depth_cpu.py) times MARGIN = 4: the device's expf / logf and the wave's summation
order against torch's. The ratios seen on MI355X are in profiles/depth_loss_float64_ratios.txt (every test prints them before it
asserts; the largest is 1.80).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
import depth_reference as dr
from test_depth_cpu import MARGIN, NAMES, case_bounds, check, f64_of, fixture_inputs, fixture_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"


def to_dev(inp):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return {"t_bins": [t(b) for b in inp["t_bins"]], "weights": [t(w) for w in inp["weights"]],
            "termination_depth": t(inp["termination_depth"]), "directions_norm": t(inp["directions_norm"]),
            "predicted_depth": t(inp["predicted_depth"])}


def launch(d, sigma, lt, euc, scale, accumulate=False, prior=None, grads=True):
    """-> (per_ray [levels, n], d_weights, d_predicted) of one nsamd_depth_loss launch; prior: what the gradient buffers hold."""
    from nerfstudio_amd import functional as F

    levels, n = len(d["weights"]), d["termination_depth"].shape[0]
    per_ray = torch.full((levels, n), float("nan"), device=DEV)
    fresh = lambda x: torch.full_like(x, float("nan"))  # noqa: E731
    dws = None if not grads else [fresh(w) for w in d["weights"]] if prior is None else [p.clone() for p in prior[0]]
    dpred = None
    if lt == dr.URF and grads:
        dpred = fresh(d["predicted_depth"]) if prior is None else prior[1].clone()
    F.depth_loss_launch(d["weights"], d["t_bins"], d["termination_depth"], None if euc else d["directions_norm"],
                        d["predicted_depth"] if lt == dr.URF else None, float(sigma), lt, scale, per_ray, dws, dpred, accumulate)
    torch.cuda.synchronize()
    return per_ray, dws, dpred


def report(tag, got, f64, e):
    rows = [("per_ray", dr.rel_err(got["per_ray"], f64["per_ray"]), e[0]),
            ("d_weights", max(dr.rel_err(a, b) for a, b in zip(got["d_weights"], f64["d_weights"])), e[1]),
            ("loss", dr.rel_err(got["loss"], f64["loss"]), e[3])]
    if f64["d_predicted"] is not None:
        rows.append(("d_predicted", dr.rel_err(got["d_predicted"], f64["d_predicted"]), e[2]))
    for name, err, ref in rows:
        print(f"depth-ratio {tag} {name}: err {err:.3e} e_ref {ref:.3e} ratio {err / ref:.2f} (bound {MARGIN:.0f})")


# every size with z-depths; the Euclidean convention (one multiplication per ray less) at one size
PARITY = [(lt, n, False) for lt in (dr.DS_NERF, dr.URF) for n in dr.GPU_RAYS] + [(dr.DS_NERF, 65, True), (dr.URF, 65, True)]


@pytest.mark.parametrize("lt,n,euc", PARITY)
def test_entry_point_matches_float64_entry_by_entry(lt, n, euc):
    g = load_golden("depth_losses")
    inp = dr.make_inputs(n, dr.GPU_COUNTS, seed=n)
    levels = len(dr.GPU_COUNTS)
    scale = 1.0 / (n * levels)
    per_ray, dws, dpred = launch(to_dev(inp), inp["sigma"], lt, euc, scale)
    got = {"per_ray": per_ray.cpu().numpy(), "d_weights": [x.cpu().numpy() for x in dws],
           "d_predicted": None if dpred is None else dpred.cpu().numpy()}
    got["loss"] = np.float32(got["per_ray"].astype(np.float64).sum() * scale)
    report(f"{NAMES[lt]} n={n} euclidean={euc}", got, f64_of(inp, lt, euc), case_bounds(g, inp, lt, euc))
    check(got, inp, lt, euc, g)
    masked = inp["termination_depth"] == 0
    if masked.any():  # exactly zero, not merely small
        assert not got["per_ray"][:, masked].any() and all(not x[masked].any() for x in got["d_weights"])
    assert all(np.isfinite(x).all() for x in got["d_weights"])
    assert not inp["weights"][-1][-1].any() and inp["termination_depth"][-1] > 0  # the ray without weight is among them


@pytest.mark.parametrize("lt", [dr.DS_NERF, dr.URF])
def test_accumulate_adds_to_the_buffers_bit_for_bit_and_runs_repeat(lt):
    inp = dr.make_inputs(65, dr.GPU_COUNTS, seed=65)
    d = to_dev(inp)
    scale = 1e-3 / (65 * len(dr.GPU_COUNTS))
    per_ray, dws, dpred = launch(d, inp["sigma"], lt, False, scale)
    per_ray2, dws2, dpred2 = launch(d, inp["sigma"], lt, False, scale)  # the same launch again: the same bits
    assert torch.equal(per_ray, per_ray2) and all(torch.equal(a, b) for a, b in zip(dws, dws2))
    gen = torch.Generator(device=DEV).manual_seed(5)
    prior_w = [torch.randn(w.shape, device=DEV, generator=gen) * float(g.abs().mean()) for w, g in zip(d["weights"], dws)]
    prior_w[0][7, 0] = -0.0  # a signed zero in a masked ray's buffer: -0 + 0 = +0, as an addition gives
    prior_p = torch.randn(65, device=DEV, generator=gen)
    per_ray3, acc_w, acc_p = launch(d, inp["sigma"], lt, False, scale, accumulate=True, prior=(prior_w, prior_p))
    assert torch.equal(per_ray3, per_ray)
    for p, g, a in zip(prior_w, dws, acc_w):
        assert torch.equal((p + g).view(torch.int32), a.view(torch.int32))
    if lt == dr.URF:
        assert torch.equal(dpred, dpred2) and torch.equal(prior_p + dpred, acc_p)
    # value only: no gradient buffers at all, or some levels without one
    assert torch.equal(launch(d, inp["sigma"], lt, False, scale, grads=False)[0], per_ray)
    from nerfstudio_amd import functional as F

    only_last = [None] * (len(dws) - 1) + [torch.empty_like(dws[-1])]
    F.depth_loss_launch(d["weights"], d["t_bins"], d["termination_depth"], d["directions_norm"],
                        d["predicted_depth"] if lt == dr.URF else None, float(inp["sigma"]), lt, scale, None, only_last, None)
    assert torch.equal(only_last[-1], dws[-1])


@pytest.mark.parametrize("euc", [True, False])
@pytest.mark.parametrize("lt", [dr.DS_NERF, dr.URF])
def test_functional_depth_loss_under_autograd_matches_the_fixture(lt, euc):
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.model_components import losses as L

    g = load_golden("depth_losses")
    inp = fixture_inputs(g)
    d = to_dev(inp)
    ws = [w.clone().requires_grad_(True) for w in d["weights"]]
    pred = d["predicted_depth"][:, None].clone().requires_grad_(True)
    sigma = torch.tensor([float(inp["sigma"])])
    loss = F.depth_loss(ws, d["t_bins"], d["termination_depth"][:, None], pred, sigma, d["directions_norm"][:, None], euc, lt)
    assert loss.dim() == 0
    loss.backward()
    got = {"loss": loss.item(), "d_weights": [w.grad.cpu().numpy() for w in ws],
           "d_predicted": None if pred.grad is None else pred.grad[:, 0].cpu().numpy()}
    f64 = f64_of(inp, lt, euc)
    report(f"autograd {NAMES[lt]} euclidean={euc}", dict(got, per_ray=f64["per_ray"]), f64, case_bounds(g, inp, lt, euc))
    check(got, inp, lt, euc, g, ref=fixture_reference(g, lt, euc))
    # levels whose weights take no gradient get none; the value is the same bits
    ws2 = [w.detach() for w in ws[:2]] + [ws[2].detach().clone().requires_grad_(True)]
    loss2 = F.depth_loss(ws2, d["t_bins"], d["termination_depth"], pred.detach(), sigma, d["directions_norm"], euc, lt)
    loss2.backward()
    assert torch.equal(loss2, loss.detach()) and torch.equal(ws2[2].grad, ws[2].grad)
    # the reference's per-level signature sums to the same loss
    from test_depth_cpu import package_samples

    samples = package_samples(inp, DEV)
    total = sum(L.depth_loss(w.detach()[..., None], rs, d["termination_depth"][:, None], pred.detach(), sigma,
                             d["directions_norm"][:, None], euc, L.DepthLossType(lt)) for w, rs in zip(ws, samples)) / 3
    assert float(total) == pytest.approx(loss.item(), rel=1e-6)


def test_explicit_schedule_adds_the_depth_gradients_and_nothing_else():
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig
    from nerfstudio_amd.train_step import NerfactoTrainStep
    from oracle import nerfacto_oracle as orc

    torch.manual_seed(0)
    n, mult, sigma = 65, 1e-3, 0.05
    mc = NerfactoModelConfig(log2_hashmap_size=12, proposal_net_args_list=[
        {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": r, "use_linear": False} for r in (128, 256)])
    model = NerfactoModel(mc, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4).cuda().train()
    step = NerfactoTrainStep(model, n, torch.device(DEV))
    o, dirs, cam, tgt = orc.synthetic_rays(n, 4, seed=2)
    step.set_batch(o.cuda(), dirs.cuda(), cam.cuda(), tgt.cuda())
    step.apply_camera_corrections()
    step.forward_proposals(draw_jitter=True, need_enc=True)
    step.forward_main()
    keep = lambda: {"dw_dist": step.dw_dist.clone(), "dw_prop": [x.clone() for x in step.dw_prop], "rgb": step.rgb.clone(),  # noqa: E731
                    "weights": [w.clone() for w in step.weights], "sq_err": step.sq_err.clone(),
                    "dist": step.dist_per_ray.clone(), "inter": [x.clone() for x in step.inter_per_ray],
                    "losses": {k: v.clone() for k, v in step.loss_dict().items()}}
    step.losses(True)
    base = keep()
    assert set(base["losses"]) == {"rgb_loss", "interlevel_loss", "distortion_loss"}
    td = (step.depth_exp.clone() * 0.9)
    td[0] = 0.0  # a masked ray
    dn = torch.full((n,), 1.05, device=DEV)
    levels = len(step.counts)
    scale = mult / (n * levels)
    per_ray = torch.empty(levels, n, device=DEV)
    alone = [torch.empty_like(w) for w in step.weights]
    F.depth_loss_launch(step.weights, step.t_bins, td, dn, None, sigma, 1, scale, per_ray, alone, None)
    assert all(float(a.abs().max()) > 0 for a in alone)
    step.set_depth_target(td[:, None], dn[:, None], sigma=sigma, mult=mult, is_euclidean=False)
    step.losses(True)
    with_depth = keep()
    # the gradients differ by exactly what the standalone launch writes: one fp32 addition per entry, in the kernel's order
    assert torch.equal(with_depth["dw_dist"], base["dw_dist"] + alone[-1])
    for lvl in range(step.n_prop):
        assert torch.equal(with_depth["dw_prop"][lvl], base["dw_prop"][lvl] + alone[lvl])
    assert torch.equal(with_depth["rgb"], base["rgb"]) and torch.equal(with_depth["sq_err"], base["sq_err"])
    assert torch.equal(with_depth["dist"], base["dist"])
    assert all(torch.equal(a, b) for a, b in zip(with_depth["weights"], base["weights"]))
    assert all(torch.equal(a, b) for a, b in zip(with_depth["inter"], base["inter"]))
    for k in ("rgb_loss", "interlevel_loss", "distortion_loss"):
        assert torch.equal(with_depth["losses"][k], base["losses"][k])
    value = F.depth_loss(step.weights, step.t_bins, td, None, sigma, dn, False, 1)
    assert float(with_depth["losses"]["depth_loss"]) == pytest.approx(mult * float(value), rel=1e-5)
    assert float(value) > 0 and torch.equal(step.depth["per_ray"], per_ray)
    # a step that does not update the proposal networks: their weights carry no gradient, dw_prop is untouched
    for x in step.dw_prop:
        x.fill_(-7.0)
    step.losses(False)
    assert all(bool((x == -7.0).all()) for x in step.dw_prop)
    assert torch.equal(step.dw_dist, base["dw_dist"] + alone[-1])
    # no target again: today's launches, today's bits
    step.set_depth_target(None)
    step.losses(True)
    again = keep()
    assert torch.equal(again["dw_dist"], base["dw_dist"]) and "depth_loss" not in again["losses"]
    assert all(torch.equal(a, b) for a, b in zip(again["dw_prop"], base["dw_prop"]))
    # what the schedule does not cover is declined, not approximated
    with pytest.raises(NotImplementedError, match="module path"):
        step.set_depth_target(td, dn, loss_type=2)


def test_fused_train_step_of_a_depth_model_matches_the_module_path():
    """DepthNerfactoModel(fused_train_step=True) driven as a trainer drives a model — get_outputs -> get_metrics_dict ->
    get_loss_dict -> sum(losses).backward() — against the same model on the module path: four loss terms, `directions_norm`
    from the bundle's metadata, sigma decayed once per iteration, the depth gradients in the main and the proposal tables."""
    import functools

    from nerfstudio_amd.cameras.rays import RayBundle
    from nerfstudio_amd.depth_nerfacto import DepthNerfactoModel, DepthNerfactoModelConfig
    from oracle import nerfacto_oracle as orc

    n = 65
    args = [{"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": r, "use_linear": False} for r in (128, 256)]

    def build(fused):
        torch.manual_seed(4)
        cfg = DepthNerfactoModelConfig(log2_hashmap_size=12, proposal_net_args_list=args, depth_loss_mult=0.05,
                                       should_decay_sigma=True, starting_depth_sigma=0.4, depth_sigma=0.05, sigma_decay_rate=0.5,
                                       fused_train_step=fused)
        m = DepthNerfactoModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4).cuda().train()
        m.set_step(137)
        return m

    ma, mb = build(False), build(True)
    mb.load_state_dict(ma.state_dict())
    o, d, cam, tgt = orc.synthetic_rays(n, 4, seed=9)
    rs = np.random.RandomState(2)
    jit = torch.from_numpy(rs.uniform(0, 1, (3, n)).astype(np.float32)).cuda()
    depth = torch.from_numpy(rs.uniform(0.5, 2.5, (n, 1)).astype(np.float32)).cuda()
    depth[::9] = 0.0  # pixels without a depth
    dn = torch.from_numpy(rs.uniform(1.0, 1.1, (n, 1)).astype(np.float32)).cuda()
    batch = {"image": tgt.cuda(), "depth_image": depth}

    def iteration(m):
        rb = RayBundle(origins=o.cuda(), directions=d.cuda(), pixel_area=torch.full((n, 1), 1e-6).cuda(),
                       camera_indices=cam.cuda()[:, None], metadata={"directions_norm": dn})
        out = m(rb, jitters=[jit[i][:, None] for i in range(3)])
        metrics = m.get_metrics_dict(out, batch)
        losses = m.get_loss_dict(out, batch, metrics)
        functools.reduce(torch.add, losses.values()).backward()  # engine/trainer.py:514
        return out, losses

    for it in range(2):  # sigma 0.2, then 0.1: decayed once per iteration on both paths
        for m in (ma, mb):
            m.zero_grad(set_to_none=True)
        out_a, ld_a = iteration(ma)
        out_b, ld_b = iteration(mb)
        assert "fused_step" in out_b and "fused_step" not in out_a and torch.equal(out_b["directions_norm"], dn)
        assert set(ld_a) == set(ld_b) == {"rgb_loss", "interlevel_loss", "distortion_loss", "depth_loss"}
        assert float(ma.depth_sigma) == pytest.approx(0.4 * 0.5 ** (it + 1)) == float(mb.depth_sigma)
        for k in ld_a:
            print(f"fused-depth it={it} {k}: module {float(ld_a[k]):.8e} fused {float(ld_b[k]):.8e}")
            assert float(ld_b[k]) == pytest.approx(float(ld_a[k]), rel=1e-5, abs=1e-9), k
        assert float(ld_a["depth_loss"]) > 0
        pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
        for k in ("field.mlp_base.model.0.hash_table", "proposal_networks.0.encoding.hash_table"):
            ga, gb = pa[k].grad, pb[k].grad
            assert (ga is None) == (gb is None), k
            if ga is not None:
                rel = float((gb.double() - ga.double()).norm() / ga.double().norm())
                print(f"fused-depth it={it} {k}: relative L2 distance of the gradients {rel:.3e}")
                assert rel <= 2e-5 and float(ga.abs().max()) > 0, k
    # the depth term reaches the gradients: without it the main table's gradient is another one
    with_depth = pb["field.mlp_base.model.0.hash_table"].grad.clone()
    mb.zero_grad(set_to_none=True)
    mb.config.depth_loss_mult = 0.0
    iteration(mb)
    assert not torch.equal(pb["field.mlp_base.model.0.hash_table"].grad, with_depth)
