"""forward_step.NerfactoForward against train_step.NerfactoTrainStep, its subclass, on one model and the same rays: the eval forward
as eval_render.EvalRenderer issues it — forward_proposals(stratified=False), forward_main(app_const=row), weights, compositing
with the clamp — leaves the same BITS in every buffer the two share, whether the schedule owns the training buffers or not.

Shapes, each the smallest at which the paths differ (proposal samples (8, 8)):
  32 rays x 16 main samples   the ray terms are on, whole 16-point tiles
  31 rays x 24 main samples   the ray terms are off; 744 points, so the last 16-point tile is partial
and one EvalRenderer.render of the 31-ray bundle through its captured chunk, replayed twice."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PROP = (8, 8)


def _model(main_samples):
    from nerfstudio_amd.cameras.camera_optimizers import CameraOptimizerConfig
    from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig

    torch.manual_seed(5)
    cfg = NerfactoModelConfig(log2_hashmap_size=10, num_proposal_samples_per_ray=PROP, num_nerf_samples_per_ray=main_samples,
                              camera_optimizer=CameraOptimizerConfig(mode="off"),
                              proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 8, "num_levels": 5, "max_res": r,
                                                       "use_linear": False} for r in (128, 256)])
    model = NerfactoModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 7)
    with torch.no_grad():  # tables that make the densities differ from sample to sample
        for net in (model.field.mlp_base, *model.proposal_networks):
            net.encoding.hash_table.normal_(0.0, 0.4)
    model.proposal_sampler.set_anneal(0.37)
    return model.cuda().eval()


def _rays(n):
    g = torch.Generator().manual_seed(n)
    o = torch.rand((n, 3), generator=g) - 0.5
    d = torch.nn.functional.normalize(torch.randn((n, 3), generator=g), dim=-1)
    return o.cuda(), d.cuda()


def _eval_forward(step, proposals, o, d, anneal, row):
    """The launches of EvalRenderer._launch_chunk on `step`'s buffers -> {name: int32 view of the buffer's bits}."""
    from nerfstudio_amd import functional as F

    step.nears.zero_()
    step.anneal_dev.fill_(anneal)
    step.origins.copy_(o)
    step.directions.copy_(d)
    proposals(step)
    step.forward_main(app_const=row)
    L = step.n_prop
    F.weights_launch(step.t_bins[L], step.f_dens, step.weights[L])
    F.composite_launch(step.f_rgb, step.weights[L], step.t_bins[L], step.bg_mode, step.bg_vals, True, step.rgb, step.acc,
                       step.depth_exp, step.depth_med[L], None, step.minmax_ws)
    torch.cuda.synchronize()
    out = {}
    for name in ("p_dens", "t_bins", "weights", "f_dens", "f_rgb", "rgb", "acc", "depth_med"):
        value = getattr(step, name)
        for i, t in enumerate(value) if isinstance(value, list) else [("", value)]:
            out[f"{name}{i}"] = t.clone().view(torch.int32)
    return out


@pytest.mark.parametrize("num_rays,main_samples,ray_terms", [(32, 16, True), (31, 24, False)])
def test_eval_forward_bits_do_not_depend_on_the_training_buffers(num_rays, main_samples, ray_terms):
    from nerfstudio_amd.cameras.rays import RayBundle
    from nerfstudio_amd.eval_render import EvalRenderer
    from nerfstudio_amd.forward_step import NerfactoForward
    from nerfstudio_amd.train_step import NerfactoTrainStep

    model = _model(main_samples)
    o, d = _rays(num_rays)
    renderer = EvalRenderer(model, chunk=num_rays, use_graph=True)
    renderer._refresh_constants()
    anneal, row = float(model.proposal_sampler._anneal), renderer.app_const
    assert row is not None and row.shape == (32,)
    forward = NerfactoForward(model, num_rays, torch.device("cuda"))
    train = NerfactoTrainStep(model, num_rays, torch.device("cuda"))
    assert forward.ray_terms_on is ray_terms and train.ray_terms_on is ray_terms and forward.m_main % 16 == (0 if ray_terms else 8)
    assert forward.saved_hb is None and forward.ray_inputs is None and train.saved_hb is not None
    a = _eval_forward(forward, lambda s: s.forward_proposals(stratified=False), o, d, anneal, row)
    b = _eval_forward(train, lambda s: s.forward_proposals(need_enc=False, stratified=False), o, d, anneal, row)
    assert a.keys() == b.keys() and len(a) == 2 + 3 + 3 + 4 + 3
    for name in a:
        assert torch.equal(a[name], b[name]), name
    rgb = forward.rgb
    assert bool(torch.isfinite(rgb).all()) and float(rgb.std()) > 0 and float(forward.f_dens.std()) > 0  # (not a trivial image)
    assert all(x is None for x in (*forward.p_enc, *forward.p_sel, *forward.p_pre))  # the fused forward kept nothing
    if num_rays == 31:
        # the renderer's captured chunk: the capture pass and a replay, then a replay alone — the same bits, and the schedule's
        rb = RayBundle(origins=o, directions=d, pixel_area=torch.full((num_rays, 1), 1e-6).cuda(),
                       camera_indices=torch.zeros((num_rays, 1), dtype=torch.int64).cuda())
        first = {k: v.clone() for k, v in renderer.render(rb).items()}
        assert renderer.graph is not None and isinstance(renderer.step, NerfactoForward)
        assert not isinstance(renderer.step, NerfactoTrainStep)
        second = renderer.render(rb)
        for k in first:
            assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k
        assert torch.equal(second["rgb"].view(torch.int32), a["rgb"]) and torch.equal(second["depth"].view(torch.int32)[:, 0],
                                                                                      a["depth_med2"])
