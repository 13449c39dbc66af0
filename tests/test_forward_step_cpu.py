"""forward_step.NerfactoForward on the CPU (no kernels): the schedule an eval render builds owns exactly the forward's buffers at
their full sizes — no one-element stand-in a kernel could write past —, nothing of the training runner's, and cannot be asked to
keep the proposal levels' features it has no buffers for."""
import inspect

import pytest
import torch

from nerfstudio_amd import _native as N
from nerfstudio_amd.forward_step import NerfactoForward
from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig
from nerfstudio_amd.train_step import NerfactoTrainStep

RAYS, PROP, MAIN = 32, (8, 8), 16
M = RAYS * MAIN

# every tensor the object holds (lists by index), and the buffers it states it does not have
BUFFERS = {
    "origins": (RAYS, 3), "directions": (RAYS, 3), "camera_indices": (RAYS,), "nears": (RAYS,), "fars": (RAYS,),
    "jitter": (len(PROP) + 1, RAYS), "jitter_edges": None, "anneal_dev": (1,), "edges": (PROP[0] + 1,),
    "u_base.0": None, "u_base.1": (PROP[1] + 1,), "u_base.2": (MAIN + 1,),
    "s_bins.0": (RAYS, 9), "s_bins.1": (RAYS, 9), "s_bins.2": (RAYS, 17),
    "t_bins.0": (RAYS, 9), "t_bins.1": (RAYS, 9), "t_bins.2": (RAYS, 17),
    "weights.0": (RAYS, 8), "weights.1": (RAYS, 8), "weights.2": (RAYS, 16),
    "p_enc.0": None, "p_enc.1": None, "p_sel.0": None, "p_sel.1": None, "p_pre.0": None, "p_pre.1": None,
    "p_dens.0": (RAYS * 8,), "p_dens.1": (RAYS * 8,),
    "f_enc": (32, M), "f_sel": (M,), "f_dens": (M,), "f_rgb": (M, 3),
    "rgb": (RAYS, 3), "acc": (RAYS,), "depth_exp": (RAYS,), "minmax_ws": (2 + 2 * (RAYS // 4),),
    "depth_med.0": (RAYS,), "depth_med.1": (RAYS,), "depth_med.2": (RAYS,),
    "ray_terms": (RAYS, 64), "bg_vals": None,  # (16 samples per ray: whole tiles, the ray terms are on; "last_sample": no colour)
}
TRAINING_ONLY = ("dw_dist", "dw_prop", "d_rgb_s", "d_dens_main", "f_denc", "p_ddens", "p_denc", "field_ws", "density_ws",
                 "prop_gates", "prop_ray_masks", "side_stream", "reduce_stream", "target", "loss_vals", "cam_opt", "normals", "depth")


@pytest.fixture(scope="module")
def forward():
    cfg = NerfactoModelConfig(log2_hashmap_size=8, num_proposal_samples_per_ray=PROP, num_nerf_samples_per_ray=MAIN,
                              proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 7, "num_levels": 5, "max_res": r,
                                                       "use_linear": False} for r in (32, 64)])
    model = NerfactoModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 7).eval()
    return NerfactoForward(model, RAYS, "cpu")


def test_forward_owns_exactly_its_buffers_at_full_size(forward):
    found = {}
    for name, value in vars(forward).items():
        items = {f"{name}.{i}": v for i, v in enumerate(value)} if isinstance(value, list) else {name: value}
        found.update({k: None if v is None else tuple(v.shape) for k, v in items.items()
                      if v is None or isinstance(v, torch.Tensor)})
    assert found == BUFFERS
    for name in ("bg_rays", "ray_inputs", "saved_hb"):  # read by the shared forward; only the training runner allocates them
        assert getattr(forward, name) is None, name


def test_forward_carries_nothing_of_the_training_runner(forward):
    for name in TRAINING_ONLY:
        assert not hasattr(forward, name) and not hasattr(NerfactoForward, name), name
    assert isinstance(NerfactoTrainStep.__mro__[1], type) and NerfactoTrainStep.__mro__[1] is NerfactoForward


def test_forward_refuses_to_keep_proposal_features_before_any_launch(forward, monkeypatch):
    def no_launch():
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(N, "load", no_launch)
    assert "need_enc" not in inspect.signature(NerfactoForward.forward_proposals).parameters
    with pytest.raises(TypeError):
        forward.forward_proposals(need_enc=True)
    with pytest.raises(RuntimeError, match="no buffers to keep"):
        forward._proposals(False, True, None, False)
    forward.ensure_proposal_features(0)  # the two-kernel pair's buffers of one level: still no pre-activation to keep
    assert forward.p_enc[0].shape == (10, RAYS * 8) and forward.p_sel[0].shape == (RAYS * 8,) and forward.p_pre[0] is None
    with pytest.raises(RuntimeError, match="no buffers to keep"):
        forward._proposals(False, True, None, False)
    forward.p_enc[0] = forward.p_sel[0] = None
