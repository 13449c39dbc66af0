"""trainer.HipTrainer with the two schedule changes that take queue hops off a replayed iteration's critical chain
(profiles/critical_chain_hops_ab.txt), each an attribute with the shipped value on:

  HipTrainer.terms_from_pool          the ray terms on the Adam branch read the pool's rows (nsamd_field_mlp.batch_slot) instead of
                                      waiting, by an event, for the launch that selects the batch
  NerfactoTrainStep.main_chain_first  update steps issue the main backward chain before the proposal chains' fork

Neither changes a dependency or an operand, so the parameters and both Adam moments must be the same BITS with each attribute
on or off, and equal to the eager in-order run (no graphs, no deferred Adam, no side branch for the terms): 256 rays, smoke()'s
model, captured graphs, 8 iterations from step 0 (every one updates the proposal networks), then 8 with the counters of late
training (one update in five). The launches per entry point are the same in every arm (the pool form is an argument of the one
ray-terms launch), so the test also watches that launch while the graphs are captured: with the attribute on, the two variants
with a pending Adam — and only those — pass the pool's slot."""
import hashlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import trainer_arrangements as A  # noqa: E402

pytestmark = pytest.mark.gpu

N_RAYS, SLOTS = 256, 3


def _pool():
    from nerfstudio_amd.cameras.rays import RayBundle
    from oracle import nerfacto_oracle as orc

    parts = [orc.synthetic_rays(N_RAYS, A.N_CAMERAS, seed=11 + k) for k in range(SLOTS)]
    pool = {"origins": torch.stack([p[0] for p in parts]).float().cuda(), "directions": torch.stack([p[1] for p in parts]).float().cuda(),
            "cameras": torch.stack([p[2].reshape(-1) for p in parts]).long().cuda(),
            "target": torch.stack([p[3] for p in parts]).float().cuda()}
    rb = RayBundle(origins=pool["origins"][0].clone(), directions=pool["directions"][0].clone(),
                   pixel_area=torch.full((N_RAYS, 1), 1e-6, device="cuda"), camera_indices=pool["cameras"][0].clone()[:, None])
    return rb, {"image": pool["target"][0].clone()}, pool


def _train(graph, terms_from_pool, main_chain_first):
    """-> (sha256 of the parameters and the two Adam moments after the 16 iterations, the kinds of iteration taken, for each
    ray-terms launch of the capture passes whether it was given the pool's slot)."""
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.trainer import HipTrainer

    F._SCATTER_WS.clear()
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    model = A.build_model("off")
    arena = ParamArena(model.get_param_groups_ordered(), lr=1e-2, eps=1e-15)
    rb, batch, pool = _pool()
    tr = HipTrainer(model, arena, rb, batch, world=1, use_graph=graph, use_runner=True, pool=pool)
    tr.terms_from_pool, tr.runner.main_chain_first = terms_from_pool, main_chain_first
    assert tr.slots == SLOTS and tr.runner.ray_terms_on and tr.runner.side_stream is not None
    from_pool, launch = [], F.ray_terms_launch

    def watched(*args, slot=None, slots=0):
        from_pool.append(slot is not None and slots == SLOTS)
        launch(*args, slot=slot, slots=slots)

    if graph:
        F.ray_terms_launch = watched
        try:
            assert tr.defer and tr.try_capture(warm=False)
        finally:
            F.ray_terms_launch = launch
    kinds = []
    for it in range(16):
        if it == 8:  # late training's counters: the proposal networks update on one step in five
            tr.finish()  # (a deferred main-field update belongs to step 7 and its learning rate)
            tr.step = 5000
            model.proposal_sampler._step = 5000
        kinds.append(bool(model.proposal_sampler.updated_this_step()))
        tr.train_iteration()
    tr.finish()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.last_loss()))
    digest = tuple(hashlib.sha256(x.detach().cpu().numpy().tobytes()).hexdigest() for x in (arena.flat, arena.exp_avg, arena.exp_avg_sq))
    return digest, kinds, from_pool


def test_each_attribute_on_or_off_and_the_eager_run_train_through_the_same_bits():
    shipped, kinds, from_pool = _train(True, True, True)
    assert from_pool == [True, False, True, False]  # (proposal update x pending Adam, in `capture`'s order)
    assert all(kinds[:8]) and set(kinds[8:]) == {True, False}, kinds
    for name, arm in (("terms behind the bins", (True, False, True)), ("proposal chains first", (True, True, False)),
                      ("both off", (True, False, False)), ("eager, in order", (False, True, True))):
        digest, arm_kinds, arm_from_pool = _train(*arm)
        assert arm_kinds == kinds, name
        assert arm_from_pool == ([True, False, True, False] if arm[:2] == (True, True) else [False] * 4 if arm[0] else []), name
        assert digest == shipped, (name, digest, shipped)

