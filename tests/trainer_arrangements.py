"""The arrangements of trainer.HipTrainer whose launches tests/test_gpu_trainer_launch_counts.py counts — TEST INFRASTRUCTURE shared
with tests/golden/make_trainer_launch_counts.py, which wrote tests/golden/trainer_launch_counts.json from the commit BEFORE the runner
interface was stated (the table is a record of that schedule; it is not regenerated from later code).

Sizes are smoke()'s: 16 rays, (256, 96, 48) samples, tables of 2^12 (main) and 2^10 (proposal) rows, 4 cameras. Every arrangement runs
one proposal-update and one other iteration uncounted (lazily built workspaces), then — where `captured` — captures its graphs with
the launches of each variant's capture pass counted, then one counted update iteration and one counted other iteration."""
from collections import Counter

import numpy as np
import torch

N_RAYS, N_CAMERAS, POOL_SLOTS = 16, 4, 2

# name -> (camera optimiser mode, NSAMD_CAMERAS_OUTSIDE, HipTrainer keywords, batches from, capture graphs)
ARRANGEMENTS = {
    "eager":          ("off", "0", dict(use_graph=False), "pool", False),
    "captured":       ("off", "0", dict(use_graph=True), "pool", True),
    "camera_inside":  ("SO3xR3", "0", dict(use_graph=True), "pool", True),
    "camera_outside": ("SO3xR3", "1", dict(use_graph=True), "pool", True),
    "force_dp":       ("off", "0", dict(use_graph=True, force_dp=True, dp_mode="allreduce"), "pool", False),
    "source":         ("off", "0", dict(use_graph=True), "source", True),
}


def build_model(camera):
    from nerfstudio_amd.cameras.camera_optimizers import CameraOptimizerConfig
    from nerfstudio_amd.nerfacto import NerfactoModel, NerfactoModelConfig

    torch.manual_seed(0)
    mc = NerfactoModelConfig(log2_hashmap_size=12, camera_optimizer=CameraOptimizerConfig(mode=camera), proposal_net_args_list=[
        {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": r, "use_linear": False} for r in (128, 256)])
    return NerfactoModel(mc, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), N_CAMERAS).cuda().train()


def build_pool():
    """-> (RayBundle of slot 0, {"image": ...}, pool) as bench.synthetic_batch lays them out."""
    from nerfstudio_amd.cameras.rays import RayBundle
    from oracle import nerfacto_oracle as orc

    parts = [orc.synthetic_rays(N_RAYS, N_CAMERAS, seed=1 + k) for k in range(POOL_SLOTS)]
    pool = {"origins": torch.stack([p[0] for p in parts]).float().cuda(), "directions": torch.stack([p[1] for p in parts]).float().cuda(),
            "cameras": torch.stack([p[2].reshape(-1) for p in parts]).long().cuda(),
            "target": torch.stack([p[3] for p in parts]).float().cuda()}
    rb = RayBundle(origins=pool["origins"][0].clone(), directions=pool["directions"][0].clone(),
                   pixel_area=torch.full((N_RAYS, 1), 1e-6, device="cuda"), camera_indices=pool["cameras"][0].clone()[:, None])
    return rb, {"image": pool["target"][0].clone()}, pool


def build_source():
    """A device_batches.DeviceBatchSource over 4 perspective cameras of 8 x 8 random pixels on a shell around the box."""
    from nerfstudio_amd.device_batches import DeviceBatchSource, DeviceImageStore

    rs = np.random.RandomState(7)
    images = torch.from_numpy(rs.randint(0, 256, size=(N_CAMERAS, 8, 8, 3)).astype(np.uint8)).cuda()
    pos = rs.standard_normal((N_CAMERAS, 3))
    back = pos / np.linalg.norm(pos, axis=-1, keepdims=True)
    right = np.cross(np.array([0.0, 0.0, 1.0]) + 0.01 * rs.standard_normal((N_CAMERAS, 3)), back)
    right /= np.linalg.norm(right, axis=-1, keepdims=True)
    c2w = torch.from_numpy(np.concatenate([np.stack([right, np.cross(back, right), back], -1), 2.5 * back[..., None]], -1).astype(np.float32))
    focal = torch.full((N_CAMERAS,), 9.0)
    store = DeviceImageStore(images, None, c2w, focal, focal, torch.full((N_CAMERAS,), 4.25), torch.full((N_CAMERAS,), 3.75),
                             torch.ones(N_CAMERAS, dtype=torch.int64), torch.zeros(N_CAMERAS, 6))
    return DeviceBatchSource(store, N_RAYS, seed=99)


def build_trainer(name, setenv):
    """`setenv(key, value)` sets an environment variable for the construction (the caller restores it: monkeypatch.setenv)."""
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.trainer import HipTrainer

    camera, outside, kw, batches, _ = ARRANGEMENTS[name]
    setenv("NSAMD_CAMERAS_OUTSIDE", outside)
    F._SCATTER_WS.clear()
    model = build_model(camera)
    arena = ParamArena(model.get_param_groups_ordered(), lr=1e-2, eps=1e-15)
    if batches == "source":
        src = build_source()
        rb, batch = src.next_batch(advance=False)
        return HipTrainer(model, arena, rb, batch, world=1, use_runner=True, source=src, **kw)
    rb, batch, pool = build_pool()
    return HipTrainer(model, arena, rb, batch, world=1, use_runner=True, pool=pool, **kw)


def plan_inputs(name):
    """The arrangement as trainer.plan_schedule's keyword arguments other than `runner` (what `build_trainer` constructs)."""
    camera, outside, kw, batches, _ = ARRANGEMENTS[name]
    return dict(own_runner=True, world=1, force_dp=kw.get("force_dp", False), dp_mode=kw.get("dp_mode", "allreduce"),
                use_graph=kw["use_graph"], on_gpu=True, cam_group=camera != "off", has_source=batches == "source",
                cameras_outside_switch=outside == "1", defer_switch=None)


def count_launches(setattr_fn):
    """Wrap every kernel entry point of the loaded library (`setattr_fn(lib, name, wrapper)`: monkeypatch.setattr) -> the Counter
    the wrappers add to. N.PROFILE is not used: it changes the schedule."""
    from nerfstudio_amd import _native as N

    lib, counts = N.load(), Counter()

    def wrap(name, fn):
        def call(*args):
            counts[name] += 1
            return fn(*args)
        return call

    for name, fn in list(vars(lib).items()):
        if name.startswith("nsamd_") and isinstance(fn, N._Entry):
            setattr_fn(lib, name, wrap(name, fn))
    return counts


def record(name, counts, setenv, setattr_fn):
    """-> (trainer, {"update": {entry: launches}, "other": {...}[, "capture": {"<updated>,<pending>": {...}}]}) of arrangement
    `name`; `counts`: count_launches' Counter. The trainer is finished and the device idle on return."""
    from nerfstudio_amd import functional as F

    direct, F.DIRECT_GRAD = F.DIRECT_GRAD, True
    try:
        tr = build_trainer(name, setenv)
        ps = tr.model.proposal_sampler
        forced = [True]
        setattr_fn(ps, "updated_this_step", lambda: forced[0])

        def iteration(updated):
            forced[0] = updated
            counts.clear()
            tr.train_iteration()
            return dict(sorted(counts.items()))

        iteration(True), iteration(False)
        out = {}
        if ARRANGEMENTS[name][4]:
            passes, body = {}, tr._body

            def counted_body(updated, pending):
                counts.clear()
                body(updated, pending)
                passes[f"{int(updated)},{int(pending)}"] = dict(sorted(counts.items()))

            setattr_fn(tr, "_body", counted_body)
            tr.capture(warm=False)
            setattr_fn(tr, "_body", body)
            assert tr.graphs is not None
            out["capture"] = passes
        out["update"], out["other"] = iteration(True), iteration(False)
        tr.finish()
        torch.cuda.synchronize()
        return tr, out
    finally:
        F.DIRECT_GRAD = direct
