"""CPU tier of the device-resident training batches (nerfstudio_amd/device_batches.py, csrc/batch_sample.h, csrc/batch.hip):

* the per-ray arithmetic the kernel runs, compiled for the host by tests/hostcheck/batch_helpers.cc — Philox-4x32-10 against the
  numpy restatement of tests/batch_reference.py, the index recipe and the colour conversion against
  tests/golden/pixel_batches.npz, written by the reference's own `PixelSampler.collate_image_dataset_batch` on recorded uniforms
  (tests/golden/make_golden_batches.py), and the clamp at the top of the uniform range;
* the host logic above the kernel with an injected launch: what `DeviceImageStore.from_dataset` declines, the byte budget, the
  pipeline seam with `device_batches` on and off, the trainer's eager form, where the draw counter starts.

The library built here is test infrastructure: the product never loads it. Everything is bit for bit."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_reference as BR  # noqa: E402

from nerfstudio_amd.runner_interface import TrainStepRunner  # noqa: E402

U32P = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
F32P = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
U8P = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libbatchcheck.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "batch_helpers.cc")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.hc_philox4x32_10.argtypes = [U32P, U32P, C.c_int64, U32P]
    lib.hc_philox4x32_10.restype = None
    lib.hc_batch_uniform.argtypes = [U32P, C.c_int64, F32P]
    lib.hc_batch_uniform.restype = None
    lib.hc_batch_pixel_index.argtypes = [F32P, C.c_int64, C.c_int32, I32P]
    lib.hc_batch_pixel_index.restype = None
    lib.hc_batch_pixel_index_clamped.argtypes = [F32P, C.c_int64, C.c_int32]
    lib.hc_batch_pixel_index_clamped.restype = C.c_int64
    lib.hc_batch_pixel_float.argtypes = [U8P, C.c_int64, F32P]
    lib.hc_batch_pixel_float.restype = None
    lib.hc_batch_draw_pixel.argtypes = [U32P, U32P, C.c_int64, C.c_int64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, I32P]
    lib.hc_batch_draw_pixel.restype = None
    lib.hc_batch_seed_xor.argtypes = []
    lib.hc_batch_seed_xor.restype = C.c_uint64
    return lib


# ------------------------------------------------------------------------------------------------- shared arithmetic
def test_philox_compiled_for_the_host_equals_the_numpy_restatement(hc):
    """A grid of counters: the prologue's layout (q lo, q hi, draw lo, draw hi) with q below and above 2^32 and draws above
    2^32, the sampler's (ray, attempt, draw), all-ones words; two keys. The known-answer vectors of the Random123 distribution
    pin the restatement itself."""
    kat = BR.philox4x32_10(np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint32),
                           np.array([[0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [0xA4093822, 0x299F31D0]], np.uint32))
    assert kat.tolist() == [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
                            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]]
    qs = [0, 1, 2, 255, 256, 4095, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33 + 12345, 2 ** 40 + 7, 2 ** 63 - 1]
    draws = [0, 1, 29999, 2 ** 32 - 1, 2 ** 32, 2 ** 35 + 3]
    ctr = np.array([[q & BR.MASK32, q >> 32, d & BR.MASK32, d >> 32] for q in qs for d in draws], np.uint32)
    ctr = np.concatenate([ctr, np.array([[r, a, d, 0] for r in (0, 1, 4095, 65535) for a in (0, 1, 100) for d in (0, 7)], np.uint32),
                          np.full((1, 4), 0xFFFFFFFF, np.uint32)])
    for key in (0x0123456789ABCDEF, 0xA0761D6478BD642F ^ 1234, 0):
        keys = np.tile(np.array([[key & BR.MASK32, key >> 32]], np.uint32), (ctr.shape[0], 1))
        out = np.empty_like(ctr)
        hc.hc_philox4x32_10(ctr, keys, ctr.shape[0], out)
        np.testing.assert_array_equal(out, BR.philox4x32_10(ctr, keys))
    words = np.array([0, 255, 256, 0xFFFFFFFF, 0x80000000, 0x12345678], np.uint32)
    u = np.empty(words.shape[0], np.float32)
    hc.hc_batch_uniform(words, words.shape[0], u)
    np.testing.assert_array_equal(u, BR.uniform(words))
    assert u[0] == 0.0 and u[1] == 0.0 and u[2] == np.float32(2.0 ** -24) and u[3] == np.float32(1 - 2.0 ** -24)
    assert hc.hc_batch_seed_xor() == BR.SEED_XOR
    # the lane's whole draw: counter layout, key split and the three indices
    rays = np.array([0, 1, 255, 256, 4095, 2 ** 32 - 1], np.uint32)
    att = np.array([0, 1, 0, 100, 3, 0], np.uint32)
    for draw in (0, 5, 2 ** 32 + 9):
        got = np.empty((rays.shape[0], 3), np.int32)
        hc.hc_batch_draw_pixel(rays, att, rays.shape[0], draw, 77 ^ BR.SEED_XOR, 100, 48, 64, got)
        np.testing.assert_array_equal(got, BR.draw_pixels(rays, att, draw, 77 ^ BR.SEED_XOR, 100, 48, 64))


@pytest.mark.parametrize("case", ["small", "single"])
def test_index_and_colour_recipes_reproduce_the_reference_fixture(hc, case):
    g = load_golden("pixel_batches")
    assert list(g["cases"]) == ["small", "single"]
    images, u = g[f"{case}_images"], g[f"{case}_uniforms"]
    assert images.dtype == np.uint8 and u.dtype == np.float32 and images.shape[:3] == ((3, 5, 7) if case == "small" else (1, 1, 1))
    assert (u == 0).any() and (u == np.float32(1 - 2.0 ** -24)).any() and u.min() >= 0 and u.max() < 1
    n = u.shape[0]
    idx = np.empty((n, 3), np.int32)
    for j, dim in enumerate(images.shape[:3]):
        col = np.empty(n, np.int32)
        hc.hc_batch_pixel_index(np.ascontiguousarray(u[:, j]), n, dim, col)
        idx[:, j] = col
    np.testing.assert_array_equal(idx, g[f"{case}_indices"])
    np.testing.assert_array_equal(BR.pixel_index(u[:, 1], images.shape[1]), g[f"{case}_indices"][:, 1])  # (the restatement too)
    if case == "small":  # products that land exactly on an integer are in the fixture: u * dim == floor(u * dim) > 0
        for j, dim in enumerate(images.shape[:3]):
            p = u[:, j] * np.float32(dim)
            assert ((p == np.floor(p)) & (p > 0)).any(), j
    gathered = np.ascontiguousarray(images[idx[:, 0], idx[:, 1], idx[:, 2]].reshape(-1))
    rgb = np.empty(gathered.shape[0], np.float32)
    hc.hc_batch_pixel_float(gathered, gathered.shape[0], rgb)
    np.testing.assert_array_equal(rgb.reshape(n, 3).view(np.uint32), g[f"{case}_image"].view(np.uint32))
    every = np.arange(256, dtype=np.uint8)
    out = np.empty(256, np.float32)
    hc.hc_batch_pixel_float(every, 256, out)
    np.testing.assert_array_equal(out, every / np.float32(255))  # base_dataset.py:107 on every byte


@pytest.mark.parametrize("dim", [1, 7, 1024, 1920, 4096, 65535])
def test_the_clamp_fires_for_no_24_bit_uniform(hc, dim):
    """Exhaustively over the top 2^12 uniforms (the product is monotone in u, so the largest ones decide)."""
    u = (np.arange(2 ** 24 - 2 ** 12, 2 ** 24, dtype=np.int64).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    assert u[-1] == np.float32(1 - 2.0 ** -24) and u.shape[0] == 4096
    assert hc.hc_batch_pixel_index_clamped(u, u.shape[0], dim) == 0
    out = np.empty(u.shape[0], np.int32)
    hc.hc_batch_pixel_index(u, u.shape[0], dim, out)
    assert out.max() == dim - 1 and out.min() >= 0 and (np.diff(out) >= 0).all()
    # ... and it does hold the line for an input outside the generator's range
    one = np.array([1.0, 1.5], np.float32)
    o2 = np.empty(2, np.int32)
    hc.hc_batch_pixel_index(one, 2, dim, o2)
    assert o2.tolist() == [dim - 1, dim - 1] and hc.hc_batch_pixel_index_clamped(one, 2, dim) == 2


# ------------------------------------------------------------------------------------------------- host logic
class _Dataset:
    """What from_dataset reads of an InputDataset: len, get_data(i, image_type="uint8"), cameras, metadata."""

    def __init__(self, n=4, h=5, w=7, types=None, channels=3, mask=False, sizes=None, depth=False, cam_meta=None):
        rs = np.random.RandomState(3)
        self.sizes = sizes or [(h, w)] * n
        self.images = [torch.from_numpy(rs.randint(0, 256, size=(hh, ww, channels)).astype(np.uint8)) for hh, ww in self.sizes]
        self.masks = [torch.from_numpy((rs.uniform(size=(hh, ww, 1)) < 0.5)) for hh, ww in self.sizes] if mask else None
        self.depth, self.metadata, self.asked = depth, {}, []
        t = torch.tensor(types if types is not None else [1] * n).reshape(n, 1)
        self.cameras = SimpleNamespace(camera_type=t, camera_to_worlds=torch.eye(4)[None, :3].repeat(n, 1, 1) + 0.0,
                                       fx=torch.full((n, 1), 50.0), fy=torch.full((n, 1), 51.0), cx=torch.full((n, 1), w / 2),
                                       cy=torch.full((n, 1), h / 2), distortion_params=None, metadata=cam_meta or {})

    def __len__(self):
        return len(self.images)

    def get_data(self, i, image_type="float32"):
        self.asked.append((i, image_type))
        data = {"image_idx": i, "image": self.images[i]}
        if self.masks is not None:
            data["mask"] = self.masks[i]
        if self.depth:
            data["depth_image"] = torch.zeros(self.sizes[i] + (1,))
        return data


def test_from_dataset_builds_the_store_and_names_every_declined_case():
    from nerfstudio_amd.device_batches import DeviceImageStore

    ds = _Dataset(mask=True, types=[1, 2, 1, 3])
    store = DeviceImageStore.from_dataset(ds, "cpu", max_bytes=1 << 20)
    assert isinstance(store, DeviceImageStore) and ds.asked == [(i, "uint8") for i in range(4)]
    assert store.images.shape == (4, 5, 7, 3) and store.images.dtype == torch.uint8 and torch.equal(store.images[2], ds.images[2])
    assert store.mask.shape == (4, 5, 7) and store.mask.dtype == torch.uint8 and torch.equal(store.mask[1].bool(), ds.masks[1][..., 0])
    assert store.camera_type.dtype == torch.int32 and store.camera_type.tolist() == [1, 2, 1, 3] and store.distortion is None
    assert store.c2w.shape == (4, 3, 4) and store.fx.shape == (4,) and store.fy[0] == 51.0
    assert store.nbytes == 4 * 5 * 7 * 4 == DeviceImageStore.bytes_needed(4, 5, 7, masked=True)
    assert DeviceImageStore.from_dataset(_Dataset(), "cpu").nbytes == 4 * 5 * 7 * 3
    declined = {
        "images of different sizes": _Dataset(sizes=[(5, 7), (5, 7), (6, 7), (5, 7)]),
        "RGBA": _Dataset(channels=4),
        "camera type 9": _Dataset(types=[1, 9, 1, 1]),
        "camera type 4": _Dataset(types=[4, 4, 4, 4]),
        "every camera is equirectangular": _Dataset(types=[3, 3, 3, 3]),
        "fisheye_crop_radius": _Dataset(types=[2, 2, 2, 2], cam_meta={"fisheye_crop_radius": 0.8}),
        "depth dataset": _Dataset(depth=True),
    }
    for words, dataset in declined.items():
        reason = DeviceImageStore.from_dataset(dataset, "cpu")
        assert isinstance(reason, str) and words in reason, (words, reason)
    reason = DeviceImageStore.from_dataset(_Dataset(), "cpu", patch_size=8)
    assert isinstance(reason, str) and "patch_size 8" in reason
    # the byte budget: exactly the store's size passes, one byte less declines — before any image is read
    need = 4 * 5 * 7 * 3
    assert isinstance(DeviceImageStore.from_dataset(_Dataset(), "cpu", max_bytes=need), DeviceImageStore)
    ds = _Dataset()
    reason = DeviceImageStore.from_dataset(ds, "cpu", max_bytes=need - 1)
    assert isinstance(reason, str) and f"{need} bytes" in reason and "max_bytes" in reason and len(ds.asked) == 1


def _cpu_launch(log):
    """Stand-in for nsamd_sample_batch on CPU tensors: the restatement's pixels, rays straight down -z from the camera."""
    def launch(store, n, seed, max_attempts, draw_counter, draw_offset, origins, directions, camera_indices, target,
               pixel_area=None, directions_norm=None, indices=None, failed=None):
        draw = int(draw_counter[0]) + int(draw_offset)
        log.append(draw)
        idx, rgb, bad = BR.sample_batch(store.images.numpy(), None if store.mask is None else store.mask.numpy(), n, seed, draw,
                                        max_attempts)
        idx = torch.from_numpy(idx)
        origins.copy_(store.c2w[idx[:, 0], :, 3])
        directions.copy_(torch.tensor([0.0, 0.0, -1.0]).expand(n, 3))
        camera_indices.copy_(idx[:, 0])
        target.copy_(torch.from_numpy(rgb))
        if indices is not None:
            indices.copy_(idx)
        if pixel_area is not None:
            pixel_area.fill_(1e-6)
        if directions_norm is not None:
            directions_norm.fill_(1.0)
        failed.add_(bad)
    return launch


def test_source_draws_counter_based_batches_through_the_injected_launch():
    from nerfstudio_amd.device_batches import DeviceBatchSource, DeviceImageStore, mix_seed

    store = DeviceImageStore.from_dataset(_Dataset(), "cpu")
    log = []
    src = DeviceBatchSource(store, 16, seed=11, launch_fn=_cpu_launch(log))
    assert src.seed == mix_seed(11, 0) != mix_seed(11, 1) and DeviceBatchSource(store, 16, seed=11, rank=1).seed == mix_seed(11, 1)
    rb, batch = src.next_batch()
    assert rb.origins.shape == (16, 3) and rb.camera_indices.shape == (16, 1) and rb.pixel_area.shape == (16, 1)
    assert set(batch) == {"image", "indices"} and batch["indices"].dtype == torch.int64 and batch["image"].shape == (16, 3)
    idx, rgb, _ = BR.sample_batch(store.images.numpy(), None, 16, src.seed, 0)
    assert np.array_equal(batch["indices"].numpy(), idx) and np.array_equal(batch["image"].numpy(), rgb)
    assert torch.equal(rb.camera_indices[:, 0], batch["indices"][:, 0])
    again = src.next_batch(advance=False)[1]["indices"]
    assert torch.equal(again, src.next_batch()[1]["indices"]) and not torch.equal(again, batch["indices"])
    assert log == [0, 1, 1] and int(src.draw_counter) == 2
    src.set_draw(40)
    src.next_batch()
    assert log[-1] == 40 and int(src.draw_counter) == 41 and src.failed_lanes() == 0
    # `launch` into caller-owned buffers reads the caller's counter and advances nothing
    o, d, t = torch.zeros(16, 3), torch.zeros(16, 3), torch.zeros(16, 3)
    c = torch.zeros(16, dtype=torch.int64)
    counter = torch.tensor([3, 9])
    src.launch(o, d, c, t, counter[1:], -1)
    assert log[-1] == 8 and counter.tolist() == [3, 9] and int(src.draw_counter) == 41


# ---- the trainer and the pipeline seam over a toy schedule (no kernels: what is under test is who supplies the batch) ----
class _ToyModel(torch.nn.Module):
    def __init__(self, step=0):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(8))
        self.pw = torch.nn.Parameter(torch.ones(4))
        self.config = SimpleNamespace(background_color="black", predict_normals=False)
        self.step = step
        self.proposal_sampler = SimpleNamespace(_anneal=1.0, anneal_dev=None, updated_this_step=lambda: True, mark_updated=lambda: None)

    def get_param_groups(self):
        return {"fields": [self.w], "proposal_networks": [self.pw]}


class _ToyRunner(TrainStepRunner):
    """The runner interface trainer.HipTrainer drives, reduced to a loss of the batch it was handed."""

    def __init__(self, model, n, device):
        self.model, self.n = model, n
        self.origins, self.directions, self.target = torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n, 3)
        self.camera_indices = torch.zeros(n, dtype=torch.int64)
        self.dist_per_ray = torch.zeros(n)
        self.batches = []

    def set_batch(self, origins, directions, camera_indices, target=None):
        self.origins.copy_(origins), self.directions.copy_(directions), self.camera_indices.copy_(camera_indices.reshape(-1))
        self.target.copy_(target)
        self.batches.append((camera_indices.reshape(-1).clone(), target.clone()))

    def written_params(self):
        return []

    def apply_camera_corrections(self):
        pass

    def forward_proposals(self, draw_jitter=True, need_enc=True, after_bins=None):
        pass

    def forward_main_and_losses(self, updated, terms_ready=False):
        self.loss = ((self.model.w.detach().mean() - self.target) ** 2).mean()

    def backward_all(self, updated):
        self.grad_lookup[id(self.model.w)].add_(1.0)
        self.grad_lookup[id(self.model.pw)].add_(1.0)

    def loss_dict(self):
        return {"rgb_loss": self.loss, "interlevel_loss": torch.zeros(()), "distortion_loss": torch.zeros(())}

    def outputs(self):
        return {"rgb": torch.zeros(self.n, 3)}


def _source(n=16, log=None, **dataset):
    from nerfstudio_amd.device_batches import DeviceBatchSource, DeviceImageStore

    store = DeviceImageStore.from_dataset(_Dataset(**dataset), "cpu")
    return DeviceBatchSource(store, n, seed=5, launch_fn=_cpu_launch([] if log is None else log))


def test_trainer_without_the_prologue_feeds_set_batch_from_next_batch_and_starts_at_the_models_step(monkeypatch):
    import cpu_runner

    from nerfstudio_amd import functional as F
    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.trainer import HipTrainer

    monkeypatch.setattr(F, "adam_step", cpu_runner.cpu_adam)
    log = []
    src = _source(log=log)
    model = _ToyModel(step=300)  # a resumed run
    arena = ParamArena(model.get_param_groups(), lr=1e-2, eps=1e-15)
    rb, batch = src.next_batch(advance=False)
    with pytest.raises(ValueError, match="mutually exclusive"):
        HipTrainer(model, arena, rb, batch, pool={"origins": torch.zeros(1, 16, 3)}, source=src, runner=_ToyRunner(model, 16, "cpu"))
    runner = _ToyRunner(model, 16, "cpu")
    tr = HipTrainer(model, arena, rb, batch, use_graph=False, source=src, runner=runner, drive_callbacks=False)
    assert not tr.prologue and not tr.source_inside  # no device prologue on this route: the eager form
    assert int(src.draw_counter) == 300, "the draw counter continues from the model's step"
    seen = len(runner.batches)
    for k in range(3):
        tr.train_iteration()
        assert len(runner.batches) == seen + k + 1 and log[-1] == 300 + k
        want = BR.sample_batch(src.store.images.numpy(), None, 16, src.seed, 300 + k)
        assert np.array_equal(runner.batches[-1][0].numpy(), want[0][:, 0]) and np.array_equal(runner.batches[-1][1].numpy(), want[1])
    assert int(src.draw_counter) == 303 and arena.step_counts["fields"] == 3
    with pytest.raises(AssertionError, match="samples its own"):
        tr.set_batch(rb, batch)


@pytest.mark.parametrize("device_batches", [True, False])
def test_seam_takes_its_batches_from_the_source_and_never_calls_next_train(monkeypatch, device_batches):
    import cpu_runner
    import trainer_restatement as R

    from nerfstudio_amd import functional as F
    from nerfstudio_amd.pipeline import EngineSeam

    monkeypatch.setattr(F, "adam_step", cpu_runner.cpu_adam)
    model = _ToyModel()
    dataset = _Dataset(n=6)
    calls = []

    class Datamanager:
        train_dataset = dataset
        train_count = 0
        config = SimpleNamespace(patch_size=1, pixel_sampler=SimpleNamespace(ignore_mask=False, rejection_sample_mask=True))

        def get_train_rays_per_batch(self):
            return 16

        def next_train(self, step):
            calls.append(step)
            if device_batches:
                raise AssertionError("next_train must not be called while the device source is active")
            self.train_count += 1
            return _host_batch(step)

    def _host_batch(step):
        from nerfstudio_amd.cameras.rays import RayBundle

        g = torch.Generator().manual_seed(step)
        return (RayBundle(origins=torch.zeros(16, 3), directions=torch.tensor([0.0, 0, -1]).expand(16, 3).contiguous(),
                          pixel_area=torch.full((16, 1), 1e-6), camera_indices=torch.zeros(16, 1, dtype=torch.int64)),
                {"image": torch.rand(16, 3, generator=g)})

    class Pipeline(EngineSeam):
        def __init__(self):
            self.datamanager = Datamanager()
            self.model = self._model = model
            self.world_size = 1

    pipe = Pipeline()
    log = []
    if device_batches:
        assert pipe.setup_device_batches("cpu", launch_fn=_cpu_launch(log)) is None and pipe._batch_source is not None
    groups = model.get_param_groups()
    cfg = {k: {"optimizer": {"lr": 1e-2, "eps": 1e-15}, "scheduler": {"lr_final": 1e-4, "max_steps": 100}} for k in groups}
    opts = R.Optimizers(cfg, groups)
    pipe.attach_optimizers(opts, None, runner_factory=_ToyRunner)
    for step in range(4):
        out, loss_dict, metrics = pipe.get_train_loss_dict(step)
        assert set(loss_dict) >= {"rgb_loss", "interlevel_loss", "distortion_loss"} and "psnr" in metrics
    eng = pipe._engine
    assert eng.reason is None and eng.trainer is not None and pipe.datamanager.train_count == 4
    if device_batches:
        assert calls == [] and eng.trainer.source is pipe._batch_source and eng.source is pipe._batch_source
        assert log == [0, 0, 1, 2, 3]  # the batch the engine was built on (not advanced), then one draw per iteration
        runner = eng.trainer.runner
        want = BR.sample_batch(pipe._batch_source.store.images.numpy(), None, 16, pipe._batch_source.seed, 3)
        assert np.array_equal(runner.batches[-1][1].numpy(), want[1])
    else:
        assert calls == [0, 1, 2, 3] and eng.trainer.source is None and pipe._batch_source is None  # today's behaviour


def test_a_declined_store_logs_its_reason_once_and_keeps_the_datamanager(capsys):
    from nerfstudio_amd.pipeline import EngineSeam

    class Pipeline(EngineSeam):
        def __init__(self, dataset, **cfg):
            self.datamanager = SimpleNamespace(train_dataset=dataset, train_count=0, get_train_rays_per_batch=lambda: 16,
                                               config=SimpleNamespace(patch_size=cfg.pop("patch_size", 1), pixel_sampler=SimpleNamespace(**cfg)))
            self.world_size = 1

    for pipe, words in ((Pipeline(_Dataset(types=[3, 3, 3, 3])), "equirectangular"),
                        (Pipeline(_Dataset(), patch_size=4), "patch_size 4"),
                        (Pipeline(_Dataset(mask=True), ignore_mask=False, rejection_sample_mask=False), "rejection_sample_mask off")):
        reason = pipe.setup_device_batches("cpu", launch_fn=_cpu_launch([]))
        err = capsys.readouterr().err
        assert words in reason and pipe._batch_source is None and pipe.batch_source_reason == reason
        assert err.count("device_batches declined") == 1 and words in err
    assert "device cpu" in Pipeline(_Dataset()).setup_device_batches("cpu")  # no kernel without a GPU, and no fallback
    capsys.readouterr()
    pipe = Pipeline(_Dataset(mask=True), ignore_mask=True, rejection_sample_mask=True)
    assert pipe.setup_device_batches("cpu", launch_fn=_cpu_launch([])) is None and pipe._batch_source.store.mask is None
    pipe = Pipeline(_Dataset(), ignore_mask=False, rejection_sample_mask=True)
    assert "max_bytes" in pipe.setup_device_batches("cpu", max_bytes=10, launch_fn=_cpu_launch([]))


def test_entry_point_validates_before_launching():
    """NSAMD_ERR_INVALID_ARG (-1) for a negative count, an empty store dimension, a null store or camera array, a mask without
    the failed counter, null outputs; NSAMD_ERR_UNSUPPORTED (-2) for dimensions the fp32 index recipe cannot hold; an empty
    launch over valid arguments is a no-op. Nothing is launched in any of them (there is no device here)."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    P = 0x1000  # any non-null address: the checks never dereference

    def call(images=P, mask=None, N_=3, H=5, W=7, cams=P, counter=P, attempts=100, n=0, outs=P, failed=None):
        return lib.nsamd_sample_batch(images, mask, N_, H, W, cams, cams, cams, cams, cams, cams, None, counter, 0, 1, attempts, n,
                                      outs, outs, None, None, outs, outs, None, failed, None)

    assert call() == 0
    assert call(n=-1) == -1 and call(N_=0) == -1 and call(H=0) == -1 and call(W=-3) == -1 and call(attempts=-1) == -1
    assert call(images=None) == -1 and call(cams=None) == -1 and call(counter=None) == -1
    assert call(mask=P) == -1 and call(mask=P, failed=P) == 0
    assert call(n=5, outs=None) == -1
    assert call(N_=1 << 24) == -2 and call(W=1 << 24) == -2 and call(n=(1 << 32) + 1) == -2
