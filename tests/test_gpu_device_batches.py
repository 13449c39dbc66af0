"""GPU box: `nsamd_sample_batch` (csrc/batch.hip) and the layers above it (nerfstudio_amd/device_batches.py,
trainer.HipTrainer(source=...)).

The oracle is tests/batch_reference.py — Philox in numpy, the fp32 index recipe, the redraw loop, the uint8 gather — which
tests/test_device_batches_cpu.py pins to the host-compiled header and to the reference's own pixel sampler. Indices, camera
indices and targets are compared bit for bit; the rays bit for bit with `nsamd_raygen_lens` over the returned indices (that
kernel is pinned to the reference's fixture in tests/test_gpu_lens.py). Nothing here is statistical except the uniformity
check, whose seed is fixed (and was checked on the restatement): 5 binomial standard deviations."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_reference as BR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_store(num_images, height, width, seed, mask=None):
    """Random uint8 images; cameras on a shell of radius 2.5 looking at the origin, types 1, 2, 3 in turn, every third camera
    with non-zero distortion, principal points off the pixel centres (no fisheye pixel at theta = 0)."""
    from nerfstudio_amd.device_batches import DeviceImageStore

    rs = np.random.RandomState(seed)
    images = torch.from_numpy(rs.randint(0, 256, size=(num_images, height, width, 3)).astype(np.uint8))
    pos = rs.standard_normal((num_images, 3))
    pos = 2.5 * pos / np.linalg.norm(pos, axis=-1, keepdims=True)
    back = pos / np.linalg.norm(pos, axis=-1, keepdims=True)  # camera +z points away from the scene (OpenGL)
    right = np.cross(np.array([0.0, 0.0, 1.0]) + 0.01 * rs.standard_normal((num_images, 3)), back)
    right /= np.linalg.norm(right, axis=-1, keepdims=True)
    up = np.cross(back, right)
    c2w = torch.from_numpy(np.concatenate([np.stack([right, up, back], -1), pos[..., None]], -1).astype(np.float32))
    focal = torch.from_numpy(rs.uniform(0.9, 1.3, num_images).astype(np.float32)) * max(width, 4)
    types = torch.tensor([1 + (i % 3) for i in range(num_images)])
    dist = torch.zeros(num_images, 6)
    dist[::3] = torch.tensor([-0.12, 0.03, 0.0, 0.0, 1e-3, -2e-3])
    store = DeviceImageStore(images.to(DEV), None if mask is None else torch.from_numpy(mask).to(DEV), c2w, focal, focal * 1.01,
                             torch.full((num_images,), width / 2 + 0.25), torch.full((num_images,), height / 2 - 0.25), types, dist)
    return store, images.numpy()


STORES = {"1x1x1": (1, 1, 1), "3x5x7": (3, 5, 7), "100x64x48": (100, 64, 48)}


@pytest.fixture(scope="module")
def stores():
    return {name: make_store(*shape, seed=40 + k) for k, (name, shape) in enumerate(STORES.items())}


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096])
@pytest.mark.parametrize("name", list(STORES))
def test_sample_batch_equals_the_restatement_and_the_lens_rays(stores, name, n):
    from nerfstudio_amd import functional as F
    from nerfstudio_amd.device_batches import DeviceBatchSource

    store, images = stores[name]
    src = DeviceBatchSource(store, n, seed=2024)
    src.set_draw(17)
    rb, batch = src.next_batch()
    torch.cuda.synchronize()
    idx, rgb, _ = BR.sample_batch(images, None, n, src.seed, 17)
    assert batch["indices"].dtype == torch.int64 and rb.camera_indices.dtype == torch.int64
    np.testing.assert_array_equal(batch["indices"].cpu().numpy(), idx)
    np.testing.assert_array_equal(rb.camera_indices[:, 0].cpu().numpy(), idx[:, 0])
    np.testing.assert_array_equal(batch["image"].cpu().numpy().view(np.uint32), rgb.view(np.uint32))
    assert int(src.draw_counter) == 18 and src.failed_lanes() == 0
    o, d, pa, dn = F.raygen_lens(batch["indices"], store.c2w, store.fx, store.fy, store.cx, store.cy, store.camera_type, store.distortion)
    for got, want, what in ((rb.origins, o, "origins"), (rb.directions, d, "directions"), (rb.pixel_area, pa, "pixel_area"),
                            (rb.metadata["directions_norm"], dn, "directions_norm")):
        assert torch.equal(_bits(got), _bits(want)), what
    if name != "1x1x1" and n >= 255:
        assert sorted(set(store.camera_type[rb.camera_indices[:, 0]].tolist())) == [1, 2, 3]  # the lens types are mixed
    # the bare launch into caller-owned buffers, nullable outputs absent: the same batch
    o2, d2, t2 = (torch.full((n, 3), float("nan"), device=DEV) for _ in range(3))
    c2 = torch.full((n,), -1, device=DEV, dtype=torch.int64)
    counter = torch.tensor([5, 18], device=DEV)
    src.launch(o2, d2, c2, t2, counter[1:], -1)
    assert torch.equal(_bits(o2), _bits(rb.origins)) and torch.equal(_bits(d2), _bits(rb.directions))
    assert torch.equal(c2, rb.camera_indices[:, 0]) and torch.equal(_bits(t2), _bits(batch["image"])) and counter.tolist() == [5, 18]


def test_draws_are_a_function_of_seed_and_draw_alone(stores):
    from nerfstudio_amd.device_batches import DeviceBatchSource

    store, _ = stores["100x64x48"]
    n = 4096

    def draw(k, rank=0):
        src = DeviceBatchSource(store, n, seed=7, rank=rank)
        src.set_draw(k)
        rb, batch = src.next_batch()
        return batch["indices"], torch.cat([_bits(rb.origins), _bits(rb.directions), _bits(batch["image"])], -1)

    a, b = draw(3), draw(3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the same (seed, draw) must give the same bits"
    for other, what in ((draw(4), "draw + 1"), (draw(3, rank=1), "another rank's seed")):
        changed = int((other[0] != a[0]).any(dim=-1).sum())
        assert changed >= n // 2, (what, changed)


def test_mask_rejection_follows_the_restatements_redraw_loop(stores):
    from nerfstudio_amd.device_batches import DeviceBatchSource, DeviceImageStore

    base, images = stores["100x64x48"]
    mask = np.zeros((100, 64, 48), np.uint8)
    mask[:, ::2, ::2] = 1  # 25 % of the pixels, a fixed pattern
    store = DeviceImageStore(base.images, torch.from_numpy(mask).to(DEV), base.c2w, base.fx, base.fy, base.cx, base.cy,
                             base.camera_type, base.distortion)
    n = 4096
    src = DeviceBatchSource(store, n, seed=31)
    rb, batch = src.next_batch()
    idx, rgb, failed = BR.sample_batch(images, mask, n, src.seed, 0)
    assert failed == 0 and src.failed_lanes() == 0
    got = batch["indices"].cpu().numpy()
    assert (mask[got[:, 0], got[:, 1], got[:, 2]] == 1).all(), "every returned pixel must be valid"
    np.testing.assert_array_equal(got, idx)
    np.testing.assert_array_equal(batch["image"].cpu().numpy().view(np.uint32), rgb.view(np.uint32))
    plain = BR.sample_batch(images, None, n, src.seed, 0)[0]
    assert (plain != idx).any(axis=-1).sum() > n // 2  # three quarters of the lanes did redraw


def test_an_all_zero_mask_ends_after_max_attempts_inside_the_store():
    from nerfstudio_amd.device_batches import DeviceBatchSource, DeviceImageStore

    base, images = make_store(2, 4, 4, seed=9)
    mask = np.zeros((2, 4, 4), np.uint8)
    store = DeviceImageStore(base.images, torch.from_numpy(mask).to(DEV), base.c2w, base.fx, base.fy, base.cx, base.cy,
                             base.camera_type, base.distortion)
    n = 300
    src = DeviceBatchSource(store, n, seed=1)
    rb, batch = src.next_batch()
    idx, rgb, failed = BR.sample_batch(images, mask, n, src.seed, 0, max_attempts=100)
    assert failed == n and src.failed_lanes() == n
    got = batch["indices"].cpu().numpy()
    assert got.min() >= 0 and (got.max(axis=0) <= [1, 3, 3]).all()
    np.testing.assert_array_equal(got, idx)  # the last of the 101 draws, as the clamped restatement replays them
    np.testing.assert_array_equal(batch["image"].cpu().numpy().view(np.uint32), rgb.view(np.uint32))
    assert bool(torch.isfinite(rb.directions).all())
    src.next_batch()
    assert src.failed_lanes() == 2 * n  # the counter accumulates over launches


def test_pixels_are_uniform_over_images_and_pixel_bins():
    """n = 65536 draws over 16 images of 32 x 32: every image's count, and every cell's of a 4 x 4 grid of pixel bins, within 5
    binomial standard deviations of n / 16. Fixed seed: deterministic (the restatement gives the same counts)."""
    from nerfstudio_amd.device_batches import DeviceBatchSource

    store, images = make_store(16, 32, 32, seed=3)
    n = 65536
    src = DeviceBatchSource(store, n, seed=12345)
    idx = src.next_batch()[1]["indices"].cpu().numpy()
    np.testing.assert_array_equal(idx, BR.sample_batch(images, None, n, src.seed, 0)[0])
    sigma = np.sqrt(n * (1 / 16) * (15 / 16))
    per_image = np.bincount(idx[:, 0], minlength=16)
    per_bin = np.bincount((idx[:, 1] // 8) * 4 + idx[:, 2] // 8, minlength=16)
    for counts, what in ((per_image, "images"), (per_bin, "pixel bins")):
        assert counts.sum() == n and np.abs(counts - n / 16).max() <= 5 * sigma, (what, counts.tolist())


@pytest.mark.parametrize("camera", ["off", "SO3xR3"])
def test_source_inside_the_iteration_graph_eager_and_set_batch_same_bits(camera):
    """Two eager iterations, then six more — replayed from captured graphs with the source's launch as a node of the body; as
    eager launches of the same body; and on a trainer WITHOUT a source that is fed through `set_batch` by the same source's
    `next_batch()`. Same loss values and the same parameter bits in all three, at the seam tests' size (bench.py's)."""
    import bench

    from nerfstudio_amd import functional as F
    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.device_batches import DeviceBatchSource
    from nerfstudio_amd.trainer import HipTrainer

    F.DIRECT_GRAD = True
    try:
        n = bench.RAYS_PER_GPU
        store, _ = make_store(100, 64, 48, seed=77)
        store.camera_type.fill_(1)
        results = {}
        for route in ("graph", "eager", "set_batch"):
            F._SCATTER_WS.clear()
            model = bench.build_model(torch.device(DEV), seed=0, camera_optimizer=camera)
            arena = ParamArena(model.get_param_groups_ordered(), lr=1e-2, eps=1e-15)
            src = DeviceBatchSource(store, n, seed=99)
            rb, batch = src.next_batch(advance=False)
            tr = HipTrainer(model, arena, rb, batch, world=1, use_graph=route == "graph", use_runner=True,
                            source=None if route == "set_batch" else src)
            assert tr.prologue and tr.prologue_ring and tr.source_inside == (route != "set_batch")
            if route != "graph":
                tr.runner.side_stream = None
            losses = []
            for it in range(8):
                if it == 2 and route == "graph":
                    tr.capture(warm=False)
                    assert tr.graphs is not None and tr.defer
                if route == "set_batch":
                    tr.set_batch(*src.next_batch())
                tr.train_iteration()
                losses.append(float(tr.last_loss()))
            tr.finish()
            torch.cuda.synchronize()
            if route == "set_batch":
                assert int(src.draw_counter) == 8
            else:
                assert int(src.draw_counter) == 0 and tr.step_counter.tolist() == [8, 8]  # the prologue's counter drew the batches
            pose = model.camera_optimizer.pose_adjustment.detach().clone() if camera != "off" else torch.zeros(1)
            results[route] = (losses, arena.flat.clone(), float(arena.flat.double().sum()), pose, tr.runner.target.clone())
            del tr, arena, model
        g = results["graph"]
        assert np.isfinite(g[0]).all() and len(set(g[0])) == 8, g[0]  # a new batch every iteration
        if camera != "off":
            assert float(g[3].abs().max()) > 0
        for other in ("eager", "set_batch"):
            o = results[other]
            assert g[0] == o[0], (other, g[0], o[0])
            assert torch.equal(g[4], o[4]), f"last batch differs between graph replay and {other}"
            assert g[2] == o[2] and torch.equal(g[1], o[1]), f"parameters differ between graph replay and {other}"
            assert torch.equal(g[3], o[3])
    finally:
        F.DIRECT_GRAD = False


def test_sample_batch_argument_statuses(stores):
    from nerfstudio_amd import _native as N

    lib = N.load()
    store, _ = stores["3x5x7"]
    n = 8
    o, d, t = (torch.zeros(n, 3, device=DEV) for _ in range(3))
    c = torch.zeros(n, device=DEV, dtype=torch.int64)
    counter = torch.zeros(1, device=DEV, dtype=torch.int64)
    failed = torch.zeros(1, device=DEV, dtype=torch.int32)

    def call(images=store.images, mask=None, N_=3, H=5, W=7, fx=store.fx, ctype=store.camera_type, ctr=counter, attempts=100, rays=n,
             origins=o, target=t, fail=None):
        return lib.nsamd_sample_batch(N.ptr(images), N.ptr(mask), N_, H, W, N.ptr(store.c2w), N.ptr(fx), N.ptr(store.fy),
                                      N.ptr(store.cx), N.ptr(store.cy), N.ptr(ctype), N.ptr(store.distortion), N.ptr(ctr), 0, 1,
                                      attempts, rays, N.ptr(origins), N.ptr(d), None, None, N.ptr(c), N.ptr(target), None,
                                      N.ptr(fail), N.stream())

    assert call() == 0 and call(rays=0) == 0 and call(rays=0, origins=None, target=None) == 0
    assert call(rays=-1) == -1 and call(N_=0) == -1 and call(H=0) == -1 and call(W=0) == -1 and call(attempts=-1) == -1
    assert call(images=None) == -1 and call(fx=None) == -1 and call(ctype=None) == -1 and call(ctr=None) == -1
    assert call(origins=None) == -1 and call(target=None) == -1
    mask = torch.ones(3, 5, 7, device=DEV, dtype=torch.uint8)
    assert call(mask=mask) == -1 and call(mask=mask, fail=failed) == 0
    assert call(N_=1 << 24, rays=0) == -2 and call(rays=(1 << 32) + 1) == -2
    torch.cuda.synchronize()
    assert int(failed) == 0
