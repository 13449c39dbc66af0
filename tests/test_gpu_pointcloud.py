"""GPU tests of the point-cloud kernels (include/nsamd_pointcloud.h, nerfstudio_amd/csrc/pointcloud.hip) and of the layers over
them (nerfstudio_amd/pointcloud.py).

nsamd_points_select: kept set, order and all four outputs bit for bit a torch composition of the selection on the device. That
composition forms the point, the opacity test, the colour and the normals as exporter_utils.py:155-178 does, but writes the box
coordinate with the KERNEL'S OWN association ((w0 x + w1 y) + w2 z) + w3, where the reference goes through a BLAS matmul: for the
box test it checks the kernel against the same formula only. Independence from the reference's box test rests on the CPU tests
against the reference-written fixture (with their face margin) and on the device-side fixture test at the end of this file.
The points are also bit for bit the float64-checked fp32 candidates; appends, overflow,
guard rows, run-to-run bits, graph capture. nsamd_knn_mean_distance + nsamd_select_below: avg within 1e-12 relative of the
float64 restatement (tests/pointcloud_reference.py: 64 terms of 1 ulp each and the summation's roundings give 3e-14; times 30),
the SAME bits whatever grid and path found the neighbours, the threshold within 1e-12, the kept indices identical (every avg
is at least 1e-6 from the threshold, asserted by the CPU tests for the restatement)."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
import pointcloud_reference as pr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097]
# The one-workgroup scan of the workgroups' counts takes 256 of them at a sweep: 65536 entries are 256 workgroups, exactly one
# full sweep; 65537 are 257, the smallest size at which a second sweep exists and the carry between the sweeps decides rows.
SWEEP_SIZES = [65536, 65537]
GUARD = 5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def rays(n, seed=0):
    rs = np.random.RandomState(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    d = rs.normal(size=(n, 3))
    return dict(origins=f(rs.uniform(-0.2, 0.2, (n, 3))), directions=f(d / np.linalg.norm(d, axis=1, keepdims=True)),
                depth=f(rs.uniform(0.05, 0.9, n)), rgb=f(rs.uniform(0, 1, (n, 3))), alpha=f(rs.uniform(0.55, 1.0, n)),
                normals01=f(rs.uniform(0, 1, (n, 3))))


def pattern(r, name):
    n = len(r["depth"])
    r = {k: v.copy() for k, v in r.items()}
    if name == "none":
        r["alpha"][:] = 0.25
    elif name == "alternating":
        r["alpha"][::2] = 0.5  # not > 0.5
    elif name == "last":
        r["alpha"][:-1] = 0.0
    elif name == "nan_depth":
        r["depth"][n // 2] = np.nan
    elif name == "nan_alpha":
        r["alpha"][n // 2] = np.nan
    return r


BOX_R = np.array([[0.8799231, -0.3720255, -0.2955202], [0.3894183, 0.921061, 0.0], [0.2721924, -0.1150804, 0.9553365]], np.float32)
BOX_T, BOX_S = np.array([0.05, -0.1, 0.02], np.float32), np.array([1.1, 0.9, 1.3], np.float32)


def crop_box():
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import pointcloud as pc

    world2box, half = pc._obb_world2box(types.SimpleNamespace(R=T(BOX_R), T=T(BOX_T), S=T(BOX_S)))
    return N.make_crop_box(world2box, half), world2box, half


def torch_select(r, use_alpha, use_normals, box, dev):
    """the selection with torch ops on the device; the box coordinate in the kernel's association, ((w0 x + w1 y) + w2 z) + w3,
    not the reference's matmul (see the module docstring)"""
    t = {k: T(v).to(dev) for k, v in r.items()}
    p = t["origins"] + t["directions"] * t["depth"][:, None]
    keep = torch.ones(len(p), dtype=torch.bool, device=dev)
    colors = t["rgb"]
    if use_alpha:
        keep &= t["alpha"] > 0.5
        colors = t["rgb"] / t["alpha"].clamp(min=1e-10)[:, None]
    if box is not None:
        _, w, h = box
        for a in range(3):
            q = ((w[4 * a] * p[:, 0] + w[4 * a + 1] * p[:, 1]) + w[4 * a + 2] * p[:, 2]) + w[4 * a + 3]
            keep &= (q > -h[a]) & (q < h[a])
    normals = (t["normals01"] * 2.0 - 1.0)[keep] if use_normals else None
    return p[keep], colors[keep], t["directions"][keep], normals


class Select:
    """buffers with guard rows past the capacity, a cursor, and the launch"""

    def __init__(self, cap, dev, normals=True):
        from nerfstudio_amd import _native as N

        self.N, self.cap, self.dev = N, cap, dev
        self.full = [torch.full((cap + GUARD, 3), -7.0, device=dev) for _ in range(4 if normals else 3)]
        self.cursor = torch.zeros(2, dtype=torch.int64, device=dev)
        self.scratch = torch.empty(64, dtype=torch.int64, device=dev)

    def launch(self, t, use_alpha, use_normals, box):
        from nerfstudio_amd import functional as F

        n = t["depth"].numel()
        words = self.N.select_scratch_words(n)
        if self.scratch.numel() < words:
            self.scratch = torch.empty(words, dtype=torch.int64, device=self.dev)
        out = [b[:self.cap] for b in self.full]
        F.points_select_launch(t["origins"], t["directions"], t["depth"], t["rgb"], t["alpha"] if use_alpha else None,
                               t["normals01"] if use_normals else None, box[0] if box is not None else self.N.make_crop_box(),
                               out[0], out[1], out[2], out[3] if use_normals else None, self.cursor, self.scratch)

    def rows(self, m):
        return [b[:m] for b in self.full]

    def guards_intact(self, m):
        return all(bool((b[m:] == -7.0).all()) for b in self.full)


@pytest.mark.parametrize("n", SIZES)
def test_points_select_is_the_torch_composition_bit_for_bit(dev, n):
    base = rays(n, seed=n)
    box = crop_box()
    for name in ("all", "none", "alternating", "last", "nan_depth", "nan_alpha"):
        r = pattern(base, name)
        t = {k: T(v).to(dev) for k, v in r.items()}
        for use_alpha, use_normals, use_box in ((False, False, False), (True, True, True), (True, False, True), (True, True, False)):
            sel = Select(n, dev, use_normals)
            sel.launch(t, use_alpha, use_normals, box if use_box else None)
            ref = torch_select(r, use_alpha, use_normals, box if use_box else None, dev)
            m = int(sel.cursor[0])
            assert m == len(ref[0]) and int(sel.cursor[1]) == 0, (name, use_alpha, use_box)
            for got, want in zip(sel.rows(m), ref):
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, use_alpha, use_normals, use_box)
            assert sel.guards_intact(m)
            if not use_box:  # the points against the fp32 candidates the float64-checked restatement forms
                f64 = pr.select_f64(r["origins"], r["directions"], r["depth"], r["rgb"], r["alpha"] if use_alpha else None)
                got, nan = sel.rows(m)[0].cpu().numpy(), np.isnan(f64["points"])  # (a NaN's payload is the processor's own)
                assert np.array_equal(np.isnan(got), nan)
                assert np.array_equal(got.view(np.int32)[~nan], f64["points"].view(np.int32)[~nan])
            if name == "none" and use_alpha:
                assert m == 0
            if name == "last" and use_alpha and not use_box:
                assert m == 1
            if name == "all" and not use_alpha:
                assert m == n


@pytest.mark.parametrize("n", SWEEP_SIZES)
def test_points_select_across_the_sweeps_of_the_count_scan(dev, n):
    """box, alpha and normals on, two keep patterns. The kept count is above 256 and no multiple of 256, so a carry lost between
    the sweeps shifts rows (and the total) and cannot cancel. The last ray sits inside the box: with the random alpha it is kept,
    so at 65537 the one entry of the second sweep's workgroup writes a row whose place is the carry; with "alternating" entry
    65536 is dropped and the carry shows in the total alone."""
    base = rays(n, seed=n)
    base["origins"][-1], base["depth"][-1] = 0.0, 0.05
    box = crop_box()
    for name in ("all", "alternating"):
        r = pattern(base, name)
        t = {k: T(v).to(dev) for k, v in r.items()}
        sel = Select(n, dev, True)
        sel.launch(t, True, True, box)
        ref = torch_select(r, True, True, box, dev)
        m = int(sel.cursor[0])
        print(f"n = {n}, {name}: {len(ref[0])} kept by the torch composition, {m} by the kernels")
        assert len(ref[0]) > 256 and len(ref[0]) % 256 != 0
        if name == "all":  # the last ray is kept (the directions tell the rays apart)
            assert torch.equal(ref[2][-1], t["directions"][-1])
        assert m == len(ref[0]) and int(sel.cursor[1]) == 0, name
        for got, want in zip(sel.rows(m), ref):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
        assert sel.guards_intact(m)


def test_points_select_appends_refuses_an_overflow_and_repeats_its_bits(dev):
    r = rays(3 * 257, seed=3)
    box = crop_box()
    t = {k: T(v).to(dev) for k, v in r.items()}
    one = Select(3 * 257, dev)
    one.launch(t, True, True, box)
    m = int(one.cursor[0])
    assert 257 < m < 3 * 257
    parts = Select(m, dev)  # exactly enough capacity
    for b in range(3):
        parts.launch({k: v[257 * b:257 * (b + 1)].contiguous() for k, v in t.items()}, True, True, box)
    assert parts.cursor.tolist() == [m, 0] and parts.guards_intact(m)
    for a, b in zip(one.rows(m), parts.rows(m)):
        assert torch.equal(a, b)
    before = [b.clone() for b in parts.full]
    parts.launch({k: v[:257].contiguous() for k, v in t.items()}, True, True, box)
    assert parts.cursor.tolist() == [m, 1]  # the cursor stays, the flag is up
    for a, b in zip(before, parts.full):
        assert torch.equal(a, b)  # nothing of the batch was written
    again = Select(3 * 257, dev)
    again.launch(t, True, True, box)
    for a, b in zip(one.full, again.full):
        assert torch.equal(a, b)  # run to run


def test_points_select_is_capturable(dev):
    r = rays(4097, seed=5)
    box = crop_box()
    t = {k: T(v).to(dev) for k, v in r.items()}
    eager = Select(2 * 4097, dev)
    eager.launch(t, True, True, box)
    eager.launch(t, True, True, box)
    sel = Select(2 * 4097, dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        sel.launch(t, True, True, box)  # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    sel.cursor.zero_()
    for b in sel.full:
        b.fill_(-7.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sel.launch(t, True, True, box)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert sel.cursor.tolist() == eager.cursor.tolist() and int(sel.cursor[0]) % 2 == 0
    for a, b in zip(eager.full, sel.full):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- the outlier rule ------------------------------------------------
@pytest.fixture(scope="module")
def clouds():
    """(points, k, std_ratio) -> the float64 restatement, computed once"""
    cases = [(pr.case_cloud(c), c["k"], c["ratio"], c) for c in pr.CASES]
    cases += [(pr.case_cloud(pr.CASES[3]), k, 2.0, None) for k in (1, 32)]
    out = []
    for pts, k, ratio, case in cases:
        avg = pr.knn_mean_distance_f64(pts, k)
        thr = pr.threshold_f64(avg, ratio) if k > 1 else None  # k = 1: every avg is 0, nothing is valid
        out.append((pts, k, ratio, case, avg, thr))
    return out


def grids_for(pts, dev):
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import pointcloud as pc

    return {"default": pc.point_grid_for(T(pts).to(dev)), "one_cell": N.make_point_grid([-3.0, -3.0, -3.0], 6.0, [1, 1, 1]),
            "fine": N.make_point_grid([-0.55, -0.5, -0.45], 0.02, [55, 50, 45])}


@pytest.mark.parametrize("i", range(len(pr.CASES) + 2))
def test_knn_mean_distance_is_exact_over_every_grid_and_path(dev, clouds, i):
    from nerfstudio_amd import pointcloud as pc

    pts, k, ratio, case, avg64, thr64 = clouds[i]
    points = T(pts).to(dev)
    n = len(pts)
    first = None
    for gname, grid in grids_for(pts, dev).items():
        for max_rings in (0, pc.DEFAULT_MAX_RINGS, 1000):
            avg, unfinished = pc.knn_mean_distances(points, k, grid, max_rings)
            brute = int(unfinished[0])
            assert (max_rings != 0 or brute == n) and (max_rings != 1000 or brute == 0), (gname, max_rings, brute)
            assert len(set(unfinished[1:1 + brute].tolist())) == brute
            first = avg if first is None else first
            assert torch.equal(avg.view(torch.int64), first.view(torch.int64)), (gname, max_rings)
    got = first.cpu().numpy()
    rel = np.abs(got - avg64) / np.where(avg64 > 0, avg64, 1.0)
    print(f"case {i}: n = {n}, k = {k}: max relative distance of avg from float64 = {rel.max():.3e}")
    assert rel.max() <= pr.AVG_RTOL and np.array_equal(got == 0, avg64 == 0)
    if k == 1:
        assert not got.any()
        return
    kept64 = pr.kept_indices(avg64, thr64)
    assert pr.margin(avg64, thr64) >= pr.MIN_MARGIN  # what lets the kept sets be compared for identity
    for options in (dict(), dict(max_rings=0), dict(dims=[1, 1, 1]), dict(grid=grids_for(pts, dev)["fine"])):
        kept, avg, thr = pc.remove_statistical_outliers(points, k, ratio, **options)
        assert torch.equal(avg, first) and abs(thr - thr64) <= pr.AVG_RTOL * thr64
        assert kept.dtype == torch.int64 and np.array_equal(kept.cpu().numpy(), kept64)
    if case is not None:
        assert n - len(kept64) == case["removed"]


def test_knn_is_exact_with_points_far_outside_the_grid_box(dev):
    """1 % of the points at radius ~1000: the quantile box leaves them out, they fall into its border cells and, isolated, to
    the brute-force phase — with the same answer as one cell over everything"""
    from nerfstudio_amd import pointcloud as pc

    pts = pr.cloud(11, 3000, 0)
    rs = np.random.RandomState(12)
    far = rs.normal(size=(30, 3))
    pts[:30] = (1000.0 * far / np.linalg.norm(far, axis=1, keepdims=True)).astype(np.float32)
    avg64 = pr.knn_mean_distance_f64(pts, 20)
    points = T(pts).to(dev)
    stats = {}
    kept, avg, thr = pc.remove_statistical_outliers(points, 20, 2.0, stats=stats)
    assert max(stats["dims"]) >= 6 and stats["cell_size"] < 0.2  # the far points did not stretch the grid
    assert stats["brute_force_queries"] < len(pts) // 4  # the surface's queries finish in the rings
    assert pr.margin(avg64, pr.threshold_f64(avg64, 2.0)) >= pr.MIN_MARGIN
    rel = np.abs(avg.cpu().numpy() - avg64) / avg64
    assert rel.max() <= pr.AVG_RTOL
    one_cell = pc.remove_statistical_outliers(points, 20, 2.0, dims=[1, 1, 1], max_rings=0)
    assert torch.equal(one_cell[1], avg) and torch.equal(one_cell[0], kept) and one_cell[2] == thr
    assert np.array_equal(kept.cpu().numpy(), pr.kept_indices(avg64, pr.threshold_f64(avg64, 2.0)))
    assert not np.isin(np.arange(30), kept.cpu().numpy()).any()


def select_below_case(n):
    rs = np.random.RandomState(n)
    avg = rs.uniform(0, 2, n)
    avg[rs.uniform(size=n) < 0.2] = 0.0
    if n > 2:
        avg[1] = np.nan
    return avg


def check_select_below(avg, dev):
    """the kept indices and their count against pointcloud_reference.kept_indices, the guard rows; returns the reference's"""
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import functional as F

    n = len(avg)
    a = T(avg).to(dev)
    kept = torch.full((n + GUARD,), -7, dtype=torch.int64, device=dev)
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    F.select_below_launch(a, torch.tensor([1.0], dtype=torch.float64, device=dev), kept[:n], count,
                          torch.empty(N.select_scratch_words(n), dtype=torch.int64, device=dev))
    want = pr.kept_indices(avg, 1.0)
    assert int(count) == len(want) and np.array_equal(kept[:len(want)].cpu().numpy(), want)
    assert bool((kept[len(want):] == -7).all())
    return want


def test_select_below_at_the_workgroup_edges(dev):
    for n in SIZES:
        check_select_below(select_below_case(n), dev)


@pytest.mark.parametrize("n", SWEEP_SIZES)
def test_select_below_across_the_sweeps_of_the_count_scan(dev, n):
    """the last entry is kept, so at 65537 the second sweep's workgroup writes an index at the row the carry gives; the kept
    count is above 256 and no multiple of 256, so a lost carry cannot cancel"""
    avg = select_below_case(n)
    avg[-1] = 0.5
    want = check_select_below(avg, dev)
    print(f"n = {n}: {len(want)} kept")
    assert len(want) > 256 and len(want) % 256 != 0 and want[-1] == n - 1


# ---------------------------------------------------------------- the layers, on the device ---------------------------------------
def test_generate_point_cloud_reproduces_the_fixture_on_the_device(dev):
    from nerfstudio_amd import pointcloud as pc

    g = load_golden("pointcloud")
    state = {"n": 0}

    def batch_fn():
        b = state["n"] % 3
        state["n"] += 1
        return types.SimpleNamespace(origins=T(g["origins"][b]).to(dev), directions=T(g["directions"][b]).to(dev))

    def render_fn(ray_bundle):
        b = (state["n"] - 1) % 3
        return {k: T(g[k][b]).to(dev) for k in ("rgb", "accumulation", "depth", "normals")}

    pipeline = types.SimpleNamespace(model=types.SimpleNamespace(renderer_rgb=types.SimpleNamespace(background_color="random")))
    obb = types.SimpleNamespace(R=T(g["box_R"]), T=T(g["box_T"]), S=T(g["box_S"]))
    kw = dict(normal_output_name="normals", crop_obb=obb, batch_fn=batch_fn, render_fn=render_fn)
    cloud = pc.generate_point_cloud(pipeline, 300, remove_outliers=False, reorient_normals=True, **kw)
    assert state["n"] == 3 and cloud.points.device.type == "cuda"
    assert np.array_equal(cloud.points.cpu().numpy().astype(np.float64), g["reorient_points"])
    assert np.array_equal(cloud.colors.cpu().numpy().astype(np.float64), g["reorient_colors"])
    assert np.array_equal(cloud.normals.cpu().numpy().astype(np.float64), g["reorient_normals"])
    state["n"] = 0
    clean = pc.generate_point_cloud(pipeline, 300, remove_outliers=True, std_ratio=1.0, **kw)
    raw = g["box_normals_points"].astype(np.float32)
    avg = pr.knn_mean_distance_f64(raw, 20)
    ind = pr.kept_indices(avg, pr.threshold_f64(avg, 1.0))
    assert 0 < len(ind) < len(raw) and np.array_equal(clean.points.cpu().numpy(), raw[ind])
    assert np.array_equal(clean.normals.cpu().numpy().astype(np.float64), g["box_normals_normals"][ind])
