"""CPU tests of point-cloud export (nerfstudio_amd/pointcloud.py over include/nsamd_pointcloud.h): the float64 restatements
(tests/pointcloud_reference.py) against the table of cases and the fixture the reference wrote (tests/golden/pointcloud.npz,
tests/golden/make_golden_pointcloud.py), the arithmetic of nerfstudio_amd/csrc/pointcloud.h compiled for the host
(tests/hostcheck/pointcloud_helpers.cc) and looped as the kernels compose it, the same build under the address and
undefined-behaviour sanitizers as a stand-alone program, every layer above the kernels with the launches replaced by the host
build, and the ABI.

Bounds: the kept sets are IDENTICAL (every avg is at least 1e-6, relative, from its threshold — asserted for the restatement);
avg and threshold within 1e-12 relative of float64 (at most 64 terms, each a sqrt within 1 ulp plus one summation rounding:
3e-14, times 30); points bit for bit; rays within 4 fp32 ulp * |half_scale| of a box face are not compared with the
reference, whose box test goes through a BLAS matmul (at most 1 % of them)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import pointcloud_reference as pr

T = torch.from_numpy
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")
HEADER = os.path.join(ROOT, "include", "nsamd_pointcloud.h")
NAMES = ["nsamd_knn_mean_distance", "nsamd_point_cell_keys", "nsamd_points_select", "nsamd_select_below"]
VARIANTS = {"plain": ("last_sample", None, False, False), "random": ("random", None, False, False),
            "box": ("random", "box", False, False), "box_normals": ("random", "box", True, False),
            "reorient": ("random", "box", True, True), "face": ("random", "face", False, False)}
NUM_POINTS = 300


@pytest.fixture(scope="module")
def g():
    return load_golden("pointcloud")


@pytest.fixture(scope="module")
def clouds():
    """case index -> (points, avg_f64, threshold, kept): computed once, never written to"""
    out = {}
    for i, case in enumerate(pr.CASES):
        pts = pr.case_cloud(case)
        avg = pr.knn_mean_distance_f64(pts, case["k"])
        thr = pr.threshold_f64(avg, case["ratio"])
        for a in (pts, avg):
            a.setflags(write=False)
        out[i] = (pts, avg, thr, pr.kept_indices(avg, thr))
    return out


# ---------------------------------------------------------------- the restatement alone ------------------------------------------
@pytest.mark.parametrize("i", range(len(pr.CASES)))
def test_restatement_gives_the_recorded_counts_with_a_margin(clouds, i):
    case = pr.CASES[i]
    pts, avg, thr, kept = clouds[i]
    assert len(pts) == case["n"] and len(pts) - len(kept) == case["removed"]
    assert pr.margin(avg, thr) >= pr.MIN_MARGIN
    if i == 4:
        assert (avg == 0).sum() == 26 and not np.isin(np.nonzero(avg == 0)[0], kept).any()  # the avg > 0 rule
    if i in (3, 5, 6):
        brute = pr.knn_mean_distance_brute(pts, case["k"])
        assert np.max(np.abs(brute - avg) / np.maximum(avg, 1e-300)) <= pr.AVG_RTOL


def variant_inputs(g, name, batches=2):
    background, box, with_normals, _ = VARIANTS[name]
    cat = lambda k: np.concatenate([g[k][b] for b in range(batches)])  # noqa: E731
    kw = dict(origins=cat("origins"), directions=cat("directions"), depth=cat("depth").reshape(-1), rgb=cat("rgb"))
    if background == "random":
        kw["alpha"] = cat("accumulation").reshape(-1)
    if with_normals:
        kw["normals01"] = cat("normals")
    if box is not None:
        kw["world2box"] = pr.world2box_f64(g[box + "_R"], g[box + "_T"])
        kw["half_scale"] = g[box + "_S"].astype(np.float64) / 2
    return kw


def reference_keep(g, name, candidates):
    """which of the candidate fp32 points are rows of the fixture's cloud; the fixture's rows are the candidates kept, in order"""
    ref = g[f"{name}_points"]
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    rows = {r.tobytes() for r in ref.astype(np.float32)}
    keep = np.array([c.tobytes() in rows for c in candidates])
    assert np.array_equal(candidates[keep], ref.astype(np.float32))
    return keep


@pytest.mark.parametrize("name", VARIANTS)
def test_float64_selection_reproduces_the_fixture_on_safe_rays(g, name):
    assert str(g["source"]).startswith("generate_point_cloud")  # the reference's own function wrote the fixture
    kw = variant_inputs(g, name)
    sel = pr.select_f64(**kw)
    candidates = kw["origins"] + (kw["directions"] * kw["depth"][:, None]).astype(np.float32)
    ref_keep = reference_keep(g, name, candidates)
    safe = ~sel["unsafe"]
    assert 1.0 - safe.mean() <= pr.UNSAFE_CAP  # the cap, for the reference alone
    assert np.array_equal(sel["keep"][safe], ref_keep[safe])
    if name == "face":  # the strict inequality: exactly on the face is outside, one ulp inside is inside (identity box: exact)
        assert not ref_keep[5] and ref_keep[6] and not sel["keep"][5] and sel["keep"][6] and sel["unsafe"][5]
        assert candidates[5, 0] == 0.5
    if not sel["unsafe"].any() or name == "face":
        assert np.array_equal(sel["points"].astype(np.float64), g[f"{name}_points"])
        assert np.array_equal(sel["colors"].astype(np.float64), g[f"{name}_colors"])
        if VARIANTS[name][2] and not VARIANTS[name][3]:
            assert np.array_equal(sel["normals"].astype(np.float64), g[f"{name}_normals"])
    first = pr.select_f64(**variant_inputs(g, name, 1))["keep"].sum()
    assert first < NUM_POINTS <= sel["keep"].sum()  # reached in the second batch
    if name == "random":
        assert not ref_keep[9] and kw["alpha"][9] == 0.5


# ---------------------------------------------------------------- pointcloud.h on the host ---------------------------------------
def _ptr(t):
    if t is None:
        return None
    assert t.is_contiguous()
    return t.data_ptr()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """pointcloud.Launches served by the host build of csrc/pointcloud.h, on CPU tensors"""
    from nerfstudio_amd import _native as N

    out = str(tmp_path_factory.mktemp("hostcheck") / "libpointcloudcheck.so")
    # -ffp-contract=off as the kernels are built (csrc/Makefile): no FMA contraction of a*b+c
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(HOSTCHECK, "pointcloud_helpers.cc")], check=True)
    lib = C.CDLL(out)
    for name, argtypes in N._POINTCLOUD_SIGNATURES.items():
        getattr(lib, name.replace("nsamd_", "hc_")).argtypes = argtypes[:-1]  # no stream

    class HostLaunches:
        calls = []

        @staticmethod
        def points_select(origins, directions, depth, rgb, alpha, normals01, box, out_points, out_colors, out_view_dirs,
                          out_normals, cursor, scratch):
            n = depth.numel()
            assert scratch.numel() >= N.select_scratch_words(n)
            HostLaunches.calls.append(n)
            assert lib.hc_points_select(_ptr(origins), _ptr(directions), _ptr(depth), _ptr(rgb), _ptr(alpha), _ptr(normals01), n,
                                        box, _ptr(out_points), _ptr(out_colors), _ptr(out_view_dirs), _ptr(out_normals),
                                        out_points.shape[0], _ptr(cursor), _ptr(scratch)) == 0

        @staticmethod
        def select_below(avg, threshold, out_indices, count, scratch):
            assert lib.hc_select_below(_ptr(avg), avg.numel(), _ptr(threshold), _ptr(out_indices), _ptr(count), _ptr(scratch)) == 0

        @staticmethod
        def point_cell_keys(points, grid, keys):
            assert lib.hc_point_cell_keys(_ptr(points), points.shape[0], grid, _ptr(keys)) == 0

        @staticmethod
        def knn_mean_distance(points, order, cell_start, grid, k, max_rings, avg, unfinished):
            assert lib.hc_knn_mean_distance(_ptr(points), points.shape[0], _ptr(order), _ptr(cell_start), grid, k, max_rings,
                                            _ptr(avg), _ptr(unfinished)) == 0

    HostLaunches.lib = lib
    return HostLaunches


def host_select(host, kw, cap, cursor=None, buffers=None):
    from nerfstudio_amd import _native as N

    n = len(kw["depth"])
    t = lambda k: None if kw.get(k) is None else T(np.ascontiguousarray(kw[k], dtype=np.float32))  # noqa: E731
    box = N.make_crop_box()
    if kw.get("world2box") is not None:
        # the fp32 matrix the product builds: torch.inverse on the host
        box = N.make_crop_box(np.asarray(kw["world2box32"]).reshape(-1).tolist(), np.asarray(kw["half_scale"], np.float32).tolist())
    if buffers is None:
        buffers = [torch.full((cap + 2, 3), -7.0) for _ in range(4)]
    cursor = torch.zeros(2, dtype=torch.int64) if cursor is None else cursor
    scratch = torch.empty(N.select_scratch_words(n), dtype=torch.int64)
    normals = t("normals01")
    host.points_select(t("origins"), t("directions"), t("depth"), t("rgb"), t("alpha"), normals, box,
                       buffers[0][:cap], buffers[1][:cap], buffers[2][:cap], buffers[3][:cap] if normals is not None else None,
                       cursor, scratch)
    return cursor, buffers


def with_fp32_box(g, name, kw):
    from nerfstudio_amd import pointcloud as pc

    box = VARIANTS[name][1]
    if box is not None:
        obb = types.SimpleNamespace(R=T(g[box + "_R"]), T=T(g[box + "_T"]), S=T(g[box + "_S"]))
        kw["world2box32"], half = pc._obb_world2box(obb)
        assert np.array_equal(np.asarray(half, np.float32), (g[box + "_S"] / 2).astype(np.float32))
    return kw


@pytest.mark.parametrize("name", VARIANTS)
def test_host_selection_matches_float64_and_the_fixture(g, host, name):
    kw = with_fp32_box(g, name, variant_inputs(g, name))
    sel = pr.select_f64(**{k: v for k, v in kw.items() if k != "world2box32"})
    n = len(kw["depth"])
    cursor, buf = host_select(host, kw, n)
    m = int(cursor[0])
    assert cursor[1] == 0
    candidates = kw["origins"] + (kw["directions"] * kw["depth"][:, None]).astype(np.float32)
    rows = {r.tobytes() for r in buf[0][:m].numpy()}
    keep = np.array([c.tobytes() in rows for c in candidates])
    safe = ~sel["unsafe"]
    assert np.array_equal(keep[safe], sel["keep"][safe]) and keep.sum() == m
    assert np.array_equal(buf[0][:m].numpy(), candidates[keep])  # ray order, points bit for bit
    colors = kw["rgb"] if "alpha" not in kw else (kw["rgb"] / np.maximum(kw["alpha"], np.float32(1e-10))[:, None]).astype(np.float32)
    assert np.array_equal(buf[1][:m].numpy(), colors[keep]) and np.array_equal(buf[2][:m].numpy(), kw["directions"][keep])
    if "normals01" in kw:
        assert np.array_equal(buf[3][:m].numpy(), (kw["normals01"] * np.float32(2) - np.float32(1))[keep])
    for b in buf[:3]:
        assert (b[m:] == -7.0).all()  # nothing past the kept rows
    if not sel["unsafe"].any() or name == "face":
        assert np.array_equal(buf[0][:m].numpy().astype(np.float64), g[f"{name}_points"])
        assert np.array_equal(buf[1][:m].numpy().astype(np.float64), g[f"{name}_colors"])


def test_host_selection_appends_across_calls_and_refuses_an_overflow(g, host):
    whole = with_fp32_box(g, "box_normals", variant_inputs(g, "box_normals", 3))
    n = len(whole["depth"])
    cursor1, one = host_select(host, whole, n)
    m = int(cursor1[0])
    cursor, buf = None, None
    for b in range(3):
        part = {k: (v[257 * b:257 * (b + 1)] if k not in ("world2box", "world2box32", "half_scale") else v) for k, v in whole.items()}
        cursor, buf = host_select(host, part, m, cursor, buf)  # exactly enough capacity
    assert int(cursor[0]) == m and cursor[1] == 0
    for a, b in zip(one, buf):
        assert torch.equal(a[:m], b[:m]) and (b[m:] == -7.0).all()
    before = [b.clone() for b in buf]
    part = {k: (v[:257] if k not in ("world2box", "world2box32", "half_scale") else v) for k, v in whole.items()}
    cursor, buf = host_select(host, part, m, cursor, buf)
    assert int(cursor[0]) == m and cursor[1] == 1  # nothing written, the cursor stays, the flag is up
    for a, b in zip(before, buf):
        assert torch.equal(a, b)
    nan = dict(part)
    nan["depth"] = part["depth"].copy()
    nan["depth"][3] = np.nan
    nan["alpha"] = part["alpha"].copy()
    nan["alpha"][4] = np.nan
    c, out = host_select(host, nan, 257)
    ref = pr.select_f64(**{k: v for k, v in nan.items() if k != "world2box32"})
    assert not ref["keep"][3] and not ref["keep"][4] and int(c[0]) == ref["keep"].sum()


def grids_for(pts):
    """a default grid, one cell, and a fine grid whose box leaves the far points out"""
    from nerfstudio_amd import _native as N
    from nerfstudio_amd import pointcloud as pc

    return {"default": pc.point_grid_for(T(pts.copy())), "one_cell": N.make_point_grid([-3.0, -3.0, -3.0], 6.0, [1, 1, 1]),
            "fine": N.make_point_grid([-0.55, -0.5, -0.45], 0.02, [55, 50, 45])}


@pytest.mark.parametrize("i", range(len(pr.CASES)))
def test_host_knn_is_exact_over_every_grid_and_path(clouds, host, i):
    from nerfstudio_amd import pointcloud as pc

    case = pr.CASES[i]
    pts, avg64, thr64, kept64 = clouds[i]
    first = None
    for gname, grid in grids_for(pts).items():
        for max_rings in (0, 2, 1000):
            avg, unfinished = pc.knn_mean_distances(T(pts.copy()), case["k"], grid, max_rings, host)
            brute = int(unfinished[0])
            assert sorted(unfinished[1:1 + brute].tolist()) == sorted(set(unfinished[1:1 + brute].tolist()))
            assert (max_rings != 0 or brute == len(pts)) and (max_rings != 1000 or brute == 0), (gname, max_rings, brute)
            first = avg if first is None else first
            assert torch.equal(avg, first), (gname, max_rings)  # the same bits whatever found the neighbours
    rel = np.abs(first.numpy() - avg64) / np.where(avg64 > 0, avg64, 1.0)
    assert rel.max() <= pr.AVG_RTOL and np.array_equal(first.numpy() == 0, avg64 == 0)
    for options in (dict(), dict(max_rings=0), dict(dims=[1, 1, 1]), dict(grid=grids_for(pts)["fine"])):
        stats = {}
        kept, avg, thr = pc.remove_statistical_outliers(T(pts.copy()), case["k"], case["ratio"], launches=host, stats=stats, **options)
        assert torch.equal(avg, first) and abs(thr - thr64) <= pr.AVG_RTOL * thr64
        assert kept.dtype == torch.int64 and np.array_equal(kept.numpy(), kept64)
        assert stats["brute_force_queries"] == (len(pts) if options.get("max_rings") == 0 else stats["brute_force_queries"])


def test_default_grid_box_ignores_far_points():
    from nerfstudio_amd import pointcloud as pc

    pts = pr.cloud(7, 3000, 0)
    pts[:20] *= 2000.0  # depth ~1000
    grid = pc.point_grid_for(T(pts))
    assert max(grid.dims) >= 6 and grid.cell_size < 0.2 and all(-0.6 < o < -0.3 for o in grid.origin)
    boxed = pc.point_grid_for(T(pts), aabb=([-1, -1, -1], [1, 1, 1]), dims=[4, 4, 4])
    assert list(boxed.dims) == [4, 4, 4] and boxed.cell_size == 0.5


@pytest.mark.parametrize("i", [3, 4, 6])
def test_host_build_is_clean_under_the_sanitizers(clouds, tmp_path, i):
    """a stand-alone program with the sanitizers' runtimes linked in statically: it runs in the environment it inherits, as it
    is, and nothing of it runs inside python"""
    exe = str(tmp_path / "pointcloud_main")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HOSTCHECK, "pointcloud_main.cc"),
                    os.path.join(HOSTCHECK, "pointcloud_helpers.cc")], check=True)
    case = pr.CASES[i]
    pts, _, _, kept = clouds[i]
    path = tmp_path / "points.f32"
    pts.tofile(path)
    run = subprocess.run([exe, str(path), str(len(pts)), str(case["k"]), str(case["ratio"])], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.strip() == f"kept {len(kept)} of {len(pts)}"


# ---------------------------------------------------------------- the layers above the kernels -----------------------------------
class Replay:
    """a pipeline that replays the fixture's batches"""

    def __init__(self, g, background="random", batches=3):
        self.g, self.n, self.batches = g, 0, batches
        self.model = types.SimpleNamespace(renderer_rgb=types.SimpleNamespace(background_color=background))
        self.datamanager = types.SimpleNamespace(next_train=self.next_train)

    def next_train(self, step):
        b = self.n % self.batches
        self.n += 1
        return types.SimpleNamespace(origins=T(self.g["origins"][b]), directions=T(self.g["directions"][b])), {"b": b}

    def render(self, ray_bundle):
        b = (self.n - 1) % self.batches
        return {k: T(self.g[k][b]) for k in ("rgb", "accumulation", "depth", "normals")}


def obb_of(g, box):
    return None if box is None else types.SimpleNamespace(R=T(g[box + "_R"]), T=T(g[box + "_T"]), S=T(g[box + "_S"]))


@pytest.mark.parametrize("name", VARIANTS)
def test_generate_point_cloud_reproduces_the_fixture(g, host, name):
    from nerfstudio_amd import pointcloud as pc

    background, box, with_normals, reorient = VARIANTS[name]
    pipe = Replay(g, background)
    host.calls.clear()
    cloud = pc.generate_point_cloud(pipe, NUM_POINTS, remove_outliers=False, reorient_normals=reorient,
                                    normal_output_name="normals" if with_normals else None, crop_obb=obb_of(g, box),
                                    render_fn=pipe.render, launches=host)
    assert host.calls == [257] * 3 and pipe.n == 3  # one launch per batch; one batch past the reference's stop, never more
    sel = pr.select_f64(**variant_inputs(g, name))
    # (no variant has an unsafe ray apart from the face variant's own: test_no_fixture_variant_has_an_unsafe_ray)
    assert np.array_equal(cloud.points.numpy().astype(np.float64), g[f"{name}_points"])  # cut where the reference stops
    assert np.array_equal(cloud.colors.numpy().astype(np.float64), g[f"{name}_colors"])
    assert np.array_equal(cloud.view_directions.numpy(), sel["view_dirs"]) and len(cloud) == len(g[f"{name}_points"])
    if with_normals:
        assert np.array_equal(cloud.normals.numpy().astype(np.float64), g[f"{name}_normals"])
        if reorient:
            assert not np.array_equal(g["reorient_normals"], g["box_normals_normals"])
            assert ((cloud.view_directions * cloud.normals).sum(-1) <= 0).all()
    else:
        assert cloud.normals is None


def test_no_fixture_variant_has_an_unsafe_ray(g):
    for name in VARIANTS:
        unsafe = pr.select_f64(**variant_inputs(g, name))["unsafe"]
        assert unsafe.sum() == (2 if name == "face" else 0)  # the ray on the face and the one an ulp inside it


def test_accumulator_reads_one_batch_late_and_cuts_where_the_reference_stops(g, host):
    from nerfstudio_amd import pointcloud as pc

    pipe = Replay(g)
    acc = pc.PointAccumulator(NUM_POINTS + 2 * 257, "cpu", False, host)
    assert tuple(acc.points.shape) == (NUM_POINTS + 514, 3) and acc.normals is None
    known = []
    for _ in range(3):
        rb, _ = pipe.next_train(0)
        known.append(acc.add(rb, pipe.render(rb), use_alpha=True))
    per_batch = [int(pr.select_f64(**{k: v[257 * b:257 * (b + 1)] for k, v in variant_inputs(g, "random", 3).items()})["keep"].sum())
                 for b in range(3)]
    totals = np.cumsum(per_batch).tolist()
    assert known == [None, totals[0], totals[1]] and acc.totals == totals[:2]  # the read lags the launch by one batch
    assert len(acc.finish(NUM_POINTS)) == totals[1] and len(acc.finish()) == totals[2] and acc.totals == totals
    small = pc.PointAccumulator(totals[0] + 5, "cpu", False, host)
    pipe = Replay(g)
    rb, _ = pipe.next_train(0)
    small.add(rb, pipe.render(rb), use_alpha=True)
    rb, _ = pipe.next_train(0)
    small.add(rb, pipe.render(rb), use_alpha=True)  # runs past the capacity; known one batch late
    with pytest.raises(RuntimeError, match="capacity"):
        small.finish()
    assert int(small.cursor[0]) == totals[0]


def test_generate_point_cloud_errors_and_signature(g, host):
    from nerfstudio_amd import pointcloud as pc

    pipe = Replay(g)
    kw = dict(render_fn=pipe.render, launches=host)
    with pytest.raises(KeyError, match="'colour'.*accumulation.*rgb"):
        pc.generate_point_cloud(pipe, 10, rgb_output_name="colour", **kw)
    with pytest.raises(KeyError, match="'z'"):
        pc.generate_point_cloud(pipe, 10, depth_output_name="z", **kw)
    with pytest.raises(KeyError, match="'n'"):
        pc.generate_point_cloud(pipe, 10, normal_output_name="n", **kw)
    with pytest.raises(ValueError, match="Cannot estimate normals and use normal_output_name"):
        pc.generate_point_cloud(pipe, 10, estimate_normals=True, normal_output_name="normals", **kw)
    with pytest.raises(NotImplementedError, match="estimate_normals"):
        pc.generate_point_cloud(pipe, 10, estimate_normals=True, **kw)
    bad = dict(g)
    bad["normals"] = g["normals"].copy()
    bad["normals"][0, 3, 1] = 1.5
    pipe = Replay(bad)
    with pytest.raises(ValueError, match=r"must be in \[0, 1\]"):
        pc.generate_point_cloud(pipe, 10, remove_outliers=False, normal_output_name="normals", render_fn=pipe.render, launches=host)
    pipe = Replay(g)
    far = types.SimpleNamespace(R=torch.eye(3), T=torch.tensor([50.0, 0, 0]), S=torch.ones(3))
    with pytest.raises(RuntimeError, match="0 of 10 points after 4 batches"):
        pc.generate_point_cloud(pipe, 10, crop_obb=far, max_batches=4, render_fn=pipe.render, launches=host)
    params = inspect.signature(pc.generate_point_cloud).parameters
    positional = [(k, p.default) for k, p in params.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert positional == [("pipeline", inspect.Parameter.empty), ("num_points", 1000000), ("remove_outliers", True),
                          ("estimate_normals", False), ("reorient_normals", False), ("rgb_output_name", "rgb"),
                          ("depth_output_name", "depth"), ("normal_output_name", None), ("crop_obb", None), ("std_ratio", 10.0)]
    # the default batch function: the device batch source when the pipeline trains from one
    source = types.SimpleNamespace(next_batch=lambda: ("bundle", {}))
    assert pc._default_batch_fn(types.SimpleNamespace(_batch_source=source))() == "bundle"
    assert pc._default_batch_fn(types.SimpleNamespace(datamanager=types.SimpleNamespace(next_train=lambda s: ("dm", s))))() == "dm"


def test_generate_point_cloud_removes_outliers_with_the_reference_bookkeeping(g, host):
    from nerfstudio_amd import pointcloud as pc

    pipe = Replay(g)
    kw = dict(normal_output_name="normals", crop_obb=obb_of(g, "box"), render_fn=pipe.render, launches=host)
    raw = pc.generate_point_cloud(pipe, NUM_POINTS, remove_outliers=False, **kw)
    pipe.n = 0
    clean = pc.generate_point_cloud(pipe, NUM_POINTS, remove_outliers=True, std_ratio=1.0, reorient_normals=True, **kw)
    avg = pr.knn_mean_distance_f64(raw.points.numpy(), 20)
    ind = pr.kept_indices(avg, pr.threshold_f64(avg, 1.0))
    assert 0 < len(ind) < len(raw) and pr.margin(avg, pr.threshold_f64(avg, 1.0)) >= pr.MIN_MARGIN
    assert torch.equal(clean.points, raw.points[ind]) and torch.equal(clean.colors, raw.colors[ind])
    assert torch.equal(clean.view_directions, raw.view_directions[ind])  # `view_directions[ind]`, exporter_utils.py:197
    normals = raw.normals[ind].clone()
    flip = (clean.view_directions * normals).sum(-1) > 0
    normals[flip] *= -1
    assert flip.any() and torch.equal(clean.normals, normals)


def test_remove_statistical_outliers_argument_errors(host):
    from nerfstudio_amd import pointcloud as pc

    pts = T(pr.cloud(3, 50, 2))
    for bad in (dict(nb_neighbors=0), dict(std_ratio=0.0), dict(std_ratio=-1.0)):
        with pytest.raises(ValueError, match="must be positive"):
            pc.remove_statistical_outliers(pts, **{**dict(nb_neighbors=5, std_ratio=1.0), **bad}, launches=host)
    with pytest.raises(ValueError, match="at most 32 neighbours"):
        pc.remove_statistical_outliers(pts, 33, 1.0, launches=host)
    kept, avg, thr = pc.remove_statistical_outliers(pts[:0], 5, 1.0, launches=host)
    assert kept.numel() == 0 and avg.numel() == 0
    with pytest.raises(RuntimeError, match="MI355X"):  # no torch fallback behind the native launches
        pc.remove_statistical_outliers(pts, 5, 1.0)


def read_ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    n = int(lines[2].split()[-1])
    kinds = {"float": "<f4", "uchar": "u1"}
    dtype = np.dtype([(ln.split()[2], kinds[ln.split()[1]]) for ln in lines[3:]])
    assert len(body) == n * dtype.itemsize
    return np.frombuffer(body, dtype=dtype)


def test_write_ply_reads_back_byte_for_byte(tmp_path):
    from nerfstudio_amd import pointcloud as pc

    rs = np.random.RandomState(1)
    pts, nrm = T(rs.normal(size=(9, 3)).astype(np.float32)), T(rs.normal(size=(9, 3)).astype(np.float32))
    colors = T(rs.uniform(0, 1, (9, 3)).astype(np.float32))
    colors[0] = torch.tensor([0.0, 1.0, 0.999])
    colors[1] = torch.tensor([1.7, -0.2, float("nan")])
    colors[2] = T((np.array([1, 128, 254]) / 255).astype(np.float32))  # level boundaries
    cloud = pc.PointCloud(pts, colors, nrm.clone(), nrm)
    cloud.write_ply(tmp_path / "a.ply")
    rows = read_ply(tmp_path / "a.ply")
    assert rows.dtype.names == ("x", "y", "z", "red", "green", "blue", "nx", "ny", "nz") and rows.dtype.itemsize == 27
    assert np.array_equal(np.stack([rows["x"], rows["y"], rows["z"]], 1), pts.numpy())
    assert np.array_equal(np.stack([rows["nx"], rows["ny"], rows["nz"]], 1), nrm.numpy())
    rgb = np.stack([rows["red"], rows["green"], rows["blue"]], 1)
    assert rgb[0].tolist() == [0, 255, 254] and rgb[1].tolist() == [255, 0, 0]  # truncated, saturated
    # the product is formed in float64, as the reference forms it from its float64 colours (scripts/exporter.py:183)
    assert np.array_equal(rgb[2:], (colors[2:].numpy().astype(np.float64) * 255).astype(np.uint8))
    pc.PointCloud(pts, colors, nrm).write_ply(tmp_path / "b.ply")
    assert read_ply(tmp_path / "b.ply").dtype.names == ("x", "y", "z", "red", "green", "blue")
    try:
        import open3d  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="open3d"):
            cloud.to_open3d()


def test_export_point_cloud_writes_the_world_frame(g, host, tmp_path):
    from nerfstudio_amd import pointcloud as pc

    pipe = Replay(g)
    transform = torch.tensor([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 2.0]])

    def to_original(poses):  # DataparserOutputs.transform_poses_to_original_space with scale 2: inverse transform, then / scale
        inv = torch.linalg.inv(torch.cat([transform, torch.tensor([[0.0, 0, 0, 1]])]))
        out = inv @ torch.cat([poses, torch.tensor([[[0.0, 0, 0, 1]]]).expand(len(poses), 1, 4)], dim=1)
        out[:, :3, 3] /= 2.0
        return out[:, :3]

    pipe.datamanager.train_dataparser_outputs = types.SimpleNamespace(transform_poses_to_original_space=to_original)
    pipe.datamanager.train_pixel_sampler = types.SimpleNamespace(num_rays_per_batch=4096)
    kw = dict(num_points=NUM_POINTS, remove_outliers=False, obb_center=(0.05, -0.1, 0.02), obb_rotation=(0.1, -0.3, 0.4),
              obb_scale=(1.1, 0.9, 1.3), num_rays_per_batch=257, render_fn=pipe.render, launches=host)
    model = pc.export_point_cloud(pipe, tmp_path / "model", **kw)
    pipe.n = 0
    world = pc.export_point_cloud(pipe, tmp_path / "world", save_world_frame=True, **kw)
    assert pipe.datamanager.train_pixel_sampler.num_rays_per_batch == 257
    rows = read_ply(tmp_path / "world" / "point_cloud.ply")
    assert len(rows) == len(world) == len(model) >= NUM_POINTS and "nx" in rows.dtype.names
    poses = torch.eye(4)[None, :3].repeat(len(model), 1, 1)
    poses[:, :3, 3] = model.points
    assert torch.equal(world.points, to_original(poses)[:, :3, 3])
    assert np.array_equal(np.stack([rows["x"], rows["y"], rows["z"]], 1), world.points.numpy())
    assert np.array_equal(read_ply(tmp_path / "model" / "point_cloud.ply")["x"], model.points[:, 0].numpy())
    # Rz(yaw) Ry(pitch) Rx(roll): the box of the fixture is Rz(0.4) Ry(-0.3)
    assert torch.allclose(pc.rpy_matrix(0.0, -0.3, 0.4), T(g["box_R"]), atol=1e-7)
    R = pc.rpy_matrix(0.1, -0.3, 0.4)
    assert R.dtype == torch.float32 and torch.allclose(R @ R.T, torch.eye(3), atol=1e-6) and abs(float(torch.det(R)) - 1) < 1e-6
    params = inspect.signature(pc.export_point_cloud).parameters  # ExportPointCloud's fields and defaults
    assert [(k, p.default) for k, p in params.items() if p.kind is p.POSITIONAL_OR_KEYWORD][2:] == [
        ("num_points", 1000000), ("remove_outliers", True), ("reorient_normals", True), ("normal_method", "model_output"),
        ("normal_output_name", "normals"), ("depth_output_name", "depth"), ("rgb_output_name", "rgb"), ("obb_center", None),
        ("obb_rotation", None), ("obb_scale", None), ("num_rays_per_batch", 32768), ("std_ratio", 10.0), ("save_world_frame", False)]


def test_module_imports_nothing_of_nerfstudio():
    src = open(os.path.join(ROOT, "nerfstudio_amd", "pointcloud.py")).read()
    assert not re.search(r"^\s*(from|import) nerfstudio\b", src, flags=re.M)


# ---------------------------------------------------------------- the entry points ------------------------------------------------
def test_entry_points_are_declared_bound_and_launched_from_one_place(tmp_path):
    from nerfstudio_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(nsamd_[a-z0-9_]+)\s*\(", header))) == sorted(N._POINTCLOUD_SIGNATURES) == NAMES
    assert not set(N._POINTCLOUD_SIGNATURES) & (set(N._SIGNATURES) | set(N._EXPORT_SIGNATURES) | set(N._RENDER_SIGNATURES))
    cdll = C.CDLL(N.LIB_PATH)
    lib = N.load()
    for name in NAMES:
        assert hasattr(cdll, name) and callable(getattr(lib, name))
    vp, i64, i32 = N.vp, N.i64, N.i32
    assert N._POINTCLOUD_SIGNATURES == {
        "nsamd_points_select": [vp] * 6 + [i64, N.CropBox] + [vp] * 4 + [i64, vp, vp, vp],
        "nsamd_select_below": [vp, i64, vp, vp, vp, vp, vp],
        "nsamd_point_cell_keys": [vp, i64, N.PointGrid, vp, vp],
        "nsamd_knn_mean_distance": [vp, i64, vp, vp, N.PointGrid, i32, i32, vp, vp, vp]}
    assert C.sizeof(N.CropBox) == 64 and C.sizeof(N.PointGrid) == 28
    assert (N.SELECT_BLOCK, N.KNN_MAX_K, N.KNN_MAX_CELLS) == tuple(
        int(eval(re.search(rf"#define {m}\s+(\S+(?: << \d+\))?)", open(HEADER).read()).group(1)))
        for m in ("NSAMD_SELECT_BLOCK", "NSAMD_KNN_MAX_K", "NSAMD_KNN_MAX_CELLS"))
    for n in (0, 1, 256, 257, 513, 10 ** 6):
        assert N.select_scratch_words(n) == 1 + ((n + 255) // 256 + 1) // 2
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "nsamd_pointcloud.h"\n'
                   "int main(void) {\n"
                   "  nsamd_crop_box box = {0, {0}, {0}};\n"
                   "  nsamd_point_grid grid = {{0, 0, 0}, 1.0f, {2, 2, 2}};\n"
                   "  int64_t words[NSAMD_SELECT_SCRATCH_WORDS(257)];\n"
                   "  if (sizeof(words) != 2 * sizeof(int64_t)) return 9;\n"
                   "  if (nsamd_points_select(NULL, NULL, NULL, NULL, NULL, NULL, 0, box, NULL, NULL, NULL, NULL, 4, NULL, NULL, NULL)"
                   " != NSAMD_OK) return 1;\n"
                   "  if (nsamd_points_select(NULL, NULL, NULL, NULL, NULL, NULL, 5, box, NULL, NULL, NULL, NULL, 4, NULL, NULL, NULL)"
                   " != NSAMD_ERR_INVALID_ARG) return 2;\n"
                   "  if (nsamd_knn_mean_distance(NULL, 5, NULL, NULL, grid, NSAMD_KNN_MAX_K + 1, 1, NULL, NULL, NULL)"
                   " != NSAMD_ERR_UNSUPPORTED) return 3;\n"
                   "  if (nsamd_point_cell_keys(NULL, 0, grid, NULL, NULL) != NSAMD_OK) return 4;\n"
                   "  if (nsamd_select_below(NULL, 3, NULL, NULL, words, words, NULL) != NSAMD_ERR_INVALID_ARG) return 5;\n"
                   "  return 0;\n}\n")
    libdir = os.path.dirname(N.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(tmp_path / "use"), "-L", libdir,
                    "-lnsamd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([str(tmp_path / "use")], check=True)
    pkg = os.path.join(ROOT, "nerfstudio_amd")
    for name in NAMES:
        sites = [f for f in os.listdir(pkg) if f.endswith(".py") and f != "_native.py" and f".{name}(" in open(os.path.join(pkg, f)).read()]
        assert sites == ["functional.py"], name
    makefile = open(os.path.join(pkg, "csrc", "Makefile")).read()
    assert " pointcloud.hip" in makefile and " pointcloud.h " in makefile and "nsamd_pointcloud.h" in makefile


def test_entry_points_validate_before_they_launch():
    """No call here reaches a launch: every one fails a check or has nothing to do (the pointers are host memory)."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    p = torch.zeros(64, dtype=torch.int64).data_ptr()
    box, grid = N.make_crop_box(), N.make_point_grid([0, 0, 0], 1.0, [2, 2, 2])

    def select(n=4, cap=4, cursor=p, scratch=p, origins=p, normals=(None, None), box=box):
        return lib.nsamd_points_select(origins, p, p, p, None, normals[0], n, box, p, p, p, normals[1], cap, cursor, scratch, None)

    assert select(n=0) == 0 and select(n=0, cursor=None, origins=None) == 0
    for bad in (dict(n=-1), dict(cap=-1), dict(cursor=None), dict(scratch=None), dict(origins=None), dict(normals=(p, None)),
                dict(normals=(None, p)), dict(box=N.make_crop_box([0.0] * 12, [1.0, -1.0, 1.0]))):
        assert select(**bad) == -1, bad
    assert select(n=2 ** 31) == -2 and select(cap=2 ** 40 + 1) == -2

    def knn(n=4, k=3, rings=1, grid=grid, points=p, avg=p):
        return lib.nsamd_knn_mean_distance(points, n, p, p, grid, k, rings, avg, p, None)

    assert knn(n=0) == 0 and knn(n=0, points=None) == 0
    for bad in (dict(n=-1), dict(k=0), dict(rings=-1), dict(points=None), dict(avg=None),
                dict(grid=N.make_point_grid([0, 0, 0], 0.0, [2, 2, 2])), dict(grid=N.make_point_grid([0, 0, 0], 1.0, [2, 0, 2])),
                dict(grid=N.make_point_grid([0, float("nan"), 0], 1.0, [2, 2, 2]))):
        assert knn(**bad) == -1, bad
    assert knn(k=33) == -2 and knn(n=2 ** 31) == -2 and knn(grid=N.make_point_grid([0, 0, 0], 1.0, [4096, 4096, 2])) == -2
    assert lib.nsamd_point_cell_keys(p, 0, grid, p, None) == 0 and lib.nsamd_point_cell_keys(None, 3, grid, p, None) == -1
    assert lib.nsamd_point_cell_keys(p, 3, N.make_point_grid([0, 0, 0], -1.0, [2, 2, 2]), p, None) == -1
    assert lib.nsamd_select_below(None, 3, p, p, p, p, None) == -1 and lib.nsamd_select_below(p, 3, p, p, None, p, None) == -1
    assert lib.nsamd_select_below(p, 2 ** 31, p, p, p, p, None) == -2
    with pytest.raises(RuntimeError, match="status -2"):
        N.check(knn(k=33), "knn_mean_distance")
