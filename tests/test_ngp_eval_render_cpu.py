"""The instant-ngp eval render (nerfstudio_amd/ngp_eval_render.py, include/nsamd_render.h) where no GPU is present:

* the ABI: header, library and `_native._RENDER_SIGNATURES` agree on exactly nsamd_packed_render_fwd and nsamd_packed_ray_points;
* the argument checks of the two entry points, called directly (every call returns before any HIP call);
* NgpEvalRenderer's HOST logic over a stand-in `launches` built from oracle/packed_oracle.py and tests/cpu_kernels.py: launch
  order per chunk with and without prefetch, slot alternation, the short last chunk, growth from a tiny candidate capacity, an
  all-empty occupancy grid, outputs against the module path on the same stand-ins;
* fallbacks and wiring: `supported`'s reasons, `runner_for`'s rules, both model classes' overrides, export.fuse_views.
"""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import cpu_kernels
from oracle import packed_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDER_HEADER = os.path.join(ROOT, "include", "nsamd_render.h")
NAMES = ["nsamd_packed_ray_points", "nsamd_packed_render_fwd"]
H, W, CHUNK = 33, 40, 256  # 1320 rays: five full chunks and one of 40


# ---------------------------------------------------------------- the ABI --------------------------------------------------
def test_render_header_library_and_binding_agree(tmp_path):
    from nerfstudio_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(RENDER_HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(nsamd_[a-z0-9_]+)\s*\(", header))) == sorted(N._RENDER_SIGNATURES) == NAMES
    assert not set(N._RENDER_SIGNATURES) & (set(N._SIGNATURES) | set(N._EXPORT_SIGNATURES))
    cdll, lib = C.CDLL(N.LIB_PATH), N.load()
    for name in NAMES:
        assert hasattr(cdll, name) and callable(getattr(lib, name))
    vp = N.vp
    assert N._RENDER_SIGNATURES["nsamd_packed_render_fwd"] == [vp, vp, vp, vp, vp, N.i64, C.c_int, C.POINTER(N.f32), C.c_int, vp, vp,
                                                               vp, vp, vp, vp]
    assert N._RENDER_SIGNATURES["nsamd_packed_ray_points"] == [vp, vp, vp, vp, vp, N.i64, vp, vp, vp]
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", RENDER_HEADER], check=True)
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "nsamd_render.h"\n'
                   "int main(void) {\n"
                   "  if (nsamd_packed_render_fwd(NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL)"
                   " != NSAMD_OK) return 1;\n"
                   "  if (nsamd_packed_render_fwd(NULL, NULL, NULL, NULL, NULL, 3, 0, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL)"
                   " != NSAMD_ERR_INVALID_ARG) return 2;\n"
                   "  if (nsamd_packed_ray_points(NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL) != NSAMD_OK) return 3;\n"
                   "  if (nsamd_packed_ray_points(NULL, NULL, NULL, NULL, NULL, 3, NULL, NULL, NULL) != NSAMD_ERR_INVALID_ARG)"
                   " return 4;\n"
                   "  return 0;\n}\n")
    libdir = os.path.dirname(N.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.dirname(RENDER_HEADER), str(src), "-o", str(tmp_path / "use"), "-L", libdir,
                    "-lnsamd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([str(tmp_path / "use")], check=True)
    # each entry point is referenced once in the package: its launch helper in functional.py
    pkg = os.path.join(ROOT, "nerfstudio_amd")
    for name in NAMES:
        sites = [f for f in sorted(os.listdir(pkg)) if f.endswith(".py") and f != "_native.py"
                 and f".{name}(" in open(os.path.join(pkg, f)).read()]
        assert sites == ["functional.py"], (name, sites)
    makefile = open(os.path.join(pkg, "csrc", "Makefile")).read()
    assert "nsamd_render.h" in makefile


def test_entry_points_validate_before_they_launch():
    """No call here reaches a launch: every one fails a check or has nothing to do (the pointers are host memory)."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    p = torch.zeros(64).data_ptr()
    bg = (C.c_float * 3)(0.25, 0.5, 0.75)

    def render(ts=p, te=p, sig=p, rgb=p, info=p, n=4, mode=0, bgv=None, ev=1, o_rgb=p, o_acc=p, o_dep=p, lo=p, hi=p):
        return lib.nsamd_packed_render_fwd(ts, te, sig, rgb, info, n, mode, bgv, ev, o_rgb, o_acc, o_dep, lo, hi, None)

    assert render(n=0) == 0 and render(n=0, ts=None, o_rgb=None, lo=None, hi=None) == 0
    for bad in (dict(ts=None), dict(te=None), dict(sig=None), dict(rgb=None), dict(info=None), dict(o_rgb=None), dict(o_acc=None),
                dict(o_dep=None), dict(n=-1), dict(mode=2), dict(mode=-1), dict(mode=1, bgv=None), dict(lo=None), dict(hi=None),
                dict(n=0, lo=None), dict(n=0, mode=3)):
        assert render(**bad) == -1, bad
    assert render(n=0, mode=1, bgv=bg) == 0
    assert render(n=4 * (2**31 - 1) + 1) == -2  # more workgroups than a launch grid holds
    with pytest.raises(RuntimeError, match="status -1"):
        N.check(render(sig=None), "packed_render_fwd")

    def points(o=p, d=p, ri=p, ts=p, te=p, n=5, pos=p, dirs=p):
        return lib.nsamd_packed_ray_points(o, d, ri, ts, te, n, pos, dirs, None)

    assert points(n=0) == 0 and points(n=0, o=None, pos=None) == 0
    for bad in (dict(o=None), dict(d=None), dict(ri=None), dict(ts=None), dict(te=None), dict(pos=None), dict(dirs=None), dict(n=-1)):
        assert points(**bad) == -1, bad
    assert points(n=256 * (2**31 - 1) + 1) == -2


# ---------------------------------------------------------------- the runner's host logic ------------------------------------
class CpuLaunches:
    """DeviceLaunches' methods from the oracle's restatements (the functions tests/cpu_kernels.py puts under the module path), with
    a log of (name, the address of the per-ray buffer or the event that tells the slot | the sample count, the ray count)."""

    def __init__(self):
        self.log, self._march = [], {}

    def host_word(self):
        return torch.zeros(1, dtype=torch.int64)

    def event(self):
        return object()

    def raygen(self, *a):
        raise AssertionError("the CPU tests render bundles")

    def _run_march(self, o, d, t_min, t_max, n, near, far, grid, step, cone):
        ri, ts, te = po.occgrid_march(o.numpy(), d.numpy(), grid.binaries.numpy().astype(bool), list(grid._roi), step, near_plane=near,
                                      far_plane=far, t_min=None if t_min is None else t_min.numpy(),
                                      t_max=None if t_max is None else t_max.numpy(), cone_angle=cone)
        return torch.from_numpy(ri).to(torch.int64), torch.from_numpy(ts), torch.from_numpy(te)

    def march_count(self, o, d, t_min, t_max, n, near, far, grid, step, cone, counts, stash):
        assert o.shape == (n, 3) and counts.shape == (n,) and stash.shape[0] == n
        self.log.append(("count", o.data_ptr(), n))
        res = self._run_march(o, d, t_min, t_max, n, near, far, grid, step, cone)
        self._march[o.data_ptr()] = res
        counts.copy_(torch.bincount(res[0], minlength=n))

    def packed_info(self, counts, n, info, total):
        self.log.append(("info", counts.data_ptr(), n))
        c = counts[:n].to(torch.int64)
        info[:n, 0], info[:n, 1] = torch.cumsum(c, 0) - c, c
        total[0] = c.sum()

    def total_copy(self, total, host, event):
        self.log.append(("copy", id(event)))
        host.copy_(total)

    def total_read(self, host, event):
        self.log.append(("read", id(event)))
        return int(host[0])

    def march_write(self, o, d, t_min, t_max, n, near, far, grid, step, cone, info, stash, ri, ts, te):
        self.log.append(("write", o.data_ptr(), n))
        res = self._march[o.data_ptr()]
        m = res[0].numel()
        assert m <= ri.numel(), "the candidate buffers were not grown"
        ri[:m], ts[:m], te[:m] = res

    def ray_points(self, o, d, ri, ts, te, m, pos, dirs):
        self.log.append(("points", o.data_ptr(), m))
        pos[:m] = cpu_kernels.packed_positions(o, d, ri[:m], ts[:m], te[:m])
        dirs[:m] = d[ri[:m]]

    def field(self, fld, pos, m, enc, sel, dirs, app_const, density, rgb):
        self.log.append(("field", m))
        from nerfstudio_amd import functional as F

        tbl = fld.mlp_base.encoding
        emb = fld.embedding_appearance.embedding.weight if fld.embedding_appearance is not None else None
        with torch.no_grad():
            dn, col = cpu_kernels.nerfacto_field(F.PointSpec(positions=pos[:m]), tbl.hash_table, fld.mlp_base.mlp.param_tensors(),
                                                 fld.mlp_head.param_tensors(), emb, dirs[:m], None, app_const, 1, tbl.spec,
                                                 fld._transform, fld._box, fld.average_init_density)
        density[:m], rgb[:m] = dn, col

    def render(self, ts, te, sig, rgb, info, n, bg_mode, bg_vals, out_rgb, acc, depth, mid_lo, mid_hi):
        self.log.append(("render", info.data_ptr(), n))
        info = info[:n]
        m = int(info[:, 1].sum())
        ri = cpu_kernels._ray_indices_of(info)
        bg = "random" if bg_mode == 0 else {0.0: "black", 1.0: "white"}[float(bg_vals[0])]
        w = cpu_kernels.packed_weights(sig[:m], ts[:m], te[:m], info)
        c, a, dep = cpu_kernels.packed_composite(rgb[:m], w, ri, info, ts[:m], te[:m], bg, eval_mode=True)
        out_rgb.copy_(c), acc.copy_(a), depth.copy_(dep)
        mid = (ts[:m] + te[:m]) / 2
        mid_lo.copy_(torch.full((n,), float("inf")).scatter_reduce(0, ri, mid, "amin"))
        mid_hi.copy_(torch.full((n,), float("-inf")).scatter_reduce(0, ri, mid, "amax"))


def _model(background="white", blob=True, **cfg):
    from nerfstudio_amd.instant_ngp import InstantNGPModelConfig, NGPModel
    from oracle import nerfacto_oracle as orc

    ocfg = orc.NerfactoCfg(main_grid=orc.HashGridCfg(16, 16, 2048, 10), prop_grids=(), num_images=4, average_init_density=1.0)
    params = orc.init_params(ocfg, seed=45, table_std=0.5)
    mc = InstantNGPModelConfig(grid_resolution=16, grid_levels=2, log2_hashmap_size=10, background_color=background, cone_angle=0.004,
                               render_step_size=0.05, eval_num_rays_per_chunk=CHUNK, **cfg)
    model = NGPModel(mc, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4)
    own = model.state_dict()  # (a model without the embedding keeps its own, narrower first head layer)
    model.load_state_dict({k: v.clone() for k, v in params.items() if k.startswith("field.") and k in own and own[k].shape == v.shape},
                          strict=False)
    if blob:  # a blob of occupied cells off the centre, and one of the coarse level between it and the camera
        g = torch.stack(torch.meshgrid(*[torch.arange(16.0)] * 3, indexing="ij"), dim=-1)
        model.occupancy_grid.binaries[0] = ((g - torch.tensor([9.0, 7.0, 8.0])).norm(dim=-1) < 4.5).to(torch.uint8)
        model.occupancy_grid.binaries[1] = ((g - torch.tensor([10.0, 8.0, 13.0])).norm(dim=-1) < 1.6).to(torch.uint8)
    return model.eval()


def _frame(with_bounds=False):
    """A 40 x 33 pinhole frame looking at the blob from outside the finest level."""
    from nerfstudio_amd.cameras.rays import RayBundle

    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = torch.stack([(xs + 0.5 - W / 2) / 45.0, -(ys + 0.5 - H / 2) / 45.0, -torch.ones_like(xs)], dim=-1)
    d = d / d.norm(dim=-1, keepdim=True)
    o = torch.tensor([0.1, -0.05, 1.7]).expand(H, W, 3).contiguous()
    kw = {}
    if with_bounds:
        g = torch.Generator().manual_seed(3)
        kw["nears"] = 0.9 + 0.5 * torch.rand(H, W, 1, generator=g)
        kw["fars"] = kw["nears"] + 0.3 + 0.8 * torch.rand(H, W, 1, generator=g)
    return RayBundle(origins=o, directions=d.contiguous(), pixel_area=torch.full((H, W, 1), 1e-6),
                     camera_indices=torch.zeros(H, W, 1, dtype=torch.long), **kw)


def _runner(model, **kw):
    from nerfstudio_amd.ngp_eval_render import NgpEvalRenderer

    return NgpEvalRenderer(model, launches=CpuLaunches(), **kw)


def _equal(a, b):
    assert sorted(a) == sorted(b) == ["accumulation", "depth", "num_samples_per_ray", "rgb"]
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _chunk_of(runner, entry):
    """Which slot a logged launch used (its origins / counts / info buffer or its event)."""
    for i, s in enumerate(runner.slots):
        if entry[1] in (s.origins.data_ptr(), s.counts.data_ptr(), s.info.data_ptr(), id(s.event)):
            return i
    raise AssertionError(entry)


def test_runner_launch_order_slots_and_short_last_chunk():
    model = _model()
    frame = _frame()
    on, off = _runner(model, prefetch=True), _runner(model, prefetch=False)
    out_on, out_off = on.render(frame), off.render(frame)
    _equal(out_on, out_off)  # the double buffering changes no bit
    sizes = [CHUNK] * 5 + [40]
    head, tail = ["count", "info", "copy"], ["write", "points", "field", "render"]
    # without prefetch: count, prefix, copy, read, then the chunk's launches, strictly in turn
    names = [e[0] for e in off.launches.log]
    assert names == (head + ["read"] + tail) * 6
    # with prefetch: chunk c + 1's count pass, prefix and copy sit between chunk c's read and chunk c's launches
    names = [e[0] for e in on.launches.log]
    assert names == head + (["read"] + head + tail) * 5 + ["read"] + tail
    for r in (on, off):
        log = r.launches.log
        slot = {name: [_chunk_of(r, e) for e in log if e[0] == name] for name in ("count", "info", "copy", "read", "write", "render")}
        for name, used in slot.items():
            assert used == [0, 1, 0, 1, 0, 1], name  # chunk c lives in slot c & 1, for every launch that names a per-ray array
        for name in ("count", "write", "render"):
            assert [e[2] for e in log if e[0] == name] == sizes, name  # the ray count of every launch: 256 x 5, then 40
        reads = [e for e in log if e[0] == "read"]
        copies = [e for e in log if e[0] == "copy"]
        assert [e[1] for e in reads] == [e[1] for e in copies]  # each read waits for its own chunk's event
    # the sample counts the launches took by value are the frame's
    per_chunk = out_on["num_samples_per_ray"].reshape(-1).split(CHUNK)
    assert [e[1] for e in on.launches.log if e[0] == "field"] == [int(c.sum()) for c in per_chunk]
    assert all(int(c.sum()) > 0 for c in per_chunk) and out_on["num_samples_per_ray"].dtype == torch.int64
    assert out_on["rgb"].shape == (H, W, 3) and out_on["depth"].shape == (H, W, 1)
    # a second frame through the same runner: the same bits, no growth
    _equal(on.render(frame), out_on)
    assert on.grown == 0


def test_runner_grows_from_a_tiny_capacity():
    model = _model()
    frame = _frame()
    ample, tiny = _runner(model), _runner(model, cap_candidates=8)
    assert tiny.cap_c == 8
    out = tiny.render(frame)
    most = max(e[1] for e in tiny.launches.log if e[0] == "field")
    assert most > 8 and tiny.cap_c >= most and 1 <= tiny.grown <= 6
    assert tiny.c_enc.numel() == 32 * tiny.cap_c and tiny.c_rgb.shape == (tiny.cap_c, 3)
    _equal(out, ample.render(frame))
    assert ample.grown == 0


@pytest.mark.parametrize("background", ["white", "random"])
def test_runner_all_empty_grid_takes_the_fake_sample(background):
    """No candidate in any chunk: the reference's fake sample (ray 0, [1, 1]) through the same launches with ONE sample —
    num_samples_per_ray 1 on each chunk's first ray, depth 1 (the clip range is [1, 1]), rgb = the background."""
    model = _model(background=background, blob=False)
    r = _runner(model)
    out = r.render(_frame())
    names = [e[0] for e in r.launches.log]
    assert "write" not in names and names.count("render") == 6
    assert [e[1] for e in r.launches.log if e[0] == "field"] == [1] * 6
    expect = torch.zeros(H * W, dtype=torch.int64)
    expect[::CHUNK] = 1
    assert torch.equal(out["num_samples_per_ray"].reshape(-1), expect)
    assert torch.equal(out["depth"], torch.ones(H, W, 1))
    nspr = out["num_samples_per_ray"].reshape(-1)
    rgb, acc = out["rgb"].reshape(-1, 3), out["accumulation"].reshape(-1)
    assert torch.equal(acc[nspr == 0], torch.zeros(int((nspr == 0).sum())))
    assert torch.equal(rgb[nspr == 0], torch.full((int((nspr == 0).sum()), 3), 1.0 if background == "white" else 0.0))
    assert torch.equal(acc[nspr == 1], torch.zeros(6))  # an interval of length 0 carries no weight


@pytest.mark.parametrize("case", ["white", "random", "bounds", "average_appearance", "no_embedding"])
def test_runner_equals_the_module_path_on_the_same_stand_ins(monkeypatch, case):
    model = _model(background="random" if case == "random" else "white", use_appearance_embedding=case == "no_embedding")
    assert (model.field.embedding_appearance is None) == (case == "no_embedding")  # (sic) 32 wide when the flag is False
    if case == "average_appearance":
        model.field.use_average_appearance_embedding = True
    frame = _frame(with_bounds=case == "bounds")
    r = _runner(model)
    out = r.render(frame)
    assert (r.app_const is None) == (case == "no_embedding")
    if case == "average_appearance":
        assert torch.equal(r.app_const, model.field.embedding_appearance.embedding.weight.mean(dim=0)) and bool(r.app_const.any())
    with cpu_kernels.installed(monkeypatch):
        ref = model.get_outputs_for_camera_ray_bundle(frame)  # (CPU: runner_for gives None — the Python loop over forward)
    assert torch.equal(out["num_samples_per_ray"].reshape(-1), ref["num_samples_per_ray"].reshape(-1))
    assert int(ref["num_samples_per_ray"].sum()) > 2000
    # the same restatements under both routes: what may differ is the order of two fp32 roundings in the position
    np.testing.assert_allclose(out["rgb"].numpy(), ref["rgb"].numpy(), atol=2e-6)
    np.testing.assert_allclose(out["accumulation"].numpy(), ref["accumulation"].numpy(), atol=2e-6)
    np.testing.assert_allclose(out["depth"].numpy(), ref["depth"].numpy(), rtol=1e-5, atol=1e-6)
    if case == "bounds":
        free = _runner(model).render(_frame())
        assert not torch.equal(free["num_samples_per_ray"], out["num_samples_per_ray"])  # the interval matters on this frame


# ---------------------------------------------------------------- fallbacks and wiring -----------------------------------------
def test_supported_names_every_reason():
    from nerfstudio_amd import eval_render, ngp_eval_render
    from nerfstudio_amd.ngp_eval_render import NgpEvalRenderer

    model = _model()
    assert ngp_eval_render.supported(model) is None
    assert eval_render.supported(model) == "not a nerfacto model"  # (unchanged: export's error for other models quotes it)
    for missing in ("occupancy_grid", "sampler", "field"):
        stub = types.SimpleNamespace(**{a: getattr(model, a) for a in ("occupancy_grid", "sampler", "field") if a != missing})
        assert ngp_eval_render.supported(stub) == "not an instant-ngp model"
    spec = model.field.mlp_base.encoding.spec
    for levels, dim in ((8, 16), (16, 64)):
        fake = types.SimpleNamespace(mlp_base=types.SimpleNamespace(encoding=types.SimpleNamespace(
            spec=types.SimpleNamespace(num_levels=levels, out_dim=dim))))
        stub = types.SimpleNamespace(occupancy_grid=model.occupancy_grid, sampler=model.sampler, field=fake)
        assert ngp_eval_render.supported(stub) == "the main-field kernels take 16 levels x 2 features"
    assert (spec.num_levels, spec.out_dim) == (16, 32)
    model.renderer_rgb.background_color = "last_sample"
    assert ngp_eval_render.supported(model) == "background last_sample is not implemented for packed samples"
    with pytest.raises(ValueError, match="last_sample"):
        NgpEvalRenderer(model, launches=CpuLaunches())


def test_runner_for_rules(monkeypatch):
    from nerfstudio_amd import ngp_eval_render

    model = _model()
    made = []
    monkeypatch.setattr(ngp_eval_render, "NgpEvalRenderer", lambda m: made.append(m) or types.SimpleNamespace(chunk=m.config.eval_num_rays_per_chunk))
    assert ngp_eval_render.runner_for(model, "cpu") is None and ngp_eval_render.runner_for(model, torch.device("cpu")) is None
    first = ngp_eval_render.runner_for(model, "cuda:0")  # (the device of the RAYS decides; nothing is launched here)
    assert first is not None and ngp_eval_render.runner_for(model, torch.device("cuda", 0)) is first and len(made) == 1
    assert model._ngp_eval_runner is first
    model.config.eval_num_rays_per_chunk = 512
    assert ngp_eval_render.runner_for(model, "cuda:0") is not first and len(made) == 2  # rebuilt for the new chunk size
    model.train()
    assert ngp_eval_render.runner_for(model, "cuda:0") is None
    model.eval()
    monkeypatch.setenv("NSAMD_EVAL_RUNNER", "0")
    assert ngp_eval_render.runner_for(model, "cuda:0") is None
    monkeypatch.delenv("NSAMD_EVAL_RUNNER")
    model.renderer_rgb.background_color = "last_sample"
    assert ngp_eval_render.runner_for(model, "cuda:0") is None and len(made) == 2


class _StubRunner:
    chunk = CHUNK

    def __init__(self):
        self.calls = []

    def render(self, bundle):
        self.calls.append(("render", bundle))
        return {"rgb": "from the runner"}

    def render_camera(self, *args, lens=None):
        self.calls.append(("render_camera", args, lens))
        h, w = args[5], args[6]
        return {"rgb": torch.full((h, w, 3), 0.5), "depth": torch.full((h, w, 1), 2.0), "accumulation": torch.ones(h, w, 1),
                "num_samples_per_ray": torch.ones(h, w, 1, dtype=torch.int64)}


def _camera(**kw):
    c2w = torch.eye(4)[:3]
    base = dict(camera_to_worlds=c2w, fx=torch.tensor([45.0]), fy=torch.tensor([45.0]), cx=torch.tensor([W / 2]), cy=torch.tensor([H / 2]),
                height=torch.tensor([H]), width=torch.tensor([W]), camera_type=torch.tensor([1]), distortion_params=None)
    base.update(kw)
    cam = types.SimpleNamespace(**base)
    cam.generated = []

    def generate_rays(camera_indices, keep_shape, obb_box=None):
        cam.generated.append((camera_indices, keep_shape, obb_box))
        return _frame()

    cam.generate_rays = generate_rays
    return cam


def test_ngp_model_falls_back_on_cpu_and_takes_a_cached_runner(monkeypatch):
    from nerfstudio_amd import ngp_eval_render

    model = _model()
    frame = _frame()
    with cpu_kernels.installed(monkeypatch):
        loop = model.get_outputs_for_camera_ray_bundle(frame)  # CPU: today's loop
        cam = _camera()
        via_camera = model.get_outputs_for_camera(cam)
    assert cam.generated == [(0, True, None)] and loop["rgb"].shape == (H, W, 3)
    _equal(loop, via_camera)
    assert getattr(model, "_ngp_eval_runner", None) is None
    # a runner cached on the model is what both entry points use once `runner_for` hands it out (its device rule aside)
    stub = model._ngp_eval_runner = _StubRunner()
    monkeypatch.setattr(ngp_eval_render, "runner_for", lambda m, dev: None if m.training else m._ngp_eval_runner)
    assert model.get_outputs_for_camera_ray_bundle(frame) == {"rgb": "from the runner"} and stub.calls[-1] == ("render", frame)
    out = model.get_outputs_for_camera(cam)
    name, args, lens = stub.calls[-1]
    assert name == "render_camera" and lens is None and args[1:] == (45.0, 45.0, W / 2, H / 2, H, W) and out["rgb"].shape == (H, W, 3)
    assert len(cam.generated) == 1  # no bundle was generated
    # a crop box keeps generate_rays; its bundle goes through `render`
    box = object()
    assert model.get_outputs_for_camera(cam, obb_box=box) == {"rgb": "from the runner"}
    assert cam.generated[-1] == (0, True, box) and stub.calls[-1][0] == "render"
    # a distorted perspective camera is generated in the loop too, through the lens generator
    dist = torch.tensor([0.1, 0.01, 0.0, 0.0, 0.001, 0.002])
    model.get_outputs_for_camera(_camera(distortion_params=dist))
    assert stub.calls[-1][0] == "render_camera" and stub.calls[-1][2][0] == 1 and torch.equal(stub.calls[-1][2][1], dist)
    model.train()
    with cpu_kernels.installed(monkeypatch):
        assert model.get_outputs_for_camera_ray_bundle(frame)["rgb"].shape == (H, W, 3)  # training mode: the loop
    assert stub.calls[-1][0] == "render_camera"


def test_plugin_model_overrides_fall_back_and_take_a_cached_runner(monkeypatch):
    """plugin.HipNGPModel's two overrides are plugin.ngp_outputs_for_camera[_ray_bundle] over the reference's base methods
    (`reference_path`): flush hook first, the reference's own path on CPU / with a collider / for rays on another device."""
    from nerfstudio_amd import ngp_eval_render, plugin

    model = _model()
    flushed, ref_calls = [], []
    object.__setattr__(model, "_hip_flush", lambda: flushed.append(1))
    model.device = torch.device("cpu")
    frame, cam = _frame(), _camera()
    ref_bundle = lambda b: ref_calls.append(("bundle", b)) or "reference loop"  # noqa: E731
    ref_camera = lambda c, obb_box=None: ref_calls.append(("camera", c, obb_box)) or "reference camera"  # noqa: E731
    assert plugin.ngp_outputs_for_camera_ray_bundle(model, frame, ref_bundle) == "reference loop"
    assert plugin.ngp_outputs_for_camera(model, cam, None, ref_camera) == "reference camera"
    assert len(flushed) == 2 and ref_calls == [("bundle", frame), ("camera", cam, None)]
    stub = model._ngp_eval_runner = _StubRunner()
    monkeypatch.setattr(ngp_eval_render, "runner_for", lambda m, dev: m._ngp_eval_runner)
    assert plugin.ngp_outputs_for_camera_ray_bundle(model, frame, ref_bundle) == {"rgb": "from the runner"}
    assert plugin.ngp_outputs_for_camera(model, cam, None, ref_camera)["depth"].shape == (H, W, 1) and stub.calls[-1][0] == "render_camera"
    box = object()
    assert plugin.ngp_outputs_for_camera(model, cam, box, ref_camera) == "reference camera" and ref_calls[-1] == ("camera", cam, box)
    fisheye = _camera(camera_type=torch.tensor([2]))
    assert plugin.ngp_outputs_for_camera(model, fisheye, None, ref_camera) == "reference camera"
    assert len(flushed) == 6 and len(stub.calls) == 2
    model.collider = object()  # Model.forward would put its nears / fars on every chunk: the reference's own loop
    assert plugin.ngp_outputs_for_camera_ray_bundle(model, frame, ref_bundle) == "reference loop"
    model.collider = None
    model.device = torch.device("meta")  # rays on another device than the model
    assert plugin.ngp_outputs_for_camera_ray_bundle(model, frame, ref_bundle) == "reference loop"
    assert len(stub.calls) == 2


def test_fuse_views_renders_an_ngp_model_through_its_runner(monkeypatch):
    from nerfstudio_amd import eval_render, export, ngp_eval_render
    from nerfstudio_amd import _native as N

    model = _model().train()
    stub = _StubRunner()
    seen = []
    monkeypatch.setattr(ngp_eval_render, "runner_for", lambda m, dev: seen.append((m.training, dev)) or stub)
    monkeypatch.setattr(eval_render, "runner_for", lambda m, dev: pytest.fail("an instant-ngp model renders through its own runner"))
    monkeypatch.setattr(N, "require_cuda", lambda *t: None)
    cams = types.SimpleNamespace(camera_to_worlds=torch.eye(4)[:3].expand(3, 3, 4).clone(), fx=torch.full((3, 1), 90.0),
                                 fy=torch.full((3, 1), 90.0), cx=torch.full((3, 1), float(W)), cy=torch.full((3, 1), float(H)),
                                 height=torch.full((3, 1), 2 * H), width=torch.full((3, 1), 2 * W), camera_type=torch.ones(3, 1))
    cams.camera_to_worlds[:, 2, 3] = torch.tensor([0.0, 0.1, 0.2])
    volume = export.TSDFVolume.from_aabb(torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), [4, 4, 4])
    integrated = []
    monkeypatch.setattr(volume, "integrate", lambda c2w, K, depth, color: integrated.append((c2w.clone(), K.clone(), depth.clone(), color.clone())))
    assert export.fuse_views(model, cams, volume, downscale_factor=2, views_per_launch=2) == 2
    assert seen == [(False, volume.device)] and model.training  # asked once, in eval mode; the mode is restored
    assert [c[0] for c in stub.calls] == ["render_camera"] * 3
    for i, (_, args, lens) in enumerate(stub.calls):
        assert lens is None and args[1:] == (45.0, 45.0, W / 2, H / 2, H, W) and torch.equal(args[0], cams.camera_to_worlds[i])
    assert [v[2].shape[0] for v in integrated] == [2, 1]
    assert torch.equal(integrated[0][2], torch.full((2, H, W), 2.0)) and torch.equal(integrated[0][3], torch.full((2, H, W, 3), 0.5))
    # every other model keeps today's path and today's error
    other = types.SimpleNamespace(config=types.SimpleNamespace(), training=False, eval=lambda: None, train=lambda mode=True: None)
    with pytest.raises(ValueError, match="not a nerfacto model"):
        export.fuse_views(other, cams, volume)
