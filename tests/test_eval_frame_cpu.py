"""CPU tests of nerfstudio_amd/eval_frame.py — what surrounds the two device-side eval chunk loops — and of the one PLY writer.

* the dispatch of the four pairs of model entry points (get_outputs_for_camera / get_outputs_for_camera_ray_bundle of the two
  models of this package and of the two plugin models) over stub models and a stub runner: the expected paths below are written
  down from the entry points as they stood before eval_frame existed (commit 795d331), not produced by running this code;
* `runner_enabled` and what both `runner_for` do with it;
* the padding of a short last chunk in EvalRenderer.render; the eval appearance row;
* the bytes of both PLY files against digests of the files commit 795d331 wrote.
"""
import hashlib
import types

import pytest
import torch

from nerfstudio_amd import eval_frame, eval_render, ngp_eval_render, plugin
from nerfstudio_amd.cameras.rays import RayBundle

H, W, CHUNK = 5, 9, 16  # 45 rays: the module loop runs `forward` three times
DIST = torch.tensor([0.1, 0.01, 0.0, 0.0, 0.001, 0.002])
LOOP = ["forward"] * 3


def _bundle(device="cpu"):
    o = torch.arange(H * W * 3, dtype=torch.float32, device=device).view(H, W, 3)
    return RayBundle(origins=o, directions=o + 1, pixel_area=torch.ones(H, W, 1, device=device))


def _camera(events, n=1, **kw):
    base = dict(camera_to_worlds=torch.eye(4)[None, :3].repeat(n, 1, 1), fx=torch.full((n, 1), 45.0), fy=torch.full((n, 1), 44.0),
                cx=torch.full((n, 1), W / 2), cy=torch.full((n, 1), H / 2), height=torch.full((n, 1), H), width=torch.full((n, 1), W),
                camera_type=torch.ones(n, 1, dtype=torch.int64), distortion_params=None)
    base.update(kw)
    cam = types.SimpleNamespace(**base)

    def generate_rays(camera_indices, keep_shape, obb_box=None):
        events.append(("generate_rays", camera_indices, keep_shape, obb_box))
        return _bundle()

    cam.generate_rays = generate_rays
    return cam


class _Runner:
    def __init__(self, events):
        self.events = events

    def render_camera(self, c2w, fx, fy, cx, cy, height, width, lens=None):
        assert (fx, fy, cx, cy, height, width) == (45.0, 44.0, W / 2, H / 2, H, W) and torch.equal(c2w, torch.eye(4)[:3])
        self.events.append(("render_camera", lens if lens is None else (lens[0], lens[1].tolist())))
        return "a frame from render_camera"

    def render(self, bundle):
        self.events.append("render")
        return "a frame from render"


@pytest.fixture()
def harness(monkeypatch):
    """events: what ran, in order; asked: the calls of the patched `runner_for` of both renderer modules, which hands out the
    stub runner while `on`; reads: the calls of the camera reader. take() -> (events, times asked, times read) since the last one."""
    h = types.SimpleNamespace(events=[], asked=[], reads=[], on=True)
    h.runner = _Runner(h.events)

    def runner_for(model, device):
        assert torch.device(device) == torch.device("cpu")  # the stub models' and their bundles' device
        h.asked.append(model)
        return h.runner if h.on else None

    monkeypatch.setattr(eval_render, "runner_for", runner_for)
    monkeypatch.setattr(ngp_eval_render, "runner_for", runner_for)
    reader = eval_frame.in_loop_camera_args
    monkeypatch.setattr(eval_frame, "in_loop_camera_args", lambda camera: h.reads.append(camera) or reader(camera))

    def take():
        got = (list(h.events), len(h.asked), len(h.reads))
        for log in (h.events, h.asked, h.reads):
            log.clear()
        return got

    h.take = take
    return h


def _cameras(events):
    """name -> (camera, crop box) of the table's rows"""
    box = object()
    return box, {"pinhole": (_camera(events), None), "distorted": (_camera(events, distortion_params=DIST[None]), None),
                 "zero distortion": (_camera(events, distortion_params=torch.zeros(1, 6)), None),
                 "fisheye": (_camera(events, camera_type=torch.full((1, 1), 2)), None), "two cameras": (_camera(events, n=2), None),
                 "crop box": (_camera(events), box)}


@pytest.mark.parametrize("kind", ["nerfacto", "ngp"])
def test_dispatch_of_the_models_of_this_package(harness, kind):
    """nerfacto.NerfactoModel / instant_ngp.NGPModel: no guard in front of `runner_for`; what the runner does not take generates
    the camera's bundle and goes through get_outputs_for_camera_ray_bundle, whose fallback is the Python loop over `forward`."""
    from nerfstudio_amd.instant_ngp import NGPModel
    from nerfstudio_amd.nerfacto import NerfactoModel

    cls = NerfactoModel if kind == "nerfacto" else NGPModel
    h = harness

    class Stub:
        config = types.SimpleNamespace(eval_num_rays_per_chunk=CHUNK)
        training = False
        get_outputs_for_camera = cls.get_outputs_for_camera
        get_outputs_for_camera_ray_bundle = cls.get_outputs_for_camera_ray_bundle

        def parameters(self):
            return iter([torch.zeros(1)])

        def forward(self, rb):
            h.events.append("forward")
            return {"rgb": rb.origins.reshape(-1, 3), "not a tensor": 1}

    model = Stub()
    box, cams = _cameras(h.events)
    gen = lambda b=None: ("generate_rays", 0, True, b)  # noqa: E731
    # (events, times runner_for was asked, times the camera was read), as commit 795d331's methods give them
    expected = {"pinhole": ([("render_camera", None)], 1, 1),
                "distorted": ([("render_camera", (1, DIST.tolist()))], 1, 1),
                "zero distortion": ([("render_camera", None)], 1, 1),
                "fisheye": ([gen(), "render"], 1, 1),      # (asked once: by the bundle method, not for the refused camera)
                "two cameras": ([gen(), "render"], 1, 1),
                "crop box": ([gen(box), "render"], 1, 0)}  # the camera is not read
    for name, (cam, obb) in cams.items():
        out = model.get_outputs_for_camera(cam, obb_box=obb)
        assert h.take() == expected[name], name
        assert out == ("a frame from render_camera" if expected[name][0][0][0] == "render_camera" else "a frame from render"), name
    assert model.get_outputs_for_camera_ray_bundle(_bundle()) == "a frame from render" and h.take() == (["render"], 1, 0)
    h.on = False  # `runner_for` gives None: the bundle route, then the Python loop
    out = model.get_outputs_for_camera(cams["pinhole"][0])
    assert h.take() == ([gen()] + LOOP, 2, 1) and torch.equal(out["rgb"], _bundle().origins) and set(out) == {"rgb"}
    out = model.get_outputs_for_camera(cams["crop box"][0], obb_box=box)
    assert h.take() == ([gen(box)] + LOOP, 1, 0) and out["rgb"].shape == (H, W, 3)
    out = model.get_outputs_for_camera_ray_bundle(_bundle())
    assert h.take() == (LOOP, 1, 0) and torch.equal(out["rgb"], _bundle().origins)


@pytest.mark.parametrize("kind", ["nerfacto", "ngp"])
def test_dispatch_of_the_plugin_models(harness, kind):
    """plugin.HipNerfactoModel / HipNGPModel, through the functions their two overrides call: the flush hook first, every time;
    then `runner_for` only behind the model's guard (rays on the model's device; a collider with the config's planes for
    nerfacto, no collider for instant-ngp); what the runner does not take is the reference's own method."""
    h = harness
    planes = types.SimpleNamespace(near_plane=0.05, far_plane=1000.0)
    model = types.SimpleNamespace(device=torch.device("cpu"), config=types.SimpleNamespace(near_plane=0.05, far_plane=1000.0),
                                  collider=planes if kind == "nerfacto" else None, training=False,
                                  _hip_flush=lambda: h.events.append("flush"))
    ref_camera = lambda cam, obb_box=None: h.events.append(("reference camera", obb_box)) or "the reference's frame"  # noqa: E731
    ref_bundle = lambda b: h.events.append("reference loop") or "the reference's frame"  # noqa: E731
    fns = ((plugin.nerfacto_outputs_for_camera, plugin.nerfacto_outputs_for_camera_ray_bundle) if kind == "nerfacto" else
           (plugin.ngp_outputs_for_camera, plugin.ngp_outputs_for_camera_ray_bundle))
    camera = lambda cam, obb: fns[0](model, cam, obb, ref_camera)  # noqa: E731
    bundle = lambda b: fns[1](model, b, ref_bundle)  # noqa: E731
    box, cams = _cameras(h.events)
    # (events, times runner_for was asked, times the camera was read). Commit 795d331 gives these events; its
    # ngp_outputs_for_camera alone also asked for the (cached) runner of a camera it then refused: no longer, as everywhere else.
    expected = {"pinhole": (["flush", ("render_camera", None)], 1, 1),
                "distorted": (["flush", ("render_camera", (1, DIST.tolist()))], 1, 1),
                "zero distortion": (["flush", ("render_camera", None)], 1, 1),
                "fisheye": (["flush", ("reference camera", None)], 0, 1),
                "two cameras": (["flush", ("reference camera", None)], 0, 1),
                "crop box": (["flush", ("reference camera", box)], 0, 0)}
    for name, (cam, obb) in cams.items():
        camera(cam, obb)
        assert h.take() == expected[name], name
    pinhole = cams["pinhole"][0]
    assert bundle(_bundle()) == "a frame from render" and h.take() == (["flush", "render"], 1, 0)
    h.on = False  # `runner_for` gives None
    assert camera(pinhole, None) == "the reference's frame" and h.take() == (["flush", ("reference camera", None)], 1, 1)
    assert bundle(_bundle()) == "the reference's frame" and h.take() == (["flush", "reference loop"], 1, 0)
    h.on = True
    # rays on another device than the model: the guard refuses before `runner_for` is asked
    assert bundle(_bundle(device="meta")) == "the reference's frame" and h.take() == (["flush", "reference loop"], 0, 0)
    # the collider: one whose planes are not the config's (nerfacto), any at all (instant-ngp)
    colliders = ([types.SimpleNamespace(near_plane=0.1, far_plane=1000.0), types.SimpleNamespace(near_plane=0.05, far_plane=6.0), None]
                 if kind == "nerfacto" else [planes, object()])
    for collider in colliders:
        model.collider = collider
        assert camera(pinhole, None) == "the reference's frame" and h.take() == (["flush", ("reference camera", None)], 0, 1)
        assert bundle(_bundle()) == "the reference's frame" and h.take() == (["flush", "reference loop"], 0, 0)
    del model._hip_flush  # a model without the hook renders all the same
    model.collider = planes if kind == "nerfacto" else None
    assert camera(pinhole, None) == "a frame from render_camera" and h.take() == ([("render_camera", None)], 1, 1)


def test_the_gate_and_both_runner_for(monkeypatch):
    model = types.SimpleNamespace(training=False)
    monkeypatch.delenv("NSAMD_EVAL_RUNNER", raising=False)
    assert eval_frame.runner_enabled(model, "cuda") and eval_frame.runner_enabled(model, torch.device("cuda", 1))
    assert not eval_frame.runner_enabled(model, "cpu") and not eval_frame.runner_enabled(model, torch.device("cpu"))
    assert not eval_frame.runner_enabled(types.SimpleNamespace(training=True), "cuda")
    monkeypatch.setenv("NSAMD_EVAL_RUNNER", "0")
    assert not eval_frame.runner_enabled(model, "cuda")
    monkeypatch.setenv("NSAMD_EVAL_RUNNER", "1")
    assert eval_frame.runner_enabled(model, "cuda")
    # both runner_for: None without looking at the model any further, nothing constructed
    built = []
    monkeypatch.setattr(eval_render, "EvalRenderer", lambda *a, **k: built.append("nerfacto"))
    monkeypatch.setattr(ngp_eval_render, "NgpEvalRenderer", lambda *a, **k: built.append("ngp"))
    for runner_for in (eval_render.runner_for, ngp_eval_render.runner_for):
        assert runner_for(model, "cpu") is None and runner_for(types.SimpleNamespace(training=True), "cuda") is None
        monkeypatch.setenv("NSAMD_EVAL_RUNNER", "0")
        assert runner_for(model, "cuda") is None
        monkeypatch.setenv("NSAMD_EVAL_RUNNER", "1")
    assert not built


@pytest.mark.parametrize("bounds", [False, True])
def test_a_short_last_chunk_is_padded_with_its_last_ray(bounds):
    """n + 7 rays at chunk n = 16 through EvalRenderer.render over a schedule that has nothing but its four input buffers: the
    last chunk leaves rows 7..15 of every buffer it loads equal to row 6; without bounds on the bundle the planes are not touched."""
    n, total = 16, 23
    step = types.SimpleNamespace(origins=torch.zeros(n, 3), directions=torch.zeros(n, 3), nears=torch.full((n,), -1.0),
                                 fars=torch.full((n,), -2.0))
    r = eval_render.EvalRenderer.__new__(eval_render.EvalRenderer)
    r.step, r.chunk, r.model = step, n, types.SimpleNamespace(config=types.SimpleNamespace(far_plane=1000.0))
    loaded = []

    def render_rays(count, dev, load_chunk):
        for a in range(0, count, n):
            load_chunk(a, min(n, count - a))
            loaded.append([t.clone() for t in (step.origins, step.directions, step.nears, step.fars)])
        return {"rgb": torch.zeros(count, 3)}

    r._render_rays = render_rays
    g = torch.Generator().manual_seed(5)
    o, d = torch.rand(total, 3, generator=g), torch.rand(total, 3, generator=g)
    nears, fars = torch.rand(total, 1, generator=g), 1 + torch.rand(total, 1, generator=g)
    kw = dict(nears=nears, fars=fars) if bounds else {}
    out = r.render(RayBundle(origins=o, directions=d, pixel_area=torch.ones(total, 1), **kw))
    assert out["rgb"].shape == (total, 3) and len(loaded) == 2
    sources = (o, d, nears[:, 0], fars[:, 0]) if bounds else (o, d)
    for buf, src in zip(loaded[0], sources):
        assert torch.equal(buf, src[:n])
    for buf, src in zip(loaded[1], sources):
        assert torch.equal(buf[:7], src[n:]) and torch.equal(buf[7:], buf[6:7].expand_as(buf[7:])) and torch.equal(buf[6], src[-1])
    if bounds:  # the planes every camera frame renders with are back
        assert (step.nears == 0).all() and (step.fars == 1000.0).all()
    else:
        assert all((c[2] == -1).all() and (c[3] == -2).all() for c in loaded) and (step.nears == -1).all() and (step.fars == -2).all()
    # the helper on its own: a full chunk is not padded, k < n is, whatever the arrays' trailing shape
    bufs = (torch.zeros(4, 3), torch.zeros(4))
    load = eval_frame.padded_loader(bufs, (o, fars[:, 0]), 4)
    load(4, 4)
    assert torch.equal(bufs[0], o[4:8]) and torch.equal(bufs[1], fars[4:8, 0])
    load(20, 3)
    assert torch.equal(bufs[0], torch.cat([o[20:23], o[22:23]])) and torch.equal(bufs[1], torch.cat([fars[20:23, 0], fars[22:23, 0]]))


def test_the_eval_appearance_row():
    emb = torch.nn.Embedding(7, 4)
    fld = types.SimpleNamespace(embedding_appearance=types.SimpleNamespace(embedding=emb), use_average_appearance_embedding=True)
    row = torch.full((4,), 9.0)
    eval_frame.eval_appearance_row(fld, row)  # (with autograd on, as a caller outside no_grad would have it)
    assert torch.equal(row, emb.weight.detach().mean(dim=0)) and not row.requires_grad and row.grad_fn is None
    fld.use_average_appearance_embedding = False
    eval_frame.eval_appearance_row(fld, row)
    assert (row == 0).all() and not row.requires_grad and row.grad_fn is None
    eval_frame.eval_appearance_row(types.SimpleNamespace(use_average_appearance_embedding=True), None)  # no embedding: no buffer


# SHA-256 of the files export.write_mesh_ply and pointcloud.PointCloud.write_ply of commit 795d331 wrote for the input below
PLY_DIGESTS = {"mesh": "113923803924af22e5b198390c7528b75562948febb842b5d4d20576e82a48ef",
               "empty mesh": "80f7b324a0f558831ca769caf853acccab085f98c8c27bf5f146b8d9e1aa1062",
               "cloud with normals": "a27e1899d21655acd3c3ae850fa21cd6c6625afe63a097fefb99d3438361acdf",
               "cloud": "30189086b5903db7e0be3e4f78fca820d1b4f22aaf9243528d2460a2fabca755"}


def test_both_ply_files_keep_their_bytes(tmp_path):
    from nerfstudio_amd.export import Mesh, write_mesh_ply
    from nerfstudio_amd.pointcloud import PointCloud

    xyz = torch.tensor([[0.0, 0.5, -1.25], [1.0, 2.0, 3.0], [-0.125, 7.5, 1e-3], [3.25, -2.0, 0.75], [1e4, -1e-4, 0.0]])
    nrm = torch.tensor([[0.0, 0.0, 1.0], [0.6, 0.0, -0.8], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.28, 0.96, 0.0]])
    # a NaN, a value below 0, one above 1, and both sides of a level's edge
    rgb = torch.tensor([[0.0, 0.5, 1.0], [float("nan"), 0.25, 0.999], [-0.5, 0.1, 0.2], [0.3, 1.5, 0.7], [1 / 255, 254.999 / 255, 0.57]])
    faces = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32)
    none = torch.zeros((0, 3))
    write_mesh_ply(Mesh(vertices=xyz, faces=faces, normals=nrm, colors=rgb), tmp_path / "mesh")
    write_mesh_ply(Mesh(vertices=none, faces=torch.zeros((0, 3), dtype=torch.int32), normals=none, colors=none), tmp_path / "empty mesh")
    PointCloud(xyz, rgb, nrm, normals=nrm).write_ply(tmp_path / "cloud with normals")
    PointCloud(xyz, rgb, nrm).write_ply(tmp_path / "cloud")
    for name, digest in PLY_DIGESTS.items():
        assert hashlib.sha256((tmp_path / name).read_bytes()).hexdigest() == digest, name
    head = (tmp_path / "mesh").read_bytes().split(b"end_header\n")[0].decode("ascii").split("\n")
    assert [line.split()[-1] for line in head if line.startswith("property")][:10] == \
        ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "alpha"]
    head = (tmp_path / "cloud with normals").read_bytes().split(b"end_header\n")[0].decode("ascii").split("\n")
    assert [line.split()[-1] for line in head if line.startswith("property")] == ["x", "y", "z", "red", "green", "blue", "nx", "ny", "nz"]
