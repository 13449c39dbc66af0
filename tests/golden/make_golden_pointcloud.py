#!/usr/bin/env python3
"""Golden fixture for point-cloud export — written by THE REFERENCE ITSELF where it can be imported (read-only import of the
reference's exporter/exporter_utils.py generate_point_cloud, torch, CPU, fp32). Authoring container only:

    python tests/golden/make_golden_pointcloud.py      ->  tests/golden/pointcloud.npz

exporter_utils imports pymeshlab, rich, the camera optimizers, the datasets and the pipelines at module level and open3d inside
the function; stand-ins go into sys.modules first (open3d's PointCloud / Vector3dVector only store arrays). The function is
driven with remove_outliers=False over a fake pipeline that replays recorded ray bundles and outputs. If that import cannot be
satisfied, the fixture falls back to the reference's own OrientedBox.within under one mask over all batches (`fallback_cloud`); `source` in the fixture says which one wrote it ("generate_point_cloud (get_rgba_image: reference|restated)" — the model's
get_rgba_image is the reference's own method where models/base_model.py can be imported, else `opacity_and_colour` — or
"within+mask").

Inputs: three batches of 257 rays (`origins`, `directions` [3,257,3], `depth`, `accumulation` [3,257,1], `rgb`, `normals`
[3,257,3] in [0,1]); `box_R`, `box_T`, `box_S`: a rotated crop box; the `face` variant uses the identity box of scale
(1, 1.5, 2), for which batch 0's ray 5 lands exactly on the face x = 0.5 and ray 6 one ulp inside it. num_points = 300 is
reached in the second batch, so every variant's cloud is the first two batches' kept rays. Per variant `<v>_points`, `<v>_colors`,
`<v>_normals` (float64, as the reference hands them to Open3D; normals only where the variant has them):
    plain           no box, no normals, the model's background is not "random" (every ray passes the opacity test)
    random          the "random" background: colour / accumulation, accumulation > 0.5
    box             random + the rotated box
    box_normals     box + normals
    reorient        box_normals + reorient_normals
    face            random + the identity box
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_refstubs"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

NUM_POINTS, BATCHES, RAYS = 300, 3, 257
USED = {"get_rgba_image": "reference"}  # whether Model.get_rgba_image itself ran or opacity_and_colour below
VARIANTS = {  # name -> (background, box, normals, reorient)
    "plain": ("last_sample", None, False, False),
    "random": ("random", None, False, False),
    "box": ("random", "rotated", False, False),
    "box_normals": ("random", "rotated", True, False),
    "reorient": ("random", "rotated", True, True),
    "face": ("random", "identity", False, False),
}


def _stub(name, **names):
    m = types.ModuleType(name)
    for k, v in names.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class _O3dPointCloud:
    def __init__(self):
        self.points = self.colors = None
        self.normals = np.zeros((0, 3))


def make_inputs():
    rs = np.random.RandomState(20)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    origins = f(rs.uniform(-0.2, 0.2, (BATCHES, RAYS, 3)))
    directions = rs.normal(size=(BATCHES, RAYS, 3))
    directions = f(directions / np.linalg.norm(directions, axis=-1, keepdims=True))
    depth = f(rs.uniform(0.05, 0.45, (BATCHES, RAYS, 1)))
    accumulation = f(np.where(rs.uniform(size=(BATCHES, RAYS, 1)) < 0.15, rs.uniform(0.0, 0.5, (BATCHES, RAYS, 1)),
                              rs.uniform(0.5, 1.0, (BATCHES, RAYS, 1))))
    accumulation[0, 9, 0] = 0.5  # not > 0.5
    rgb = f(rs.uniform(0, 1, (BATCHES, RAYS, 3)) * accumulation)
    normals = f(rs.uniform(0, 1, (BATCHES, RAYS, 3)))
    origins[0, 5:7] = 0.0
    depth[0, 5:7] = 1.0
    accumulation[0, 5:7] = 0.875
    directions[0, 5] = (0.5, 0.125, 0.25)  # exactly on the identity box's face x = 0.5
    directions[0, 6] = (np.nextafter(np.float32(0.5), np.float32(0)), 0.125, 0.25)  # one ulp inside
    a, b = 0.4, -0.3
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return dict(origins=origins, directions=directions, depth=depth, accumulation=accumulation, rgb=rgb, normals=normals,
                box_R=f(Rz @ Ry), box_T=f([0.05, -0.1, 0.02]), box_S=f([1.1, 0.9, 1.3]),
                face_R=f(np.eye(3)), face_T=f([0, 0, 0]), face_S=f([1.0, 1.5, 2.0]))


def import_reference():
    """-> (generate_point_cloud or None, OrientedBox, RayBundle)"""
    from nerfstudio.data.scene_box import OrientedBox
    from nerfstudio.cameras.rays import RayBundle
    try:
        _stub("pymeshlab")
        _stub("open3d", geometry=types.SimpleNamespace(PointCloud=_O3dPointCloud),
              utility=types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a)))
        _stub("nerfstudio.pipelines")
        _stub("nerfstudio.pipelines.base_pipeline", Pipeline=object, VanillaPipeline=object)
        _stub("nerfstudio.data.datasets")
        _stub("nerfstudio.data.datasets.base_dataset", InputDataset=object)
        _stub("nerfstudio.cameras.camera_optimizers", CameraOptimizer=object)
        from nerfstudio.exporter.exporter_utils import generate_point_cloud
        return generate_point_cloud, OrientedBox, RayBundle
    except Exception as e:  # noqa: BLE001
        print(f"generate_point_cloud cannot be imported here ({type(e).__name__}: {e}); OrientedBox.within + restatement")
        return None, OrientedBox, RayBundle


def opacity_and_colour(background, rgb, accumulation):
    """What the model's rgba image holds (models/base_model.py:216-225), as two arrays: over a "random" background the colour
    divided by the accumulation (floored at 1e-10) and the accumulation itself as opacity; otherwise the colour and opacity 1."""
    if background != "random":
        return rgb, torch.ones(rgb.shape[:-1] + (1,))
    opacity = accumulation.reshape(rgb.shape[:-1] + (1,))
    return rgb / torch.clamp(opacity, min=1e-10), opacity


def fallback_cloud(inp, background, crop_obb, with_normals, reorient):
    """Only where generate_point_cloud cannot be imported: ONE mask over all batches at once — opacity above 0.5 and the
    reference's OrientedBox.within — cut after the first batch at which the kept rays reach NUM_POINTS."""
    flat = {k: torch.from_numpy(inp[k]).reshape(BATCHES * RAYS, -1) for k in ("origins", "directions", "depth", "accumulation",
                                                                            "rgb", "normals")}
    colour, opacity = opacity_and_colour(background, flat["rgb"], flat["accumulation"])
    points = flat["origins"] + flat["directions"] * flat["depth"]
    keep = opacity[:, 0] > 0.5
    if crop_obb is not None:
        keep &= crop_obb.within(points)
    per_batch = keep.reshape(BATCHES, RAYS).sum(dim=1).cumsum(dim=0)
    keep[RAYS * (1 + int((per_batch < NUM_POINTS).sum())):] = False
    out = dict(points=points[keep].double().numpy(), colors=colour[keep].double().numpy())
    if with_normals:
        normals = (flat["normals"] * 2.0 - 1.0)[keep]
        if reorient:
            facing = (flat["directions"][keep] * normals).sum(dim=-1, keepdim=True) > 0
            normals = torch.where(facing, -normals, normals)
        out["normals"] = normals.double().numpy()
    return out


def through_reference(generate_point_cloud, RayBundle, inp, background, crop_obb, with_normals, reorient):
    calls = {"n": 0}

    def next_train(step):
        b = calls["n"]
        calls["n"] += 1
        T = lambda k: torch.from_numpy(inp[k][b])  # noqa: E731
        return RayBundle(origins=T("origins"), directions=T("directions"), pixel_area=torch.ones(RAYS, 1)), {"batch": b}

    class Model:
        renderer_rgb = types.SimpleNamespace(background_color=background)

        def __call__(self, ray_bundle):
            b = calls["n"] - 1
            return {k: torch.from_numpy(inp[k][b]) for k in ("rgb", "accumulation", "depth", "normals")}

        def get_rgba_image(self, outputs, output_name="rgb"):
            try:  # the reference's own method where models/base_model.py imports (it pulls in the writers and tensorboard)
                from nerfstudio.models.base_model import Model as ReferenceModel
            except Exception:  # noqa: BLE001
                USED["get_rgba_image"] = "restated"
                return torch.cat(opacity_and_colour(background, outputs[output_name], outputs["accumulation"]), dim=-1)
            return ReferenceModel.get_rgba_image(self, outputs, output_name)

    pipeline = types.SimpleNamespace(datamanager=types.SimpleNamespace(next_train=next_train), model=Model())
    pcd = generate_point_cloud(pipeline, num_points=NUM_POINTS, remove_outliers=False, reorient_normals=reorient,
                               normal_output_name="normals" if with_normals else None, crop_obb=crop_obb)
    assert calls["n"] == 2, calls
    out = dict(points=np.asarray(pcd.points), colors=np.asarray(pcd.colors))
    if with_normals:
        out["normals"] = np.asarray(pcd.normals)
    return out


def main():
    inp = make_inputs()
    generate_point_cloud, OrientedBox, RayBundle = import_reference()
    out = dict(inp)
    for name, (background, box, with_normals, reorient) in VARIANTS.items():
        crop_obb = None
        if box is not None:
            pre = "box" if box == "rotated" else "face"
            crop_obb = OrientedBox(R=torch.from_numpy(inp[pre + "_R"]), T=torch.from_numpy(inp[pre + "_T"]),
                                   S=torch.from_numpy(inp[pre + "_S"]))
        if generate_point_cloud is not None:
            res = through_reference(generate_point_cloud, RayBundle, inp, background, crop_obb, with_normals, reorient)
        else:
            res = fallback_cloud(inp, background, crop_obb, with_normals, reorient)
        first = (opacity_and_colour(background, torch.from_numpy(inp["rgb"][0]), torch.from_numpy(inp["accumulation"][0]))[1] > 0.5).sum()
        assert NUM_POINTS <= len(res["points"]) and first < NUM_POINTS, (name, len(res["points"]))
        for k, v in res.items():
            out[f"{name}_{k}"] = v
        print(name, {k: v.shape for k, v in res.items()})
    out["source"] = np.array(f"generate_point_cloud (get_rgba_image: {USED['get_rgba_image']})" if generate_point_cloud is not None
                             else "within+mask")
    path = os.path.join(HERE, "pointcloud.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; source:", out["source"])


if __name__ == "__main__":
    import warnings

    warnings.filterwarnings("ignore")
    main()
