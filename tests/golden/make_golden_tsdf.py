#!/usr/bin/env python3
"""Golden fixture for TSDF fusion — written by THE REFERENCE ITSELF (read-only import of the reference's
exporter/tsdf_utils.py, torch, CPU, fp32). Authoring container only:

    python tests/golden/make_golden_tsdf.py      ->  tests/golden/tsdf.npz

tsdf_utils imports pymeshlab, skimage, exporter_utils and the pipelines at module level; none of them is needed by
TSDF.from_aabb / TSDF.integrate_tsdf, so empty stand-ins are put into sys.modules first.

For every case of tests/tsdf_reference.CASES (`<case>_...`): the inputs (aabb, dims, c2w, K, depth, color), the state
TSDF.from_aabb starts from (values0, weights0, colors0, voxel_coords, voxel_size, origin, truncation) and values / weights /
colors after integrate_tsdf of the whole batch (`batch_`), of the views one at a time (`seq_`), of the batch a second time
(`twice_`) and of the batch without colour images (`nocolor_`). `e_ref_values_<case>` / `e_ref_colors_<case>`: the reference's
own fp32 distance from float64 (tsdf_reference.integrate_f64 on the same fp32 inputs) over the case's safe voxels, the largest
over the batch and the second pass — the bound the tests take. `<case>_counts`: voxels, touched, touched from behind a camera,
unsafe.

`rescale_*`: what Cameras.rescale_output_resolution (cameras/cameras.py:987-1020) leaves in a Cameras object for downscale
factors 2 and 3 — fuse_views must compute the same numbers without touching the object.
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_refstubs"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.dirname(HERE))


def _stub(name, **names):
    m = types.ModuleType(name)
    for k, v in names.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


_stub("pymeshlab")
_stub("skimage").measure = _stub("skimage.measure")
_stub("nerfstudio.exporter.exporter_utils", Mesh=object, render_trajectory=None)
_stub("nerfstudio.pipelines")
_stub("nerfstudio.pipelines.base_pipeline", Pipeline=object)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tsdf_reference as tr  # noqa: E402
from nerfstudio.cameras.cameras import Cameras, CameraType  # noqa: E402
from nerfstudio.exporter.tsdf_utils import TSDF  # noqa: E402

T = torch.from_numpy


def state(tsdf):
    return {k: getattr(tsdf, k).numpy().copy() for k in ("values", "weights", "colors")}


def run_case(name, out):
    inp = tr.make_case(name)
    for k, v in inp.items():
        out[f"{name}_{k}"] = v
    new = lambda: TSDF.from_aabb(T(inp["aabb"]), volume_dims=T(inp["dims"]))  # noqa: E731
    c2w, K, depth, color = (T(inp[k]) for k in ("c2w", "K", "depth", "color"))
    tsdf = new()
    for k, v in state(tsdf).items():
        out[f"{name}_{k}0"] = v
    out[f"{name}_voxel_coords"], out[f"{name}_voxel_size"] = tsdf.voxel_coords.numpy(), tsdf.voxel_size.numpy()
    out[f"{name}_origin"], out[f"{name}_truncation"] = tsdf.origin.numpy(), np.float64(tsdf.truncation)
    origin, voxel_size, truncation = tr.volume_geometry(inp["aabb"], inp["dims"])
    assert np.array_equal(voxel_size, tsdf.voxel_size.numpy()) and truncation == tsdf.truncation

    tsdf.integrate_tsdf(c2w, K, depth, color_images=color)
    batch = state(tsdf)
    tsdf.integrate_tsdf(c2w, K, depth, color_images=color)
    twice = state(tsdf)
    seq = new()
    for b in range(c2w.shape[0]):
        seq.integrate_tsdf(c2w[b:b + 1], K[b:b + 1], depth[b:b + 1], color_images=color[b:b + 1])
    plain = new()
    plain.integrate_tsdf(c2w, K, depth)
    for tag, st in (("batch", batch), ("twice", twice), ("seq", state(seq)), ("nocolor", state(plain))):
        for k, v in st.items():
            out[f"{name}_{tag}_{k}"] = v

    v0, w0, c0 = tr.initial_state(inp["dims"])
    f1 = tr.integrate_f64(origin, voxel_size, truncation, v0, w0, c0, inp["c2w"], inp["K"], inp["depth"], inp["color"])
    f2 = tr.integrate_f64(origin, voxel_size, truncation, batch["values"], batch["weights"], batch["colors"], inp["c2w"], inp["K"],
                          inp["depth"], inp["color"])
    safe = tr.safe_voxels(f1)
    assert np.array_equal(safe, tr.safe_voxels(f2))
    assert 1 - safe.mean() <= tr.UNSAFE_CAP, (name, 1 - safe.mean())
    for got, f in ((batch, f1), (twice, f2)):
        assert np.array_equal(got["weights"][safe].astype(np.float64), f["weights"][safe]), name
    out[f"e_ref_values_{name}"] = np.float64(max(tr.distance(batch["values"], f1, "values", safe),
                                                 tr.distance(twice["values"], f2, "values", safe)))
    out[f"e_ref_colors_{name}"] = np.float64(max(tr.distance(batch["colors"], f1, "colors", safe),
                                                 tr.distance(twice["colors"], f2, "colors", safe)))
    touched = batch["weights"] > 0
    out[f"{name}_counts"] = np.array([safe.size, touched.sum(), (f1["behind"] & touched).sum(), (~safe).sum()], np.int64)
    print(f"case {name}: {safe.size} voxels, touched {int(touched.sum())}, from behind {int((f1['behind'] & touched).sum())}, "
          f"unsafe {int((~safe).sum())} ({100 * (1 - safe.mean()):.2f} %), e_ref values {out[f'e_ref_values_{name}']:.3e} "
          f"colors {out[f'e_ref_colors_{name}']:.3e}, NaN {int(np.isnan(batch['values']).sum())}")


def run_rescale(out):
    n = 5
    base = dict(fx=torch.tensor([[30.0], [31.7], [52.25], [40.1], [33.3]]), fy=torch.tensor([[28.0], [29.9], [51.5], [40.2], [33.4]]),
                cx=torch.tensor([[16.37], [20.5], [31.9], [24.0], [17.1]]), cy=torch.tensor([[11.79], [15.5], [24.1], [18.0], [12.6]]),
                height=torch.tensor([[24], [31], [48], [37], [25]]), width=torch.tensor([[32], [41], [64], [49], [35]]))
    for k, v in base.items():
        out[f"rescale_{k}"] = v.numpy()
    for factor in (2, 3):
        cams = Cameras(camera_to_worlds=torch.eye(4)[None, :3].repeat(n, 1, 1), camera_type=CameraType.PERSPECTIVE,
                       **{k: v.clone() for k, v in base.items()})
        cams.rescale_output_resolution(1.0 / factor)
        for k in base:
            out[f"rescale_f{factor}_{k}"] = getattr(cams, k).numpy()


def main():
    torch.set_num_threads(1)
    out = {}
    for name in tr.CASES:
        run_case(name, out)
    run_rescale(out)
    path = os.path.join(HERE, "tsdf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
