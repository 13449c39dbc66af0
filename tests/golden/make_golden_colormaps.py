#!/usr/bin/env python3
"""Golden fixture for the colormaps — written by THE REFERENCE ITSELF (read-only import of the reference's utils/colormaps.py
through the import stubs, torch, CPU, fp32; the tables are matplotlib's). Authoring container only:

    python tests/golden/make_golden_colormaps.py      ->  tests/golden/colormaps.npz

Contents:
  lut_<turbo|viridis|magma|inferno>   [256, 3] fp32: matplotlib.colormaps[name].colors as the reference turns them into a tensor
  cases                               the names of the cases, one string each
  <case>_in, <case>_out               the input [n, 1] fp32 (or bool) and the reference's output [n, 3] fp32
  <case>_acc                          the accumulation [n, 1] of the depth cases that have one
  <case>_opt                          float64 [7]: depth mode, normalize, colormap_min, colormap_max, invert, near_plane, far_plane
                                      (NaN = None); <case>_map: the colormap's name
The depth cases: without and with an accumulation, with fixed near and far, with only one of them, a constant depth, a NaN
depth under fixed planes, normalize on a depth map. The plain cases: normalize on and off, invert, a min / max window, values at
exact multiples of 1 / 255 and their neighbours, "gray". A few thousand pixels in all.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402,F401  (sets up the import path of the reference and its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

NAN = float("nan")


def main():
    import matplotlib
    from nerfstudio.utils import colormaps as rc

    out = {}
    for name in ("turbo", "viridis", "magma", "inferno"):
        out[f"lut_{name}"] = torch.tensor(matplotlib.colormaps[name].colors).numpy().astype(np.float32)
        assert out[f"lut_{name}"].shape == (256, 3)
    rs = np.random.RandomState(0)
    n = 257
    depth = torch.from_numpy(rs.uniform(0.3, 7.0, (n, 1)).astype(np.float32))
    acc = torch.from_numpy(np.clip(rs.uniform(-0.1, 1.1, (n, 1)), 0, 1).astype(np.float32))
    unit = torch.from_numpy(rs.uniform(0.0, 1.0, (n, 1)).astype(np.float32))
    wide = torch.from_numpy(rs.uniform(-0.5, 1.5, (n, 1)).astype(np.float32))
    steps = torch.arange(256, dtype=torch.float32)[:, None] / 255
    around = torch.cat([steps, torch.nextafter(steps, torch.tensor(2.0)), torch.nextafter(steps, torch.tensor(-1.0)).clamp(min=0)])
    with_nan = depth.clone()
    with_nan[5], with_nan[77] = NAN, NAN
    cases = []

    def depth_case(name, d, a=None, near=None, far=None, **opt):
        o = rc.ColormapOptions(**opt)
        res = rc.apply_depth_colormap(d.clone(), None if a is None else a.clone(), near, far, o)
        record(name, d, res, o, 1, near, far, a)

    def plain_case(name, v, **opt):
        o = rc.ColormapOptions(**opt)
        record(name, v, rc.apply_colormap(v.clone(), o), o, 0, None, None, None)

    def record(name, v, res, o, mode, near, far, a):
        cases.append(name)
        assert res.dtype == torch.float32 and tuple(res.shape) == (*v.shape[:-1], 3)
        out[f"{name}_in"], out[f"{name}_out"] = v.numpy().reshape(-1, 1), res.numpy().reshape(-1, 3)
        if a is not None:
            out[f"{name}_acc"] = a.numpy().reshape(-1, 1)
        out[f"{name}_opt"] = np.array([mode, o.normalize, o.colormap_min, o.colormap_max, o.invert, NAN if near is None else near,
                                       NAN if far is None else far], np.float64)
        out[f"{name}_map"] = np.array(o.colormap)

    depth_case("depth", depth)
    depth_case("depth_acc", depth, acc)
    depth_case("depth_fixed", depth, acc, 0.5, 6.3)
    depth_case("depth_fixed_near", depth, None, 0.1, None, colormap="viridis")
    depth_case("depth_fixed_far", depth, acc, None, 4.7, colormap="magma", invert=True)
    depth_case("depth_constant", torch.full((n, 1), 2.5), acc)
    depth_case("depth_nan_fixed", with_nan, acc, 0.25, 8.0, colormap="inferno")
    depth_case("depth_normalize", depth, acc, 1.0, 5.0, normalize=True, colormap_min=0.1, colormap_max=0.8)
    depth_case("depth_gray", depth[None], acc[None], colormap="gray")  # the reference's "gray" repeats a [1, n, 1] image
    plain_case("plain", unit)
    plain_case("plain_viridis_invert", unit, colormap="viridis", invert=True)
    plain_case("plain_normalize", wide * 3 + 1, normalize=True, colormap="magma")
    plain_case("plain_window", wide, colormap_min=0.2, colormap_max=0.9, colormap="inferno")
    plain_case("plain_window_normalize_invert", wide, normalize=True, colormap_min=-0.2, colormap_max=1.3, invert=True)
    plain_case("plain_steps", around)
    plain_case("plain_gray", unit[None], colormap="gray", colormap_min=0.25, colormap_max=0.75)
    plain_case("plain_clipped", wide)
    # apply_float_colormap directly (its default is viridis), and the boolean map
    cases.append("float_viridis")
    out["float_viridis_in"], out["float_viridis_out"] = around.numpy(), rc.apply_float_colormap(around.clone()).numpy()
    out["float_viridis_opt"] = np.array([0, 0, 0, 1, 0, NAN, NAN], np.float64)
    out["float_viridis_map"] = np.array("viridis")
    flags = torch.from_numpy(rs.uniform(0, 1, (n, 1)) < 0.4)
    out["bool_in"], out["bool_out"] = flags.numpy(), rc.apply_boolean_colormap(flags).numpy()
    out["cases"] = np.array(cases)
    pixels = sum(out[f"{c}_in"].shape[0] for c in cases)
    path = os.path.join(HERE, "colormaps.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {pixels} pixels, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
