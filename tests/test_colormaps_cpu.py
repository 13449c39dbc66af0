"""CPU tests of the colormaps (include/nsamd_image.h: THE COLORMAP; nerfstudio_amd/utils/colormaps.py): the per-pixel arithmetic
of nerfstudio_amd/csrc/image_metrics.h compiled for the host (tests/hostcheck/image_helpers.cc) BIT FOR BIT against the fixture
the reference's own utils/colormaps.py wrote on the CPU (tests/golden/colormaps.npz, tests/golden/make_golden_colormaps.py),
the functions of utils.colormaps over launches served by that host build against the same fixture, the 8-bit output against
nsamd_texture.h's rule, and what the module passes through or refuses."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import image_metrics_reference as im

T = torch.from_numpy


@pytest.fixture(scope="module")
def g():
    return load_golden("colormaps")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return im.host_library(tmp_path_factory.mktemp("hostcheck"))


def case_arguments(g, case):
    """(values [n,1], lut or None, accumulation or None, make_colormap_params keywords, options keywords) of a fixture case"""
    mode, normalize, cmin, cmax, invert, near, far = g[f"{case}_opt"].tolist()
    name = str(g[f"{case}_map"])
    lut = None if name == "gray" else T(g["lut_" + ("turbo" if name == "default" else name)])
    acc = T(g[f"{case}_acc"]) if f"{case}_acc" in g else None
    kw = dict(depth=bool(mode), normalize=bool(normalize), colormap_min=cmin, colormap_max=cmax, invert=bool(invert),
              near_plane=None if np.isnan(near) else near, far_plane=None if np.isnan(far) else far)
    return T(g[f"{case}_in"]), lut, acc, kw, dict(colormap=name, normalize=bool(normalize), colormap_min=cmin, colormap_max=cmax, invert=bool(invert))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def levels(rgb):
    """nsamd_texture.h's 8-bit rule in numpy's fp32"""
    c = np.minimum(np.maximum(np.nan_to_num(rgb.astype(np.float32), nan=0.0), np.float32(0)), np.float32(1))
    return np.floor(c * np.float32(255) + np.float32(0.5)).astype(np.uint8)


def test_the_fixture_holds_what_its_generator_says(g):
    cases = [str(c) for c in g["cases"]]
    assert len(cases) == 18 and 2000 <= sum(g[f"{c}_in"].shape[0] for c in cases) <= 10000
    for name in ("turbo", "viridis", "magma", "inferno"):
        assert g[f"lut_{name}"].shape == (256, 3) and g[f"lut_{name}"].dtype == np.float32
    assert {"depth", "depth_acc", "depth_fixed", "depth_constant", "plain_normalize", "plain_window", "plain_steps"} <= set(cases)
    assert np.isnan(g["depth_nan_fixed_in"]).sum() == 2 and np.isfinite(g["depth_nan_fixed_out"]).all()


def test_host_build_matches_the_reference_bit_for_bit(g, lib, monkeypatch):
    from nerfstudio_amd import _native as N, functional as F

    im.inject(monkeypatch, lib)
    for case in (str(c) for c in g["cases"]):
        values, lut, acc, kw, _ = case_arguments(g, case)
        rgb, u8 = F.colormap(values, lut, N.make_colormap_params(**kw), accumulation=acc, u8=True)
        ref = g[f"{case}_out"]
        wrong = int((rgb.numpy().view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"{case}: {values.shape[0]} pixels, {wrong} values differ from the reference's")
        assert tuple(rgb.shape) == ref.shape and wrong == 0, case
        assert np.array_equal(u8.numpy(), levels(ref)), case


def test_module_functions_match_the_reference_bit_for_bit(g, lib, monkeypatch):
    from nerfstudio_amd.utils import colormaps as cm

    log = []
    im.inject(monkeypatch, lib, log)
    monkeypatch.setitem(sys.modules, "matplotlib", None)  # every table comes from the fixture
    for case in (str(c) for c in g["cases"]):
        values, lut, acc, kw, opt = case_arguments(g, case)
        options = cm.ColormapOptions(**opt)
        if case == "float_viridis":
            rgb = cm.apply_float_colormap(values, lut=lut)
        elif kw["depth"]:
            rgb = cm.apply_depth_colormap(values, acc, kw["near_plane"], kw["far_plane"], options, lut=lut)
        else:
            rgb = cm.apply_colormap(values, options, lut=lut)
        assert same_bits(rgb.numpy(), g[f"{case}_out"]), case
    # the range is taken exactly where the definition needs one: normalize, or a depth map without both planes
    ranges = sum(1 for e in log if e[0] == "range")
    needing = sum(1 for c in g["cases"] if g[f"{c}_opt"][1] or (g[f"{c}_opt"][0] and np.isnan(g[f"{c}_opt"][5:]).any()))
    assert ranges == needing and sum(1 for e in log if e[0] == "colormap") == len(g["cases"])
    flags = T(g["bool_in"])
    assert torch.equal(cm.apply_boolean_colormap(flags), T(g["bool_out"])) and torch.equal(cm.apply_colormap(flags), T(g["bool_out"]))
    red = cm.apply_boolean_colormap(flags, torch.tensor([1.0, 0, 0]), torch.tensor([0, 0, 1.0]))
    assert torch.equal(red[flags[:, 0]], torch.tensor([1.0, 0, 0]).expand(int(flags.sum()), 3))


def test_u8_output_and_image_shapes(g, lib, monkeypatch):
    from nerfstudio_amd import _native as N, functional as F
    from nerfstudio_amd.utils import colormaps as cm

    im.inject(monkeypatch, lib)
    lut = T(g["lut_turbo"])
    depth, acc = T(g["depth_acc_in"][:240]).reshape(12, 20, 1), T(g["depth_acc_acc"][:240]).reshape(12, 20, 1)
    rgb = cm.apply_depth_colormap(depth, acc, lut=lut)
    u8 = F.colormap(depth, lut, N.make_colormap_params(depth=True), accumulation=acc, rgb=False, u8=True)
    assert tuple(rgb.shape) == (12, 20, 3) == tuple(u8.shape) and u8.dtype == torch.uint8 and np.array_equal(u8.numpy(), levels(rgb.numpy()))
    plain = T(g["plain_in"][:240]).reshape(12, 20, 1)
    both = F.colormap(plain, lut, N.make_colormap_params(), u8=True)
    assert torch.equal(both[0], cm.apply_colormap(plain, lut=lut)) and np.array_equal(both[1].numpy(), levels(both[0].numpy()))


def test_passthrough_gray_and_refusals(g, lib, monkeypatch):
    from nerfstudio_amd.utils import colormaps as cm

    im.inject(monkeypatch, lib)
    image = torch.rand(5, 7, 3)
    assert cm.apply_colormap(image) is image
    unit = T(g["plain_in"])
    gray = cm.apply_float_colormap(unit, "gray")
    assert torch.equal(gray, unit.expand(-1, 3))  # no table, no matplotlib
    with pytest.raises(NotImplementedError, match="PCA"):
        cm.apply_colormap(torch.rand(4, 4, 8))
    with pytest.raises(NotImplementedError, match="pca"):
        cm.apply_float_colormap(unit, "pca")
    with pytest.raises(ValueError, match="one-channel"):
        cm.apply_depth_colormap(torch.rand(4, 4, 2))
    defaults = cm.ColormapOptions()
    assert (defaults.colormap, defaults.normalize, defaults.colormap_min, defaults.colormap_max, defaults.invert) == ("default", False, 0, 1, False)


def test_default_is_turbo_from_matplotlib_cached(g, lib, monkeypatch):
    pytest.importorskip("matplotlib")
    from nerfstudio_amd.utils import colormaps as cm

    im.inject(monkeypatch, lib)
    unit = T(g["plain_in"])
    assert same_bits(cm.colormap_lut("default", "cpu").numpy(), g["lut_turbo"]) and cm.colormap_lut("turbo", "cpu") is cm.colormap_lut("default", "cpu")
    assert same_bits(cm.apply_colormap(unit).numpy(), g["plain_out"])


def test_module_reads_nothing_back_and_imports_lazily():
    src = open(os.path.join(ROOT, "nerfstudio_amd", "utils", "colormaps.py")).read()
    body = re.sub(r'""".*?"""', "", src, flags=re.S)  # the docstrings speak of what the reference does
    assert not re.findall(r"^(?:import|from)\s+(?:nerfstudio|matplotlib)\b", src, re.M)
    assert not re.findall(r"\bfloat\(torch\.|\.item\(\)|\.cpu\(\)|\.tolist\(\)|\bassert .*torch\.(?:min|max)", body)
