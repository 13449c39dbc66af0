"""GPU tests of nsamd_colormap (csrc/image_metrics.hip over csrc/image_metrics.h): BIT FOR BIT against the outputs the fixture
records (tests/golden/colormaps.npz: the reference's own functions on the CPU, which tests/test_colormaps_cpu.py shows the host
build of the same arithmetic to reproduce), the 8-bit output against nsamd_texture.h's rule, both outputs at once and each alone,
guard rows, and utils.colormaps on device tensors. The tables come from the fixture: nothing here needs matplotlib."""
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_colormaps_cpu import case_arguments, levels

pytestmark = pytest.mark.gpu
T = torch.from_numpy
POISON, GUARD = -77.0, 512


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    assert _native.device_info()["arch"].startswith("gfx950")
    return functional


@pytest.fixture(scope="module")
def g():
    return load_golden("colormaps")


def guarded(numel, dtype, fill):
    slab = torch.full((GUARD + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return slab, slab[GUARD:GUARD + numel]


def intact(slab, numel, fill):
    return bool((slab[:GUARD] == fill).all()) and bool((slab[GUARD + numel:] == fill).all())


def launch(F, values, lut, acc, kw, rgb=True, u8=True, range2=None):
    """-> (rgb [n,3] fp32 or None, u8 [n,3] or None) on the host, guards asserted intact; the range the parameters need comes
    from nsamd_image_range of the values"""
    from nerfstudio_amd import _native as N

    n = values.numel()
    values = values.cuda().contiguous()
    params = N.make_colormap_params(**kw)
    needs = bool(params.normalize) or (params.mode == N.COLORMAP_DEPTH and params.fixed != 3)
    if needs and range2 is None:
        range2 = F.image_range(values)
    fslab, out_rgb = guarded(3 * n, torch.float32, POISON)
    bslab, out_u8 = guarded(3 * n, torch.uint8, 0x5A)
    F.colormap_launch(values, None if lut is None else lut.cuda(), range2 if needs else None, None if acc is None else acc.cuda().contiguous(),
                      params, out_rgb if rgb else None, out_u8 if u8 else None)
    torch.cuda.synchronize()
    assert intact(fslab, 3 * n, POISON) and intact(bslab, 3 * n, 0x5A)
    assert rgb or bool((out_rgb == POISON).all())
    assert u8 or bool((out_u8 == 0x5A).all())
    return out_rgb.view(n, 3).cpu().numpy() if rgb else None, out_u8.view(n, 3).cpu().numpy() if u8 else None


def test_every_fixture_case_bit_for_bit(F, g):
    for case in (str(c) for c in g["cases"]):
        values, lut, acc, kw, _ = case_arguments(g, case)
        rgb, u8 = launch(F, values, lut, acc, kw)
        ref = g[f"{case}_out"]
        wrong = int((rgb.view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"{case}: {values.shape[0]} pixels, {wrong} values differ from the recorded outputs")
        assert wrong == 0 and np.array_equal(u8, levels(ref)), case
        only_rgb, none = launch(F, values, lut, acc, kw, u8=False)
        none2, only_u8 = launch(F, values, lut, acc, kw, rgb=False)
        assert none is None and none2 is None and np.array_equal(only_rgb.view(np.uint32), rgb.view(np.uint32)) and np.array_equal(only_u8, u8)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_launch_edges(F, g, n):
    """cases whose pixels do not depend on one another (both planes fixed, no normalize): the first n of the fixture's"""
    for case in ("depth_fixed", "depth_nan_fixed", "plain_window", "plain_gray"):
        values, lut, acc, kw, _ = case_arguments(g, case)
        rgb, u8 = launch(F, values[:n], lut, None if acc is None else acc[:n], kw)
        ref = g[f"{case}_out"][:n]
        assert np.array_equal(rgb.view(np.uint32), ref.view(np.uint32)) and np.array_equal(u8, levels(ref)), case
    # ... and one with the range of the WHOLE map handed in
    values, lut, acc, kw, _ = case_arguments(g, "depth_acc")
    rgb, _ = launch(F, values[:n], lut, acc[:n], kw, range2=F.image_range(values.cuda()))
    assert np.array_equal(rgb.view(np.uint32), g["depth_acc_out"][:n].view(np.uint32))


def test_module_functions_on_the_device(F, g, monkeypatch):
    from nerfstudio_amd import _native as N
    from nerfstudio_amd.utils import colormaps as cm

    monkeypatch.setitem(sys.modules, "matplotlib", None)
    lut = T(g["lut_turbo"]).cuda()
    depth, acc = T(g["depth_acc_in"]).cuda(), T(g["depth_acc_acc"]).cuda()
    out = cm.apply_depth_colormap(depth.view(1, -1, 1), acc.view(1, -1, 1), lut=lut)
    assert out.is_cuda and tuple(out.shape) == (1, 257, 3) and np.array_equal(out.cpu().numpy().reshape(-1, 3).view(np.uint32), g["depth_acc_out"].view(np.uint32))
    u8 = F.colormap(depth, lut, N.make_colormap_params(depth=True), accumulation=acc, rgb=False, u8=True)
    assert np.array_equal(u8.cpu().numpy(), levels(g["depth_acc_out"]))
    unit = T(g["plain_in"]).cuda()
    assert np.array_equal(cm.apply_colormap(unit, lut=lut).cpu().numpy().view(np.uint32), g["plain_out"].view(np.uint32))
    assert np.array_equal(F.colormap(unit, lut, N.make_colormap_params(), rgb=False, u8=True).cpu().numpy(), levels(g["plain_out"]))
    assert torch.equal(cm.apply_float_colormap(unit, "gray"), unit.expand(-1, 3))
    flags = T(g["bool_in"]).cuda()
    assert torch.equal(cm.apply_boolean_colormap(flags).cpu(), T(g["bool_out"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm.apply_colormap(T(g["plain_in"]), lut=T(g["lut_turbo"]))
