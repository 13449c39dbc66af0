"""Shared by tests/test_lens_cpu.py and tests/test_gpu_lens.py: reading tests/golden/raygen_lenses.npz and the comparison of a
ray generator's output with it, under the bounds the fixture itself holds (see test_lens_cpu.py)."""
import numpy as np

CASES = ["opencv", "fisheye", "equirect", "mixed", "grid_opencv", "grid_fisheye"]


def case_arrays(g, name):
    pre = name + "_"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def check_against_fixture(g, name, o, d, pa, dn):
    """Every ray of case `name` within 2 x e_ref of float64 and 3 x e_ref of the reference's fp32; origins exact. Prints each
    figure before it asserts."""
    c = case_arrays(g, name)
    e_d, e_a, e_n = float(g["e_ref_directions"]), float(g["e_ref_pixel_area"]), float(g["e_ref_directions_norm"])
    np.testing.assert_array_equal(o, c["origins"], err_msg=f"{name}: origins")
    for what, ref_d, ref_a, ref_n, mult in (("float64", c["f64_directions"], c["f64_pixel_area"], c["f64_directions_norm"], 2.0),
                                            ("reference fp32", c["directions"], c["pixel_area"], c["directions_norm"], 3.0)):
        err_d = float(np.abs(d.astype(np.float64) - ref_d).max())
        err_a = float((np.abs(pa.astype(np.float64) - ref_a) / np.abs(ref_a)).max())
        err_n = float((np.abs(dn.astype(np.float64) - ref_n) / np.abs(ref_n)).max())
        print(f"{name} vs {what}: directions {err_d:.3e} (bound {mult * e_d:.3e}), pixel_area {err_a:.3e} rel (bound "
              f"{mult * e_a:.3e}), directions_norm {err_n:.3e} rel (bound {mult * e_n:.3e})")
        assert np.isfinite([err_d, err_a, err_n]).all(), (name, what)
        assert err_d <= mult * e_d, f"{name} directions vs {what}: {err_d:.3e} > {mult * e_d:.3e}"
        assert err_a <= mult * e_a, f"{name} pixel_area vs {what}: {err_a:.3e} > {mult * e_a:.3e}"
        assert err_n <= mult * e_n, f"{name} directions_norm vs {what}: {err_n:.3e} > {mult * e_n:.3e}"
