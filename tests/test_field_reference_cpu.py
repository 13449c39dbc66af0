"""No GPU: the reference, bounds and case generator of tests/field_reference.py, on a CORRECT fp32 evaluation of the main field's
MLPs and on deliberately wrong ones.

  1. the float64 reference equals torch's float64 autograd of the same graph (the oracle's trunc_exp and sh_levels4) to 1e-12 of
     each output's largest entry: density, rgb, denc, the ten parameter gradients, the appearance-table gradient;
  2. torch's fp32 CPU evaluation of that graph stays inside every per-entry bound on every small case (its worst
     |err| / bound per output is printed: the `cpu fp32` column of profiles/field_float64_ratios.txt), and so does an fp32
     evaluation of nsamd_field_ray_terms;
  3. the case generator leaves no undecided ReLU on any case, the two large ones included, within MAX_REDRAW_ROUNDS rounds;
  4. each defect the GPU test is meant to catch, evaluated in numpy, leaves at least one bound violated.
"""
import numpy as np
import pytest
import torch

import field_reference as fr
from float64_check import check_entries, report
from oracle import nerfacto_oracle as orc

SMALL = [c.name for c in fr.SMALL_CASES]


def violated(c, ref, got):
    """Names of the outputs in `got` with an entry outside its bound."""
    out = []
    for k, g in got.items():
        try:
            check_entries(k, g, ref[k], ref["e_" + k], {})
        except AssertionError:
            out.append(k)
    return out


def reference_outputs(ref):
    return {k: ref[k].copy() for k in fr.FORWARD_OUTPUTS + fr.BACKWARD_OUTPUTS if k in ref}


@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_float64_autograd(name):
    inp, ref = fr.case_data(name)
    got = fr.torch_evaluate(inp, torch.float64)
    assert set(got) == set(reference_outputs(ref))
    for k, g in got.items():
        scale = float(np.abs(ref[k]).max())
        assert g.shape == ref[k].shape and float(np.abs(g - ref[k]).max()) <= 1e-12 * scale, (name, k)


@pytest.mark.parametrize("name", SMALL)
def test_fp32_cpu_evaluation_is_inside_every_bound(name):
    c = fr.BY_NAME[name]
    inp, ref = fr.case_data(name)
    worst = {}
    got = fr.torch_evaluate(inp, torch.float32)
    assert all(g.dtype == np.float32 for g in got.values())
    try:
        fr.check(c, ref, got, worst)
    finally:
        report(f"field-f64 cpu fp32 {fr.launch_note(c)}", worst)
    assert max(worst.values()) < 1.0


@pytest.mark.parametrize("R,app,keep", fr.RAY_TERM_CASES)
def test_fp32_ray_terms_are_inside_their_bounds(R, app, keep):
    inp = fr.draw_inputs(f"terms-{R}-{app}", R, 1, app)
    ref = fr.ray_terms64(inp)
    sh = orc.sh_levels4((torch.from_numpy(inp["directions"]) + 1.0) / 2.0)
    rows = [sh]
    if app == "cams":
        rows.append(torch.from_numpy(inp["appearance"])[torch.from_numpy(inp["camera_indices"])])
    elif app == "const":
        rows.append(torch.from_numpy(inp["appearance_const"]).expand(R, 32))
    x = torch.cat(rows, -1)
    W = torch.from_numpy(inp["head_W0"])
    cols = list(range(16)) + list(range(31, 31 + fr.app_dim_of(app)))
    terms = x @ W[:, cols].t() + torch.from_numpy(inp["head_b0"])
    worst = {}
    check_entries("ray_terms", terms.numpy(), ref["ray_terms"], ref["e_ray_terms"], worst)
    if keep:
        assert ref["ray_inputs"].shape == (R, 16 + fr.app_dim_of(app))
        check_entries("ray_inputs", x.numpy(), ref["ray_inputs"], ref["e_ray_inputs"], worst)
    report(f"field-f64 cpu fp32 ray terms R={R} {app}", worst)


@pytest.mark.parametrize("name", [c.name for c in fr.CASES])
def test_case_generator_leaves_no_undecided_relu(name):
    c = fr.BY_NAME[name]
    inp, ref = fr.case_data(name)
    assert inp["rounds"] < fr.MAX_REDRAW_ROUNDS
    assert int(ref["undecided"].sum()) == 0
    for k in ("pre0", "p0", "p1"):  # the statement itself, not the generator's flag
        assert not ((np.abs(ref[k]) <= fr.AMBIGUITY_MARGIN * ref["e_" + k]) & (ref["e_" + k] > 0)).any()
    if c.app == "cams":
        rays = -(-c.M // c.dir_group)  # one ray uses the camera: with dir_group 1 that is exactly one point
        assert ref["camera_points"][fr.SINGLE_CAMERA] in (min(c.dir_group, c.M), c.M - (rays - 1) * c.dir_group)
        assert ref["camera_points"][fr.UNUSED_CAMERA] == 0
    if c.spread == "o0":
        o0 = ref["o"][:, 0]
        assert o0.min() < -15.5 and o0.max() > 15.5 and ((o0 > -14) & (o0 < 14)).any()
    if c.spread == "p2":
        assert (ref["p2"].min(0) < -25).all() and (ref["p2"].max(0) > 25).all()
    print(f"\nfield-f64 generator {name}: {inp['rounds']} redraw rounds, largest e(pre) {ref['unit_bound_max']:.2e}")


def test_every_case_states_the_branch_the_host_takes():
    seen = set()
    for c in fr.CASES:
        assert fr.expected_branch(c) == c.expect
        seen.add(c.expect)
        seen.update(c.expect.split("/")[2:])
    for part in ("partials", "atomics", "tile_rows", "point_rows", "none"):
        assert part in seen
    assert {"rayc/rayc/partials/tile_rows", "rayc/plain/partials/atomics", "plain/plain/atomics/atomics"} <= seen
    big = [c for c in fr.PERSISTENT]
    for c in big:  # the second pass of a persistent workgroup, forward and backward
        tiles = -(-c.M // 16)
        assert tiles > fr.NUM_CUS * fr.K_FWD_WAVES and tiles > fr.NUM_CUS * fr.K_COOP_WAVES


# ---- deliberately wrong evaluations ------------------------------------------------------------------------------------------

def _with(ref, **changed):
    got = reference_outputs(ref)
    got.update(changed)
    return got


def mutant_cross_term_dropped():
    """coop_dw_pk without the h m' product, on head layer 1's weight gradient."""
    c = fr.BY_NAME["edge-M129-g1-cams-ws_full"]
    inp, ref = fr.case_data(c.name)
    (gh, gm), (xh, xm) = fr.bf16_pieces(ref["g_hb"]), fr.bf16_pieces(ref["ha"])
    full = (gh + gm).T @ (xh + xm)
    assert not violated(c, ref, _with(ref, dhead_W1=full)), "the complete two-piece product has to pass"
    return c, ref, _with(ref, dhead_W1=full - gh.T @ xm), "dhead_W1"


def mutant_last_point_twice():
    """The clamped dead lanes of the last tile (point M - 1) contribute, M = 17."""
    c = fr.BY_NAME["edge-M17-g1-cams-ws_full"]
    inp, ref = fr.case_data(c.name)
    got = reference_outputs(ref)
    for G, X, k in (("g2", "hb", "head_W2"), ("g_hb", "ha", "head_W1"), ("g_ha", "hin", "head_W0"), ("g_o", "h1", "base_W1"),
                    ("g_h1", "x", "base_W0")):
        got["d" + k] = got["d" + k] + np.outer(ref[G][-1], ref[X][-1])
        got["d" + k.replace("W", "b")] = got["d" + k.replace("W", "b")] + ref[G][-1]
    return c, ref, got, "dhead_W1"


def mutant_head0_columns_shifted():
    """head0_col's hole at slot 16 ignored: head layer 0's weight gradient one column off from column 16 on."""
    c = fr.BY_NAME["app-M100-g1-cams-ws_full"]
    inp, ref = fr.case_data(c.name)
    dW = ref["dhead_W0"].copy()
    dW[:, 16:] = np.roll(dW[:, 16:], 1, axis=1)
    return c, ref, _with(ref, dhead_W0=dW), "dhead_W0"


def mutant_no_appearance_read_with_63_columns():
    """app_dim = 0 (head layer 0 has 31 columns) evaluated with the 63-column row stride."""
    c = fr.BY_NAME["app-M100-g1-none-ws_full"]
    inp, ref = fr.case_data(c.name)
    flat = inp["head_W0"].ravel()
    idx = (np.arange(64)[:, None] * 63 + np.arange(31)[None, :]) % flat.size
    wrong = dict(inp)
    wrong["head_W0"] = flat[idx]
    return c, ref, _with(ref, rgb=fr.forward64(wrong)["rgb"]), "rgb"


def _backward_mutant(name, mutate, key):
    c = fr.BY_NAME[name]
    inp, ref = fr.case_data(name)
    bad = fr.backward64(inp, fr.forward64(inp), fr.field_chains(c), mutate=mutate)
    return c, ref, _with(ref, **{k: bad[k] for k in fr.BACKWARD_OUTPUTS if k in bad}), key


def mutant_trunc_exp_backward_without_clamp():
    return _backward_mutant("spread-M200-g1-cams-ws_full-spread_o0", "no_clamp", "denc")


def mutant_sigmoid_derivative_of_the_wrong_channel():
    return _backward_mutant("spread-M200-g1-cams-ws_full-spread_p2", "wrong_channel", "dhead_b2")


def mutant_selector_ignored_on_the_density_gradient():
    return _backward_mutant("fwd-M100-g1-cams-sel_zeros-ws_full", "selector_ignored", "denc")


def mutant_single_camera_gradient_dropped():
    c = fr.BY_NAME["edge-M257-g1-cams-ws_full"]
    inp, ref = fr.case_data(c.name)
    assert ref["camera_points"][fr.SINGLE_CAMERA] == 1
    dapp = ref["dappearance"].copy()
    dapp[fr.SINGLE_CAMERA] = 0.0
    return c, ref, _with(ref, dappearance=dapp), "dappearance"


MUTANTS = [mutant_cross_term_dropped, mutant_last_point_twice, mutant_head0_columns_shifted,
           mutant_no_appearance_read_with_63_columns, mutant_trunc_exp_backward_without_clamp,
           mutant_sigmoid_derivative_of_the_wrong_channel, mutant_single_camera_gradient_dropped,
           mutant_selector_ignored_on_the_density_gradient]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m.__name__ for m in MUTANTS])
def test_a_wrong_evaluation_violates_a_bound(mutant):
    c, ref, got, key = mutant()
    assert not violated(c, ref, reference_outputs(ref))
    bad = violated(c, ref, got)
    print(f"\nfield-f64 {mutant.__name__} on {c.name}: caught, outside the bound of {', '.join(bad) or 'NOTHING'}")
    assert key in bad, f"{mutant.__name__} passes the bound of {key} on {c.name} (violated: {bad})"


def test_saturated_channels_are_held_to_an_absolute_allowance():
    """The spread case has channels with sg (1 - sg) < 1e-10 on both sides, and there the bound of the derivative is the absolute
    u sg term near sg = 1 and a relative one near sg = 0: torch's fp32 sigmoid backward stays inside both."""
    inp, ref = fr.case_data("spread-M200-g1-cams-ws_full-spread_p2")
    assert (ref["sgd"] < 1e-10).any() and (ref["rgb"] > 1 - 1e-10).any() and (ref["rgb"] < 1e-10).any()
    y = torch.sigmoid(torch.from_numpy(ref["p2"].astype(np.float32)))
    d32 = (y * (1 - y)).double().numpy()
    p64 = ref["p2"].astype(np.float32).astype(np.float64)
    sg = 1 / (1 + np.exp(-p64))
    d64 = 1 / ((1 + np.exp(-p64)) * (1 + np.exp(p64)))
    e_sg = d64 * fr.E_EXP + 2 * fr.U * sg
    bound = np.abs(1 - 2 * sg) * e_sg + 2 * fr.U * d64 + fr.U * sg
    ratio = float((np.abs(d32 - d64) / bound).max())
    print(f"\nfield-f64 sigmoid derivative, torch fp32 against float64 over [-30, 30]: worst |err| / bound {ratio:.3f}")
    assert ratio < 1.0
