"""tests/position_gradient_reference.py without a GPU: its bounds hold for a correct fp32 evaluation of every case the GPU tests
run, and each of twelve seeded defects pushes at least one entry outside them.

* The fp32 evaluation is composed from the host-compiled kernel helpers (tests/hostcheck/helpers.cc: hc_positions, hc_normalise,
  hc_hash_forward_and_gradient, hc_position_gradient_tail = the end of position_gradient with contract_linf_bwd) in
  position_gradient's order, reduced per ray in numpy fp32 in the kernel's order (lane l adds samples l, l + 64, ..., then six
  butterfly steps); the table paths add the fp32 corner_share values of hc_gradient_shares in a shuffled order. Its raw
  positions, grid inputs and selectors must equal the reference's fp32 restatement bit for bit, so both take the same branches.
* contract_linf_bwd alone, per entry, against float64 autograd through orc.contract_linf on the branch-covering points (ties,
  mag == 1, a zero coordinate, a negative maximum), inside the bound derived for it with an exact incoming gradient.
* The defects are wrong restatements of the float64 expression (as test_kernel_helpers_cpu.py seeds its own), rounded to fp32.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import position_gradient_reference as pg
from float64_check import check_entries, report
from oracle import nerfacto_oracle as orc
from test_kernel_helpers_cpu import F32P, hc  # noqa: F401  (the fixture that builds tests/hostcheck)

F32 = np.float32
RATIOS = {}  # printed by the last test: the figures of profiles/hash_position_gradient_float64_ratios.txt


@pytest.fixture(scope="module")
def lib(hc):  # noqa: F811
    hc.hc_position_gradient_tail.argtypes = [F32P, F32P, C.c_int64, C.c_int, F32P, F32P, F32P]
    return hc


def _keep(group, worst):
    for k, v in worst.items():
        RATIOS.setdefault(group, {})[k] = max(RATIOS.get(group, {}).get(k, 0.0), v)


def fp32_dpositions(lib, case):
    """position_gradient of every point of the case from the host-compiled helpers, [M,3] fp32."""
    M = case.M
    if case.rays:
        raw = np.zeros((M, 3), F32)
        lib.hc_positions(case.points["origins"], case.points["directions"], case.points["t_bins"], case.n, case.S, raw)
    else:
        raw = case.points["positions"].copy()
    assert np.array_equal(pg.bits(raw), pg.bits(case.raw)), "load_position differs from positions32"
    x, sel = raw.copy(), np.zeros(M, F32)
    lo, hi = case.box[0].copy(), case.box[1].copy()
    lib.hc_normalise(x, M, case.transform, lo, hi, sel)
    assert np.array_equal(pg.bits(x), pg.bits(case.x)) and np.array_equal(sel, case.sel), "normalise_position differs from normalise32"
    out, dx = np.zeros((M, 2 * case.L), F32), np.zeros((M, 3), F32)
    lib.hc_hash_forward_and_gradient(x, M, case.table, case.scal, case.L, case.log2_T, case.denc, out, dx)
    lib.hc_position_gradient_tail(raw, dx, M, case.transform, lo, hi, sel)
    return dx


def fp32_ray_sums(case, dpos):
    """hash_encode_bwd_rays_kernel's reduction of dpos [n S, 3] in numpy fp32: (d_origins, d_directions) [n,3]."""
    n, S = case.n, case.S
    t = case.points["t_bins"]
    half = ((t[:, :-1] + t[:, 1:]).astype(F32) / F32(2.0)).astype(F32)
    p = dpos.reshape(n, S, 3)
    so, sd = np.zeros((n, 64, 3), F32), np.zeros((n, 64, 3), F32)
    for s0 in range(0, S, 64):
        k = min(64, S - s0)
        so[:, :k] = so[:, :k] + p[:, s0:s0 + k]
        sd[:, :k] = sd[:, :k] + (p[:, s0:s0 + k] * half[:, s0:s0 + k, None]).astype(F32)
    lanes = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        so, sd = so + so[:, lanes ^ m], sd + sd[:, lanes ^ m]
    assert so.dtype == F32 and sd.dtype == F32
    return so[:, 0].copy(), sd[:, 0].copy()


def fp32_table(lib, case, prefill, seed, defect=None):
    """The scratch-free table gradient on top of `prefill` [L T, 2]: fp32 corner shares added in a shuffled order."""
    tab = (np.zeros((case.L * case.T, 2), F32) if prefill is None else prefill.copy()).reshape(-1)
    live = (case.denc != 0).any(axis=1)
    rs = np.random.RandomState(seed)
    M = case.M
    for lvl, scale in enumerate(case.scal):
        idx, corner, pair = np.zeros((M, 8), np.int64), np.zeros((M, 8, 2), F32), np.zeros((M, 4, 2), F32)
        lib.hc_hash_corners(case.x, M, float(scale), case.log2_T, idx)
        lib.hc_gradient_shares(case.x, M, float(scale), np.ascontiguousarray(case.denc[:, 2 * lvl:2 * lvl + 2]), corner, pair)
        if defect == "corner_pair_exchanged" and lvl == 2:
            idx[:, [0, 1]] = idx[:, [1, 0]]
        flat = ((2 * (idx[live] + lvl * case.T))[:, :, None] + np.arange(2)).reshape(-1)
        vals = corner[live].reshape(-1)
        if defect == "contribution_twice_on_a_hot_entry" and lvl == 0:
            hot = np.bincount(flat).argmax()
            at = np.flatnonzero(flat == hot)
            j = at[np.abs(vals[at]).argmax()]
            flat, vals = np.append(flat, flat[j]), np.append(vals, vals[j])
        order = rs.permutation(flat.size)
        np.add.at(tab, flat[order], vals[order])
    return tab.reshape(-1, 2)


def _prefill(case, kind):
    if kind == "zero":
        return None
    return (np.random.RandomState(5).standard_normal((case.L * case.T, 2)) * 1e-3).astype(F32)


# ---------------------------------------------------------------- a correct fp32 evaluation passes ---------------------------------
@pytest.mark.parametrize("transform", list(pg.TRANSFORMS))
@pytest.mark.parametrize("grid", list(pg.GRIDS))
def test_fp32_dpositions_within_every_bound(lib, grid, transform):
    tf = pg.TRANSFORMS[transform]
    worst = {}
    for M in pg.POS_M:
        for mode in ("positions", "rays") if M % pg.POS_RAY_S == 0 else ("positions",):
            case = pg.position_case(grid, tf, M, mode)
            pg.check_dpositions(case, fp32_dpositions(lib, case), worst)
    report(f"fp32 dpositions {grid} {transform}", worst)
    _keep(f"dpositions {grid} {transform}", worst)


@pytest.mark.parametrize("transform", list(pg.TRANSFORMS))
@pytest.mark.parametrize("grid", pg.RAY_GRIDS)
def test_fp32_ray_gradients_within_every_bound(lib, grid, transform):
    tf = pg.TRANSFORMS[transform]
    worst = {}
    shapes = pg.RAY_SHAPES[grid]
    assert {S for _, S in shapes} == set(pg.RAY_S) and {n for n, _ in shapes} == set(pg.RAY_N)
    for n, S in shapes:
        case = pg.ray_case(grid, tf, n, S)
        dpos = fp32_dpositions(lib, case)
        d_o, d_d = fp32_ray_sums(case, dpos)
        pg.check_dpositions(case, dpos, worst)
        pg.check_rays(case, d_o, d_d, worst)
        pg.check_rays_against_dpositions(case, dpos, d_o, d_d, worst)
        prior = np.random.RandomState(n + S).standard_normal((n, 3)).astype(F32)
        pg.check_accumulate(case.name, prior, d_o, (prior + d_o).astype(F32))
    report(f"fp32 ray gradients {grid} {transform}", worst)
    _keep(f"rays {grid} {transform}", worst)


@pytest.mark.parametrize("batch", ["spread", "identical"])
@pytest.mark.parametrize("M", pg.TABLE_M)
@pytest.mark.parametrize("grid", list(pg.TABLE_GRIDS))
def test_fp32_table_gradient_within_every_bound(lib, grid, M, batch):
    case = pg.table_case(grid, M, batch)
    worst = {}
    for kind in ("zero", "random"):
        pre = _prefill(case, kind)
        pg.check_table(case, fp32_table(lib, case, pre, seed=M), pre, worst, name=f"dtable[{kind} prefill]")
    n = case.table_reference()[2]
    report(f"fp32 table gradient {case.name} (largest n_e {int(n.max())})", worst)
    _keep(f"table {grid} {batch} M={M}", worst)


def test_the_reference_is_the_moved_torch_evaluation_in_float64():
    """grid_gradient64 + position_gradient64 against _position_grad (the evaluation test_gpu_table_scatter.py's aggregate test
    uses, generalised to the three transforms) in float64: two restatements of one expression, equal to 1e-12 of the absolute terms."""
    for transform in pg.TRANSFORMS.values():
        case = pg.position_case("L5-T12", transform, 257)
        ref, bound = case.reference()["dpos"]
        moved = pg._position_grad(torch.from_numpy(case.raw), torch.from_numpy(case.table), [float(s) for s in case.scal], case.T,
                                  torch.from_numpy(case.denc), torch.float64, transform, torch.from_numpy(case.box)).numpy()
        assert bool((np.abs(moved - ref) <= 1e-5 * bound + 1e-300).all()), transform


def test_contract_linf_bwd_per_entry_against_float64_autograd(lib):
    """The host-compiled contract_linf_bwd on the branch-covering points and 2000 random ones against float64 autograd through
    orc.contract_linf (amax shares the norm's gradient equally between tied maxima), inside gamma_6 T1 + gamma_13 T2; and the
    reference's own float64 expression equal to autograd's to 1e-12 of its absolute terms."""
    rs = np.random.RandomState(11)
    pts = np.concatenate([pg.CONTRACT_POINTS, pg._random_points(rs, 2000, pg.XFORM_CONTRACT)]).astype(F32)
    g = (rs.choice([-1.0, 1.0], pts.shape) * 10.0 ** rs.uniform(-4, 1, pts.shape)).astype(F32)
    t = torch.from_numpy(pts).double().requires_grad_(True)
    orc.contract_linf(t).backward(torch.from_numpy(g).double())
    auto = t.grad.numpy()
    # position_gradient64 with G = 4 g and A = 0: an exact incoming gradient, the bound is the operation's own
    ref, bound = pg.position_gradient64(pts, np.ones(len(pts)), pg.XFORM_CONTRACT, None, 4.0 * g.astype(np.float64),
                                        np.zeros(pts.shape), 5)
    assert bool((np.abs(ref - auto) <= 1e-5 * bound + 1e-300).all())
    ax = np.abs(pts)
    far = ax.max(1) >= 1
    assert int(((ax == ax.max(1, keepdims=True)).sum(1)[far] >= 2).sum()) >= 7 and int((ax.max(1) == 1).sum()) >= 2
    mine = g.copy()
    lib.hc_contract_bwd(pts, mine, len(pts))
    worst = {}
    check_entries("contract_linf_bwd", mine, auto, bound, worst)
    assert np.array_equal(pg.bits(mine[~far]), pg.bits(g[~far]))  # the identity inside the unit cube
    report("contract_linf_bwd (host) against float64 autograd", worst)
    _keep("contract_linf_bwd against autograd", worst)


# ---------------------------------------------------------------- seeded defects ---------------------------------------------------
def _wrong(case, variant):
    return {k: v[0].astype(F32) for k, v in case.reference(variant).items()}


@pytest.mark.parametrize("variant,transform", [("scale_dropped_on_level_1", "none"), ("quarter_dropped", "contract"),
                                               ("aabb_other_axis", "aabb"), ("tie_to_the_first_maximum", "contract"),
                                               ("sign_taken_as_plus", "contract"), ("selector_ignored", "aabb"),
                                               ("selector_ignored", "contract")])
def test_a_defect_in_the_position_gradient_is_outside_a_bound(variant, transform):
    case = pg.position_case("L5-T12", pg.TRANSFORMS[transform], 257)
    pg.check_dpositions(case, _wrong(case, None)["dpos"], {})  # (the rounded reference itself passes)
    with pytest.raises(AssertionError):
        pg.check_dpositions(case, _wrong(case, variant)["dpos"], {})


@pytest.mark.parametrize("variant,shape", [("half_is_t_s", (5, 48)), ("sample_64_dropped", (257, 65)),
                                           ("credited_to_ray_r_plus_1", (5, 64))])
def test_a_defect_in_the_ray_sums_is_outside_a_bound(variant, shape):
    case = pg.ray_case("L5-T12", pg.XFORM_CONTRACT, *shape)
    good, bad = _wrong(case, None), _wrong(case, variant)
    pg.check_rays(case, good["d_origins"], good["d_directions"], {})
    with pytest.raises(AssertionError):
        pg.check_rays(case, bad["d_origins"], bad["d_directions"], {})
    if variant == "half_is_t_s":  # d_origins does not see the weight: the defect is d_directions' alone
        pg.check_rays(case, bad["d_origins"], good["d_directions"], {})


def test_accumulate_ignoring_the_prior_is_caught():
    case = pg.ray_case("L5-T12", pg.XFORM_CONTRACT, 5, 48)
    plain = _wrong(case, None)["d_origins"]
    prior = np.random.RandomState(3).standard_normal(plain.shape).astype(F32)
    pg.check_accumulate("d_origins", prior, plain, (prior + plain).astype(F32))
    with pytest.raises(AssertionError):
        pg.check_accumulate("d_origins", prior, plain, plain)


@pytest.mark.parametrize("defect", ["corner_pair_exchanged", "contribution_twice_on_a_hot_entry"])
def test_a_defect_in_the_table_scatter_is_outside_a_bound(lib, defect):
    """The exchanged pair: corners 0 and 1 of level 2 swap their entries. The doubled contribution: the largest one of the entry of
    level 0 that receives the most."""
    case = pg.table_case("L5-T12-one-slice", 8191, "spread")
    with pytest.raises(AssertionError):
        pg.check_table(case, fp32_table(lib, case, None, seed=1, defect=defect), None, {})


def test_zz_print_the_fp32_ratios():
    """Prints what the tests above measured (profiles/hash_position_gradient_float64_ratios.txt holds a copy); no criterion."""
    for group, worst in RATIOS.items():
        print(f"poshash-f64 cpu32 {group}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
