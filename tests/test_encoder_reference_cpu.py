"""tests/encoder_reference.py checked where there is no GPU: against the fixtures the reference wrote (tests/golden/hashgrid.npz,
vanilla.npz, kat.npz) and against the fp32 oracle, on the very cases tests/test_gpu_encoders_float64.py launches — the fp32 oracle
alone has to stay inside every bound those tests hold the kernels to (the bounds are derived in that module's docstring)."""
import os

import numpy as np
import pytest
import torch

import encoder_reference as er
from float64_check import E_SIN, U, check_entries, report
from oracle import nerfacto_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    """Bit equality of two fp32 arrays, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def test_hash_features64_against_the_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "hashgrid.npz"))
    L = g["scalings"].shape[0]
    log2_T = int(np.log2(g["table"].shape[0] // L))
    assert L << log2_T == g["table"].shape[0]
    enc64, A = er.hash_features64(g["x"], g["table"], g["scalings"], log2_T)
    worst = {}
    check_entries("fixture", g["out"], enc64, er.HASH_ROUNDINGS * U * A, worst)
    assert float(A.min()) > 0 and bool((np.abs(enc64) <= A * (1 + 1e-12)).all())
    report("hash_features64 vs hashgrid.npz", worst)


@pytest.mark.parametrize("grid", list(er.HASH_GRIDS) + list(er.FUSED_GRIDS))
@pytest.mark.parametrize("transform", list(er.TRANSFORMS))
def test_fp32_oracle_stays_inside_the_hash_bound_on_every_gpu_case(grid, transform):
    """orc.hashgrid_encode (the fp32 reference the kernels are bit-equal to) within 9 u A of hash_features64 on the points of every
    hash-grid and fused-forward case; positions32 / normalise32 bit-equal to orc.sample_positions / orc.normalise_positions."""
    if grid in er.HASH_GRIDS:
        L, lo, hi, log2_T = er.HASH_GRIDS[grid]
        cases = er.hash_cases
    else:
        L, _, lo, hi, log2_T = er.FUSED_GRIDS[grid]
        cases = er.fused_cases
    tf = er.TRANSFORMS[transform]
    table, scal = er.table32(L, log2_T), er.scalings32(L, lo, hi)
    worst, zeros = {}, 0
    for mode in ("positions", "rays"):
        for label, pts, M in cases(mode, tf, lo):
            raw = er.positions32(pts)
            assert raw.shape == (M, 3) and np.isfinite(raw).all()
            if mode == "rays":
                want = orc.sample_positions(*(torch.from_numpy(pts[k]) for k in ("origins", "directions", "t_bins")))
                assert _same_bits(raw, want.reshape(-1, 3).numpy()), label
            x, sel = er.normalise32(raw, tf)
            if tf != er.XFORM_NONE:
                wx, ws = orc.normalise_positions(torch.from_numpy(raw), tf == er.XFORM_CONTRACT, torch.from_numpy(er.BOX))
                assert _same_bits(x, wx.numpy()) and np.array_equal(sel, ws.numpy().astype(np.float32)), label
                zeros += int((sel == 0).sum())
            else:
                assert _same_bits(x, raw) and bool((sel == 1).all())
            enc32 = orc.hashgrid_encode(torch.from_numpy(x), torch.from_numpy(table), torch.from_numpy(scal), 1 << log2_T).numpy()
            enc64, A = er.hash_features64(x, table, scal, log2_T)
            check_entries(mode, enc32, enc64, er.HASH_ROUNDINGS * U * A, worst)
    assert tf == er.XFORM_NONE or zeros > 0  # the selector's zero side is among the cases
    report(f"fp32 oracle vs hash_features64, {grid} {transform}", worst)


def test_position_cases_hold_their_edges():
    """The positions cases carry what they promise: lattice planes of the coarsest level, exact 0 and 1 under NONE, both selector
    values and the contraction's edges under CONTRACT."""
    none = er.position_case(257, er.XFORM_NONE, 16, 1)["positions"]
    assert (none == 0).any() and (none == 1).any() and ((none * 16 == np.round(none * 16)) & (none > 0) & (none < 1)).any()
    for tf in (er.XFORM_CONTRACT, er.XFORM_AABB):
        x, sel = er.normalise32(er.position_case(257, tf, 16, 1)["positions"], tf)
        assert 0 < int(sel.sum()) < 257
        inside = x[sel == 1]
        assert ((inside * 16 == np.round(inside * 16)).all(-1)).any()
    edges = er.contract_edges()
    mag = np.abs(edges).max(-1)
    for m in (1.0, float(np.nextafter(np.float32(1), np.float32(0))), 3.0, 1e3, 1e30):
        assert (mag == np.float32(m)).any()
    ties = (np.abs(edges) == mag[:, None]).sum(-1)
    assert (ties == 2).any() and (ties == 3).any()


def test_contract32_is_the_oracle_bit_for_bit():
    for M in (1, 255, 257):
        x = er.contract_inputs(M, M)
        assert _same_bits(er.contract32(x), orc.contract_linf(torch.from_numpy(x)).numpy())
    x = er.contract_inputs(257, 0)
    assert np.isnan(x).any() and np.isinf(x).any() and (np.abs(x).max(-1) == 1).any()
    kat = np.load(os.path.join(GOLDEN, "kat.npz"))
    assert _same_bits(er.contract32(kat["contract_in"]), kat["contract_out"])


def test_nerf_rows64_against_the_reference_fixture():
    """The rows the reference's NeRFEncoding wrote (fp32 torch) lie within an fp32 sine's distance, E_SIN |sin| + u 2^-23, of the
    float64 rows; the raw-input columns are copies."""
    g = np.load(os.path.join(GOLDEN, "vanilla.npz"))
    x = g["enc_x"]
    worst = {}
    for name, (F, e, inc) in (("enc_pos", (10, 8.0, True)), ("enc_dir", (4, 4.0, True)), ("enc_plain", (6, 5.0, False))):
        rows = er.nerf_rows64(x, er.nerf_freqs(F, e), inc)
        assert rows.shape == g[name].shape
        check_entries(name, g[name][:, : 6 * F], rows[:, : 6 * F], E_SIN * np.abs(rows[:, : 6 * F]) + U * 2.0**-23, worst)
        if inc:
            assert _same_bits(g[name][:, 6 * F :], x)
    report("nerf_rows64 vs vanilla.npz", worst)


def test_nerf_rows64_non_finite_and_layout():
    x = er.nerf_inputs(9, 0)
    rows = er.nerf_rows64(x, er.nerf_freqs(2, 1), True)
    assert rows.shape == (9, 15)
    bad = ~np.isfinite(x)
    assert bad.sum() == 3
    s_nan = np.repeat(bad, 2, axis=1)  # column d F + f
    assert np.array_equal(np.isnan(rows[:, :6]), s_nan) and np.array_equal(np.isnan(rows[:, 6:12]), s_nan)
    assert rows[4, 0] == 0.0 and rows[4, 6] == pytest.approx(1.0)  # sin(0), sin(pi / 2)


def test_sh4_64_known_answers_and_the_fp32_oracle():
    kat = np.load(os.path.join(GOLDEN, "kat.npz"))
    worst = {}
    sh, mono = er.sh4_64(kat["sh_in"])
    check_entries("kat", kat["sh_out"], sh, er.SH_ROUNDINGS * U * mono, worst)
    for M in (65, 257):
        d = er.sh_inputs(M, M)
        sh, mono = er.sh4_64(d)
        assert bool((np.abs(sh) <= mono * (1 + 1e-12))[np.isfinite(sh)].all())
        check_entries("oracle", orc.sh_levels4(torch.from_numpy(d)).numpy(), sh, er.SH_ROUNDINGS * U * mono, worst)
    report("sh4_64 vs the known answer and the fp32 oracle", worst)


def test_density64_bounds_shrink_with_the_feature_error():
    """density64 is orc.density_mlp_fwd64 plus the bounds: with exact features dpre is the bound test_density_mlp_forward_vs_float64
    uses, a feature error adds |W1| . (|W0| @ err), and a zero selector gives density and bound 0."""
    rs = np.random.RandomState(0)
    enc = rs.standard_normal((33, 10))
    sel = (rs.uniform(0, 1, 33) > 0.3).astype(np.float64)
    mlp = er.mlp_params(10, 16, 3)
    r0 = er.density64(enc, np.zeros_like(enc), sel, mlp, 0.01)
    r1 = er.density64(enc, np.full_like(enc, 1e-6), sel, mlp, 0.01)
    W0, _, W1, _ = mlp
    base = 10 * U * (r0["a_abs"] @ W1.double().abs().reshape(-1)) + 16 * U * r0["pre_abs"]
    assert torch.allclose(r0["dpre"], base, rtol=1e-12, atol=0)
    extra = 1e-6 * (W0.double().abs().sum(1) @ W1.double().abs().reshape(-1))
    assert torch.allclose(r1["dpre"] - r0["dpre"], torch.full((33,), float(extra), dtype=torch.float64), rtol=1e-9, atol=0)
    off = torch.from_numpy(sel == 0)
    assert bool((r0["density"][off] == 0).all()) and bool((r0["ddensity"][off] == 0).all()) and bool((r0["density"][~off] > 0).all())
