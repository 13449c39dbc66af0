"""The references of tests/occupancy_reference.py (what tests/test_gpu_occupancy_float64.py holds the occupancy-grid refresh
kernels to) against each other, against oracle/packed_oracle.py, and OccGridEstimator on CPU tensors against them. No GPU."""
import numpy as np
import pytest
import torch

import occupancy_reference as oref
from float64_check import check_entries
from oracle import packed_oracle as po

f32 = np.float32


def _grid(levels, R, roi=oref.ROI_SYM):
    from nerfstudio_amd.model_components.occupancy import OccGridEstimator

    return OccGridEstimator(torch.tensor(roi), resolution=R, levels=levels).train()


# ---------------------------------------------------------------- cell positions ---------------------------------------------

@pytest.mark.parametrize("roi", sorted(oref.ROIS))
@pytest.mark.parametrize("levels,R", oref.SHAPES)
def test_position_restatement_within_the_float64_bound_inside_its_cell_and_equal_to_the_cpu_path(levels, R, roi):
    """The fp32 restatement: within the derived bound of float64 per entry, inside the closed float64 box of its cell, and bit
    for bit what OccGridEstimator._cell_positions gives on CPU tensors."""
    g = _grid(levels, R, oref.ROIS[roi])
    worst = {}
    for name, cells, M, jit in oref.position_cases(levels, R):
        x = oref.cell_positions_fp32(cells, M, R, oref.ROIS[roi], jit)
        x64, bound = oref.cell_positions64(cells, M, R, oref.ROIS[roi], jit)
        check_entries(name.split()[-1], x, x64, bound, worst)
        lo, hi = oref.cell_boxes64(cells, M, R, oref.ROIS[roi])
        assert ((x >= lo) & (x <= hi)).all(), name
        got = g._cell_positions(None if cells is None else torch.from_numpy(cells), M, torch.from_numpy(jit))
        assert np.array_equal(oref.bits(got.numpy()), oref.bits(x)), name
    assert max(worst.values()) <= 1.0


def test_unclamped_fp32_positions_leave_their_cell_at_the_edges_of_the_offset_range():
    """Why the kernel clamps: at R = 5 (cell edges that are no fp32 numbers) the plain fp32 evaluation with offset 0 or
    nextafter(1, 0) lands outside the closed box of its cell for a good share of the entries, by about an ulp."""
    M = 125
    for jit in (np.zeros((M, 3), f32), np.full((M, 3), oref.JITTER_ONE, f32)):
        x = oref.cell_positions_fp32(None, M, 5, oref.ROI_SYM, jit, clamp=False)
        lo, hi = oref.cell_boxes64(None, M, 5, oref.ROI_SYM)
        out = (x < lo) | (x > hi)
        assert 0.05 < out.mean() < 0.9 and np.maximum(lo - x, x - hi).max() < 4 * 2.0**-24


def test_positions_of_cells_with_flat_indices_beyond_int32():
    """levels = 8, R = 1024: the last cell is 8 * 2^30 - 1; the restatement splits it into level 7 and the last index."""
    total = 8 * 2**30
    cells = np.array([total - 1, total - 2, 2**31, 2**31 - 1, 2**32 + 5, 7 * 2**30], np.int64)
    x = oref.cell_positions_fp32(cells, len(cells), 1024, oref.ROI_SYM, np.full((len(cells), 3), 0.5, f32))
    assert np.array_equal(x[0], np.full(3, 128.0 - 0.125, f32))           # level 7: box [-128, 128], cells of 0.25
    assert np.array_equal(x[5], np.full(3, -128.0 + 0.125, f32))          # first cell of level 7
    assert np.array_equal(x[2], np.full(3, -4.0, f32) + f32(8.0 / 1024 * 0.5))  # first cell of level 2


# ---------------------------------------------------------------- update -----------------------------------------------------

@pytest.mark.parametrize("M,listed", [(1, True), (257, True), (5000, True), (375, False)])
def test_update_reference_properties(M, listed):
    total = 375
    old, cells, est, = oref.update_case(total, M, listed, 3)
    new = oref.update_reference(old, cells, est, 0.95)
    lst = np.arange(M) if cells is None else cells
    untouched = np.ones(total, bool)
    untouched[lst] = False
    assert np.array_equal(oref.bits(new)[untouched], oref.bits(old)[untouched])
    got_nan = np.zeros(total, bool)
    got_nan[lst[np.isnan(est)]] = True
    assert np.array_equal(np.isnan(new), got_nan) and got_nan.any()
    decayed = (old * f32(0.95)).astype(f32)
    ok = ~untouched & ~got_nan
    assert (new[ok] >= decayed[ok]).all() and not np.signbit(new[ok]).any()
    if M >= 257:  # gradual underflow is part of the case: denormal products that are not zero
        assert ((decayed[~untouched] > 0) & (decayed[~untouched] < 2.0**-126)).sum() > 5
    perm = np.random.RandomState(0).permutation(M)  # the order of the list does not matter
    again = oref.update_reference(old, lst[perm], est[perm], 0.95)
    assert oref.same_bits_nan_any(again, new)
    if M == 5000:
        assert np.bincount(cells).max() >= 2000 and (cells == 0).any() and cells[-1] == total - 1


# ---------------------------------------------------------------- thresholds, binaries, coarse bits --------------------------

@pytest.mark.parametrize("levels,R", oref.SHAPES)
def test_threshold_reference_equals_the_oracle_and_the_cpu_path_and_its_means_are_clear_of_midpoints(levels, R):
    """For every input of the GPU test: binaries == oracle/packed_oracle.occgrid_thresholds; the float64 mean is further than
    n 2^-53 |mean| from every fp32 rounding midpoint (what lets the GPU test ask for the threshold bit for bit); and
    OccGridEstimator._refresh_derived on CPU tensors gives the same binaries and the same mean."""
    g = _grid(levels, R)
    for kind in oref.BINARISE_KINDS:
        occs = oref.binarise_inputs(levels, R, kind)
        for thre in oref.binarise_thresholds_for(occs):
            B, mean, t, n = oref.thresholds(occs, thre)
            assert np.array_equal(B, po.occgrid_thresholds(occs, thre)), (kind, thre)
            assert oref.mean_clear_of_midpoints(mean, n), (kind, mean)
            g.occs.copy_(torch.from_numpy(occs))
            g._refresh_derived(thre)
            assert np.array_equal(g.binaries.numpy().reshape(-1).astype(bool), B), (kind, thre)
            if np.isfinite(mean):
                assert abs(g._occ_mean - mean) <= abs(mean) * (2.0**-24 + n * 2.0**-53), (kind, g._occ_mean, mean)
            else:
                assert g._occ_mean == mean
        if kind in ("nan1", "nanfew", "negfew"):
            assert n == occs.size - min(occs.size, 1 if kind == "nan1" else 5)
        if kind == "equal":  # equal values: the mean is the value itself; empty unless occ_thre is below it
            assert not oref.thresholds(occs, 0.5)[0].any() and oref.thresholds(occs, 0.01)[0].all()


def test_threshold_reference_of_a_grid_without_a_seen_cell_is_zero():
    occs = np.full(64, np.nan, f32)
    B, mean, t, n = oref.thresholds(occs, 0.01)
    assert n == 0 and mean == 0.0 and t == 0.0 and not B.any()
    g = _grid(1, 4)
    g.occs.copy_(torch.from_numpy(occs))
    g._refresh_derived(0.01)
    assert g._occ_mean == 0.0 and not g.binaries.any()


@pytest.mark.parametrize("levels,R", [s for s in oref.SHAPES if s[1] % 4 == 0])
def test_coarse_reference_equals_the_module_rebuild_bit_for_bit(levels, R):
    """coarse_from_binaries against OccGridEstimator._rebuild_coarse_from_binaries on CPU tensors, random, full (bit 31 of
    every full word set) and single-cell binaries; the bits beyond the last block are zero."""
    words = oref.coarse_words_formula(levels, R)
    blocks = levels * (R // 4) ** 3
    assert words == (blocks + 31) // 32 > 0
    g = _grid(levels, R)
    rs = np.random.RandomState(R)
    last = np.zeros((levels, R, R, R), bool)
    last[-1, -1, -1, -1] = True
    for B in (rs.rand(levels, R, R, R) > 0.97, np.ones((levels, R, R, R), bool), last):
        ref = oref.coarse_from_binaries(B)
        g.binaries.copy_(torch.from_numpy(B.astype(np.uint8)))
        g._coarse = torch.full((words,), -1, dtype=torch.int32)
        g._rebuild_coarse_from_binaries()
        assert np.array_equal(g._coarse.numpy().view(np.uint32), ref)
        bits = ((ref[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)
        assert not bits[blocks:].any() and bits[:blocks].sum() == B.reshape(levels, R // 4, 4, R // 4, 4, R // 4, 4).any(axis=(2, 4, 6)).sum()
    assert bits[blocks - 1] and bits.sum() == 1  # the last cell sets the last block's bit and no other


def test_coarse_words_formula_table():
    f = oref.coarse_words_formula
    assert f(2, 256) == 16384 and f(3, 256) == 0 and f(1, 1024) == 0 and f(1, 5) == 0 and f(3, 5) == 0 and f(2, 254) == 0
    assert f(1, 4) == 1 and f(2, 12) == 2 and f(2, 16) == 4 and f(8, 4) == 1 and f(2, 84) == 579 and f(1, 128) == 1024
    assert oref.BOUNDARY_SHAPE in oref.COARSE_WORDS_TABLE


# ---------------------------------------------------------------- module level -----------------------------------------------

def test_one_nan_estimate_does_not_empty_the_grid_on_cpu_tensors():
    """update_every_n_steps with a field that returns NaN (inf * 0) for one position: binaries == the oracle's thresholds of
    the refreshed occs (a quarter of the 8^3 grid occupied; with the mean taken over EVERY cell the threshold was NaN and the
    grid came out empty), and the cached mean is the finite mean of the seen cells."""
    g = _grid(1, 8)
    torch.manual_seed(0)
    est = oref.nan_refresh(g, 77, lambda v: torch.full_like(v, float("inf")) * 0.0)
    assert np.isnan(est.numpy()[77]).all()
    oref.check_nan_refresh(g, 77)


def test_cell_draws_after_warm_up_on_cpu_tensors():
    oref.draws_case("cpu")
