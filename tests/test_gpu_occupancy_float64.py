"""The six kernels that keep the instant-ngp occupancy grid alive (csrc/packed.hip: occgrid_cell_positions / _decay / _max /
_sum / _binarise / _coarse) ENTRY BY ENTRY against the references of tests/occupancy_reference.py (checked without a GPU in
tests/test_occupancy_reference_cpu.py), through the C ABI: nsamd_occgrid_cell_positions, _update, _binarise, _coarse_words,
and the marcher on the coarse bitfield that _binarise builds. Outputs are filled with NaN (bytes 0xFF, words -1) before a
launch and sit between guard rows of a sentinel that must come back untouched. Shapes: occupancy_reference.SHAPES.

Bounds (u = 2^-24; every bound times 1 + 2^-6 plus 2^-140, float64_check.check_entries). None is fitted to a result.

* Cell positions, x = (c - h) + (2 q) h with q = (ix + j) / R, c = (a + b) / 2, h = (b - a) / 2 * 2^level.
  - Bit for bit against the same fp32 operations in numpy (the library is built with -ffp-contract=off), including the final
    clamp to the fp32 numbers inside the cell's closed float64 box.
  - Against float64 of the fp32 inputs: s = fl(ix + j) and q = fl(s / R) leave q with 2u relative (ix is exact, q * 2 is
    exact); c = fl(fl(a + b) / 2) carries u |c|, h = fl(b - a) / 2 * 2^l carries u |h| (halving and the power of two are
    exact); lo = fl(c - h): u (|c| + |h| + |lo|); p = fl(2q h): 3u |p| from its factors + u |p|; x = fl(lo + p): + u |x|.
    Bound u (|c| + |h| + |lo| + 4 |p| + |x|). The clamp replaces x by the fp32 neighbour of a box edge only when x is outside
    the box that holds the float64 value: the result is within one ulp <= 2u |x| <= u (|c| + |h| + |x|) of it.
  - Containment: lo64 <= x <= hi64 of the cell's closed box, (c - h) + (ix / R) (2 h) and the same with ix + 1 in float64
    from the fp32 region of interest. WITHOUT the clamp the fp32 evaluation fails this at offsets 0 and nextafter(1, 0) for
    every R that is not a power of two (about half the entries at R = 84, by up to 4.1e-7 = one ulp; 10 - 20 of 7e6 entries
    with random offsets): that is what the clamp in the kernel and in OccGridEstimator._cell_positions is for.
  - Marcher: a ray through the position of a shell cell keeps steps only inside that cell. The slack on the midpoints is
    16 u times the largest coordinate in play (the marcher's own fp32 midpoint and index arithmetic: six roundings), five
    orders of magnitude below a cell.
* Update: exact. new[c] = fl32(old[c] * decay) is one IEEE fp32 product (gradual underflow), the maximum with estimates
  clamped at +0 is exact, a NaN estimate of either sign leaves NaN. Compared bit for bit, a NaN matching any NaN.
* Binarise: the mean runs over the n cells with occs >= 0, summed in double: any order is within n 2^-53 |mean| (all terms
  are >= 0, so sum |terms| = |sum|), the quotient adds 2^-53 and the cast to fp32 2^-24: threshold_out[1] within
  |mean| (2^-24 + n 2^-53). threshold_out[0] bit for bit: legitimate because every input's float64 mean is further than
  n 2^-53 |mean| from every fp32 rounding midpoint (asserted on the reference alone, here and in the CPU file). Binaries and
  coarse words are then exact.

Measured on the MI355X (worst |err| / bound over all shapes and cases of a check):
  cell positions vs float64     0.512  ((2,84), off-centre region, offset nextafter(1, 0); 0.472 at offset 0, 0.418 random;
                                        power-of-two R with the symmetric region: 0.000 at offset 0, <= 0.20 otherwise)
  ... flat indices beyond int32 0.246
  cell positions vs the fp32 restatement, containment, marcher agreement: exact / no entry outside, every shape
  update                        bit for bit on every shape; 0 cells differ
  threshold_out[1] (mean)       0.531  ((8,4); 0.35 - 0.53 on the other shapes, 0.000 at (1,1))
  threshold_out[0], binaries, coarse words: bit for bit on every shape and input
  marcher with / without the bitfield / oracle: identical at (2,12), (2,84) and (2,256)
Observed on the device:
  * NaN sign. `inf * 0` evaluated by the device (a torch elementwise kernel standing in for a diverged field) gives
    0xFFC00000, the NaN with the sign bit SET — the pattern an integer maximum on the raw bits drops. With the kernel's
    canonicalisation taken out, the update test and the module test with the device's own NaN fail.
  * Denormals survive. Every decayed value that is denormal in IEEE arithmetic came back with the reference's bits
    (556 635 of 556 635 such cells at (2,84), 3 714 of 3 714 at (2,16)): fp32 products are not flushed in this build, and
    denormal estimates are kept by the maximum.
  * The 64 KiB boundary. (2,256) launches: both marcher passes accept 65 536 bytes of dynamic LDS (the write pass on top of
    256 bytes of static LDS); coarse_words()'s admission rule stands as it is.
"""
import numpy as np
import pytest
import torch

import occupancy_reference as oref
from float64_check import check_entries, report
from oracle import packed_oracle as po

pytestmark = pytest.mark.gpu

f32 = np.float32
U = oref.U
GUARD = 64
S_F32, S_U8, S_I32, S_F64 = -7777.0, 0xA5, 0x5A5A5A5A, -7777.0
INVALID_ARG = -1


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


def _n():
    from nerfstudio_amd import _native as N

    return N


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()


def _p(t):
    return None if t is None else _n().ptr(t)


class Guarded:
    """`n` elements between two guard rows of `sentinel`; the interior starts as `fill`."""

    def __init__(self, n, dtype, sentinel, fill, row=1):
        self.n, self.g, self.sentinel = n * row, GUARD * row, sentinel
        self.whole = torch.full((self.n + 2 * self.g,), sentinel, dtype=dtype, device="cuda")
        self.t = self.whole[self.g:self.g + self.n]
        self.t.fill_(fill)

    def intact(self):
        w = self.whole
        return bool((w[:self.g] == self.sentinel).all()) and bool((w[self.g + self.n:] == self.sentinel).all())

    def np(self):
        return self.t.cpu().numpy()


def _grid_desc(levels, R, roi, binaries=None, coarse=None):
    g = _n().OccGrid()
    g.binaries = _p(binaries)
    g.levels, g.resolution = levels, R
    for i, v in enumerate(roi):
        g.aabb[i] = float(v)
    g.coarse = _p(coarse)
    return g


def run_positions(cells, M, levels, R, roi, jit):
    N = _n()
    out = Guarded(M, torch.float32, S_F32, float("nan"), row=3)
    cd = None if cells is None else _dev(cells)
    N.check(N.load().nsamd_occgrid_cell_positions(_p(cd), M, _grid_desc(levels, R, roi), _p(_dev(jit)), _p(out.t), N.stream()),
            "occgrid_cell_positions")
    torch.cuda.synchronize()
    assert out.intact(), "cell positions wrote outside [M, 3]"
    return out.np().reshape(M, 3)


def check_positions(tag, x, cells, M, R, roi, jit, worst):
    ref32 = oref.cell_positions_fp32(cells, M, R, roi, jit)
    assert not np.isnan(x).any(), f"{tag}: {int(np.isnan(x).sum())} entries not written"
    bad = np.flatnonzero((oref.bits(x) != oref.bits(ref32)).any(axis=1))
    assert bad.size == 0, f"{tag}: {bad.size} positions differ from the fp32 restatement, first {bad[:4]}: {x[bad[:2]]} vs {ref32[bad[:2]]}"
    x64, bound = oref.cell_positions64(cells, M, R, roi, jit)
    check_entries(tag, x, x64, bound, worst)
    lo, hi = oref.cell_boxes64(cells, M, R, roi)
    out = (x < lo) | (x > hi)
    assert not out.any(), f"{tag}: {int(out.sum())} entries outside their cell, by up to {np.maximum(lo - x, x - hi).max():.3e}"


# ---------------------------------------------------------------- 1. cell positions ------------------------------------------

@pytest.mark.parametrize("roi", sorted(oref.ROIS))
@pytest.mark.parametrize("levels,R", oref.SHAPES)
def test_cell_positions_bit_exact_within_float64_bound_and_inside_the_cell(F, levels, R, roi):
    worst = {}
    for name, cells, M, jit in oref.position_cases(levels, R):
        x = run_positions(cells, M, levels, R, oref.ROIS[roi], jit)
        check_positions(name.split()[-1], x, cells, M, R, oref.ROIS[roi], jit, worst)
    report(f"occgrid cell positions ({levels},{R}) {roi}", worst)


def test_cell_positions_of_flat_indices_beyond_int32(F):
    """levels = 8, R = 1024 through the raw entry point (the kernel touches no grid memory; none is allocated): cells next to
    8 * 2^30 - 1, on both sides of 2^31 and 2^32."""
    total = 8 * 2**30
    cells = np.array([total - 1, total - 2, total - 1025, 2**31, 2**31 - 1, 2**32 + 5, 2**32 - 1, 7 * 2**30, 0, 3 * 2**30 + 12345],
                     np.int64)
    rs = np.random.RandomState(2)
    worst = {}
    for roi in oref.ROIS.values():
        for jit in (np.full((len(cells), 3), 0.5, f32), rs.uniform(0, 1, (len(cells), 3)).astype(f32), np.zeros((len(cells), 3), f32)):
            x = run_positions(cells, len(cells), 8, 1024, roi, jit)
            check_positions("int64", x, cells, len(cells), 1024, roi, jit, worst)
    report("occgrid cell positions, flat indices beyond int32", worst)


@pytest.mark.parametrize("levels,R", [(1, 4), (3, 5), (2, 12), (8, 4), (2, 16)])
def test_cell_positions_agree_with_the_marcher(F, levels, R):
    """Only one shell cell set in `binaries`; an axis-parallel ray through the position cell_positions returns for offset 0.5
    keeps steps, every kept midpoint lies in that cell's box, and the same ray keeps nothing on an all-zero grid."""
    cells = oref.shell_cells(levels, R)
    for roi in oref.ROIS.values():
        a = np.asarray(roi, f32).astype(np.float64)
        c, h = (a[:3] + a[3:]) / 2, (a[3:] - a[:3]) / 2 * 2.0 ** (levels - 1)
        binaries = torch.zeros((levels, R, R, R), dtype=torch.uint8, device="cuda")
        x = F.occgrid_cell_positions(_dev(cells), len(cells), binaries, roi, _dev(np.full((len(cells), 3), 0.5, f32))).cpu().numpy()
        lo, hi = oref.cell_boxes64(cells, len(cells), R, roi)
        o, d = x.copy(), np.zeros_like(x)
        axis = np.arange(len(cells)) % 3
        o[np.arange(len(cells)), axis] = (c - h - 1.0)[axis]
        d[np.arange(len(cells)), axis] = 1.0
        steps = ((hi - lo)[np.arange(len(cells)), axis] / 6).astype(f32)
        slack = 16 * U * (np.abs(c) + h + 1.0).max()
        none = F.occgrid_march(_dev(o), _dev(d), binaries, roi, float(steps.min()), 0.0, 1e10)
        assert none[0].numel() == 0
        flat = binaries.view(-1)
        for k, cell in enumerate(cells):
            flat[int(cell)] = 1
            ri, ts, te, _ = F.occgrid_march(_dev(o[k:k + 1]), _dev(d[k:k + 1]), binaries, roi, float(steps[k]), 0.0, 1e10)
            flat[int(cell)] = 0
            ts, te = ts.cpu().numpy().astype(np.float64), te.cpu().numpy().astype(np.float64)
            assert 4 <= len(ts) <= 8, f"cell {cell}: {len(ts)} kept steps of a sixth of the cell"
            p = o[k].astype(np.float64) + d[k] * ((ts + te) / 2)[:, None]
            assert ((p >= lo[k] - slack) & (p <= hi[k] + slack)).all(), f"cell {cell}: a kept midpoint outside the cell"


# ---------------------------------------------------------------- 2. update --------------------------------------------------

def run_update(old, cells, est, decay, M=None):
    N = _n()
    total = len(old)
    occs = Guarded(total, torch.float32, S_F32, 0.0)
    occs.t.copy_(_dev(old))
    scratch = Guarded(total, torch.float32, S_F32, float("nan"))
    cd = None if cells is None else _dev(cells)
    N.check(N.load().nsamd_occgrid_update(_p(occs.t), total, _p(cd), _p(_dev(est)), len(est) if M is None else M, float(decay),
                                          _p(scratch.t), N.stream()), "occgrid_update")
    torch.cuda.synchronize()
    assert occs.intact() and scratch.intact(), "occgrid_update wrote outside occs / scratch"
    return occs.np()


@pytest.mark.parametrize("levels,R", oref.SHAPES)
def test_update_equals_the_reference_bit_for_bit(F, levels, R):
    total = oref.total_cells(levels, R)
    seen = dict(nan_pos=0, nan_neg=0, denormal_products=0, denormal_kept=0)
    for M, listed in [(m, True) for m in oref.UPDATE_LISTS] + [(total, False)]:
        old, cells, est = oref.update_case(total, M, listed, 1)
        ref = oref.update_reference(old, cells, est, 0.95)
        got = run_update(old, cells, est, 0.95)
        lst = np.arange(M) if cells is None else cells
        nan_cells = np.zeros(total, bool)
        nan_cells[lst[np.isnan(est)]] = True
        assert np.array_equal(np.isnan(got), nan_cells), f"M={M}: NaN cells {np.flatnonzero(np.isnan(got))[:6]} want {np.flatnonzero(nan_cells)[:6]}"
        bad = np.flatnonzero(~nan_cells & (oref.bits(got) != oref.bits(ref)))
        assert bad.size == 0, f"M={M} listed={listed}: {bad.size} cells differ, first {bad[:4]}: {got[bad[:4]]} vs {ref[bad[:4]]} (old {old[bad[:4]]})"
        untouched = np.ones(total, bool)
        untouched[lst] = False
        assert np.array_equal(oref.bits(got)[untouched], oref.bits(old)[untouched])
        assert oref.same_bits_nan_any(run_update(old, cells, est, 0.95), got), "a second run from the same state differs"
        assert np.array_equal(oref.bits(run_update(old, cells, est, 0.95, M=0)), oref.bits(old)), "M = 0 changed the grid"
        eb = est.view(np.uint32)
        seen["nan_pos"] += int((eb == oref.NAN_POS).sum())
        seen["nan_neg"] += int((eb == oref.NAN_NEG).sum())
        den = ~nan_cells & (ref > 0) & (ref < 2.0**-126)
        seen["denormal_products"] += int(den.sum())
        seen["denormal_kept"] += int((den & (oref.bits(got) == oref.bits(ref))).sum())
    assert seen["nan_pos"] > 0 and seen["nan_neg"] > 0
    print(f"\noccgrid update ({levels},{R}): {seen}")


# ---------------------------------------------------------------- 3. binarise ------------------------------------------------

def run_binarise(occs_d, levels, R, thre, with_stats=True, with_coarse=True, words=0, expect=0):
    N = _n()
    total = oref.total_cells(levels, R)
    B = Guarded(total, torch.uint8, S_U8, 0xFF)
    coarse = Guarded(max(words, 1), torch.int32, S_I32, -1)
    stats = Guarded(2, torch.float32, S_F32, float("nan"))
    scratch = Guarded(1024, torch.float64, S_F64, float("nan"))
    st = N.load().nsamd_occgrid_binarise(_p(occs_d), levels, R, float(thre), _p(B.t), _p(coarse.t) if with_coarse else None,
                                         _p(scratch.t), _p(stats.t) if with_stats else None, N.stream())
    torch.cuda.synchronize()
    assert st == expect, f"nsamd_occgrid_binarise returned {st}, expected {expect}"
    assert B.intact() and coarse.intact() and stats.intact() and scratch.intact(), "binarise wrote outside an output"
    return B, coarse, stats


@pytest.mark.parametrize("levels,R", oref.SHAPES)
def test_binarise_threshold_binaries_and_coarse_words(F, levels, R):
    from nerfstudio_amd.model_components.occupancy import OccGridEstimator

    words = oref.coarse_words_formula(levels, R)
    total = oref.total_cells(levels, R)
    blocks = levels * (R // 4) ** 3
    worst = {}
    module = OccGridEstimator(torch.tensor(oref.ROI_SYM), resolution=R, levels=levels)
    for kind in oref.BINARISE_KINDS:
        occs = oref.binarise_inputs(levels, R, kind)
        occs_d = _dev(occs)
        for thre in oref.binarise_thresholds_for(occs):
            ref_B, mean, ref_t, n = oref.thresholds(occs, thre)
            assert oref.mean_clear_of_midpoints(mean, n), (kind, mean)
            B, coarse, stats = run_binarise(occs_d, levels, R, thre, True, words > 0, words)
            got_t, got_mean = stats.np()
            check_entries("mean", [got_mean], [mean], [abs(mean) * (2.0**-24 + n * 2.0**-53)], worst)
            assert oref.bits([got_t])[0] == oref.bits([ref_t])[0], f"{kind} occ_thre {thre}: threshold {got_t!r} vs {ref_t!r} (mean {mean!r})"
            got_B = B.np()
            assert np.isin(got_B, (0, 1)).all(), f"{kind}: {int((got_B > 1).sum())} binaries not written"
            bad = np.flatnonzero(got_B.astype(bool) != ref_B)
            assert bad.size == 0, f"{kind} occ_thre {thre}: {bad.size} binaries differ, first {bad[:4]} occs {occs[bad[:4]]} threshold {ref_t!r}"
            if words:
                got_w = coarse.np().view(np.uint32)
                ref_w = oref.coarse_from_binaries(ref_B.reshape(levels, R, R, R))
                assert np.array_equal(got_w, ref_w), f"{kind}: coarse words differ at {np.flatnonzero(got_w != ref_w)[:4]}"
                bits = ((got_w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)
                assert not bits[blocks:].any()
                module.binaries.copy_(torch.from_numpy(got_B.reshape(levels, R, R, R)))
                module._coarse = torch.full((words,), -1, dtype=torch.int32)
                module._rebuild_coarse_from_binaries()
                assert np.array_equal(module._coarse.numpy().view(np.uint32), got_w)
            else:
                assert int(coarse.t[0]) == -1
            # without threshold_out / without the coarse words: the same binaries, nothing else written
            for with_stats, with_coarse in ((False, words > 0), (True, False), (False, False)):
                B2, coarse2, stats2 = run_binarise(occs_d, levels, R, thre, with_stats, with_coarse, words)
                assert torch.equal(B2.t, B.t)
                assert bool(torch.isnan(stats2.t).all()) != with_stats
                assert torch.equal(coarse2.t, coarse.t) if with_coarse else bool((coarse2.t == -1).all())
    if words == 0 and R % 4:  # a coarse pointer for a shape without a bitfield: refused, nothing launched
        B, coarse, stats = run_binarise(occs_d, levels, R, 0.01, True, True, 0, expect=INVALID_ARG)
        assert bool((B.t == 0xFF).all()) and bool(torch.isnan(stats.t).all()) and int(coarse.t[0]) == -1
    report(f"occgrid binarise ({levels},{R})", worst)


def test_coarse_words_equal_the_formula(F):
    lib = _n().load()
    for levels, R in oref.COARSE_WORDS_TABLE:
        assert int(lib.nsamd_occgrid_coarse_words(levels, R)) == oref.coarse_words_formula(levels, R), (levels, R)
    assert int(lib.nsamd_occgrid_coarse_words(2, 256)) == 16384
    assert int(lib.nsamd_occgrid_coarse_words(3, 256)) == 0 and int(lib.nsamd_occgrid_coarse_words(1, 1024)) == 0
    assert int(lib.nsamd_occgrid_coarse_words(1, 5)) == 0


# ---------------------------------------------------------------- 4. marcher on the new coarse shapes ------------------------

@pytest.mark.parametrize("levels,R", [(2, 12), (2, 84), oref.BOUNDARY_SHAPE])
def test_marcher_on_coarse_bits_with_a_partial_last_word_and_at_the_lds_boundary(F, levels, R):
    """Binaries and coarse words from nsamd_occgrid_binarise (clustered and random grids); 64 rays; the marcher with the
    bitfield, without it and the oracle agree bit for bit. (2,256) asks for exactly 64 KiB of dynamic LDS."""
    words = oref.coarse_words_formula(levels, R)
    assert words > 0 and (words == 16384 or (levels * (R // 4) ** 3) % 32 != 0)
    o, d, jit = oref.march_rays(64, 5)
    for kind in ("clustered", "random"):
        occs = oref.march_grid(levels, R, kind)
        B, coarse, _ = run_binarise(_dev(occs), levels, R, 0.01, True, True, words)
        binaries = B.t.view(levels, R, R, R)
        ref_B = po.occgrid_thresholds(occs, 0.01).reshape(levels, R, R, R)
        assert np.array_equal(B.np().astype(bool).reshape(ref_B.shape), ref_B)
        assert np.array_equal(coarse.np().view(np.uint32), oref.coarse_from_binaries(ref_B))
        args = (_dev(o), _dev(d), binaries, oref.ROI_SYM, 0.02, 0.05, 50.0, None, None, 0.004, _dev(jit))
        with_bits = F.occgrid_march(*args, coarse=coarse.t)
        without = F.occgrid_march(*args)
        ref = po.occgrid_march(o, d, ref_B, oref.ROI_SYM, 0.02, near_plane=0.05, far_plane=50.0, cone_angle=0.004, jitter=jit)
        assert len(ref[0]) > 50
        for a, b, c_ in zip(with_bits[:3], without[:3], ref):
            np.testing.assert_array_equal(a.cpu().numpy(), c_)
            np.testing.assert_array_equal(b.cpu().numpy(), c_)
        assert torch.equal(with_bits[3], without[3])


# ---------------------------------------------------------------- 5. module level --------------------------------------------

def _planted(pattern):
    return lambda v: torch.tensor([pattern - (1 << 32) if pattern >= 1 << 31 else pattern], dtype=torch.int32,
                                  device=v.device).view(torch.float32)


@pytest.mark.parametrize("source", ["inf_times_zero", "positive_nan", "negative_nan"])
def test_one_nan_estimate_does_not_empty_the_grid_on_the_device(F, source):
    """update_every_n_steps(step = 0) on the device with a field that returns NaN for one position — from the device's own
    arithmetic (inf * 0; the bit pattern it produced is printed) and with both quiet patterns planted —: the cell is NaN,
    binaries == the oracle's thresholds, the cached mean is the finite mean of the seen cells, sampling returns samples."""
    from nerfstudio_amd.model_components.occupancy import OccGridEstimator

    g = OccGridEstimator(torch.tensor(oref.ROI_SYM), resolution=8, levels=1).cuda().train()
    make = {"inf_times_zero": lambda v: torch.full_like(v, float("inf")) * torch.zeros_like(v),
            "positive_nan": _planted(oref.NAN_POS), "negative_nan": _planted(oref.NAN_NEG)}[source]
    torch.manual_seed(0)
    est = oref.nan_refresh(g, 77, make)
    pattern = int(est.numpy().view(np.uint32)[77, 0])
    print(f"\nNaN estimate ({source}): bits 0x{pattern:08X}")
    assert pattern & 0x7FFFFFFF > 0x7F800000
    oref.check_nan_refresh(g, 77)
    o = torch.tensor([[0.0, 0.0, -3.0], [0.1, -3.0, 0.05]], device="cuda")
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], device="cuda")
    ri, ts, te = g.sampling(o, d, render_step_size=0.05, near_plane=0.0, far_plane=10.0, alpha_thre=0.01)
    assert ri.numel() > 4 and np.isfinite(g._occ_mean)


def test_cell_draws_after_warm_up_on_the_device(F):
    oref.draws_case("cuda")
