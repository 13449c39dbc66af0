"""The kernels that turn a position or a direction into network inputs, ENTRY BY ENTRY against the float64 references of
tests/encoder_reference.py: nsamd_density_field_fwd (all four instantiations of density_field_fwd_kernel), the three forward kernels
of nsamd_hashgrid_encode_fwd (four levels per thread, lane pairs with and without the XCD level sweep) in the point-major,
feature-major and padded layouts with and without the selector, nsamd_nerf_encode, nsamd_sh4_encode and nsamd_contract_linf.
The arithmetic helpers are checked on the CPU (tests/test_kernel_helpers_cpu.py); what only exists on the GPU is checked here:
indexing, strides, the lane-pair exchange, the level sweep, the dispatch, the device sinf / expf and the edges of M.

The rounding-free part of every operation (load_position, normalise_position, the cell and its weights, the hash; the sine's
argument) is restated in fp32 by the reference, so a bound only has to cover what comes after it. Every check is |got - ref64| <=
bound per entry through float64_check.check_entries (x SAFE = 1 + 2^-6 for second-order terms, + TINY), u = 2^-24:

* Hash feature (common.h trilinear_blend). The weights w = sx - floor(sx) are exact in fp32. A lerp stage is
  fl(fl(q1 w) + fl(q0 fl(1 - w))): the term q1 w passes the product and the sum (2 roundings), the term q0 (1 - w) passes fl(1 - w)
  (at most u relative: exact for w >= 1/2, an absolute 2^-25 on a value > 1/2 otherwise), the product and the sum (3). Three stages
  (x, y, z), each acting on the results of the one before: at most 9 roundings on any path from a table value to the feature, so
  |enc - enc64| <= 9 u A with A the same blend of |q_k| (every stage's |result| is at most the blend of the |operands|). The
  bound does not depend on the order of the corners, of the axes or of a stage's two products.
* Fused pre-activation. Hidden a_j = fmaf chain over IN features on top of b0: IN u a_abs_j, plus the features' own error through
  |W0|; ReLU is 1-Lipschitz, so no point is left out; pre = fmaf chain over H: dpre = |W1| . (|W0| @ enc_err) + IN u (a_abs @ |W1|)
  + H u pre_abs — the bound of test_gpu_proposal_backward.py::test_density_mlp_forward_vs_float64 plus the propagated term.
* Fused density = (avg expf(pre)) sel: density64 (dpre (1 + dpre) + E_EXP + 2u) (exp(d) - 1 <= d (1 + d) for small d; E_EXP: the
  device expf charged 2 ulp, an assumption, float64_check.py); exactly 0 where the selector is 0.
* nsamd_nerf_encode. The argument s = fl(fl(2pi x) freq) (and fl(s + pi/2)) is reproduced in fp32, so the only error is the
  device sinf: E_SIN |sin64| + u 2^-23, the second term for results next to a zero of the sine. E_SIN = 2 ulp ASSUMED, as E_EXP
  is: the toolchain ships no ULP table of the device math library to take a documented figure from. It is not fitted to the
  kernel. The raw-input columns are copies: bit-exact.
* nsamd_sh4_encode (common.h sh4_components): k_i u mono_i with mono_i the sum of the |monomials| of component i and k_i the
  largest number of fp32 roundings any of its monomials passes through — the rounding of the float64 constant to fp32 counts,
  3.0f and 5.0f are exact, both factors of a product count:
    c0 = C: 1.   c1..c3 = C v: constant, product: 2.   c4, c5, c7 = (C a) b: 3.   c10 = ((C x) y) z: 4.
    c6 = C zz - C': zz, C, product, difference: 4.   c8 = C (xx - yy): xx, difference, C, product: 4.
    c9, c15 = (C a) (3 bb - cc) and c11, c12, c13 = (C a) (5 zz - n): C, C a, the square, its multiple, the difference, the
    product: 6.   c14 = (C z) (xx - yy): C, C z, xx, difference, product: 5.
* nsamd_contract_linf: bit-exact against contract32 (IEEE division; no transcendental), a NaN matching a NaN.
The selector and everything the two-kernel pair also computes are bit-exact.

Every output buffer is prefilled with NaN and sits between two guards of four rows; the guards, the padding columns and everything a
call must not address have to come back untouched.

Worst |err| / bound measured on MI355X over all parametrisations (every test prints its own line):
  fused forward   enc 0.446   pre 0.027   density 0.049       hash forward (all three kernels, all layouts)   0.376
  nerf_encode     sin 0.504 (F = 64; 0.471 at arguments up to 1.6e6: about one ulp, inside the assumed two at every size)
  sh4_encode      degree 0: 0.858 (the constant's own rounding)   degree 1: 0.587   degree 2: 0.823   degree 3: 0.459
  contract_linf, the selector, the raw-input columns, fused = pair: no bit differs.
The first run found nsamd_contract_linf wrong on rows that hold a NaN beside finite values: fmaxf drops a NaN operand, so the row's
norm came out finite and (NaN, 3, 0.5) gave (NaN, 1.667, 0.278) where the reference gives three NaN. common.h's contract_linf now
makes the norm of such a row NaN; finite rows take the same operations as before.
"""
import numpy as np
import pytest
import torch

import encoder_reference as er
from float64_check import E_SIN, U, check_entries, report
from oracle import nerfacto_oracle as orc

pytestmark = pytest.mark.gpu

OK, ERR_INVALID_ARG, ERR_UNSUPPORTED = 0, -1, -2
AVG = 0.01
NAN = float("nan")
INSTANTIATIONS = [g for g in er.FUSED_GRIDS if "shipped" not in g]


@pytest.fixture(scope="module")
def N():
    from nerfstudio_amd import _native

    _native.load()
    return _native


def _same_bits(a, b):
    """Bit equality of two fp32 arrays, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


class Guarded:
    """n floats of NaN on the device between two guards of NaN (four rows of `row` floats each, 256-byte granules)."""

    def __init__(self, n, row):
        self.n, self.pad = n, -(-4 * max(row, 1) // 64) * 64
        self.buf = torch.full((n + 2 * self.pad,), NAN, device="cuda")

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.pad

    def body(self):
        return self.buf[self.pad : self.pad + self.n].cpu().numpy()

    def guards_untouched(self):
        return bool(torch.isnan(self.buf[: self.pad]).all()) and bool(torch.isnan(self.buf[self.pad + self.n :]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


_DEVICE = {}


def _table(L, log2_T):
    key = (L, log2_T)
    if key not in _DEVICE:
        _DEVICE[key] = torch.from_numpy(er.table32(L, log2_T)).cuda()
    return er.table32(L, log2_T), _DEVICE[key]


def _points(N, pts):
    """(nsamd_points, the device tensors it points into)."""
    if pts.get("positions") is not None:
        keep = (torch.from_numpy(pts["positions"]).cuda(),)
        return N.make_points(positions=keep[0]), keep
    keep = tuple(torch.from_numpy(pts[k]).cuda() for k in ("origins", "directions", "t_bins"))
    return N.make_points(None, *keep, pts["t_bins"].shape[1] - 1), keep


def _box(N, transform):
    return N.make_aabb(torch.from_numpy(er.BOX)) if transform == er.XFORM_AABB else N.Aabb()


class _Mlp:
    def __init__(self, N, in_dim, hidden, seed):
        self.host = er.mlp_params(in_dim, hidden, seed)
        self.dev = [t.cuda().contiguous() for t in self.host]
        self.native = N.DensityMlp(*[N.ptr(t) for t in self.dev], in_dim, hidden, AVG)


def _fused(N, P, M, tf, table, grid, mlp, enc, sel, dens, pre):
    p = lambda b: None if b is None else b.ptr  # noqa: E731
    rc = N.load().nsamd_density_field_fwd(P, M, tf, _box(N, tf), N.ptr(table), grid, mlp.native, p(enc), p(sel), p(dens), p(pre),
                                          N.stream())
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------- nsamd_density_field_fwd -----------------------------------------

@pytest.mark.parametrize("mode", ["positions", "rays"])
@pytest.mark.parametrize("transform", list(er.TRANSFORMS))
@pytest.mark.parametrize("grid", list(er.FUSED_GRIDS))
def test_fused_proposal_forward_vs_float64(N, grid, transform, mode):
    """enc, selector, pre and density of the fused forward against float64 for positions M in {1, 63, 64, 255, 256, 257, 513} or
    rays (n, S) in {(1, 1), (3, 85), (257, 1), (5, 96)}; the densities with the optional outputs NULL bit-equal to those with them
    given; guards untouched."""
    L, H, lo, hi, log2_T = er.FUSED_GRIDS[grid]
    tf = er.TRANSFORMS[transform]
    IN = 2 * L
    host_table, table = _table(L, log2_T)
    scal = er.scalings32(L, lo, hi)
    g = N.make_grid(L, log2_T, scal)
    mlp = _Mlp(N, IN, H, 100 * L + H)
    worst, zeros = {}, 0
    for label, pts, M in er.fused_cases(mode, tf, lo):
        x, sel = er.normalise32(er.positions32(pts), tf)
        enc64, A = er.hash_features64(x, host_table, scal, log2_T)
        enc_err = er.HASH_ROUNDINGS * U * A
        r = er.density64(enc64, enc_err, sel, mlp.host, AVG)
        P, keep = _points(N, pts)
        enc, so, dens, pre = Guarded(IN * M, M), Guarded(M, M), Guarded(M, M), Guarded(M, M)
        assert _fused(N, P, M, tf, table, g, mlp, enc, so, dens, pre) == OK
        check_entries("enc", enc.body().reshape(IN, M).T, enc64, enc_err, worst)
        assert np.array_equal(so.body(), sel), f"{label}: selector"
        check_entries("pre", pre.body(), r["pre"], r["dpre"], worst)
        check_entries("density", dens.body(), r["density"], r["ddensity"], worst)
        assert bool((dens.body()[sel == 0] == 0).all()), f"{label}: density where the selector is 0"
        zeros += int((sel == 0).sum())
        alone = Guarded(M, M)
        assert _fused(N, P, M, tf, table, g, mlp, None, None, alone, None) == OK
        assert _same_bits(alone.body(), dens.body()), f"{label}: densities without the optional outputs"
        for b in (enc, so, dens, pre, alone):
            assert b.guards_untouched(), label
    assert tf == er.XFORM_NONE or zeros > 0
    report(f"fused proposal forward {grid} {transform} {mode}", worst)


def test_fused_proposal_forward_status_codes(N):
    """(7, 16) and (5, 32) answer NSAMD_ERR_UNSUPPORTED, in_dim != 2 levels NSAMD_ERR_INVALID_ARG, M = 0 NSAMD_OK; none writes."""
    M = 64
    pts = er.position_case(M, er.XFORM_NONE, 16, 5)
    P, keep = _points(N, pts)
    _, table = _table(8, 12)
    for L, in_dim, H, want in ((7, 14, 16, ERR_UNSUPPORTED), (5, 10, 32, ERR_UNSUPPORTED), (5, 16, 16, ERR_INVALID_ARG),
                               (8, 10, 16, ERR_INVALID_ARG)):
        g = N.make_grid(L, 12, er.scalings32(L, 16, 128))
        mlp = _Mlp(N, in_dim, H, 1)
        bufs = [Guarded(in_dim * M, M), Guarded(M, M), Guarded(M, M), Guarded(M, M)]
        assert _fused(N, P, M, er.XFORM_NONE, table, g, mlp, *bufs) == want, (L, in_dim, H)
        assert all(b.untouched() for b in bufs), (L, in_dim, H)
    g = N.make_grid(5, 12, er.scalings32(5, 16, 128))
    mlp = _Mlp(N, 10, 16, 1)
    bufs = [Guarded(10 * M, M), Guarded(M, M), Guarded(M, M), Guarded(M, M)]
    assert _fused(N, P, 0, er.XFORM_NONE, table, g, mlp, *bufs) == OK
    assert all(b.untouched() for b in bufs)
    report("fused proposal forward status codes", {"untouched": 0.0})


@pytest.mark.parametrize("transform", list(er.TRANSFORMS))
@pytest.mark.parametrize("grid", INSTANTIATIONS)
def test_fused_proposal_forward_equals_the_two_kernel_pair(N, grid, transform):
    """include/nsamd.h promises nsamd_density_field_fwd bit-identical to nsamd_hashgrid_encode_fwd + nsamd_density_mlp_fwd: all four
    instantiations, the three transforms, 257 positions and 5 x 96 rays (test_gpu_kernels.py holds (5, 16) at 211 x 96 rays)."""
    L, H, lo, hi, log2_T = er.FUSED_GRIDS[grid]
    tf = er.TRANSFORMS[transform]
    IN = 2 * L
    _, table = _table(L, log2_T)
    g = N.make_grid(L, log2_T, er.scalings32(L, lo, hi))
    mlp = _Mlp(N, IN, H, 100 * L + H)
    lib = N.load()
    for pts, M in ((er.position_case(257, tf, lo, 11), 257), (er.ray_case(5, 96, tf, 12), 480)):
        P, keep = _points(N, pts)
        fused = [Guarded(IN * M, M), Guarded(M, M), Guarded(M, M), Guarded(M, M)]
        assert _fused(N, P, M, tf, table, g, mlp, *fused) == OK
        enc, sel, dens, pre = Guarded(IN * M, M), Guarded(M, M), Guarded(M, M), Guarded(M, M)
        N.check(lib.nsamd_hashgrid_encode_fwd(P, M, tf, _box(N, tf), N.ptr(table), g, enc.ptr, 1, M, sel.ptr, N.stream()), "hash")
        N.check(lib.nsamd_density_mlp_fwd(enc.ptr, sel.ptr, M, mlp.native, dens.ptr, pre.ptr, N.stream()), "mlp")
        torch.cuda.synchronize()
        for name, a, b in zip(("enc", "selector", "density", "pre"), fused, (enc, sel, dens, pre)):
            assert not np.isnan(b.body()).any() and _same_bits(a.body(), b.body()), name
            assert a.guards_untouched() and b.guards_untouched(), name
        assert float(dens.body().max()) > 0
    report(f"fused forward = the two-kernel pair, {grid} {transform}", {"bitwise": 0.0})


# ---------------------------------------------------------------- nsamd_hashgrid_encode_fwd ---------------------------------------

@pytest.mark.parametrize("mode", ["positions", "rays"])
@pytest.mark.parametrize("transform", list(er.TRANSFORMS))
@pytest.mark.parametrize("grid", list(er.HASH_GRIDS))
def test_hashgrid_forward_layouts_and_selector(N, grid, transform, mode):
    """Each forward kernel at M in {1, 2, 255, 256, 257} or 3 x 85 rays, point-major (2L, 1), feature-major (1, M) and padded rows
    (2L + 3, 1), selector given and NULL: features bit-equal to orc.hashgrid_encode on normalise32's points and within 9 u A of
    float64, selector bit-exact, padding columns and guards untouched."""
    L, lo, hi, log2_T = er.HASH_GRIDS[grid]
    tf = er.TRANSFORMS[transform]
    K = 2 * L
    host_table, table = _table(L, log2_T)
    scal = er.scalings32(L, lo, hi)
    g = N.make_grid(L, log2_T, scal)
    lib = N.load()
    worst = {}
    for label, pts, M in er.hash_cases(mode, tf, lo):
        x, sel = er.normalise32(er.positions32(pts), tf)
        enc32 = orc.hashgrid_encode(torch.from_numpy(x), torch.from_numpy(host_table), torch.from_numpy(scal), 1 << log2_T).numpy()
        enc64, A = er.hash_features64(x, host_table, scal, log2_T)
        P, keep = _points(N, pts)
        for layout, (sp, sk, size, row) in (("point-major", (K, 1, M * K, K)), ("feature-major", (1, M, K * M, M)),
                                            ("padded", (K + 3, 1, M * (K + 3), K + 3))):
            for with_selector in (True, False):
                out, so = Guarded(size, row), Guarded(M, M)
                N.check(lib.nsamd_hashgrid_encode_fwd(P, M, tf, _box(N, tf), N.ptr(table), g, out.ptr, sp, sk,
                                                      so.ptr if with_selector else None, N.stream()), "hash")
                torch.cuda.synchronize()
                what = f"{label} {layout} selector={with_selector}"
                body = out.body()
                if layout == "feature-major":
                    got = body.reshape(K, M).T
                elif layout == "padded":
                    got = body.reshape(M, K + 3)[:, :K]
                    assert np.isnan(body.reshape(M, K + 3)[:, K:]).all(), f"{what}: padding columns"
                else:
                    got = body.reshape(M, K)
                check_entries(layout, got, enc64, er.HASH_ROUNDINGS * U * A, worst)
                assert _same_bits(got, enc32), f"{what}: features differ from the fp32 oracle"
                assert np.array_equal(so.body(), sel) if with_selector else so.untouched(), f"{what}: selector"
                assert out.guards_untouched() and so.guards_untouched(), what
    report(f"hash forward {grid} {transform} {mode}", worst)


# ---------------------------------------------------------------- nsamd_nerf_encode -----------------------------------------------

def _nerf(N, P, M, freqs, F, include_input, out):
    rc = N.load().nsamd_nerf_encode(P, M, N.ptr(freqs), F, include_input, out.ptr, N.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("mode", ["positions", "rays"])
@pytest.mark.parametrize("include_input", [0, 1])
@pytest.mark.parametrize("F,e", [(1, 0), (2, 1), (4, 4), (4, 16), (10, 8), (64, 8)])
def test_nerf_encode_vs_float64(N, F, e, include_input, mode):
    """Frequencies 2 ** linspace(0, e, F) (e = 16: arguments up to ~1.6e6, where sinf's range reduction does the work). Positions: M
    = 1, 1000 and the two M whose thread counts 3 F M lie around 256; inputs uniform in [-4, 4] with 0, -0, a denormal, 1e-20 and
    rows with NaN, +Inf, -Inf (NaN results exactly where the reference has them). Rays: (7, 48) and (2, 130), against the float64
    rows of positions32. The include_input columns are bit-exact."""
    freqs = er.nerf_freqs(F, e)
    fd = torch.from_numpy(freqs).cuda()
    per, width = 3 * F, 6 * F + 3 * include_input
    if mode == "positions":
        cases = [(f"M={M}", {"positions": er.nerf_inputs(M, er.case_seed(M, F, e))}, M)
                 for M in sorted({1, 1000, 256 // per, 256 // per + 1} - {0})]
    else:
        cases = [(f"rays={n}x{S}", er.ray_case(n, S, er.XFORM_AABB, er.case_seed(n, S, F)), n * S) for n, S in ((7, 48), (2, 130))]
    worst = {}
    for label, pts, M in cases:
        x = er.positions32(pts)
        rows = er.nerf_rows64(x, freqs, bool(include_input))
        P, keep = _points(N, pts)
        out = Guarded(M * width, width)
        assert _nerf(N, P, M, fd, F, include_input, out) == OK
        got = out.body().reshape(M, width)
        check_entries("sin", got[:, : 2 * per], rows[:, : 2 * per], E_SIN * np.abs(rows[:, : 2 * per]) + U * 2.0**-23, worst)
        if include_input:
            assert _same_bits(got[:, 2 * per :], x), f"{label}: raw-input columns"
        assert out.guards_untouched(), label
    report(f"nerf_encode F={F} e={e} include_input={include_input} {mode}", worst)


def test_nerf_encode_status_codes(N):
    M = 8
    P, keep = _points(N, {"positions": er.nerf_inputs(M, 1)})
    fd = torch.ones(65, device="cuda")
    for F in (0, 65):
        out = Guarded(M * (6 * 65 + 3), 6 * 65 + 3)
        assert _nerf(N, P, M, fd, F, 1, out) == ERR_INVALID_ARG
        assert out.untouched()
    out = Guarded(M * 9, 9)
    assert _nerf(N, P, 0, fd, 1, 1, out) == OK and out.untouched()
    report("nerf_encode status codes", {"untouched": 0.0})


# ---------------------------------------------------------------- nsamd_sh4_encode, nsamd_contract_linf ---------------------------

@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_sh4_encode_vs_float64(N, M):
    """Unit vectors with the axis directions, vectors within 1e-4 of an axis (where the degree-3 terms cancel) and the diagonals;
    non-unit input evaluated as given (the zero vector, lengths 1e-3 and 10); a row with a NaN."""
    d = er.sh_inputs(M, M)
    sh, mono = er.sh4_64(d)
    dd = torch.from_numpy(d).cuda()
    out = Guarded(16 * M, 16)
    assert N.load().nsamd_sh4_encode(N.ptr(dd), M, out.ptr, N.stream()) == OK
    torch.cuda.synchronize()
    worst = {}
    got = out.body().reshape(M, 16)
    for i in range(16):
        check_entries(f"c{i}", got[:, i], sh[:, i], er.SH_ROUNDINGS[i] * U * mono[:, i], worst)
    assert out.guards_untouched()
    by_degree = {f"degree {n}": max(worst[f"c{i}"] for i in range(n * n, (n + 1) * (n + 1))) for n in range(4)}
    report(f"sh4_encode M={M}", by_degree)


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_contract_linf_bitwise(N, M):
    """Random normal x 3, |x| in {1, nextafter(1, 0), 3, 1e3, 1e30}, ties between two and three axes, +-0, a denormal, 3e38, rows
    with +-Inf and rows with a NaN (the L-inf norm of such a row is NaN, so the whole row is): the same bits as contract32."""
    x = er.contract_inputs(M, M)
    xd = torch.from_numpy(x).cuda()
    out = Guarded(3 * M, 3)
    assert N.load().nsamd_contract_linf(N.ptr(xd), M, out.ptr, N.stream()) == OK
    torch.cuda.synchronize()
    got, want = out.body().reshape(M, 3), er.contract32(x)
    bad = ~((got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), f"{int(bad.sum())} entries differ; first rows {np.flatnonzero(bad.any(-1))[:4]}: in {x[bad.any(-1)][:4]} " \
                          f"got {got[bad.any(-1)][:4]} want {want[bad.any(-1)][:4]}"
    assert out.guards_untouched()
    report(f"contract_linf M={M}", {"entries that differ": float(bad.sum())})
