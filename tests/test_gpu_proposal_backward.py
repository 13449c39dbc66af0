"""The proposal backward chain and the per-ray losses ENTRY BY ENTRY against float64 references of the same operations on
the kernels' own fp32 inputs (oracle: weights_bwd64, composite_bwd64, interlevel_bwd64, distortion_bwd64,
density_mlp_fwd64 / density_mlp_bwd64): csrc/ray_bodies.h (weights_bwd_body, composite_bwd_body's density tail,
interlevel_body, distortion_body) and csrc/density_mlp.hip (forward, persistent chunk loop, MFMA partials, the fixed-order
reduce or the float atomics, gated calls with ray masks, the two-level pair kernel).

Every check is |got - ref64| <= bound per entry, with the bound built from the code's operation sequence, not fitted:

* u = 2^-24 (fp32 rounding); the wave scans in double count as exact to 2^-53 of their abs sums per term (S terms).
* E_EXP: the device expf is assumed within 2 ulp (relative 2 * 2^-23 = 4u). The device library documents about 1 ulp;
  test_expf_budget checks the assumption through nsamd_weights_fwd at S = 1 (w = 1 - expf(-dd)).
* Weights backward (weights_bwd_body; composite_bwd_body's tail is the same arithmetic). dd = fl(fl(t1 - t0) * density):
  2u relative. X (double scan of the fp32 dd, cast to float): dX <= 2u sum_{i<j}|dd_i| + u |X| + S 2^-53 sum|dd|. T = expf(-X):
  relative dX + E_EXP. e = expf(-dd): relative 2u |dd| + E_EXP. alpha = 1 - e: the cancellation for small dd is carried as it
  is, an ABSOLUTE error e (2u|dd| + E_EXP) + u |alpha| (about 4u, i.e. relative 4u / dd when dd is small). w = alpha T: the two
  errors + u. The suffix sum (double, cast): sum_{i>j} (|g_i| dw_i + dg_i w_i + u |g_i w_i|) + S 2^-53 suf_abs + u |suf|. The
  own term g T e: two products + the errors of T and e. The difference + u, delta (u) and the product (u). Where the upstream
  gradient g itself carries an error dg (render_train_bwd: the compositing's d_weights) it enters both terms.
* Compositing backward: d_weights = ((g.c) - (g.bg)) + d_weights_add, six products and five additions: 8u of the sum of
  |terms|; d_rgb = g * (w [+ 1 - acc for the last sample under last_sample]): acc is a wave sum of ceil(S/64) + 6 terms.
* Interlevel: outer = cy[hi+1] - cy[lo] with cy the fp32-rounded double prefix sums: u (|cy[hi+1]| + |cy[lo]|) + u |outer|;
  clip is 1-Lipschitz; loss_i = c^2 / (w + eps) three roundings; the per-ray sum a wave sum of ceil(Sf/64) + 6 terms. dwp_k =
  -(sum over the fine intervals covering k of rr_i) * grad_scale: the rr_i errors summed over the cover, the double prefix sums
  (Sf 2^-53 of their abs sum), the cast and the scale (2u); on the direct-loop branch (unsorted rows) an fp32 sum over the
  cover: + n_cover u of its abs sum. The cover ranges lo / hi are integers: the reference takes _outer_bound's searchsorted on
  the same fp32 edges, so an off-by-one shows as a whole missing or extra rr_i.
* Distortion: midpoints u; |m_i - m_k| u (|m_i| + |m_k|) + u; inner_i an fp32 sum of S products: (S + 2) u of inner_abs; dw and
  the loss terms four more roundings, the per-ray loss a wave sum.
* Density MLP (IN -> H -> 1): the hidden pre-activation a is an fmaf chain of IN steps: da <= IN u a_abs; points whose float64 a
  lies within that of zero have their upstream gradient taken out on both sides (the count is printed, and small). Forward:
  dpre <= sum_j |W1_j| da_j + H u pre_abs; density relative dpre + E_EXP + 2u. Backward: g_pre = ((gd sel) avg) expf(clamp(pre))
  relative 3u + E_EXP = 7u; gh = g_pre W1 8u; denc an fmaf chain over H: (H + 8) u denc_abs. Weight gradients: the summation
  chain comes from the launch geometry, restated below from density_mlp.hip (kMlpBlock, kMaxBlocks, kDwGroups):
  blocks = min(kMaxBlocks, chunks), cpw = ceil(chunks / blocks) 256-point chunks per workgroup. dW0: 16 MFMA k-steps per chunk,
  each step counted as 4 additions (the order inside one step is not documented), times cpw; + 4 waves (LDS); + the reduce,
  ceil(rows / 16) + 16 + 1 (rows = blocks), or `blocks` float atomics without a workspace. db0, dW1, db1: the 256-long serial
  per-chunk sum + cpw, then the same reduce. Each such sum: (chain + product roundings) u of the sum of |terms|.
Every bound is multiplied by 1 + 2^-6 (second-order terms, the float64 reference's own rounding) and carries n 2^-140 for
products that underflow. The sign-coherent cases (enc, gd of one sign: sum |terms| = |sum|) and the cases with 1-3 live rays
make a lost or doubled chunk, wave partial or reduce row exceed the bound instead of hiding under a random-sign abs sum.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from float64_check import D53, E_EXP, SAFE, TINY, U, _np, check_entries, report  # noqa: F401
from oracle import nerfacto_oracle as orc

pytestmark = pytest.mark.gpu

FTZ = 2.0**-124    # an fp32 product below FLT_MIN = 2^-126 may be flushed (x4 for the factors it is carried through)
ERR_UNSUPPORTED = -2
# density_mlp.hip restated
K_MLP_BLOCK = 256
K_MAX_BLOCKS = 768
K_DW_GROUPS = 16
K_LOSS_RAYS = 4
MLP_SHAPES = [(10, 16), (16, 16), (10, 64), (16, 64)]


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


def _n():
    from nerfstudio_amd import _native as N

    return N


# ---------------------------------------------------------------- bounds ------------------------------------------------

def weights_bound(r, g_err=None):
    """Per-entry bound of the weights backward (module docstring) from weights_bwd64's float64 quantities."""
    S = r["dd"].shape[-1]
    dd, X, E, e, alpha, w, g = (torch.nan_to_num(r[k], nan=0.0, posinf=0.0, neginf=0.0) for k in
                                ("dd", "X", "E", "e", "alpha", "w", "g"))
    delta = r["delta"]
    ddabs = dd.abs()
    Xabs = torch.cat([torch.zeros_like(dd[:, :1]), torch.cumsum(ddabs[:, :-1], -1)], -1)
    dX = 2 * U * Xabs + U * X.abs() + S * D53 * Xabs
    dT = E * (dX + E_EXP)
    de = e * (2 * U * ddabs + E_EXP)
    dalpha = de + U * alpha.abs()
    dw = dalpha * E + alpha.abs() * dT + U * w.abs()
    ge = torch.zeros_like(g) if g_err is None else g_err
    dgw = g.abs() * dw + ge * w.abs() + U * (g * w).abs()
    tail = torch.cat([torch.flip(torch.cumsum(torch.flip(dgw[:, 1:], [-1]), -1), [-1]), torch.zeros_like(dd[:, :1])], -1)
    suf = torch.nan_to_num(r["suf"], nan=0.0, posinf=0.0, neginf=0.0)
    dsuf = tail + S * D53 * r["suf_abs"] + U * suf.abs()
    own = g * E * e
    down = g.abs() * (dT * e + E * de) + ge * E * e + 2 * U * own.abs()
    inner = own - suf
    dinner = down + dsuf + U * inner.abs()
    return delta.abs() * dinner + 2 * U * (delta * inner).abs()


def gate_predicate(t_bins, density, dweights):
    """include/nsamd.h: a ray carries gradient when a sample has dweights != 0 (NaN included) or an optical thickness
    fl(fl(t1 - t0) * density) outside [0, FLT_MAX] (NaN, Inf, negative)."""
    t, dn, dw = (x.detach().cpu().numpy().astype(np.float32) for x in (t_bins, density, dweights))
    with np.errstate(all="ignore"):
        dd = (t[:, 1:] - t[:, :-1]) * dn
        carries = (dw != 0) | ~((dd >= 0) & (dd <= np.float32(3.4028234663852886e38)))
    return carries.any(-1)


def mlp_chains(M, atomics):
    """(dW0 chain, serial-sum chain) of density_mlp_bwd for M points: the launch geometry of launch_bwd restated."""
    chunks = -(-M // K_MLP_BLOCK)
    blocks = min(K_MAX_BLOCKS, chunks)
    cpw = -(-chunks // blocks)
    red = blocks if atomics else -(-blocks // K_DW_GROUPS) + K_DW_GROUPS + 1
    return 4 * 16 * cpw + 4 + red, K_MLP_BLOCK + cpw + red


def mlp_bounds(r, IN, H, M, atomics):
    n0, n1 = mlp_chains(M, atomics)
    # a g_pre (or gh) below FLT_MIN may be flushed to zero: FTZ per point in denc, M of them in the sums
    ftz = FTZ * float(r["W1W0"].max())
    return dict(denc=(H + 8) * U * r["denc_abs"] + FTZ * r["W1W0"], dW0=(n0 + 9) * U * r["dW0_abs"] + M * ftz,
                db0=(n1 + 8) * U * r["db0_abs"] + M * ftz, dW1=IN * U * r["dW1_a"] + (n1 + 9) * U * r["dW1_abs"] + M * ftz,
                db1=(n1 + 7) * U * r["db1_abs"] + M * ftz)


def relu_ambiguous(a, a_abs, IN):
    return ((a.abs() <= 1.02 * IN * U * a_abs + TINY)).any(-1)


# ---------------------------------------------------------------- E_EXP ------------------------------------------------

def test_expf_budget(F):
    """nsamd_weights_fwd at S = 1 is w = (1 - expf(-dd)) * expf(-0): the device expf within E_EXP of exp, over 1e-9 .. 88."""
    N = _n()
    lib = N.load()
    x = torch.cat([torch.logspace(-9, math.log10(88.0), 200000), torch.rand(100000) * 20]).float()
    n = x.numel()
    t = torch.stack([torch.zeros(n), torch.ones(n)], -1).cuda()
    w = torch.empty(n, 1, device="cuda")
    xd = x.cuda().contiguous()  # (every device input is held by a name until the kernel has run)
    N.check(lib.nsamd_weights_fwd(N.ptr(t), N.ptr(xd), n, 1, N.ptr(w), N.stream()), "weights_fwd")
    e64 = torch.exp(-x.double())
    got = w[:, 0].cpu().double()
    ref = 1 - e64
    err = (got - ref).abs()
    # 1 - expf(-x): the expf error (relative E_EXP of e) + the subtraction's rounding
    ulps = float(((err - U * ref) / (e64 * 2 * 2.0**-23)).max())
    print(f"\nexpf through weights_fwd: worst |1 - expf(-x) - (1 - exp(-x))| = {ulps:.3f} ulp of exp(-x) (budget 2)")
    assert bool((err <= E_EXP * e64 + U * ref + TINY).all()), ulps


# ---------------------------------------------------------------- weights backward -------------------------------------

def _weights_case(n, S, seed):
    """t_bins [n, S+1], density, dweights [n, S] with the edge rows described in the test."""
    g = torch.Generator().manual_seed(seed)
    _, t = orc.piecewise_bins(torch.full((n, 1), 0.05), torch.full((n, 1), 1000.0), S, torch.rand(n, 1, generator=g))
    t = t.contiguous()
    dens = torch.rand(n, S, generator=g) * 10.0 ** (torch.rand(n, S, generator=g) * 4 - 3)
    dw = torch.randn(n, S, generator=g) * 10.0 ** (torch.rand(n, 1, generator=g) * 4 - 4)
    dens[0] = 0.0                                   # zero densities
    dens[1] = torch.logspace(-2, 4, S) if S > 1 else 1e4  # optical depth to full extinction: T subnormal, then 0
    t[2, S // 2:] = t[2, S // 2]                    # duplicate edges: delta = 0 from the middle on
    dw[3] = 0.0                                     # a ray without gradient (the early-out)
    dens[4, S // 3] = -1.0e30                       # negative: a non-finite weight (exp overflows in fp32 and float64)
    dens[5, S // 2] = float("nan")
    dens[6, (2 * S) // 3] = float("inf")
    dw[7, S // 4] = float("nan")
    dw[8, S // 2] = float("inf")
    dw[9] = 0.0
    dens[9, S - 1] = float("nan")                   # no gradient but a NaN thickness: carries
    dw[10] = 0.0
    dens[10, 0] = -1e-3                             # no gradient, a negative thickness: carries
    dw[11:14] = 0.0                                 # more rays without gradient
    return t, dens, dw


@pytest.mark.parametrize("S", [1, 47, 48, 63, 64, 65, 96, 256, 257, 1024])
def test_weights_backward_vs_float64(F, S):
    """nsamd_weights_bwd and nsamd_weights_bwd_gate (gate word and ray mask against the documented predicate) on zero
    densities, extinction to subnormal / zero transmittance, duplicate edges, negative / NaN / Inf densities and NaN / Inf
    upstream gradients; ray counts not a multiple of 4."""
    N = _n()
    lib, st = N.load(), N.stream()
    n = 37 if S == 1024 else 203
    t, dens, dw = _weights_case(n, S, S)
    r = orc.weights_bwd64(t, dens, dw)
    bound = weights_bound(r)
    td, dd, dwd = t.cuda(), dens.cuda(), dw.cuda()
    worst = {}
    out = torch.full((n, S), 7.0, device="cuda")
    N.check(lib.nsamd_weights_bwd(N.ptr(td), N.ptr(dd), N.ptr(dwd), n, S, N.ptr(out), st), "weights_bwd")
    check_entries("ddensity", out, r["ddensity"], bound, worst)
    gate = torch.full((4,), 5, dtype=torch.int32, device="cuda")
    mask = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    out2 = torch.full((n, S), 7.0, device="cuda")
    N.check(lib.nsamd_weights_bwd_gate(N.ptr(td), N.ptr(dd), N.ptr(dwd), n, S, N.ptr(out2), gate.data_ptr(), N.ptr(mask), 0,
                                       st), "weights_bwd_gate")
    check_entries("ddensity (gate)", out2, r["ddensity"], bound, worst)
    pred = gate_predicate(t, dens, dw)
    assert np.array_equal(mask.cpu().numpy(), pred.astype(np.uint8))
    assert int(gate[0]) == int(pred.any()) and pred.any() and not pred.all()
    # all rays without gradient: the gate word stays clear, the mask all zero, the result delta * 0
    z = torch.zeros_like(dwd)
    dn_ok = dd.clone().nan_to_num_(0.0, 0.0, 0.0).clamp_(min=0.0)
    N.check(lib.nsamd_weights_bwd_gate(N.ptr(td), N.ptr(dn_ok), N.ptr(z), n, S, N.ptr(out2), gate.data_ptr(), N.ptr(mask), 0,
                                       st), "weights_bwd_gate")
    torch.cuda.synchronize()
    assert int(gate[0]) == 0 and int(mask.sum()) == 0 and float(out2.abs().max()) == 0.0
    report(f"weights backward S={S}", worst)


def test_weights_backward_unsupported(F):
    N = _n()
    lib = N.load()
    t = torch.zeros(4, 1026, device="cuda")
    d = torch.zeros(4, 1025, device="cuda")
    gate = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.nsamd_weights_bwd(N.ptr(t), N.ptr(d), N.ptr(d), 4, 1025, N.ptr(d), N.stream()) == ERR_UNSUPPORTED
    assert lib.nsamd_weights_bwd_gate(N.ptr(t), N.ptr(d), N.ptr(d), 4, 1025, N.ptr(d), gate.data_ptr(), None, 0,
                                      N.stream()) == ERR_UNSUPPORTED


# ---------------------------------------------------------------- render_train_bwd -------------------------------------

@pytest.mark.parametrize("background", [0, 1, 2, 3])
def test_render_train_bwd_vs_float64(F, background):
    """nsamd_render_train_bwd at S = 48, 4096 rays, with and without d_weights_add: d_rgb and d_density entry by entry (the
    compositing backward, then composite_bwd_body's own copy of the weights backward)."""
    N = _n()
    lib, st = N.load(), N.stream()
    n, S = 4096, 48
    g = torch.Generator().manual_seed(40 + background)
    _, t = orc.piecewise_bins(torch.full((n, 1), 0.05), torch.full((n, 1), 1000.0), S, torch.rand(n, 1, generator=g))
    t = t.contiguous()
    dens = torch.rand(n, S, generator=g) * 10.0 ** (torch.rand(n, S, generator=g) * 4 - 2)
    dens[0] = 0.0
    dens[1] = torch.logspace(-2, 4, S)
    rgb = torch.rand(n, S, 3, generator=g)
    d_out = torch.randn(n, 3, generator=g) * 1e-3
    bg_rays = torch.rand(n, 3, generator=g)
    bgv = (C.c_float * 3)(0.25, 0.5, 0.75)
    td, dd, rd = t.cuda(), dens.cuda(), rgb.cuda()
    w = torch.empty(n, S, device="cuda")
    N.check(lib.nsamd_weights_fwd(N.ptr(td), N.ptr(dd), n, S, N.ptr(w), st), "weights_fwd")
    worst = {}
    for with_add in (False, True):
        dwa = (torch.randn(n, S, generator=g) * 1e-4) if with_add else None
        drgb, dden = torch.empty(n, S, 3, device="cuda"), torch.empty(n, S, device="cuda")
        dod, dwad, bgd = d_out.cuda(), dwa.cuda() if with_add else None, bg_rays.cuda()
        N.check(lib.nsamd_render_train_bwd(N.ptr(rd), N.ptr(w), N.ptr(dd), N.ptr(td), n, S, background,
                                           bgv if background == 2 else None, N.ptr(dod),
                                           N.ptr(dwad), N.ptr(drgb), N.ptr(dden),
                                           N.ptr(bgd) if background == 3 else None, st), "render_train_bwd")
        c = orc.composite_bwd64(rgb, w.cpu(), d_out, background, (0.25, 0.5, 0.75), bg_rays, dwa)
        wsum = w.cpu().double().sum(-1)
        b_rgb = U * c["d_rgb"].abs()
        if background == 1:
            rem = (1 - wsum).abs()
            drem = (math.ceil(S / 64) + 6) * U * wsum + U * rem + U * (rem + w.cpu().double()[:, -1])
            b_rgb[:, -1, :] += d_out.double().abs() * drem[:, None]
        check_entries(f"d_rgb add={with_add}", drgb, c["d_rgb"], b_rgb, worst)
        r = orc.weights_bwd64(t, dens, c["d_weights"])
        check_entries(f"d_density add={with_add}", dden, r["ddensity"], weights_bound(r, 8 * U * c["dw_abs"]), worst)
    report(f"render_train_bwd background={background}", worst)


# ---------------------------------------------------------------- interlevel / distortion ------------------------------

def interlevel_row_floats(Sf, Sp):  # ray_bodies.h restated
    return (2 * (Sf + 2) + 2 * (Sp + 1) + (Sf + 1) + 4 * Sf + 1) & ~1


def _lds_fits(Sf, Sp):
    return 4 * interlevel_row_floats(Sf, Sp) * K_LOSS_RAYS <= 64 * 1024


def _largest_sp(Sf):
    Sp = 1
    while _lds_fits(Sf, Sp + 1):
        Sp += 1
    return Sp


def _interlevel_case(n, Sf, Sp, seed):
    """Sorted fine / proposal edges in [0, 1] with the edge rows of the test; weights such that w - outer takes both signs."""
    g = torch.Generator().manual_seed(seed)
    cp = torch.sort(torch.rand(n, Sp + 1, generator=g), -1).values
    cp[:, 0], cp[:, -1] = 0.0, 1.0
    c = torch.sort(torch.rand(n, Sf + 1, generator=g) * 1.1 - 0.05, -1).values
    if Sp >= Sf:  # row 0: the fine edges ARE proposal edges (ties of side="right")
        pick = torch.sort(torch.randperm(Sp + 1, generator=g)[: Sf + 1]).values
        c[0] = cp[0, pick]
    else:
        pick = torch.sort(torch.randperm(Sf + 1, generator=g)[: Sp + 1]).values
        cp[0] = c[0, pick]
    if Sf > 2:
        c[1, 1:3] = c[1, 1]                          # zero-width fine bins
    if Sp > 2:
        cp[1, 2:4] = cp[1, 2]                        # zero-width proposal bins
    wp = torch.rand(n, Sp, generator=g) * 2 / Sp
    w = torch.rand(n, Sf, generator=g) * 3 / Sf
    w[:, ::5] *= 0.01
    wp[2] = 0.0                                      # all-zero proposal weights
    if Sf > 4:                                       # one unsorted row: the direct-loop branch
        c[3, 1 : Sf // 2] = torch.flip(c[3, 1 : Sf // 2], [0])
    return c.contiguous(), w.contiguous(), cp.contiguous(), wp.contiguous()


def interlevel_bounds(r, Sf, scale, unsorted_rows):
    d_outer = U * r["outer_abs"] + U * r["outer"].abs() + Sf * D53 * r["outer_abs"]
    dc = d_outer + U * r["diff"].abs()
    clipped, den = torch.clamp(r["diff"], min=0), r["den"]
    loss_i = clipped * clipped / den
    dloss_i = (2 * clipped * dc + dc * dc) / den + 3 * U * loss_i
    b_loss = dloss_i.sum(-1) + (math.ceil(Sf / 64) + 6) * U * loss_i.sum(-1)
    drr = 2 * dc / den + 2 * U * r["rr"]
    lo, hi = r["lo"], r["hi"]
    fwd = lo <= hi
    start, end = torch.where(fwd, lo, hi + 1), torch.where(fwd, hi, lo - 1)
    Sp = r["dwp"].shape[-1]
    cover_drr = orc._cover_sum(start, end, drr, Sp).clamp(min=0)  # (a difference array's cumsum: not exactly 0 off the cover)
    R_abs = r["rr"].abs().sum(-1, keepdim=True)
    cover_abs, cover_n = r["cover_abs"].clamp(min=0), r["cover_n"].clamp(min=0)
    b = cover_drr + 2 * Sf * D53 * R_abs + U * cover_abs
    b = b + unsorted_rows[:, None] * cover_n * U * cover_abs
    return b_loss, (b + U * (r["dwp"].abs())) * abs(scale) + U * (r["dwp"] * scale).abs()


def _sorted_rows(r):
    lo, hi = r["lo"], r["hi"]
    return ((lo[:, 1:] >= lo[:, :-1]) & (hi[:, 1:] >= hi[:, :-1])).all(-1)


PAIRS = [(48, 96), (48, 256), (96, 256), (1, 1), (63, 65), (65, 63), (200, 700)]


@pytest.mark.parametrize("Sf,Sp", PAIRS + [(48, "max")])
def test_interlevel_vs_float64(F, Sf, Sp):
    """nsamd_interlevel_loss: per-ray loss and dw_prop; fine edges equal to proposal edges, zero-width bins, rows where w -
    outer crosses 0, all-zero proposal weights, one unsorted row (direct loop; the reference there is autograd's
    [k <= hi] - [k < lo] on the oracle's searchsorted ranges). The largest Sp whose LDS row fits, and the next one
    (ERR_UNSUPPORTED), come from interlevel_row_floats."""
    N = _n()
    lib, st = N.load(), N.stream()
    if Sp == "max":
        Sp = _largest_sp(Sf)
        z = torch.zeros(8 * (Sp + 2), device="cuda")
        assert lib.nsamd_interlevel_loss(N.ptr(z), N.ptr(z), Sf, N.ptr(z), N.ptr(z), Sp + 1, 2, 1.0, N.ptr(z), N.ptr(z),
                                         st) == ERR_UNSUPPORTED
    n = 23 if Sp > 1000 else 203
    c, w, cp, wp = _interlevel_case(n, Sf, Sp, Sf * 1000 + Sp)
    r = orc.interlevel_bwd64(c, w, cp, wp)
    unsorted = (~_sorted_rows(r)).double()
    if Sf > 4:
        assert bool(unsorted[3]) and int(unsorted.sum()) == 1
    diff = r["diff"]
    assert bool((diff > 0).any()) and bool((diff < 0).any())
    scale = 0.37
    b_loss, b_dwp = interlevel_bounds(r, Sf, scale, unsorted)
    per, dwp = torch.empty(n, device="cuda"), torch.full((n, Sp), 7.0, device="cuda")
    cd, wd, cpd, wpd = c.cuda(), w.cuda(), cp.cuda(), wp.cuda()
    N.check(lib.nsamd_interlevel_loss(N.ptr(cd), N.ptr(wd), Sf, N.ptr(cpd), N.ptr(wpd), Sp, n, scale,
                                      N.ptr(per), N.ptr(dwp), st), "interlevel")
    worst = {}
    check_entries("loss", per, r["loss"], b_loss, worst)
    check_entries("dw_prop", dwp, r["dwp"] * scale, b_dwp, worst)
    report(f"interlevel Sf={Sf} Sp={Sp}", worst)


@pytest.mark.parametrize("S", [1, 48, 64, 65, 256, 2048])
def test_distortion_vs_float64(F, S):
    N = _n()
    lib, st = N.load(), N.stream()
    n = 9 if S == 2048 else 203
    g = torch.Generator().manual_seed(S)
    s = torch.sort(torch.rand(n, S + 1, generator=g), -1).values.contiguous()
    if S > 3:
        s[0, 2:4] = s[0, 2]
    w = (torch.rand(n, S, generator=g) * 2 / S).contiguous()
    w[1] = 0.0
    r = orc.distortion_bwd64(s, w)
    scale = 0.011
    wd = w.double()
    d_inner = U * r["mid_abs"] + (S + 2) * U * r["inner_abs"]
    wdelta = (wd * r["delta"]).abs()
    b_dw = (2 * d_inner + 2 * wdelta / 3 * 4 * U + U * (2 * r["inner"].abs() + 2 * wdelta / 3)) * scale + U * (r["dw"] * scale).abs()
    terms = (wd * r["inner"]).abs() + (wd * wd * r["delta"]).abs() / 3
    b_loss = (wd.abs() * d_inner + 5 * U * terms).sum(-1) + (math.ceil(S / 64) + 6) * U * terms.sum(-1)
    per, dw = torch.empty(n, device="cuda"), torch.empty(n, S, device="cuda")
    sd, wd = s.cuda(), w.cuda()
    N.check(lib.nsamd_distortion_loss(N.ptr(sd), N.ptr(wd), S, n, scale, N.ptr(per), N.ptr(dw), st), "distortion")
    worst = {}
    check_entries("loss", per, r["loss"], b_loss, worst)
    check_entries("dw", dw, r["dw"] * scale, b_dw, worst)
    report(f"distortion S={S}", worst)
    if S == 2048:
        z = torch.zeros(4 * 2051, device="cuda")
        assert lib.nsamd_distortion_loss(N.ptr(z), N.ptr(z), 2049, 1, 1.0, N.ptr(z), N.ptr(z), st) == ERR_UNSUPPORTED


@pytest.mark.parametrize("levels", [1, 2, 4])
def test_proposal_losses_vs_float64(F, levels):
    """nsamd_proposal_losses: every level's interlevel loss and dw_prop, the distortion loss and dw, one launch."""
    N = _n()
    lib, st = N.load(), N.stream()
    n, Sf = 203, 48
    Sps = [96, 256, 63, 700][:levels]
    worst = {}
    cases = [_interlevel_case(n, Sf, Sp, 77 + Sp) for Sp in Sps]
    c, w = cases[0][0], cases[0][1]
    c[3] = torch.sort(c[3]).values  # (the fine edges are shared: keep them sorted here)
    parr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    cps = [x[2].cuda() for x in cases]
    wps = [x[3].cuda() for x in cases]
    per = [torch.empty(n, device="cuda") for _ in Sps]
    dwp = [torch.empty(n, Sp, device="cuda") for Sp in Sps]
    dist, dwd = torch.empty(n, device="cuda"), torch.empty(n, Sf, device="cuda")
    cd, wd = c.cuda(), w.cuda()
    N.check(lib.nsamd_proposal_losses(N.ptr(cd), N.ptr(wd), Sf, levels, parr(cps), parr(wps), (C.c_int32 * levels)(*Sps), n,
                                      0.37, 0.011, parr(per), parr(dwp), N.ptr(dist), N.ptr(dwd), st), "proposal_losses")
    for i, Sp in enumerate(Sps):
        r = orc.interlevel_bwd64(c, w, cases[i][2], cases[i][3])
        b_loss, b_dwp = interlevel_bounds(r, Sf, 0.37, (~_sorted_rows(r)).double())
        check_entries(f"loss[{i}]", per[i], r["loss"], b_loss, worst)
        check_entries(f"dw_prop[{i}]", dwp[i], r["dwp"] * 0.37, b_dwp, worst)
    r = orc.distortion_bwd64(c, w)
    w64 = w.double()
    d_inner = U * r["mid_abs"] + (Sf + 2) * U * r["inner_abs"]
    wdelta = (w64 * r["delta"]).abs()
    b_dw = (2 * d_inner + 2 * wdelta / 3 * 4 * U + U * (2 * r["inner"].abs() + 2 * wdelta / 3)) * 0.011 + U * (r["dw"] * 0.011).abs()
    terms = (w64 * r["inner"]).abs() + (w64 * w64 * r["delta"]).abs() / 3
    b_loss = (w64.abs() * d_inner + 5 * U * terms).sum(-1) + (math.ceil(Sf / 64) + 6) * U * terms.sum(-1)
    check_entries("distortion loss", dist, r["loss"], b_loss, worst)
    check_entries("distortion dw", dwd, r["dw"] * 0.011, b_dw, worst)
    report(f"proposal_losses levels={levels}", worst)


# ---------------------------------------------------------------- density MLP -------------------------------------------

def _mlp_params(IN, H, seed, coherent):
    g = torch.Generator().manual_seed(seed)
    W0 = torch.randn(H, IN, generator=g) / math.sqrt(IN)
    b0 = torch.randn(H, generator=g) * 0.1
    W1 = torch.randn(1, H, generator=g) / math.sqrt(H)
    b1 = torch.randn(1, generator=g) * 0.1
    if coherent:
        W1 = W1.abs()
    return W0, b0, W1, b1


def _mlp_inputs(IN, M, seed, coherent):
    g = torch.Generator().manual_seed(seed)
    if coherent:  # one sign throughout: sum |terms| = |sum|
        enc = torch.rand(M, IN, generator=g) * 0.9 + 0.1
        pre = torch.rand(M, generator=g) * 4 - 2
        gd = torch.rand(M, generator=g) * 0.5 + 0.5
        sel = torch.ones(M)
    else:
        enc = torch.randn(M, IN, generator=g)
        pre = torch.rand(M, generator=g) * 50 - 25  # beyond the clamp at +-15
        gd = torch.randn(M, generator=g) * 10.0 ** (torch.rand(M, generator=g) * 4 - 4)
        sel = (torch.rand(M, generator=g) > 0.1).float()
    return enc, pre, gd, sel


class _Mlp:
    def __init__(self, F, W0, b0, W1, b1, avg):
        self.t = [x.cuda().contiguous() for x in (W0, b0, W1, b1)]
        self.host = (W0, b0, W1, b1)
        self.avg = avg
        self.native = F.density_mlp(*self.t, avg)


def _mlp_bwd_ref(enc, sel, pre, gd, mlp, IN):
    W0, b0, W1, b1 = mlp.host
    r = orc.density_mlp_bwd64(enc, sel, pre, gd, W0, b0, W1, b1, mlp.avg)
    amb = relu_ambiguous(r["a"], r["a_abs"], IN)
    if bool(amb.any()):  # take the ReLU-ambiguous points' upstream gradient out (both sides)
        gd = gd.clone()
        gd[amb] = 0.0
        r = orc.density_mlp_bwd64(enc, sel, pre, gd, W0, b0, W1, b1, mlp.avg)
    return r, gd, int(amb.sum())


def _run_bwd(F, enc, sel, pre, gd, mlp, M, workspace, gate=None, mask=None, spr=1):
    N = _n()
    lib, st = N.load(), N.stream()
    IN, H = mlp.host[0].shape[1], mlp.host[0].shape[0]
    encT = enc.t().contiguous().cuda()
    denc = torch.full((IN, M), 123.0, device="cuda")
    grads = [torch.zeros(H, IN, device="cuda"), torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda"),
             torch.zeros(1, device="cuda")]
    ws = None
    if workspace:
        ws = torch.empty(K_MAX_BLOCKS * ((H * IN + 2 * H + 1 + 3) & ~3), device="cuda")
    seld, pred, gdd = sel.cuda(), pre.cuda(), gd.cuda()
    args = (N.ptr(encT), N.ptr(seld), N.ptr(pred), N.ptr(gdd), M, mlp.native, N.ptr(denc),
            *[N.ptr(x) for x in grads], N.ptr(ws), 0 if ws is None else ws.numel())
    if gate is None:
        N.check(lib.nsamd_density_mlp_bwd(*args, st), "density_mlp_bwd")
    else:
        N.check(lib.nsamd_density_mlp_bwd_gated(*args, gate.data_ptr(), N.ptr(mask), spr, st), "density_mlp_bwd_gated")
    torch.cuda.synchronize()
    return denc.t().cpu(), grads


def _check_mlp(tag, r, denc, grads, IN, H, M, atomics, worst, W0, W1, rows=None):
    r = dict(r, W1W0=W1.double().abs().reshape(-1) @ W0.double().abs())
    b = mlp_bounds(r, IN, H, M, atomics)
    if rows is None:
        check_entries(f"{tag} denc", denc, r["denc"], b["denc"], worst)
    else:
        check_entries(f"{tag} denc", denc[rows], r["denc"][rows], b["denc"][rows], worst)
    for k, gt in zip(("dW0", "db0", "dW1", "db1"), grads):
        check_entries(f"{tag} {k}", gt.reshape(-1), r[k].reshape(-1), b[k].reshape(-1), worst)


@pytest.mark.parametrize("IN,H", MLP_SHAPES)
def test_density_mlp_forward_vs_float64(F, IN, H):
    N = _n()
    lib, st = N.load(), N.stream()
    worst = {}
    for M in (1, 255, 256, 257, 768 * 256 + 1):
        mlp = _Mlp(F, *_mlp_params(IN, H, M + IN, False), 0.01)
        enc, _, _, sel = _mlp_inputs(IN, M, M, False)
        dens, pre = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        encd, seld = enc.t().contiguous().cuda(), sel.cuda()
        N.check(lib.nsamd_density_mlp_fwd(N.ptr(encd), N.ptr(seld), M, mlp.native, N.ptr(dens),
                                          N.ptr(pre), st), "density_mlp_fwd")
        W0, b0, W1, b1 = mlp.host
        r = orc.density_mlp_fwd64(enc, sel, W0, b0, W1, b1, mlp.avg)
        dpre = IN * U * (r["a_abs"] @ W1.double().abs().reshape(-1)) + H * U * r["pre_abs"]
        check_entries("pre", pre, r["pre"], dpre, worst)
        check_entries("density", dens, r["density"], r["density"] * (dpre * (1 + dpre) + E_EXP + 2 * U), worst)
    report(f"density MLP forward ({IN},{H})", worst)


M_SMALL = [1, 255, 256, 257, 768 * 256, 768 * 256 + 1]
M_LARGE = [4096 * 96, 4096 * 256]


@pytest.mark.parametrize("IN,H", MLP_SHAPES)
@pytest.mark.parametrize("workspace", [True, False])
def test_density_mlp_backward_vs_float64(F, IN, H, workspace):
    """nsamd_density_mlp_bwd at M in {1, 255, 256, 257, 768*256, 768*256 + 1} (the step from one chunk per workgroup to
    two) and, for H = 16, 4096*96 and 4096*256; with the workspace (fixed-order reduce) and without (float atomics);
    random-sign inputs with pre beyond +-15 and selector zeros, and sign-coherent inputs."""
    Ms = M_SMALL + (M_LARGE if H == 16 else [])
    worst, amb_total = {}, 0
    for M in Ms:
        for coherent in (False, True):
            mlp = _Mlp(F, *_mlp_params(IN, H, M + 7 * IN + H, coherent), 0.01 if not coherent else 1.0)
            enc, pre, gd, sel = _mlp_inputs(IN, M, M + 1, coherent)
            r, gd, amb = _mlp_bwd_ref(enc, sel, pre, gd, mlp, IN)
            amb_total += amb
            denc, grads = _run_bwd(F, enc, sel, pre, gd, mlp, M, workspace)
            _check_mlp(f"coh={int(coherent)}", r, denc, grads, IN, H, M, not workspace, worst, *mlp.host[0:3:2])
    report(f"density MLP backward ({IN},{H}) workspace={workspace}; {amb_total} ReLU-ambiguous points taken out", worst)
    assert amb_total <= 200


@pytest.mark.parametrize("spr", [48, 96, 256])
@pytest.mark.parametrize("live", [0.03, 0.4, 1.0, "3 rays"])
def test_density_mlp_backward_gated_vs_float64(F, spr, live):
    """nsamd_density_mlp_bwd_gated with a ray mask (the rays without gradient have zero upstream gradient, as the mask's
    producer guarantees): the float64 reference is over the live rays; denc is compared on their points. At spr 48 rays
    straddle the 256-point chunks. The 1-3 live rays are sign-coherent."""
    IN, H = 10, 16
    n = 4096
    M = n * spr
    g = torch.Generator().manual_seed(spr)
    if live == "3 rays":
        keep = torch.zeros(n, dtype=torch.bool)
        keep[[5, 2047, 4095]] = True
        coherent = True
    else:
        keep = torch.rand(n, generator=g) < live
        coherent = False
    mlp = _Mlp(F, *_mlp_params(IN, H, spr, coherent), 1.0 if coherent else 0.01)
    enc, pre, gd, sel = _mlp_inputs(IN, M, spr + 5, coherent)
    pts = keep.repeat_interleave(spr)
    gd = gd * pts
    r, gd, amb = _mlp_bwd_ref(enc, sel, pre, gd, mlp, IN)
    worst = {}
    gate = torch.ones(4, dtype=torch.int32, device="cuda")
    for ws in (True, False):
        denc, grads = _run_bwd(F, enc, sel, pre, gd, mlp, M, ws, gate, keep.to(torch.uint8).cuda(), spr)
        _check_mlp(f"ws={int(ws)}", r, denc, grads, IN, H, M, not ws, worst, *mlp.host[0:3:2], rows=pts)
    report(f"gated density MLP backward spr={spr} live={live} ({amb} ReLU-ambiguous)", worst)


def _screen_enc(enc, mlp, IN):
    """Replace the features of points whose hidden pre-activation is within the forward bound of zero by those of the
    first unambiguous point (for chains whose upstream gradient the test cannot edit)."""
    W0, b0 = mlp.host[0].double(), mlp.host[1].double()
    a = enc.double() @ W0.t() + b0
    a_abs = enc.double().abs() @ W0.abs().t() + b0.abs()
    amb = relu_ambiguous(a, a_abs, IN)
    if bool(amb.any()):
        enc = enc.clone()
        enc[amb] = enc[int(torch.nonzero(~amb)[0])].clone()
    return enc, int(amb.sum())


def test_proposal_levels_pair_vs_float64(F):
    """nsamd_proposal_levels_bwd on two levels of very different M (4096 x 256 and 37 x 96): the merged weights-backward and
    density-MLP launches, where the level with fewer blocks takes the `blockIdx.x >= nblocks` exit. Each level's density
    gradient, ray mask, gate and MLP gradients against its own float64 result (the MLP reference takes the chain's own
    density gradient as its input)."""
    N = _n()
    lib, st = N.load(), N.stream()
    IN, H = 10, 16
    spec = F.HashGridSpec(5, 16, 128, 12)
    shapes = [(4096, 256), (37, 96)]
    keep_alive, levels, hosts = [], (N.ProposalLevelBwd * 2)(), []  # (the structs hold raw pointers into keep_alive)
    gates = torch.zeros(8, dtype=torch.int32, device="cuda")
    for i, (n, S) in enumerate(shapes):
        M = n * S
        t, dens, dw = _weights_case(n, S, 300 + i)
        dens = dens.nan_to_num(0.0, 0.0, 0.0).clamp(min=0.0)
        live = torch.rand(n, generator=torch.Generator().manual_seed(i)) < 0.4
        dw = dw.nan_to_num(0.0, 0.0, 0.0) * live[:, None]
        mlp = _Mlp(F, *_mlp_params(IN, H, 500 + i, False), 0.01)
        enc, pre, _, sel = _mlp_inputs(IN, M, 600 + i, False)
        enc, _ = _screen_enc(enc, mlp, IN)
        g = torch.Generator().manual_seed(700 + i)
        o = torch.randn(n, 3, generator=g) * 0.5
        d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
        dev = [x.cuda().contiguous() for x in (t, dens, dw, enc.t(), sel, pre, o, d)]
        ddens, denc = torch.empty(n, S, device="cuda"), torch.empty(IN, M, device="cuda")
        grads = [torch.zeros(H, IN, device="cuda"), torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda"),
                 torch.zeros(1, device="cuda")]
        mws = torch.empty(K_MAX_BLOCKS * ((H * IN + 2 * H + 1 + 3) & ~3), device="cuda")
        mask = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        table = torch.randn(5 * spec.table_size * 2, device="cuda") * 0.1
        dtable = torch.zeros_like(table)
        ws, ws_n = F._scatter_workspace(spec, torch.device("cuda"), M)
        assert ws is not None
        e = levels[i]
        e.num_rays, e.samples_per_ray = n, S
        e.t_bins, e.density, e.dweights = N.ptr(dev[0]), N.ptr(dev[1]), N.ptr(dev[2])
        e.ddensity, e.gate, e.ray_mask = N.ptr(ddens), gates.data_ptr() + 16 * i, N.ptr(mask)
        e.enc, e.selector, e.pre = N.ptr(dev[3]), N.ptr(dev[4]), N.ptr(dev[5])
        e.mlp = mlp.native
        e.denc = N.ptr(denc)
        e.dW0, e.db0, e.dW1, e.db1 = (N.ptr(x) for x in grads)
        e.mlp_workspace, e.mlp_workspace_floats = N.ptr(mws), mws.numel()
        e.origins, e.directions = N.ptr(dev[6]), N.ptr(dev[7])
        e.transform, e.aabb = N.XFORM_CONTRACT, N.Aabb()
        e.table, e.grid = N.ptr(table), spec.native()
        e.dtable = N.ptr(dtable)
        e.scatter_workspace, e.scatter_workspace_floats = N.ptr(ws), ws_n
        keep_alive += [dev, ddens, denc, grads, mws, mask, table, dtable, ws, mlp]
        hosts.append((n, S, M, t, dens, dw, enc, pre, sel, mlp, ddens, denc, grads, mask, live))
    N.check(lib.nsamd_proposal_levels_bwd(levels, 2, 0, st), "proposal_levels_bwd")
    torch.cuda.synchronize()
    worst = {}
    for i, (n, S, M, t, dens, dw, enc, pre, sel, mlp, ddens, denc, grads, mask, live) in enumerate(hosts):
        r = orc.weights_bwd64(t, dens, dw)
        check_entries(f"L{i} ddensity", ddens, r["ddensity"], weights_bound(r), worst)
        pred = gate_predicate(t, dens, dw)
        assert np.array_equal(mask.cpu().numpy(), pred.astype(np.uint8)) and int(gates[4 * i]) == int(pred.any())
        gd = ddens.cpu().reshape(-1)
        W0, b0, W1, b1 = mlp.host
        rm = orc.density_mlp_bwd64(enc, sel, pre, gd, W0, b0, W1, b1, mlp.avg)
        rows = torch.from_numpy(pred).repeat_interleave(S)
        _check_mlp(f"L{i}", rm, denc.t().cpu(), grads, IN, 16, M, False, worst, W0, W1, rows=rows)
    report("proposal levels pair", worst)


# ---------------------------------------------------------------- merged chain == per-level chain, bit for bit ---------

CHAIN_OUTPUTS = ("ddens", "denc", "mask", "dW0", "db0", "dW1", "db1", "dtable")
DENC_PREFILL = 123.0  # (the chain does not write the rows of rays without gradient)


def _chain_levels(F, shapes, one_network=False, zero_dw=()):
    """nsamd_proposal_level_bwd structs for `shapes` = [(rays, samples)], set up as test_proposal_levels_pair_vs_float64 does:
    grid (5, 16, 128, 12), IN, H = 10, 16, about a third of the rays carrying dweights (other rays per level; none on the
    levels in `zero_dw`). one_network: every level has the same MLP gradients, table, dtable, MLP and scatter workspaces.
    Returns (struct array, gates, per-level dicts of tensors and launch arguments)."""
    N = _n()
    IN, H = 10, 16
    spec = F.HashGridSpec(5, 16, 128, 12)
    levels, out = (N.ProposalLevelBwd * len(shapes))(), []
    gates = torch.zeros(4 * len(shapes), dtype=torch.int32, device="cuda")
    for i, (n, S) in enumerate(shapes):
        M = n * S
        t, dens, dw = _weights_case(n, S, 900 + i)
        dens = dens.nan_to_num(0.0, 0.0, 0.0).clamp(min=0.0)
        live = torch.rand(n, generator=torch.Generator().manual_seed(40 + i)) < 0.33
        dw = dw.nan_to_num(0.0, 0.0, 0.0) * live[:, None]
        if i in zero_dw:
            dw = torch.zeros_like(dw)
        enc, pre, _, sel = _mlp_inputs(IN, M, 950 + i, False)
        g = torch.Generator().manual_seed(980 + i)
        o = torch.randn(n, 3, generator=g) * 0.5
        d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
        L = dict(n=n, S=S, M=M, spec=spec)
        for k, x in zip(("t", "dens", "dw", "enc", "sel", "pre", "o", "d"), (t, dens, dw, enc.t(), sel, pre, o, d)):
            L[k] = x.cuda().contiguous()
        L["ddens"], L["denc"] = torch.empty(n, S, device="cuda"), torch.empty(IN, M, device="cuda")
        L["mask"] = torch.empty(n, dtype=torch.uint8, device="cuda")
        if one_network and i > 0:
            for k in ("mlp", "dW0", "db0", "dW1", "db1", "mws", "table", "dtable"):
                L[k] = out[0][k]
        else:
            L["mlp"] = _Mlp(F, *_mlp_params(IN, H, 990 + i, False), 0.01)
            L["dW0"], L["db0"] = torch.empty(H, IN, device="cuda"), torch.empty(H, device="cuda")
            L["dW1"], L["db1"] = torch.empty(H, device="cuda"), torch.empty(1, device="cuda")
            L["mws"] = torch.empty(K_MAX_BLOCKS * ((H * IN + 2 * H + 1 + 3) & ~3), device="cuda")
            L["table"] = torch.randn(5 * spec.table_size * 2, device="cuda") * 0.1
            L["dtable"] = torch.empty_like(L["table"])
        L["ws"], L["ws_n"] = F._scatter_workspace(spec, torch.device("cuda"), M)
        assert L["ws"] is not None
        L["gate"] = gates.data_ptr() + 16 * i
        e = levels[i]
        e.num_rays, e.samples_per_ray = n, S
        e.t_bins, e.density, e.dweights = N.ptr(L["t"]), N.ptr(L["dens"]), N.ptr(L["dw"])
        e.ddensity, e.gate, e.ray_mask = N.ptr(L["ddens"]), L["gate"], N.ptr(L["mask"])
        e.enc, e.selector, e.pre = N.ptr(L["enc"]), N.ptr(L["sel"]), N.ptr(L["pre"])
        e.mlp = L["mlp"].native
        e.denc = N.ptr(L["denc"])
        e.dW0, e.db0, e.dW1, e.db1 = (N.ptr(L[k]) for k in ("dW0", "db0", "dW1", "db1"))
        e.mlp_workspace, e.mlp_workspace_floats = N.ptr(L["mws"]), L["mws"].numel()
        e.origins, e.directions = N.ptr(L["o"]), N.ptr(L["d"])
        e.transform, e.aabb = N.XFORM_CONTRACT, N.Aabb()
        e.table, e.grid = N.ptr(L["table"]), spec.native()
        e.dtable = N.ptr(L["dtable"])
        e.scatter_workspace, e.scatter_workspace_floats = N.ptr(L["ws"]), L["ws_n"]
        out.append(L)
    return levels, gates, out


def _chain_reset(gates, lv):
    """Equal starting state for a run: zeroed gradients, `denc` and `ddensity` pre-filled, gates and masks set to junk."""
    gates.fill_(5)
    for L in lv:
        for k in ("dW0", "db0", "dW1", "db1", "dtable"):
            L[k].zero_()
        L["ddens"].fill_(7.0)
        L["denc"].fill_(DENC_PREFILL)
        L["mask"].fill_(9)


def _chain_results(gates, lv):
    torch.cuda.synchronize()
    return [gates[::4].clone().cpu()] + [{k: L[k].clone().cpu() for k in CHAIN_OUTPUTS} for L in lv]


def _chain_per_level(lv, stage_major=False):
    """The per-level gated entry points: level by level (each level's three stages, then the next level), or stage_major —
    each stage over all levels before the next stage, the order nsamd_proposal_levels_bwd runs them in."""
    N = _n()
    lib, st = N.load(), N.stream()

    def weights(L):
        N.check(lib.nsamd_weights_bwd_gate(N.ptr(L["t"]), N.ptr(L["dens"]), N.ptr(L["dw"]), L["n"], L["S"], N.ptr(L["ddens"]),
                                           L["gate"], N.ptr(L["mask"]), 0, st), "weights_bwd_gate")

    def density(L):
        grads = [N.ptr(L[k]) for k in ("dW0", "db0", "dW1", "db1")]
        N.check(lib.nsamd_density_mlp_bwd_gated(N.ptr(L["enc"]), N.ptr(L["sel"]), N.ptr(L["pre"]), N.ptr(L["ddens"]), L["M"],
                                                L["mlp"].native, N.ptr(L["denc"]), *grads, N.ptr(L["mws"]), L["mws"].numel(),
                                                L["gate"], N.ptr(L["mask"]), L["S"], st), "density_mlp_bwd_gated")

    def scatter(L):
        pts = N.make_points(origins=L["o"], directions=L["d"], t_bins=L["t"], samples_per_ray=L["S"])
        N.check(lib.nsamd_hashgrid_encode_bwd_gated(pts, L["M"], N.XFORM_CONTRACT, N.Aabb(), N.ptr(L["table"]),
                                                    L["spec"].native(), N.ptr(L["denc"]), 1, L["M"], N.ptr(L["dtable"]),
                                                    N.ptr(L["ws"]), L["ws_n"], L["gate"], N.ptr(L["mask"]), st),
                "hashgrid_encode_bwd_gated")

    stages = (weights, density, scatter)
    for stage, L in ([(f, L) for f in stages for L in lv] if stage_major else [(f, L) for L in lv for f in stages]):
        stage(L)


def _assert_same_bits(tag, got, want):
    assert torch.equal(got[0], want[0]), f"{tag}: gates {got[0].tolist()} != {want[0].tolist()}"
    for i, (g, w) in enumerate(zip(got[1:], want[1:])):
        for k in CHAIN_OUTPUTS:
            a, b = (x.view(torch.int32) if x.dtype == torch.float32 else x for x in (g[k], w[k]))
            diff = int((a != b).sum())
            assert diff == 0, f"{tag}: level {i} {k}: {diff} of {a.numel()} entries differ from the per-level entry points"


@pytest.mark.parametrize("zero_level0", [False, True])
def test_proposal_levels_smaller_call_first_and_odd_level(F, zero_level0):
    """nsamd_proposal_levels_bwd on THREE levels (37 x 96), (300 x 256), (50 x 48): levels 0 and 1 are all run-routed and share
    every launch with the SMALLER call first — slice 0 has fewer workgroups than slice 1 in the weights, density-MLP and route
    launches, so it takes the corner exits —; level 2 runs alone, through the fine route and the single-call launches. Against
    the per-level gated entry points level by level, on equal inputs, zeroed gradients and the same workspaces: density
    gradient, denc, gates, ray masks, the four MLP gradients and the table gradient bit for bit. The call runs twice (the
    scatter workspace's self-cleaning header serves the second). zero_level0: level 0 carries no gradient — its gate stays
    clear, its denc keeps the pre-filled value, its gradients stay zero; level 1 is as without."""
    N = _n()
    lib, st = N.load(), N.stream()
    shapes = [(37, 96), (300, 256), (50, 48)]
    levels, gates, lv = _chain_levels(F, shapes, zero_dw=(0,) if zero_level0 else ())
    assert lv[0]["ws"].data_ptr() != lv[1]["ws"].data_ptr()  # (levels 0 and 1 may share launches)
    _chain_reset(gates, lv)
    _chain_per_level(lv)
    want = _chain_results(gates, lv)
    assert want[0].tolist() == [0 if zero_level0 else 1, 1, 1]
    for i, L in enumerate(lv):
        live = int(want[1 + i]["mask"].sum())
        assert (live == 0) if (zero_level0 and i == 0) else (0 < live < L["n"])
        assert bool((want[1 + i]["dtable"] != 0).any()) == (live > 0)
    if zero_level0:
        z = want[1]
        assert bool((z["denc"] == DENC_PREFILL).all()) and float(z["ddens"].abs().max()) == 0.0
        assert all(float(z[k].abs().max()) == 0.0 for k in ("dW0", "db0", "dW1", "db1", "dtable"))
    for run in range(2):
        _chain_reset(gates, lv)
        N.check(lib.nsamd_proposal_levels_bwd(levels, 3, 0, st), "proposal_levels_bwd")
        _assert_same_bits(f"run {run}", _chain_results(gates, lv), want)
    for L in lv:
        ev = F.scatter_events(L["ws"])
        assert ev[1] == 0 and ev[2] == 0, ev


def test_proposal_levels_one_network_runs_in_turn(F):
    """Two levels (37 x 96), (64 x 256) with ONE network: the same MLP gradients, table, table gradient and scatter workspace.
    The density and scatter stages must then run level after level (the weights stage may still pair), accumulating into the
    same gradients: bit for bit what the per-level entry points give, called in the same order."""
    N = _n()
    lib, st = N.load(), N.stream()
    levels, gates, lv = _chain_levels(F, [(37, 96), (64, 256)], one_network=True)
    assert lv[0]["ws"].data_ptr() == lv[1]["ws"].data_ptr() and lv[0]["dtable"].data_ptr() == lv[1]["dtable"].data_ptr()
    _chain_reset(gates, lv)
    _chain_per_level(lv, stage_major=True)
    want = _chain_results(gates, lv)
    assert want[0].tolist() == [1, 1] and bool((want[1]["dtable"] != 0).any())
    _chain_reset(gates, lv)
    N.check(lib.nsamd_proposal_levels_bwd(levels, 2, 0, st), "proposal_levels_bwd")
    _assert_same_bits("one network", _chain_results(gates, lv), want)


# ---------------------------------------------------------------- identical inputs from the product ---------------------

def test_bench_shape_proposal_chain_vs_float64(F):
    """The benchmark's shape (4096 rays x (256, 96, 48), bench tables) through NerfactoTrainStep on a proposal-update
    iteration; every proposal stage is then checked against float64 on the step's OWN buffers: the interlevel dw_prop
    (nsamd_proposal_losses), the weights backward with its gate and masks, the density MLP backward of each level (its
    ReLU-ambiguous points' upstream gradient taken out on both sides, then rerun through the gated entry point), and
    render_train_bwd on the fine level."""
    from test_gpu_kernels import _hip_model

    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.train_step import NerfactoTrainStep

    N = _n()
    lib, st = N.load(), N.stream()
    cfg = orc.NerfactoCfg()
    params = orc.init_params(cfg, seed=0, table_std=0.3)
    model = _hip_model(cfg, params)
    arena = ParamArena(model.get_param_groups_ordered(), lr=1e-2, eps=1e-15)
    n = 4096
    step = NerfactoTrainStep(model, n, torch.device("cuda"))
    step.side_stream = None
    o, d, cam, tgt = orc.synthetic_rays(n, cfg.num_images, seed=31)
    step.set_batch(o.cuda(), d.cuda(), cam.cuda(), tgt.cuda())
    step.jitter.copy_(torch.from_numpy(np.random.RandomState(3).uniform(0, 1, (3, n)).astype(np.float32)))
    step.anneal_dev.fill_(1.0)
    arena.zero_grad()
    step.forward_and_losses(True, draw_jitter=False)
    torch.cuda.synchronize()
    L = step.n_prop
    Sf = step.counts[L]
    worst = {}
    scale = float(cfg.interlevel_loss_mult) / (n * Sf)
    c, w = step.s_bins[L].cpu(), step.weights[L].cpu()
    for lvl in range(L):
        r = orc.interlevel_bwd64(c, w, step.s_bins[lvl].cpu(), step.weights[lvl].cpu())
        assert bool(_sorted_rows(r).all())
        _, b_dwp = interlevel_bounds(r, Sf, scale, torch.zeros(n, dtype=torch.float64))
        check_entries(f"L{lvl} dw_prop", step.dw_prop[lvl], r["dwp"] * scale, b_dwp, worst)
    amb_total = 0
    for lvl in range(L):
        S = step.counts[lvl]
        M = n * S
        gate = torch.zeros(4, dtype=torch.int32, device="cuda")
        mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
        ddens = torch.empty(n, S, device="cuda")
        t, dens, dwp = step.t_bins[lvl], step.p_dens[lvl], step.dw_prop[lvl].view(n, S)
        N.check(lib.nsamd_weights_bwd_gate(N.ptr(t), N.ptr(dens), N.ptr(dwp), n, S, N.ptr(ddens), gate.data_ptr(), N.ptr(mask),
                                           0, st), "weights_bwd_gate")
        torch.cuda.synchronize()
        r = orc.weights_bwd64(t.cpu(), dens.cpu().view(n, S), dwp.cpu())
        check_entries(f"L{lvl} ddensity", ddens, r["ddensity"], weights_bound(r), worst)
        pred = gate_predicate(t, dens.view(n, S), dwp)
        assert np.array_equal(mask.cpu().numpy(), pred.astype(np.uint8)) and int(gate[0]) == int(pred.any())
        net = step.props[lvl]
        W0, b0, W1, b1 = (x.detach() for x in net.mlp_base[1].param_tensors())
        mlp = _Mlp(F, W0.cpu(), b0.cpu(), W1.cpu(), b1.cpu(), net.average_init_density)
        IN = W0.shape[1]
        enc, sel, pre = step.p_enc[lvl].t().contiguous().cpu(), step.p_sel[lvl].cpu(), step.p_pre[lvl].cpu()
        rm, gd, amb = _mlp_bwd_ref(enc, sel, pre, ddens.cpu().reshape(-1), mlp, IN)
        amb_total += amb
        denc, grads = _run_bwd(F, enc, sel, pre, gd, mlp, M, True, torch.ones(4, dtype=torch.int32, device="cuda"), mask, S)
        rows = torch.from_numpy(pred).repeat_interleave(S)
        _check_mlp(f"L{lvl} mlp", rm, denc, grads, IN, W0.shape[0], M, False, worst, W0.cpu(), W1.cpu(), rows=rows)
        rel = {k: float(np.linalg.norm(_np(gt).reshape(-1) - _np(rm[k]).reshape(-1)) / max(1e-30, float(rm[k].norm())))
               for k, gt in zip(("dW0", "db0", "dW1", "db1"), grads)}
        print(f"\nL{lvl}: {int(pred.sum())} of {n} rays carry gradient; MLP weight gradients rel-L2 vs float64 " +
              ", ".join(f"{k} {v:.1e}" for k, v in rel.items()))
    # render_train_bwd on the step's fine-level buffers
    drgb, dden = torch.empty(n, Sf, 3, device="cuda"), torch.empty(n, Sf, device="cuda")
    N.check(lib.nsamd_render_train_bwd(N.ptr(step.f_rgb), N.ptr(step.weights[L]), N.ptr(step.f_dens), N.ptr(step.t_bins[L]), n,
                                       Sf, step.bg_mode, step.bg_vals, N.ptr(step.d_rgb_out), N.ptr(step.dw_dist), N.ptr(drgb),
                                       N.ptr(dden), N.ptr(step.bg_rays), st), "render_train_bwd")
    torch.cuda.synchronize()
    bgc = tuple(step.bg_vals) if step.bg_vals is not None else None
    cb = orc.composite_bwd64(step.f_rgb.cpu().view(n, Sf, 3), step.weights[L].cpu(), step.d_rgb_out.cpu(), step.bg_mode, bgc,
                             step.bg_rays.cpu() if step.bg_mode == 3 else None, step.dw_dist.cpu().view(n, Sf))
    rw = orc.weights_bwd64(step.t_bins[L].cpu(), step.f_dens.cpu().view(n, Sf), cb["d_weights"])
    check_entries("main d_density", dden, rw["ddensity"], weights_bound(rw, 8 * U * cb["dw_abs"]), worst)
    report(f"bench-shape proposal chain ({amb_total} ReLU-ambiguous points)", worst)
