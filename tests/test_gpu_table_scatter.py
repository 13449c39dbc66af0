"""The hash table's gradient scatter (csrc/scatter.hip, scatter.h, and the record emission of nsamd_field_mlp_bwd_scatter in
csrc/field_mlp.hip) ENTRY BY ENTRY against a float64 scatter of the same contributions (orc.hashgrid_scatter64), on every
route the kernels take: fine static segments and their dynamic overflow, run merging, spill fold and the float-atomic
tail, straddling pairs, selector-masked points, gated calls with ray masks, and the fused producer.

Per-entry bound (entry e of level l, n_e contributions c_j = g_j * w_j, ref64 = sum c_j, abs64 = sum |c_j|):

    |got - ref64| <= c1 * 2^-24 * abs64 + n_e * 2^-k + 2^-24 * |ref64| + n_e * 2^-126

derived from the code, not fitted:
* c1: a contribution reaches pass 2 as the fp32 product ((g * bz) * by) * bx, three roundings, relative error
  <= (1 + 2^-24)^3 - 1 < 3.0001 * 2^-24 (fine route, the producer, run records of one sample); a run record
  (scatter_route_runs_body) adds up to kRunLen = 4 such products in fp32 registers, recursive summation
  <= (kRunLen - 1) * 2^-24 * sum |terms| more: c1 = 3 + 3. A further 1/64 covers the float64 reference's own rounding and
  the second-order products of the terms.
* 2^-k: to_fixed truncates every summand toward zero, |error| < 2^-k, one summand per contribution at most (a pair
  record is one summand per corner; a merged run record stands for several contributions). scatter.h:
  k = 188 - headroom - e_max, e_max the exponent field of hdr[level]: the largest |gradient| the level's records were
  built from (fine route and producer: max |g|; run route: max |g| with exponent + 2, the x kRunLen bump). This is
  2^(headroom - 61) * 2^(e_max - 127) <= 2^(headroom - 61) * R_l with R_l = max |g| (x 4 on run levels), the largest value
  a record of the level can carry. The headroom is reproduced exactly, 2 + bit_length(Q + kSpillFold - 1) from the
  level's queue capacity Q, which `_plan` / `_producer_plan` restate from scatter_plan / scatter_plan_producers
  (scatter.hip) and check against the library's workspace size. So the term is exact, not an upper bound: a scale a bit
  off shows on the entries whose contributions are small against the level's maximum (denc is drawn log-uniform over
  eight decades for that reason).
* 2^-24 * |ref64|: from_fixed rounds the exact fixed-point sum to fp32 once.
* n_e * 2^-126: a product below FLT_MIN may be flushed to zero, one such loss per contribution.
Accumulating calls add one more fp32 rounding (2^-24 * |prefill + ref64|); spill records beyond kSpillFold go in as
float atomics (scatter_finish_body), so there the first term grows to max(c1, n_e) * 2^-24 * (abs64 + |prefill|).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import nerfacto_oracle as orc
from position_gradient_reference import _contract_bwd, _position_grad  # noqa: F401  (moved there; _position_grad uses the first)

pytestmark = pytest.mark.gpu

# constants of scatter.hip / scatter.h / field_mlp.hip restated (the plan and the headroom are derived from them)
K_RUN_LEN = 4
K_SPILL_FOLD = 8192
K_FINE_THREADS = 1024
K_TARGET_TILES = 512
K_SLICE_LOG2_MAX = 13
K_MAX_LOG2_BINS = 10
K_PRODUCER_MAX_LOG2_BINS = 6
K_PRODUCER_SEG_CAP = 256
K_COOP_WAVES = 8
K_HDR_WORDS = 64
U = 2.0**-24
TINY = 2.0**-126
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


def _r4(v):
    return (v + 3) & ~3


def _ceil(a, b):
    return -(-a // b)


def _tiles(scal, log2_T):
    """slice_log2 / log2_bins as scatter_plan and scatter_plan_producers choose them."""
    L = len(scal)
    bits = 0
    while (L << bits) < K_TARGET_TILES:
        bits += 1
    sl = log2_T - bits
    sl_pair = 1
    while (1 << sl_pair) < int(max(scal)) + 2 and sl_pair < K_SLICE_LOG2_MAX:
        sl_pair += 1
    sl = max(sl, sl_pair)
    sl = K_SLICE_LOG2_MAX if sl > K_SLICE_LOG2_MAX else max(sl, 8)
    sl = min(sl, log2_T)
    return sl, log2_T - sl


def _plan(scal, log2_T, M, write_only):
    """scatter_plan (scatter.hip) restated: tiles, static segments, per-level queue capacity, spill list, words."""
    L = len(scal)
    sl, lb = _tiles(scal, log2_T)
    if M <= 0 or lb > K_MAX_LOG2_BINS:
        return None
    bins = 1 << lb
    segs = _ceil(M, K_FINE_THREADS)
    C_ = max(_r4(2 * _ceil(4 * K_FINE_THREADS, bins)), 16)
    expect = _ceil(4 * M, bins)
    Qn = _r4(max(segs * C_ + expect // 2 + 64, 2 * expect + expect // 2 + 64))
    Qs = _r4(max(segs * C_ + 6 * expect + 64, 8 * expect + 64))
    caps = [Qs if (float(s) + 1.0) ** 3 * 2.0 <= float(1 << log2_T) else Qn for s in scal]
    spill = 4 * M * L + 64 if write_only else min(4 * M * L + 64, M * L + 4096)
    tiles = bins * L
    words = K_HDR_WORDS + _r4(tiles) + _r4(tiles * segs) + 4 * bins * sum(caps) + 4 * spill + _r4(spill)
    return dict(sl=sl, lb=lb, segs=segs, C=C_, caps=caps, spill=spill, words=words, state=K_HDR_WORDS + _r4(tiles))


def _producer_plan(scal, log2_T, M, cus):
    """scatter_plan_producers with field_bwd_blocks(M) workgroups and kProducerSegCap (field_mlp.hip)."""
    L = len(scal)
    sl, lb = _tiles(scal, log2_T)
    assert lb <= K_PRODUCER_MAX_LOG2_BINS
    bins = 1 << lb
    segs = min(cus, _ceil(_ceil(M, 16), K_COOP_WAVES))
    C_ = _r4(K_PRODUCER_SEG_CAP)
    Q = _r4(segs * C_ + _ceil(4 * M, bins) // 2 + 64)
    spill = 4 * M * L + 64
    tiles = bins * L
    words = K_HDR_WORDS + _r4(tiles) + _r4(tiles * segs) + 4 * bins * L * Q + 4 * spill + _r4(spill)
    return dict(sl=sl, lb=lb, segs=segs, C=C_, caps=[Q] * L, words=words, state=K_HDR_WORDS + _r4(tiles))


def _headroom(Q):
    return 2 + (Q + K_SPILL_FOLD - 1).bit_length()


def _coarse_levels(scal, S):
    """classify_levels (scatter.hip): ray mode with >= 96 samples per ray goes through the run kernel."""
    if S is None or S < 96:
        return [False] * len(scal)
    below = float(S) if S >= 192 else 1e30
    return [float(s) < below for s in scal]


class Case:
    """Points of one scatter call (ray mode or positions), their fp32 grid inputs on the host and the native structs."""

    def __init__(self, F, L, min_res, max_res, log2_T, M, pts, keep, x, transform, box, S=None):
        self.spec = F.HashGridSpec(L, min_res, max_res, log2_T)
        self.scal = [float(s) for s in self.spec.scalings()]
        self.L, self.T, self.log2_T, self.M = L, 1 << log2_T, log2_T, M
        self.pts, self.keep, self.x, self.transform, self.box, self.S = pts, keep, x, transform, box, S
        self.coarse = _coarse_levels(self.scal, S)


def _rays(F, L, min_res, max_res, log2_T, n, S, seed, concentrated=False, same=False):
    from nerfstudio_amd import _native as N

    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g) * 0.5
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    if same:
        o, d = o[:1].expand(n, 3).contiguous(), d[:1].expand(n, 3).contiguous()
    if concentrated:  # samples bunched within +-1 % of one depth per ray
        centre = torch.rand(n, 1, generator=g) * 2 + 0.3
        t = centre * (1 + 0.02 * (torch.linspace(0, 1, S + 1)[None] - 0.5))
    else:  # the piecewise sampler's bins (the kernels only read them), single jitter per ray
        jit = torch.rand(n, 1, generator=g)
        if same:
            jit = jit[:1].expand(n, 1)
        _, t = orc.piecewise_bins(torch.full((n, 1), 0.05), torch.full((n, 1), 1000.0), S, jit)
    t = t.contiguous()
    od, dd, td = o.cuda(), d.cuda(), t.cuda()
    x, _ = orc.normalise_positions(orc.sample_positions(o, d, t).reshape(-1, 3), True)
    return Case(F, L, min_res, max_res, log2_T, n * S, N.make_points(None, od, dd, td, S), (od, dd, td), x.contiguous(),
                N.XFORM_CONTRACT, N.Aabb(), S), (o, d, t)


def _positions(F, L, min_res, max_res, log2_T, M, seed, transform, outside=0.0, outside_frac=0.0):
    from nerfstudio_amd import _native as N

    rs = np.random.RandomState(seed)
    raw = rs.uniform(0, 1, (M, 3)).astype(np.float32)
    out = rs.uniform(0, 1, M) < outside_frac  # a share of the points up to `outside` beyond [0, 1] on some axis
    raw[out] = rs.uniform(-outside, 1 + outside, (int(out.sum()), 3)).astype(np.float32)
    k = min(M, 64)
    raw[: k // 2] = np.round(raw[: k // 2] * min_res) / min_res  # on lattice planes of the coarsest level
    raw[k // 2 : k] = rs.randint(0, 2, (k - k // 2, 3))          # the box's corners
    raw = torch.from_numpy(raw)
    if transform == N.XFORM_AABB:
        lo, hi = [-0.5, -1.0, 0.25], [1.5, 1.0, 2.25]
        raw = raw * torch.tensor([2.0, 2.0, 2.0]) + torch.tensor(lo)
        box = N.make_aabb(torch.tensor([lo, hi]))
        x, _ = orc.normalise_positions(raw, False, torch.tensor([lo, hi]))
    else:
        box, x = N.Aabb(), raw
    dev = raw.cuda()
    return Case(F, L, min_res, max_res, log2_T, M, N.make_points(dev), (dev,), x.contiguous(), transform, box)


def _denc(case, seed, zero_frac=0.2, scales=None):
    """[M, 2L] fp32: normal values spread log-uniformly over eight decades, a share of exact zeros."""
    rs = np.random.RandomState(seed)
    g = rs.standard_normal((case.M, 2 * case.L)) * 10.0 ** rs.uniform(-8, 0, (case.M, 2 * case.L))
    g *= rs.uniform(0, 1, (case.M, 1)) >= zero_frac
    if scales is not None:
        g *= np.repeat(np.asarray(scales, dtype=np.float64), 2)[None]
    return torch.from_numpy(g.astype(np.float32))


def _device_denc(case, denc):
    """the feature-major layout of the training step in ray mode (stride_p 1, stride_k M), point-major otherwise."""
    if case.S is not None:
        return denc.t().contiguous().cuda(), 1, case.M
    return denc.contiguous().cuda(), 2 * case.L, 1


def _check_features(F, case):
    """Precondition: the forward kernel's features on these points are the oracle's bit for bit, so the reference's cells
    and weights are the kernel's."""
    from nerfstudio_amd import _native as N

    g = torch.Generator().manual_seed(7)
    table = torch.randn(case.L * case.T, 2, generator=g)
    enc = torch.empty(case.M, 2 * case.L, device="cuda")
    N.check(N.load().nsamd_hashgrid_encode_fwd(case.pts, case.M, case.transform, case.box, N.ptr(table.cuda()),
                                               case.spec.native(), N.ptr(enc), 2 * case.L, 1, None, N.stream()), "fwd")
    ref = orc.hashgrid_encode(case.x, table, torch.tensor(case.scal), case.T)
    assert torch.equal(enc.cpu().view(torch.int32), ref.view(torch.int32)), "forward features differ from the oracle's"


def _workspace(F, case, write_only):
    """a fresh workspace (state words zero), its size checked against the restated plan"""
    from nerfstudio_amd import _native as N

    lib, g = N.load(), case.spec.native()
    words = int(lib.nsamd_hashgrid_encode_bwd_workspace(g, case.M, 1 if write_only else 0))
    state = int(lib.nsamd_hashgrid_encode_bwd_workspace_state(g, case.M))
    p = _plan(case.scal, case.log2_T, case.M, write_only)
    assert p is not None and (words, state) == (p["words"], p["state"]), ("plan restatement", words, state, p)
    ws = torch.empty(words, device="cuda")
    ws[:state].zero_()
    return ws


def _scatter(F, case, denc_dev, sp, sk, out, write_only, ws, gate=None, mask=None):
    from nerfstudio_amd import _native as N

    lib = N.load()
    table = torch.empty(1, device="cuda")  # (the table scatter reads no table)
    if gate is not None:
        rc = lib.nsamd_hashgrid_encode_bwd_gated(case.pts, case.M, case.transform, case.box, N.ptr(table), case.spec.native(),
                                                 N.ptr(denc_dev), sp, sk, N.ptr(out), N.ptr(ws), ws.numel(),
                                                 C.cast(gate.data_ptr(), C.c_void_p), N.ptr(mask), N.stream())
    else:
        fn = lib.nsamd_hashgrid_encode_bwd_set if write_only else lib.nsamd_hashgrid_encode_bwd
        rc = fn(case.pts, case.M, case.transform, case.box, N.ptr(table), case.spec.native(), N.ptr(denc_dev), sp, sk,
                N.ptr(out), None, N.ptr(ws), ws.numel(), N.stream())
    N.check(rc, "table scatter")


def _level_steps(case, denc, Q=None):
    """per level: (truncation step 2^-k, c1), from max |g| of the level and the queue capacity as pass 2 sees them"""
    caps = Q if Q is not None else _plan(case.scal, case.log2_T, case.M, True)["caps"]
    gm = denc.abs().view(case.M, case.L, 2).amax(dim=(0, 2)) if case.M else torch.zeros(case.L)
    steps, c1 = [], []
    for l in range(case.L):
        bits = int(gm[l : l + 1].view(torch.int32))
        if case.coarse[l] and bits:
            bits = min(bits + (2 << 23), NAN_BITS)
        e = (bits >> 23) & 0xFF
        k = 188 - _headroom(caps[l]) - e
        steps.append(math.ldexp(1.0, -k))
        c1.append(3.0 + (K_RUN_LEN - 1 if case.coarse[l] else 0) + 1.0 / 64)
    return steps, c1


def _check(name, case, got, ref, ab, cnt, steps, c1, prefill=None, unordered=False, levels=None):
    """the per-entry bound on every level (or `levels`); entries no contribution reaches: +0.0 (write-only) or the
    prefill's bits. -> worst |err| / bound"""
    L = case.L
    got = got.detach().cpu().view(L, -1)
    gb = got.view(torch.int32)
    ref, ab, cnt = ref.view(L, -1), ab.view(L, -1), cnt.view(L, -1)
    pre = prefill.detach().cpu().view(L, -1) if prefill is not None else None
    worst = 0.0
    for l in levels if levels is not None else range(L):
        untouched = cnt[l] == 0
        if pre is None:
            assert bool((gb[l][untouched] == 0).all()), f"{name}: level {l}: an entry without contributions is not +0.0"
            target, base = ref[l], 0.0
        else:
            assert torch.equal(gb[l][untouched], pre[l].view(torch.int32)[untouched]), f"{name}: level {l}: untouched entry changed"
            target, base = pre[l].double() + ref[l], pre[l].double().abs()
        t = ~untouched
        n = cnt[l][t]
        first = (torch.maximum(n, torch.full_like(n, c1[l])) if unordered else c1[l]) * U * (ab[l][t] + (base[t] if pre is not None else 0.0))
        bound = first + n * steps[l] + U * target[t].abs() + n * TINY
        if pre is not None:
            bound = bound + U * target[t].abs()
        err = (got[l][t].double() - target[t]).abs()
        assert bool(torch.isfinite(got[l][t]).all()), f"{name}: level {l}: non-finite result"
        ratio = err / bound
        r = float(ratio.max()) if ratio.numel() else 0.0
        if not r <= 1.0:
            i = int(ratio.argmax())
            raise AssertionError(f"{name}: level {l}: |err| {float(err[i]):.3e} > bound {float(bound[i]):.3e} (ref "
                                 f"{float(target[t][i]):.3e}, abs {float(ab[l][t][i]):.3e}, n {int(n[i])}, step {steps[l]:.3e})")
        worst = max(worst, r)
    return worst


def _fine_spills(case, denc, plan):
    """Records each fine level routes, per (pass-1 workgroup, tile): whether a static segment overflowed into the dynamic
    area, and the spill records the plan predicts (dynamic area full, straddling pairs)."""
    M, sl, lb, segs, C_ = case.M, plan["sl"], plan["lb"], plan["segs"], plan["C"]
    nz = (denc.view(M, case.L, 2) != 0).any(dim=2)
    seg = torch.arange(M) // K_FINE_THREADS
    overflow, spills = False, 0
    for l in range(case.L):
        if case.coarse[l]:
            continue
        pts = nz[:, l].nonzero().squeeze(1)
        if pts.numel() == 0:
            continue
        scaled = case.x[pts] * case.scal[l]
        lo, hi = torch.floor(scaled).numpy().astype(np.int32), torch.ceil(scaled).numpy().astype(np.int32)
        per = torch.zeros(segs << lb, dtype=torch.int64)
        for q in range(4):
            iy, iz = (hi if q & 1 else lo)[:, 1], (hi if q & 2 else lo)[:, 2]
            ia = torch.from_numpy(orc.hash_corner_index(lo[:, 0], iy, iz, 0, case.T))
            ib = torch.from_numpy(orc.hash_corner_index(hi[:, 0], iy, iz, 0, case.T))
            straddle = (ia >> sl) != (ib >> sl)
            spills += 2 * int(straddle.sum())
            keep = ~straddle
            per += torch.bincount(seg[pts][keep] * (1 << lb) + (ia[keep] >> sl), minlength=segs << lb)
        per = per.view(segs, 1 << lb)
        over = (per - C_).clamp(min=0).sum(dim=0)
        overflow |= bool((over > 0).any())
        spills += int((over - (plan["caps"][l] - segs * C_)).clamp(min=0).sum())
    return overflow, spills


def _events(F, ws):
    return F.scatter_events(ws)


def _full_case(F, name, case, denc, perm=None, expect_overflow=None, allow_unordered=False):
    """write-only (NaN-filled buffer) and accumulating (random prefill) calls on fresh workspaces, the bound, the events,
    the predicted spills of the fine levels; `perm(case, denc)` -> (permuted case, denc): bit-identical result."""
    _check_features(F, case)
    ref, ab, cnt = orc.hashgrid_scatter64(case.x, denc, torch.tensor(case.scal), case.T)
    steps, c1 = _level_steps(case, denc)
    dd, sp, sk = _device_denc(case, denc)
    plan_w = _plan(case.scal, case.log2_T, case.M, True)
    overflow, spill_pred = _fine_spills(case, denc, plan_w)
    out = torch.full((case.L * case.T, 2), float("nan"), device="cuda")
    ws = _workspace(F, case, True)
    _scatter(F, case, dd, sp, sk, out, True, ws)
    ev_w = _events(F, ws)
    unordered = ev_w[1] > 0
    w_worst = _check(f"{name} write-only", case, out, ref, ab, cnt, steps, c1, unordered=unordered)
    g = torch.Generator().manual_seed(3)
    prefill = torch.randn(case.L * case.T, 2, generator=g) * 10.0 ** (torch.rand(case.L * case.T, 2, generator=g) * 6 - 5)
    acc = prefill.cuda()
    ws_a = _workspace(F, case, False)
    _scatter(F, case, dd, sp, sk, acc, False, ws_a)
    ev_a = _events(F, ws_a)
    a_worst = _check(f"{name} accumulate", case, acc, ref, ab, cnt, steps, c1, prefill=prefill, unordered=ev_a[1] > 0)
    routes = ("run " if any(case.coarse) else "") + ("fine" if not all(case.coarse) else "")
    print(f"\n{name}: M {case.M}, routes [{routes.strip()}] (run levels {[l for l in range(case.L) if case.coarse[l]]}), "
          f"static-segment overflow {overflow}, events write-only {ev_w} / accumulate {ev_a} (fine-level spills predicted "
          f"{spill_pred}); worst err/bound {w_worst:.3f} / {a_worst:.3f}")
    for ev in (ev_w, ev_a):
        assert ev[2] == 0, f"{name}: records lost {ev}"
        assert allow_unordered or ev[1] == 0, f"{name}: records on the unordered path {ev}"
        if all(not c for c in case.coarse):  # every level routed by the fine kernel: the spills are known exactly, and
            # pass 2 folds the first kSpillFold of them, the finish pass adds the rest with float atomics
            assert (ev[0], ev[1]) == (spill_pred, max(0, spill_pred - K_SPILL_FOLD)), (name, ev, spill_pred)
    if expect_overflow is not None:
        assert overflow == expect_overflow, f"{name}: the dynamic-overflow route was {'not ' if expect_overflow else ''}reached"
    if perm is not None:
        case2, denc2 = perm(case, denc)
        dd2, sp2, sk2 = _device_denc(case2, denc2)
        out2 = torch.full_like(out, float("nan"))
        _scatter(F, case2, dd2, sp2, sk2, out2, True, _workspace(F, case2, True))
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), f"{name}: permuted input, different bits"
        print(f"{name}: permuted input gives the same bits")
    return out, ref, ab, cnt


def _permute_rays(F, o, d, t, L, min_res, max_res, log2_T):
    from nerfstudio_amd import _native as N

    def perm(case, denc):
        n, S = o.shape[0], case.S
        p = torch.randperm(n, generator=torch.Generator().manual_seed(5))
        od, dd, td = o[p].contiguous().cuda(), d[p].contiguous().cuda(), t[p].contiguous().cuda()
        x = case.x.view(n, S, 3)[p].reshape(-1, 3)
        c2 = Case(F, L, min_res, max_res, log2_T, n * S, N.make_points(None, od, dd, td, S), (od, dd, td), x, case.transform,
                  case.box, S)
        return c2, denc.view(n, S, -1)[p].reshape(n * S, -1)

    return perm


def _permute_points(F):
    from nerfstudio_amd import _native as N

    def perm(case, denc):
        p = torch.randperm(case.M, generator=torch.Generator().manual_seed(6))
        raw = case.keep[0].cpu()[p].contiguous().cuda()
        c2 = Case(F, case.L, case.spec.min_res, case.spec.max_res, case.log2_T, case.M, N.make_points(raw), (raw,),
                  case.x[p].contiguous(), case.transform, case.box)
        return c2, denc[p]

    return perm


MAIN = (16, 16, 2048, 19)


@pytest.mark.parametrize("concentrated", [False, True])
def test_main_table_at_bench_shape(F, concentrated):
    """4096 rays x 48 samples on the main grid: every level through the fine kernel, static segments and (concentrated
    bins) their dynamic overflow; ray permutation gives the same bits."""
    case, (o, d, t) = _rays(F, *MAIN, 4096, 48, seed=11, concentrated=concentrated)
    _full_case(F, f"main 4096x48 {'concentrated' if concentrated else 'uniform'}", case, _denc(case, 1),
               perm=_permute_rays(F, o, d, t, *MAIN), expect_overflow=True)


@pytest.mark.parametrize("max_res,S", [(256, 256), (128, 256), (256, 96)])
def test_proposal_tables(F, max_res, S):
    """The proposal grids (5 levels, T = 2^17): 256 samples per ray on the max_res 256 grid mixes run-merged and fine
    levels; the other two are all-run (the benchmark's pairing)."""
    grid = (5, 16, max_res, 17)
    case, (o, d, t) = _rays(F, *grid, 4096, S, seed=12)
    assert any(case.coarse)
    assert all(case.coarse) != (max_res == 256 and S == 256), case.coarse
    _full_case(F, f"proposal max_res {max_res}, 4096x{S}", case, _denc(case, 2, zero_frac=0.5),
               perm=_permute_rays(F, o, d, t, *grid))


@pytest.mark.parametrize("grid,S", [(MAIN, 97), (MAIN, 193), ((5, 16, 256, 17), 97), ((5, 16, 256, 17), 193)])
def test_runs_straddling_rays(F, grid, S):
    """257 rays of 97 / 193 samples: a run of kRunLen consecutive samples crosses from one ray into the next."""
    case, _ = _rays(F, *grid, 257, S, seed=13)
    assert any(case.coarse)
    _full_case(F, f"L={grid[0]} max_res {grid[2]}, 257x{S}", case, _denc(case, 3))


@pytest.mark.parametrize("n", [200, 4096])
def test_degenerate_batch(F, n):
    """Every ray identical: a handful of tiles receive everything. 200 rays: the dynamic areas overflow into the spill
    list, which pass 2 folds (exact, ordered). 4096 rays: beyond kSpillFold spills the tail goes in as float atomics
    (counted as unordered: allowed here only, with the fp32-summation bound); the write-only call's list holds the worst
    case (nothing lost)."""
    case, _ = _rays(F, *MAIN, n, 48, seed=14, same=True)
    denc = _denc(case, 4, zero_frac=0.0)
    _full_case(F, f"degenerate {n}x48", case, denc, allow_unordered=n > 200)
    plan = _plan(case.scal, case.log2_T, case.M, True)
    spills = _fine_spills(case, denc, plan)[1]
    print(f"degenerate {n}x48: predicted spill records {spills} (fold limit {K_SPILL_FOLD})")
    assert (0 < spills <= K_SPILL_FOLD) if n == 200 else spills > K_SPILL_FOLD


def _max_levels(F):
    from nerfstudio_amd import _native as N

    for L in range(N.MAX_LEVELS, 0, -1):
        if int(N.load().nsamd_hashgrid_encode_bwd_workspace(F.HashGridSpec(L, 16, 512, 19).native(), 50000, 1)) > 0:
            return L
    raise AssertionError("no level count accepted")


@pytest.mark.parametrize("which", ["dense_T4096", "one_level", "max_levels"])
@pytest.mark.parametrize("xform", ["none", "aabb"])
def test_small_grids_positions(F, which, xform):
    """Positions mode (fine route only), point-major gradient: a 2^12 table whose levels fill it, one level, the largest
    level count the workspace query accepts; XFORM_NONE with points outside [0,1] (negative corners, pairs straddling
    tiles) and XFORM_AABB with points outside the box (selector-masked: scattered at the origin's cell)."""
    from nerfstudio_amd import _native as N

    grid = {"dense_T4096": (5, 16, 128, 12), "one_level": (1, 16, 16, 19), "max_levels": (_max_levels(F), 16, 512, 19)}[which]
    tf = N.XFORM_NONE if xform == "none" else N.XFORM_AABB
    case = _positions(F, *grid, 50000, seed=15, transform=tf, outside=0.25, outside_frac=0.02)
    _full_case(F, f"{which} L={grid[0]} T=2^{grid[3]} {xform}", case, _denc(case, 5), perm=_permute_points(F))


@pytest.mark.parametrize("M", [1, 63, 65, K_FINE_THREADS - 1, K_FINE_THREADS + 1, 65535, 65537])
def test_point_count_edges(F, M):
    """M around one point, a wavefront, one fine-route workgroup and a 64 k workspace bucket, on the main grid."""
    from nerfstudio_amd import _native as N

    case = _positions(F, *MAIN, M, seed=16 + M, transform=N.XFORM_NONE)
    _full_case(F, f"main, M = {M}", case, _denc(case, 6, zero_frac=0.0), perm=_permute_points(F) if M > 64 else None)


def test_zero_points(F):
    """M = 0: the write-only call writes zeros everywhere, the accumulating call changes nothing."""
    from nerfstudio_amd import _native as N

    case = _positions(F, *MAIN, 1, seed=17, transform=N.XFORM_NONE)
    case.M = 0
    lib = N.load()
    out = torch.full((case.L * case.T, 2), float("nan"), device="cuda")
    dummy = torch.zeros(1, device="cuda")
    N.check(lib.nsamd_hashgrid_encode_bwd_set(case.pts, 0, case.transform, case.box, N.ptr(dummy), case.spec.native(),
                                              N.ptr(dummy), 1, 1, N.ptr(out), None, None, 0, N.stream()), "M = 0, set")
    assert bool((out.view(torch.int32) == 0).all())
    acc = torch.randn(case.L * case.T, 2, device="cuda")
    before = acc.clone()
    N.check(lib.nsamd_hashgrid_encode_bwd(case.pts, 0, case.transform, case.box, N.ptr(dummy), case.spec.native(),
                                          N.ptr(dummy), 1, 1, N.ptr(acc), None, None, 0, N.stream()), "M = 0")
    assert torch.equal(acc, before)


def test_cached_workspace_serves_its_bucket(F):
    """One `_scatter_workspace` for a bucket of 64 k points, used first for the bucket's largest M and then for smaller
    ones (the ngp path changes M every step): each call equals a fresh workspace's result bit for bit and meets the
    bound."""
    from nerfstudio_amd import _native as N

    F._SCATTER_WS.clear()
    case, _ = _rays(F, *MAIN, 4096, 48, seed=18)
    denc = _denc(case, 7)
    ws, ws_n = F._scatter_workspace(case.spec, torch.device("cuda"), case.M, write_only=True)
    for n in (4096, 3001, 2731):  # 196 608, 144 048, 131 088 points: one bucket
        sub, _ = _rays(F, *MAIN, 4096, 48, seed=18)
        keep = tuple(k[:n].contiguous() for k in sub.keep)
        sub.pts, sub.keep, sub.M = N.make_points(None, *keep, 48), keep, n * 48
        sub.x, d_sub = case.x[: n * 48], denc[: n * 48]
        dd, sp, sk = _device_denc(sub, d_sub)
        got = torch.full((sub.L * sub.T, 2), float("nan"), device="cuda")
        _scatter(F, sub, dd, sp, sk, got, True, ws)
        fresh = torch.full_like(got, float("nan"))
        _scatter(F, sub, dd, sp, sk, fresh, True, _workspace(F, sub, True))
        assert torch.equal(got.view(torch.int32), fresh.view(torch.int32)), f"cached workspace at M = {sub.M}"
        ref, ab, cnt = orc.hashgrid_scatter64(sub.x, d_sub, torch.tensor(sub.scal), sub.T)
        steps, c1 = _level_steps(sub, d_sub)
        worst = _check(f"cached workspace, M = {sub.M}", sub, got, ref, ab, cnt, steps, c1)
        print(f"\ncached workspace (bucket of {ws_n} words), M = {sub.M}: same bits as a fresh one, worst err/bound {worst:.3f}")
    ev = _events(F, ws)
    assert ev[1] == 0 and ev[2] == 0, ev


def test_magnitudes_across_levels(F):
    """denc scaled per level to 1e-30, 1e-6, 1, 1e20, all zero, and entirely below FLT_MIN, in one call."""
    from nerfstudio_amd import _native as N

    case = _positions(F, *MAIN, 60000, seed=19, transform=N.XFORM_NONE)
    scales = ([1e-30, 1e-6, 1.0, 1e20, 0.0, 1e-39] * 3)[: case.L]  # 1e-39 x (|N(0,1)| <= 6): below FLT_MIN throughout
    denc = _denc(case, 8, zero_frac=0.0, scales=scales)
    g = denc.view(case.M, case.L, 2)
    assert bool((g[:, 5].abs() < 2.0**-126).all()) and bool((g[:, 5] != 0).any()) and bool((g[:, 4] == 0).all())
    _full_case(F, "magnitudes 1e-30 .. 1e20 by level", case, denc)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_gradient_poisons_its_level(F, bad):
    """One non-finite value on one level: that level comes back NaN (scatter.h), every other level meets the bound."""
    from nerfstudio_amd import _native as N

    case = _positions(F, *MAIN, 40000, seed=20, transform=N.XFORM_NONE)
    denc = _denc(case, 9)
    lvl = 7
    denc[1234, 2 * lvl + 1] = bad
    ref, ab, cnt = orc.hashgrid_scatter64(case.x, denc, torch.tensor(case.scal), case.T)
    steps, c1 = _level_steps(case, denc)
    dd, sp, sk = _device_denc(case, denc)
    others = [l for l in range(case.L) if l != lvl]
    for write_only in (True, False):
        prefill = None if write_only else torch.randn(case.L * case.T, 2)
        out = torch.full((case.L * case.T, 2), float("nan"), device="cuda") if write_only else prefill.cuda()
        _scatter(F, case, dd, sp, sk, out, write_only, _workspace(F, case, write_only))
        got = out.cpu().view(case.L, -1)
        assert bool(torch.isnan(got[lvl]).all()), "the poisoned level is not NaN throughout"
        assert not bool(torch.isfinite(ref.view(case.L, -1)[lvl]).all())
        worst = _check(f"{bad} on level {lvl}", case, out, ref, ab, cnt, steps, c1, prefill=prefill, levels=others)
        print(f"\n{bad} on level {lvl} ({'write-only' if write_only else 'accumulate'}): level NaN, others worst err/bound {worst:.3f}")


def test_exact_cancellation(F):
    """Pairs of identical points with opposite gradients: every entry is exactly 0.0."""
    from nerfstudio_amd import _native as N

    half = _positions(F, *MAIN, 30000, seed=21, transform=N.XFORM_NONE)
    raw = torch.cat([half.keep[0].cpu()] * 2).cuda()
    case = Case(F, *MAIN, 60000, N.make_points(raw), (raw,), torch.cat([half.x] * 2), N.XFORM_NONE, N.Aabb())
    g = _denc(half, 10, zero_frac=0.0)
    denc = torch.cat([g, -g])
    dd, sp, sk = _device_denc(case, denc)
    for write_only in (True, False):
        out = torch.full((case.L * case.T, 2), float("nan"), device="cuda") if write_only else torch.zeros(case.L * case.T, 2, device="cuda")
        _scatter(F, case, dd, sp, sk, out, write_only, _workspace(F, case, write_only))
        assert bool((out == 0).all()), "cancelling contributions left a residue"


def _gate(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("grid,S", [(MAIN, 48), ((5, 16, 256, 17), 96)])
def test_gated_calls(F, grid, S):
    """nsamd_hashgrid_encode_bwd_gated / _rays_gated: with the gate clear and denc all NaN nothing changes; with it raised
    and a ray mask 3 % / 40 % / 100 % live (the masked rays' denc NaN) the result is the float64 scatter of the live rays."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    case, _ = _rays(F, *grid, 4096, S, seed=22)
    n = 4096
    table = torch.randn(case.L * case.T, 2, device="cuda")
    nan_denc = torch.full((2 * case.L, case.M), float("nan"), device="cuda")
    prefill = torch.randn(case.L * case.T, 2)
    out = prefill.cuda()
    ws = _workspace(F, case, False)
    _scatter(F, case, nan_denc, 1, case.M, out, False, ws, gate=_gate(0))
    assert torch.equal(out.cpu().view(torch.int32), prefill.view(torch.int32)), "gate clear: gradient changed"
    d_o, d_d = torch.randn(n, 3, device="cuda"), torch.randn(n, 3, device="cuda")
    o0, d0 = d_o.clone(), d_d.clone()
    N.check(lib.nsamd_hashgrid_encode_bwd_rays_gated(case.pts, case.M, case.transform, case.box, N.ptr(table), case.spec.native(),
                                                     N.ptr(nan_denc), 1, case.M, N.ptr(d_o), N.ptr(d_d), 1,
                                                     C.cast(_gate(0).data_ptr(), C.c_void_p), None, N.stream()), "rays gated")
    assert torch.equal(d_o, o0) and torch.equal(d_d, d0), "gate clear: ray gradients changed"
    _check_features(F, case)
    denc = _denc(case, 11)
    for live_frac in (0.03, 0.4, 1.0):
        mask = torch.rand(n, generator=torch.Generator().manual_seed(int(live_frac * 100))) < live_frac
        live = mask.repeat_interleave(S)
        dm = torch.where(live[:, None], denc, torch.full_like(denc, float("nan")))
        d_live = torch.where(live[:, None], denc, torch.zeros_like(denc))
        ref, ab, cnt = orc.hashgrid_scatter64(case.x, d_live, torch.tensor(case.scal), case.T)
        steps, c1 = _level_steps(case, d_live)
        out = prefill.cuda()
        gate = _gate(1)
        _scatter(F, case, dm.t().contiguous().cuda(), 1, case.M, out, False, ws, gate=gate, mask=mask.to(torch.uint8).cuda())
        worst = _check(f"gated, {live_frac:.0%} live", case, out, ref, ab, cnt, steps, c1, prefill=prefill)
        ev = _events(F, ws)
        assert ev[1] == 0 and ev[2] == 0, ev
        print(f"\ngated L={case.L} 4096x{S}, {int(mask.sum())} live rays: worst err/bound {worst:.3f}, events {ev}")


# ---------------------------------------------------------------- fused producer ----------------------------------------
@pytest.mark.parametrize("init", ["default", "n(0,0.3)"])
def test_fused_producer_route_against_float64(F, init):
    """nsamd_field_mlp_bwd_scatter at the benchmark's size (the setup of
    test_backward_that_emits_the_scatter_records_equals_the_two_launches, keep_denc): its written table gradient against the
    float64 scatter of the `f_denc` it stores, with the producer plan's headroom."""
    from test_gpu_kernels import _hip_model

    import bench
    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.train_step import NerfactoTrainStep

    cfg = orc.NerfactoCfg()
    params = orc.init_params(cfg, seed=0, table_std=None if init == "default" else 0.3)
    F._SCATTER_WS.clear()
    dev = torch.device("cuda")
    model = _hip_model(cfg, params)
    arena = ParamArena(model.get_param_groups_ordered(), lr=1e-2, eps=1e-15)
    n = bench.RAYS_PER_GPU
    o, d, cam, tgt = (torch.from_numpy(a).to(dev) for a in bench.synthetic_rays(1003))
    r = NerfactoTrainStep(model, n, dev)
    r.side_stream = None
    r.keep_denc = True
    r.fuse_route = True
    r.set_batch(o, d, cam[:, 0], tgt)
    rs = np.random.RandomState(4)
    r.jitter.copy_(torch.from_numpy(rs.uniform(0, 1, (3, n)).astype(np.float32)))
    r.forward_and_losses(False, draw_jitter=False)
    table = model.field.mlp_base.encoding.hash_table
    spec = model.field.mlp_base.encoding.spec
    off = next(o_ for p_, o_ in zip(arena.params, arena.offsets) if p_ is table)
    arena.zero_grad(["fields"])
    arena.grad[off:off + table.numel()].fill_(float("nan"))
    r.backward_main()
    torch.cuda.synchronize()
    assert any(k[3] == "producer" for k in F._SCATTER_WS), "the fused entry point was not taken"
    L = r.n_prop
    S, M = r.counts[L], r.m_main
    x, _ = orc.normalise_positions(orc.sample_positions(r.origins.cpu(), r.directions.cpu(), r.t_bins[L].cpu()).reshape(-1, 3), True)
    scal = [float(s) for s in spec.scalings()]
    T = spec.table_size
    enc_ref = orc.hashgrid_encode(x, table.detach().cpu(), torch.tensor(scal), T)
    assert torch.equal(r.f_enc.t().cpu().view(torch.int32), enc_ref.view(torch.int32)), "forward features differ from the oracle's"
    denc = r.f_denc.t().contiguous().cpu()
    got = arena.grad[off:off + table.numel()].view(-1, 2)
    case = Case(F, spec.num_levels, spec.min_res, spec.max_res, spec.log2_hashmap_size, M, None, (), x, None, None, S=None)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pp = _producer_plan(scal, spec.log2_hashmap_size, M, cus)
    from nerfstudio_amd import _native as N

    state = C.c_int64(0)
    assert int(N.load().nsamd_field_mlp_bwd_scatter_workspace(spec.native(), M, C.byref(state))) == pp["words"], "producer plan"
    assert int(state.value) == pp["state"]
    ref, ab, cnt = orc.hashgrid_scatter64(x, denc, torch.tensor(scal), T)
    steps, c1 = _level_steps(case, denc, Q=pp["caps"])
    worst = _check(f"fused producer [{init}]", case, got, ref, ab, cnt, steps, c1)
    evs = {k[3]: F.scatter_events(ws) for k, ws in F._SCATTER_WS.items()}
    for k, ev in evs.items():
        assert ev[1] == 0 and ev[2] == 0, (k, ev)
    print(f"\nfused producer [{init}], M = {M}: worst err/bound {worst:.3f}, events {evs}")


# ---------------------------------------------------------------- position and ray gradients ---------------------------
def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(1e-300, float(b.norm())))


def test_position_and_ray_gradients_vs_float64(F):
    """dpositions of nsamd_hashgrid_encode_bwd and d_origins / d_directions of nsamd_hashgrid_encode_bwd_rays (ungated and
    gated) at the main grid's bench shape, against float64 evaluations of the same expression from the fp32 cells and
    weights: the kernel's relative L2 error at most 3x that of torch's fp32 CPU evaluation (as the field MLP backward test)."""
    from nerfstudio_amd import _native as N

    lib = N.load()
    case, (o, d, t) = _rays(F, *MAIN, 4096, 48, seed=23)
    n, S = 4096, 48
    _check_features(F, case)
    g = torch.Generator().manual_seed(9)
    table = torch.randn(case.L * case.T, 2, generator=g) * 0.3
    denc = _denc(case, 12, zero_frac=0.0)
    tab_d, (dd, sp, sk) = table.cuda(), _device_denc(case, denc)
    dpos = torch.empty(case.M, 3, device="cuda")
    N.check(lib.nsamd_hashgrid_encode_bwd(case.pts, case.M, case.transform, case.box, N.ptr(tab_d), case.spec.native(),
                                          N.ptr(dd), sp, sk, None, N.ptr(dpos), None, 0, N.stream()), "dpositions")
    raw = orc.sample_positions(o, d, t).reshape(-1, 3)
    r64 = _position_grad(raw, table, case.scal, case.T, denc, torch.float64)
    r32 = _position_grad(raw, table, case.scal, case.T, denc, torch.float32)
    half64 = ((t[:, :-1] + t[:, 1:]) / 2).double()
    rays = {}
    for name, ref in (("64", r64), ("32", r32)):
        p = ref.view(n, S, 3)
        hf = half64.to(ref.dtype)[..., None]
        rays[name] = (p.sum(1), (p * hf).sum(1))
    d_o, d_d = torch.empty(n, 3, device="cuda"), torch.empty(n, 3, device="cuda")
    N.check(lib.nsamd_hashgrid_encode_bwd_rays(case.pts, case.M, case.transform, case.box, N.ptr(tab_d), case.spec.native(),
                                               N.ptr(dd), sp, sk, N.ptr(d_o), N.ptr(d_d), 0, N.stream()), "rays")
    mask = torch.rand(n, generator=torch.Generator().manual_seed(2)) < 0.4
    go, gd = torch.full((n, 3), float("nan"), device="cuda"), torch.full((n, 3), float("nan"), device="cuda")
    N.check(lib.nsamd_hashgrid_encode_bwd_rays_gated(case.pts, case.M, case.transform, case.box, N.ptr(tab_d), case.spec.native(),
                                                     N.ptr(dd), sp, sk, N.ptr(go), N.ptr(gd), 0,
                                                     C.cast(_gate(1).data_ptr(), C.c_void_p), N.ptr(mask.to(torch.uint8).cuda()),
                                                     N.stream()), "rays gated")
    mk = mask.cuda()
    assert torch.equal(go[mk], d_o[mk]) and torch.equal(gd[mk], d_d[mk]), "gated ray gradients differ from the ungated"
    assert bool((go[~mk] == 0).all()) and bool((gd[~mk] == 0).all()), "masked rays' gradients are not zero"
    rows, bad = [], []
    for name, got, e64, e32 in (("dpositions", dpos, r64, r32), ("d_origins", d_o, rays["64"][0], rays["32"][0]),
                                ("d_directions", d_d, rays["64"][1], rays["32"][1])):
        e_gpu, e_cpu = _rel_l2(got.cpu(), e64), _rel_l2(e32, e64)
        rows.append(f"  {name}: gpu-f64 {e_gpu:.2e}  cpu32-f64 {e_cpu:.2e}")
        if not e_gpu <= max(3.0 * e_cpu, 2e-6):
            bad.append(name)
    print("\nposition / ray gradients at 4096 x 48 against float64:\n" + "\n".join(rows))
    assert not bad, f"{bad}\n" + "\n".join(rows)
