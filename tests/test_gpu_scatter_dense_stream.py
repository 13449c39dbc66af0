"""The table scatter's apply pass (csrc/scatter.hip, scatter_apply_body) BIT FOR BIT against a CPU restatement of its
fixed-point sum. The pass takes the static segments of a tile as one dense record stream per wave (prefix sum of the segment
counts, 64 records per batch whatever segment they sit in), then the dynamic area and the folded spill list; which lane adds
which record must not reach the result.

The reference is exact, not a bound: every record share is the fp32 product ((g * bz) * by) * bx of scatter.h / common.h
(pair records carry (g * bz) * by and pass 2 applies the x factor: the same three roundings), a run record of the coarse
route is the fp32 sum, in sample order, of up to kRunLen such products; each share enters the sum as trunc(v * 2^k),
k = 188 - headroom - e_max (scatter.h: e_max the exponent field of the level's largest |gradient|, + 2 on run levels;
headroom = 2 + bit_length(Q + kSpillFold - 1) from the level's queue capacity), the int64 sum is converted once
(double, * 2^-k, float). Integer sums have no order, so whatever route a record took — static segment, dynamic area, spill
fold — the bits are these. Gradients are drawn so that no product is a denormal (a flushed and a kept denormal both
truncate to 0 at these k, the restatement does not depend on it either way).

Shapes are the smallest that reach each branch of the stream; the test asserts from the restated segment counts that the
branch is reached (a stream that ends inside a batch, streams shorter than a batch, one record per wave, a segment longer
than 64 and than 128 records, static segments followed by the dynamic area and the spill fold).
"""
import numpy as np
import pytest
import torch

from oracle import nerfacto_oracle as orc
from test_gpu_table_scatter import (K_FINE_THREADS, K_RUN_LEN, K_SPILL_FOLD, MAIN, NAN_BITS, Case, _check_features, _denc,
                                    _device_denc, _events, _fine_spills, _headroom, _plan, _producer_plan,
                                    _rays, _scatter, _workspace)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


def _cells(x, scale):
    """locate_cell (common.h) on fp32 grid inputs: floor / ceil corners and the fp32 weights toward the ceil corner"""
    scaled = x * scale
    lo = torch.floor(scaled)
    return lo.numpy().astype(np.int32), torch.ceil(scaled).numpy().astype(np.int32), scaled - lo


def _corner_terms(lo, hi, w, g, T):
    """-> [(flat table index [n], share [n, 2] fp32)] x 8: corner_share(c, k, g) = ((g * bz) * by) * bx, three fp32 roundings"""
    om = 1.0 - w
    out = []
    for k in range(8):
        cx, cy, cz = bool(k & 1), bool(k & 2), bool(k & 4)
        idx = orc.hash_corner_index((hi if cx else lo)[:, 0], (hi if cy else lo)[:, 1], (hi if cz else lo)[:, 2], 0, T)
        v = ((g * (w if cz else om)[:, 2:3]) * (w if cy else om)[:, 1:2]) * (w if cx else om)[:, 0:1]
        out.append((torch.from_numpy(idx), v))
    return out


def _fixed_sum(case, denc, caps):
    """-> (int64 fixed-point sums [L, T, 2], k per level (None: nothing recorded), non-finite flag per level)"""
    L, T, M = case.L, case.T, case.M
    acc = torch.zeros(L, T, 2, dtype=torch.int64)
    ks, bad = [], []
    g_all = denc.view(M, L, 2)
    for l in range(L):
        g = g_all[:, l].contiguous()
        bits = int(g.abs().max().view(torch.int32)) if M else 0
        if case.coarse[l] and bits:
            bits = min(bits + (2 << 23), NAN_BITS)  # a run record carries up to kRunLen gradients (scatter.hip)
        e = (bits >> 23) & 0xFF
        bad.append(e == 255)
        if e == 0 or e == 255:
            ks.append(None)
            continue
        k = 188 - _headroom(caps[l]) - e
        ks.append(k)
        lo, hi, w = _cells(case.x, case.scal[l])

        def add(idx, v):  # v fp32 [n, 2]: one truncation per share
            acc[l].index_add_(0, idx, torch.trunc(v.double() * 2.0**k).to(torch.int64))

        if not case.coarse[l]:
            live = (g != 0).any(dim=1)  # (a zero gradient emits nothing: it would add zero)
            for idx, v in _corner_terms(lo[live.numpy()], hi[live.numpy()], w[live], g[live], T):
                add(idx, v)
            continue
        # the run route (scatter_route_runs_body): a thread walks kRunLen consecutive samples; live samples that stay in one
        # cell merge (fp32 per-corner sums in sample order, indices of the run's first cell); zero-gradient samples are skipped
        n = -(-M // K_RUN_LEN)
        pad = n * K_RUN_LEN - M
        P = lambda a, fill=0: torch.cat([a, torch.full((pad, *a.shape[1:]), fill, dtype=a.dtype)]).view(n, K_RUN_LEN, *a.shape[1:])
        lo_t, hi_t = P(torch.from_numpy(lo)), P(torch.from_numpy(hi))
        terms = _corner_terms(lo, hi, w, g, T)
        share = P(torch.stack([v for _, v in terms], dim=1))      # [n, 4, 8, 2]
        index = P(torch.stack([i for i, _ in terms], dim=1))      # [n, 4, 8]
        live = P((g != 0).any(dim=1), False)
        has = torch.zeros(n, dtype=torch.bool)
        cur_lo, cur_hi = torch.zeros(n, 3, dtype=torch.int32), torch.zeros(n, 3, dtype=torch.int32)
        cur_idx = torch.zeros(n, 8, dtype=torch.int64)
        run = torch.zeros(n, 8, 2)

        def flush(m):
            if bool(m.any()):
                add(cur_idx[m].reshape(-1), run[m].reshape(-1, 2))

        for s in range(K_RUN_LEN):
            lv = live[:, s]
            same = has & lv & (lo_t[:, s] == cur_lo).all(dim=1) & (hi_t[:, s] == cur_hi).all(dim=1)
            flush(has & lv & ~same)
            start = lv & ~same
            run[start], cur_idx[start] = share[start, s], index[start, s]
            cur_lo[start], cur_hi[start] = lo_t[start, s], hi_t[start, s]
            run[same] = run[same] + share[same, s]
            has = has | lv
        flush(has)
    return acc, ks, bad


def _expected(case, denc, caps, prefill=None):
    """the gradient the apply pass must leave: write-only (prefill None) or added to `prefill`"""
    acc, ks, bad = _fixed_sum(case, denc, caps)
    out = torch.zeros(case.L, case.T, 2) if prefill is None else prefill.view(case.L, case.T, 2).clone()
    for l in range(case.L):
        if bad[l]:
            out[l] = float("nan")
        elif ks[l] is not None:
            v = (acc[l].double() * 2.0 ** -ks[l]).float()
            out[l] = v if prefill is None else out[l] + v
    return out.view(-1, 2)


def _segment_counts(case, denc, plan):
    """records per (fine level, pass-1 workgroup = static segment, tile), before the clip at seg_cap: [segs, bins] per level"""
    sl, lb, segs = plan["sl"], plan["lb"], plan["segs"]
    seg = torch.arange(case.M) // K_FINE_THREADS
    out = {}
    for l in range(case.L):
        if case.coarse[l]:
            continue
        live = (denc.view(case.M, case.L, 2)[:, l] != 0).any(dim=1).numpy()
        lo, hi, _ = _cells(case.x, case.scal[l])
        per = torch.zeros(segs << lb, dtype=torch.int64)
        for q in range(4):
            iy, iz = (hi if q & 1 else lo)[live, 1], (hi if q & 2 else lo)[live, 2]
            ia = torch.from_numpy(orc.hash_corner_index(lo[live, 0], iy, iz, 0, case.T))
            per += torch.bincount(seg[torch.from_numpy(live)] * (1 << lb) + (ia >> sl), minlength=segs << lb)
        out[l] = per.view(segs, 1 << lb)
    return out


def _apply_waves(plan):
    return (1024 if plan["sl"] > 11 else 512 if plan["sl"] > 9 else 256) // 64  # apply_threads (scatter.hip)


def _stream_totals(counts, plan):
    """records per (wave, tile) stream of the apply pass: wave w owns segments w, w + nw, ... (clipped at seg_cap)"""
    nw = _apply_waves(plan)
    c = counts.clamp(max=plan["C"])
    return torch.stack([c[w::nw].sum(dim=0) if w < c.shape[0] else torch.zeros(c.shape[1], dtype=torch.int64) for w in range(nw)])


def _bit_equal_both_ways(F, name, case, denc, allow_spill=True):
    """write-only into a NaN-filled buffer and accumulating into a random prefill, fresh workspaces: the restatement's bits"""
    _check_features(F, case)
    dd, sp, sk = _device_denc(case, denc)
    caps = _plan(case.scal, case.log2_T, case.M, True)["caps"]
    out = torch.full((case.L * case.T, 2), float("nan"), device="cuda")
    ws = _workspace(F, case, True)
    _scatter(F, case, dd, sp, sk, out, True, ws)
    want = _expected(case, denc, caps)
    diff = int((out.cpu().view(torch.int32) != want.view(torch.int32)).sum())
    assert diff == 0, f"{name}, write-only: {diff} entries differ from the fixed-point restatement"
    g = torch.Generator().manual_seed(3)
    prefill = torch.randn(case.L * case.T, 2, generator=g) * 10.0 ** (torch.rand(case.L * case.T, 2, generator=g) * 6 - 5)
    acc = prefill.cuda()
    ws_a = _workspace(F, case, False)
    _scatter(F, case, dd, sp, sk, acc, False, ws_a)
    want_a = _expected(case, denc, caps, prefill)
    diff = int((acc.cpu().view(torch.int32) != want_a.view(torch.int32)).sum())
    assert diff == 0, f"{name}, accumulating: {diff} entries differ from the fixed-point restatement"
    for ev in (_events(F, ws), _events(F, ws_a)):
        assert ev[1] == 0 and ev[2] == 0, f"{name}: records on the unordered path / lost {ev}"
        assert allow_spill or ev[0] == 0, f"{name}: spill records {ev}"
    return _events(F, ws)


def _uniform_points(F, grid, M, seed):
    from nerfstudio_amd import _native as N

    raw = torch.from_numpy(np.random.RandomState(seed).uniform(0.01, 0.99, (M, 3)).astype(np.float32))
    dev = raw.cuda()
    return Case(F, *grid, M, N.make_points(dev), (dev,), raw, N.XFORM_NONE, N.Aabb())


def _one_cell_points(F, grid, M, seed):
    """M points inside one cell of the grid's finest level (so of every level)"""
    from nerfstudio_amd import _native as N

    rs = np.random.RandomState(seed)
    res = float(grid[2])
    raw = torch.from_numpy(((np.array([[733.0, 1201.0, 389.0]]) % res + rs.uniform(0.05, 0.95, (M, 3))) / res).astype(np.float32))
    dev = raw.cuda()
    return Case(F, *grid, M, N.make_points(dev), (dev,), raw, N.XFORM_NONE, N.Aabb())


def test_main_table_streams(F):
    """4096 rays x 48 samples on the main grid (16 levels, T = 2^19): 192 static segments per tile, 12 per wave of the apply
    pass, half full on average; a stream is several full batches and ends inside one."""
    case, _ = _rays(F, *MAIN, 4096, 48, seed=31)
    denc = _denc(case, 21)
    plan = _plan(case.scal, case.log2_T, case.M, True)
    counts = _segment_counts(case, denc, plan)
    tot = torch.cat([_stream_totals(c, plan).reshape(-1) for c in counts.values()])
    assert plan["segs"] // _apply_waves(plan) == 12
    assert bool((tot % 64 != 0).any()) and bool((tot >= 256).any()), "streams of several full batches that end inside one"
    fill = torch.cat([c.reshape(-1).double() for c in counts.values()]).mean() / plan["C"]
    ev = _bit_equal_both_ways(F, "main 4096x48", case, denc)
    print(f"\nmain 4096x48: mean segment fill {float(fill):.2f} of {plan['C']}, stream lengths {int(tot.min())} .. {int(tot.max())}, events {ev}")


@pytest.mark.parametrize("M", [64, 1])
def test_sparse_and_single(F, M):
    """64 points: most of a tile's streams are empty, none fills a batch. One point: at most one record per wave."""
    case = _uniform_points(F, MAIN, M, seed=32 + M)
    denc = _denc(case, 22, zero_frac=0.0)
    plan = _plan(case.scal, case.log2_T, case.M, True)
    tot = torch.cat([_stream_totals(c, plan).reshape(-1) for c in _segment_counts(case, denc, plan).values()])
    assert int(tot.max()) < 64 and bool((tot == 0).any()) and bool((tot > 0).any())
    if M == 1:
        assert int(tot.sum()) == 4 * case.L
    _bit_equal_both_ways(F, f"main grid, M = {M}", case, denc, allow_spill=False)


def test_proposal_shape_run_route(F):
    """A proposal level's shape (5 levels, T = 2^17, 96 samples per ray): every level through the run route, so the tiles have
    no static segments and the apply pass is its dynamic area alone (the body scatter_apply_pair_kernel runs as well)."""
    grid = (5, 16, 256, 17)
    case, _ = _rays(F, *grid, 64, 96, seed=33)
    assert all(case.coarse)
    _bit_equal_both_ways(F, "proposal 64x96", case, _denc(case, 23, zero_frac=0.5))


def test_proposal_levels_pair_launch(F):
    """nsamd_proposal_levels_bwd on the two proposal levels of nerfacto (5 levels, T = 2^17; 256 samples per ray on the
    max_res 128 grid, 96 on the max_res 256 grid): both levels go through the run route, so their route, apply and finish
    passes are ONE launch each — scatter_apply_pair_kernel, whose grid is the larger of the two calls' —, gated, with ray
    masks (a third of the rays carries gradient, other rays per level). Both table gradients bit for bit the restatement on
    the feature gradients the chain stored. The entry point only accumulates (a gated call never overwrites: scatter.hip),
    so the two variants are a zero and a random gradient to add to."""
    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.train_step import NerfactoTrainStep
    from test_gpu_kernels import _hip_model

    cfg = orc.NerfactoCfg()
    assert [(g.num_levels, g.max_res, g.log2_hashmap_size) for g in cfg.prop_grids] == [(5, 128, 17), (5, 256, 17)]
    n = 300
    o, d, cam, tgt = orc.synthetic_rays(n, cfg.num_images, seed=11)
    F._SCATTER_WS.clear()
    model = _hip_model(cfg, orc.init_params(cfg, seed=7, table_std=0.4))
    arena = ParamArena(model.get_param_groups_ordered())
    step = NerfactoTrainStep(model, n, torch.device("cuda"))
    assert step.gate_proposals and step.merge_prop_levels and step.cam_opt is None and list(step.counts[:2]) == [256, 96]
    step.side_stream = None
    step.set_batch(o.cuda(), d.cuda(), cam.cuda(), tgt.cuda())
    step.jitter.copy_(torch.from_numpy(np.random.RandomState(4).uniform(0, 1, (3, n)).astype(np.float32)).cuda())
    step.anneal_dev.fill_(1.0)
    arena.zero_grad()
    step.forward_and_losses(True, draw_jitter=False)
    assert step._proposal_level_structs([0, 1]) is not None, "a level without a binned-scatter workspace: no merged launch"
    g = torch.Generator(device="cuda").manual_seed(5)
    for lvl in range(2):
        dw = torch.randn(n, step.counts[lvl], device="cuda", generator=g) * 1e-3
        keep = torch.rand(n, device="cuda", generator=g) < 0.33
        step.dw_prop[lvl].copy_((dw * keep[:, None]).view_as(step.dw_prop[lvl]))
    tables = [step.props[lvl].encoding.hash_table for lvl in range(2)]
    cases = []
    for lvl in range(2):
        spec = step.props[lvl].encoding.spec
        x, _ = orc.normalise_positions(orc.sample_positions(step.origins.cpu(), step.directions.cpu(), step.t_bins[lvl].cpu()).reshape(-1, 3), True)
        scal = [float(v) for v in spec.scalings()]
        enc_ref = orc.hashgrid_encode(x, tables[lvl].detach().cpu(), torch.tensor(scal), spec.table_size)
        assert torch.equal(step.p_enc[lvl].t().cpu().view(torch.int32), enc_ref.view(torch.int32)), "forward features differ from the oracle's"
        M = n * step.counts[lvl]
        case = Case(F, spec.num_levels, spec.min_res, spec.max_res, spec.log2_hashmap_size, M, None, (), x.contiguous(), None, None,
                    S=step.counts[lvl])
        assert all(case.coarse)
        cases.append((case, _plan(case.scal, case.log2_T, M, False)["caps"]))
    gen = torch.Generator().manual_seed(3)
    for variant in ("zero", "random"):
        prefill = []
        for lvl in range(2):
            tg = step._grad(tables[lvl])
            pf = torch.zeros(tg.numel()) if variant == "zero" else \
                torch.randn(tg.numel(), generator=gen) * 10.0 ** (torch.rand(tg.numel(), generator=gen) * 6 - 5)
            tg.copy_(pf.view_as(tg))
            prefill.append(pf.view(-1, 2))
            step.p_denc[lvl].zero_()  # (the chain does not write the rows of rays without gradient)
        if step.gates_precleared:
            step.prop_gates.zero_()
        step.backward_proposals()
        torch.cuda.synchronize()
        for lvl in range(2):
            case, caps = cases[lvl]
            assert 0 < int(step.prop_ray_masks[lvl].sum()) < n
            denc = step.p_denc[lvl].t().contiguous().cpu()
            assert bool((denc != 0).any())
            want = _expected(case, denc, caps, prefill[lvl])
            got = step._grad(tables[lvl]).view(-1, 2).cpu()
            diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
            assert diff == 0, f"pair launch, level {lvl}, {variant} gradient to add to: {diff} entries differ from the restatement"
    for k, ws in F._SCATTER_WS.items():
        ev = F.scatter_events(ws)
        assert ev[1] == 0 and ev[2] == 0, (k, ev)


def test_proposal_grid_static_segments(F):
    """The proposal grid in positions mode (fine route): tiles of 2^10 entries, 8 waves per apply workgroup, 3 segments."""
    grid = (5, 16, 256, 17)
    case = _uniform_points(F, grid, 3000, seed=34)
    denc = _denc(case, 24)
    plan = _plan(case.scal, case.log2_T, case.M, True)
    assert _apply_waves(plan) == 8 and plan["segs"] == 3
    _bit_equal_both_ways(F, "proposal grid, 3000 positions", case, denc)


def test_more_than_64_segments_per_wave(F):
    """258 pass-1 workgroups on a 2^12 table (tiles of 256 entries, 4 waves per apply workgroup): two waves own 65 segments,
    so their counts take a second round of the stream (a wave holds 64 counts at a time)."""
    grid = (5, 16, 128, 12)
    case = _uniform_points(F, grid, 257 * K_FINE_THREADS + 1, seed=38)
    plan = _plan(case.scal, case.log2_T, case.M, True)
    assert _apply_waves(plan) == 4 and plan["segs"] == 258
    _bit_equal_both_ways(F, "258 segments, 4 waves", case, _denc(case, 28))


@pytest.mark.parametrize("M", [100, 200])
def test_hot_segment(F, M):
    """All points in one cell, one pass-1 workgroup: a static segment of more than 64 (M = 100) and of more than 128
    (M = 200) records — a segment that spans batches. (16 levels on a 2^15 table: 8 tiles per level, segments of 1024.)"""
    grid = (16, 16, 2048, 15)
    case = _one_cell_points(F, grid, M, seed=35)
    denc = _denc(case, 25, zero_frac=0.0)
    plan = _plan(case.scal, case.log2_T, case.M, True)
    counts = _segment_counts(case, denc, plan)
    assert plan["segs"] == 1 and plan["C"] >= 4 * M
    lengths = torch.cat([c.reshape(-1) for c in counts.values()])
    assert bool(((lengths > 64) & (lengths <= 128)).any()) if M == 100 else bool((lengths > 128).any())
    _bit_equal_both_ways(F, f"hot segment, {M} points in one cell", case, denc, allow_spill=False)


def test_static_segment_then_dynamic_area(F):
    """220 points in one cell of the main grid: the cell's tiles fill their static segment (128 records) and put the rest in
    the dynamic area and, where that is full, the spill list the apply pass folds: a dense stream followed by both."""
    case = _one_cell_points(F, MAIN, 220, seed=36)
    denc = _denc(case, 26, zero_frac=0.0)
    plan = _plan(case.scal, case.log2_T, case.M, True)
    overflow, spills = _fine_spills(case, denc, plan)
    assert plan["C"] == 128 and overflow and 0 < spills <= K_SPILL_FOLD
    ev = _bit_equal_both_ways(F, "220 points in one cell", case, denc)
    assert ev[0] == spills, (ev, spills)


def test_level_maximum_in_one_lane_and_nan(F):
    """The level's scale comes from its largest |gradient|: on level 3 it sits in the LAST point alone (2^20 above the
    rest), level 9 has one NaN. A maximum missed changes k and with it every bit of the level; the NaN level comes back NaN."""
    case = _uniform_points(F, MAIN, 2 * K_FINE_THREADS + 16, seed=37)
    denc = _denc(case, 27, zero_frac=0.0)
    denc[-1, 2 * 3] = denc[:, 6:8].abs().max() * 2.0**20
    denc[777, 2 * 9 + 1] = float("nan")
    _bit_equal_both_ways(F, "level maximum in the last point, NaN on level 9", case, denc)


def _producer_setup(F, n):
    """The first `n` rays of the benchmark's batch through the forward pass of the explicit schedule: the train step, where the
    main table's gradient sits in the arena, the oracle's grid inputs of the main field's samples and the producer plan."""
    import ctypes as C

    import bench
    from nerfstudio_amd import _native as N
    from nerfstudio_amd.arena import ParamArena
    from nerfstudio_amd.train_step import NerfactoTrainStep
    from test_gpu_kernels import _hip_model

    cfg = orc.NerfactoCfg()
    params = orc.init_params(cfg, seed=0, table_std=None)
    F._SCATTER_WS.clear()
    dev = torch.device("cuda")
    model = _hip_model(cfg, params)
    arena = ParamArena(model.get_param_groups_ordered(), lr=1e-2, eps=1e-15)
    o, d, cam, tgt = (torch.from_numpy(a[:n]).contiguous().to(dev) for a in bench.synthetic_rays(1003))
    r = NerfactoTrainStep(model, n, dev)
    r.side_stream = None
    r.keep_denc = True
    r.fuse_route = True
    r.set_batch(o, d, cam[:, 0], tgt)
    r.jitter.copy_(torch.from_numpy(np.random.RandomState(4).uniform(0, 1, (3, n)).astype(np.float32)))
    r.forward_and_losses(False, draw_jitter=False)
    table = model.field.mlp_base.encoding.hash_table
    spec = model.field.mlp_base.encoding.spec
    off = next(o_ for p_, o_ in zip(arena.params, arena.offsets) if p_ is table)
    M = r.m_main
    x, _ = orc.normalise_positions(orc.sample_positions(r.origins.cpu(), r.directions.cpu(), r.t_bins[r.n_prop].cpu()).reshape(-1, 3), True)
    scal = [float(s) for s in spec.scalings()]
    enc_ref = orc.hashgrid_encode(x, table.detach().cpu(), torch.tensor(scal), spec.table_size)
    assert torch.equal(r.f_enc.t().cpu().view(torch.int32), enc_ref.view(torch.int32)), "forward features differ from the oracle's"
    case = Case(F, spec.num_levels, spec.min_res, spec.max_res, spec.log2_hashmap_size, M, None, (), x.contiguous(), None, None)
    pp = _producer_plan(scal, spec.log2_hashmap_size, M, torch.cuda.get_device_properties(0).multi_processor_count)
    state = C.c_int64(0)
    assert int(N.load().nsamd_field_mlp_bwd_scatter_workspace(spec.native(), M, C.byref(state))) == pp["words"], "producer plan"
    grad = lambda: arena.grad[off:off + table.numel()]
    return dict(r=r, arena=arena, grad=grad, case=case, caps=pp["caps"], segs=pp["segs"])


@pytest.fixture(scope="module")
def producer(F):
    import bench

    return _producer_setup(F, bench.RAYS_PER_GPU)


def _producer_backward(F, P, upstream=None):
    """the main field's backward that emits the scatter's records, from the step's own upstream gradients or, after
    `upstream(d_density, d_rgb)` has changed them in place, from those -> (table gradient written, denc stored), on the host"""
    r = P["r"]
    P["arena"].zero_grad(["fields"])
    P["grad"]().fill_(float("nan"))  # write-only: every entry must be written
    r.backward_main(field=False)
    if upstream is not None:
        upstream(r.d_dens_main, r.d_rgb_s)
    r.backward_field_and_table()
    torch.cuda.synchronize()
    assert any(k[3] == "producer" for k in F._SCATTER_WS), "the fused entry point was not taken"
    for k, ws in F._SCATTER_WS.items():
        ev = F.scatter_events(ws)
        assert ev[1] == 0 and ev[2] == 0, (k, ev)
    return P["grad"]().view(-1, 2).cpu(), r.f_denc.t().contiguous().cpu()


def test_field_backward_producer_path(F, producer):
    """nsamd_field_mlp_bwd_scatter (the main field's backward emits the records, one static segment per persistent
    workgroup, ~48 records each at this size): the table gradient it writes, bit for bit the restatement on the `denc` it
    stores, with the producer plan's queue capacity. (The two-launch path has another capacity, so another k: it is not
    bit-comparable.)"""
    got, denc = _producer_backward(F, producer)
    want = _expected(producer["case"], denc, producer["caps"])
    diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    assert diff == 0, f"producer path: {diff} entries differ from the fixed-point restatement"


def test_field_backward_producer_path_one_tile_per_wave(F):
    """The same at 16 rays x 48 samples = 16 * 8 * 6 points: six workgroups with one tile per wave, so every record leaves
    in the flush after the tile loop and the running maxima are published without having been carried across tiles."""
    P = _producer_setup(F, 16)
    assert P["case"].M == 16 * 8 * 6 and P["segs"] == 6
    got, denc = _producer_backward(F, P)
    want = _expected(P["case"], denc, P["caps"])
    diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    assert diff == 0, f"producer path, one tile per wave: {diff} entries differ from the fixed-point restatement"


def test_producer_level_maximum_in_the_last_lane(F, producer):
    """Every upstream gradient but the LAST point's scaled by 2^-20: each level's largest |gradient| — the workgroups'
    running maxima, folded once per wave and level — sits in one lane of the last tile. A maximum missed leaves the level
    with a k that is too large: other bits everywhere."""
    def upstream(dd, drgb):
        dd[:-1] *= 2.0**-20
        drgb.view(-1, 3)[:-1] *= 2.0**-20

    got, denc = _producer_backward(F, producer, upstream)
    case = producer["case"]
    g = denc.view(case.M, case.L, 2).abs().amax(dim=2)
    alone = [l for l in range(case.L) if int(g[:, l].argmax()) == case.M - 1 and float(g[-1, l]) > 4.0 * float(g[:-1, l].max())]
    assert alone, "no level has its maximum in the last point alone"
    want = _expected(case, denc, producer["caps"])
    diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    assert diff == 0, f"maximum in the last lane (levels {alone}): {diff} entries differ from the fixed-point restatement"


def test_producer_nan_gradient(F, producer):
    """One NaN in the upstream density gradient: that point's feature gradients are NaN on every level, the levels' maxima
    are non-finite, the table gradient is NaN throughout."""
    def upstream(dd, drgb):
        dd[dd.numel() // 3] = float("nan")

    got, denc = _producer_backward(F, producer, upstream)
    case = producer["case"]
    assert bool(torch.isnan(denc.view(case.M, case.L, 2)).any(dim=2).any(dim=0).all()), "a level without a NaN"
    want = _expected(case, denc, producer["caps"])
    assert bool(torch.isnan(want).all()) and bool(torch.isnan(got).all()), "a NaN level did not come back NaN"
