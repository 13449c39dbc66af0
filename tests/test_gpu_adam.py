"""nsamd_adam_step (csrc/misc.hip adam_kernel) and the row exchange kernels nsamd_rows_gather / nsamd_rows_scatter through the
Python launch layer, BIT FOR BIT: Adam against tests/adam_reference.py (torch/optim/adam.py's operation order in IEEE fp32, held to
torch.optim.Adam on the CPU by tests/test_adam_reference_cpu.py), the row kernels against torch.index_select / index_copy_.
No tolerance anywhere: parameters and both moments carry the reference's bits after every step, NaN where it has NaN. That
asks of the device: fp32 denormals kept (not flushed), correctly rounded sqrtf and division, fmaf a single rounding, no
contraction elsewhere — the header's "same bits as torch.optim.Adam's".

Sizes, each at the smallest that makes it bite (adam_reference.TRIP = 786432 floats is what one trip of the grid-stride loop
covers: the launch is capped at 768 workgroups x 256 lanes x one float4):
* trips: 2 TRIP + 1027 (two full trips, a partial third, a tail of 3), TRIP + 4 (one float4 of work in the second trip), TRIP
  (exactly one trip, no tail);
* tails: n = 1 .. 7 (n < 4: the tail alone) and 1021 .. 1025 around one workgroup's 1024 floats; n = 0 writes nothing;
* zero-skip: groups of four with g = m = v = 0 (untouched bits of p, -0.0 and subnormals among them), one live lane of four,
  g = 0 with live moments, g = -0.0, a first gradient at step 3 — in the float4 body and in the tail, which has no skip;
* grad_scale 0.5, 1/3, 1/8 (only 1/3 is not a power of two: a scale applied at another place of the chain shows there);
* |g| from 1e-22 to 1e18 with eps 1e-15 and 1e-8; +-inf / NaN gradients; steps 1, 2, 1000, 100000 from given moments.
Every case runs twice: with the host-derived step scalars, and with hyper_dev = adam_hyper(step, lr) on the device beside
deliberately wrong step / lr arguments.

Every test prints the number of entries whose bits differ (the bound is zero) before it asserts."""
import numpy as np
import pytest
import torch

import adam_reference as ar

pytestmark = pytest.mark.gpu

INVALID = "invalid argument"


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native
    from nerfstudio_amd import functional as F

    _native.load()
    return F


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def differing(got, ref):
    """Number of entries of the device tensor whose bits differ from the fp32 array (NaN matches NaN)."""
    return int((~ar.same_bits(got.detach().cpu().numpy(), ref)).sum())


def run_device(F, case, hyper):
    """The case's steps on the device -> [(name, step, entries that differ)] against the reference, and the final tensors."""
    p, m, v = dev(case["p"]), dev(case["m"]), dev(case["v"])
    ref = ar.run(case)
    bad = []
    for k, g in enumerate(case["grads"]):
        step = case["step"] + k
        if hyper:
            hd = torch.tensor(ar.adam_hyper(step, case["lr"], ar.BETAS), dtype=torch.float32).cuda()
            F.adam_step(p, dev(g), m, v, step + 5, lr=123.0, betas=ar.BETAS, eps=case["eps"], grad_scale=case["grad_scale"], hyper_dev=hd)
        else:
            F.adam_step(p, dev(g), m, v, step, lr=case["lr"], betas=ar.BETAS, eps=case["eps"], grad_scale=case["grad_scale"])
        for name, t, r in (("p", p, ref[k][0]), ("exp_avg", m, ref[k][1]), ("exp_avg_sq", v, ref[k][2])):
            bad.append((name, step, differing(t, r)))
    return bad, (p, m, v), ref


@pytest.mark.parametrize("name", list(ar.CASES))
def test_adam_bits(F, name):
    case = ar.CASES[name]()
    for hyper in (False, True):
        bad, (p, m, v), ref = run_device(F, case, hyper)
        print(f"\n{name} ({'hyper_dev' if hyper else 'host scalars'}, n = {case['p'].size}): entries with other bits "
              + ", ".join(f"{a}@{s} {c}" for a, s, c in bad))
        assert all(c == 0 for _, _, c in bad), bad
        if "kinds" in case:  # lanes that never receive a gradient: the very bits they started with, moments +0
            for kind in "AD":
                lanes = case["kinds"] == ord(kind)
                assert differing(p[dev(lanes)], case["p"][lanes]) == 0
                assert differing(m[dev(lanes)], np.zeros(int(lanes.sum()), np.float32)) == 0
                assert differing(v[dev(lanes)], np.zeros(int(lanes.sum()), np.float32)) == 0
        if "special" in case:  # non-finite gradients: NaN exactly where the reference has it, the neighbours finite
            nan = np.isnan(ref[-1][0])
            assert nan[case["special"]].all() and nan.sum() == case["special"].size
            assert np.array_equal(torch.isnan(p).cpu().numpy(), nan)


def test_adam_empty_and_refusals(F):
    """n = 0 is accepted and writes nothing; step = 0 and a base pointer 4 bytes off the 16-byte alignment of the float4 accesses
    (each of the four arrays in turn) are refused with the invalid-argument status, every buffer still holding its sentinel."""
    n = 64
    bufs = [torch.full((n + 4,), float(k + 2), device="cuda") for k in range(4)]  # p, g, m, v
    before = [b.clone() for b in bufs]

    def unchanged():
        torch.cuda.synchronize()
        return all(torch.equal(b.view(torch.int32), c.view(torch.int32)) for b, c in zip(bufs, before))

    F.adam_step(bufs[0][:0], bufs[1][:0], bufs[2][:0], bufs[3][:0], 1, lr=1e-2)
    assert unchanged()
    with pytest.raises(RuntimeError, match=INVALID):
        F.adam_step(bufs[0][:n], bufs[1][:n], bufs[2][:n], bufs[3][:n], 0, lr=1e-2)
    assert unchanged()
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    for off in range(4):
        views = [b[1:1 + n] if k == off else b[:n] for k, b in enumerate(bufs)]
        with pytest.raises(RuntimeError, match=INVALID):
            F.adam_step(*views, 1, lr=1e-2)
        assert unchanged()
    F.adam_step(bufs[0][4:4 + n], bufs[1][4:4 + n], bufs[2][4:4 + n], bufs[3][4:4 + n], 1, lr=1e-2)  # 16 bytes off: accepted
    assert not unchanged() and all(torch.equal(b[:4], c[:4]) for b, c in zip(bufs, before))


def test_arena_groups_step_alone(F):
    """ParamArena on the device, two groups of a few small parameters: step(groups=[one]) leaves the other group's parameters,
    moments and step counter alone bit for bit; the zero padding between and after the parameters (to 64 floats per tensor, to
    53760 per group) stays zero through 3 steps; each group equals the reference run over its slice with its own step count."""
    from nerfstudio_amd.arena import ParamArena

    torch.manual_seed(3)
    shapes = {"a": [(5, 3), (7,), (130,)], "b": [(33, 2), (1,), (64,)]}
    params = {k: [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in v] for k, v in shapes.items()}
    arena = ParamArena(params, lr=1e-2)
    assert arena.eps == 1e-15 and set(arena.groups) == {"a", "b"}
    live = torch.zeros(arena.numel, dtype=torch.bool)
    for p, off in zip(arena.params, arena.offsets):
        live[off:off + p.numel()] = True
    live = live.numpy()
    state = {k: [t.cpu().numpy().copy() for t in (arena.flat, arena.exp_avg, arena.exp_avg_sq)] for k in "ab"}

    def snapshot():
        return [t.clone() for t in (arena.flat, arena.exp_avg, arena.exp_avg_sq)]

    gen = torch.Generator().manual_seed(4)
    bad = []
    for it, groups in enumerate((["a"], ["a", "b"], ["a"])):
        g = torch.zeros(arena.numel)
        g[torch.from_numpy(live)] = torch.randn(int(live.sum()), generator=gen)
        arena.grad.copy_(g.cuda())
        assert all(torch.equal(p.grad.reshape(-1), arena.grad[off:off + p.numel()]) for p, off in zip(arena.params, arena.offsets))
        before, counts = snapshot(), dict(arena.step_counts)
        arena.step(groups=groups)
        after = snapshot()
        for name, (a, b) in arena.groups.items():
            if name not in groups:
                assert arena.step_counts[name] == counts[name]
                assert all(torch.equal(x[a:b].view(torch.int32), y[a:b].view(torch.int32)) for x, y in zip(before, after))
                continue
            assert arena.step_counts[name] == counts[name] + 1
            p, m, v = (s[a:b] for s in state[name])
            new = ar.adam_step(p, g.numpy()[a:b], m, v, arena.step_counts[name], arena.lr, arena.eps)
            for s, x in zip(state[name], new):
                s[a:b] = x
            bad += [(name, it, differing(t[a:b], x)) for t, x in zip(after, new)]
        for t in after:
            assert not bool(t.cpu()[torch.from_numpy(~live)].view(torch.int32).any()), "the padding holds +0 for ever"
    print(f"\narena: entries with other bits (group, iteration, count) {bad}; step counts {arena.step_counts}")
    assert arena.step_counts == {"a": 3, "b": 1} and all(c == 0 for _, _, c in bad)


# ------------------------------------------------------------------------------------------------------ row exchange
def _rows_case(n, feat, seed):
    g = torch.Generator().manual_seed(seed)
    rows = 3 * n + 5
    index = torch.sort(torch.randperm(rows, generator=g)[:n]).values  # sorted, unique
    table = torch.randn(rows, feat, generator=g)
    return rows, index, table


@pytest.mark.parametrize("feat", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 1000])  # n feat around one workgroup's 256 lanes and around three
def test_rows_gather_scatter_bits(F, n, feat):
    from nerfstudio_amd import arena as A

    rows, index, table = _rows_case(n, feat, 100 * n + feat)
    idx = index.cuda()
    # gather == index_select; one sentinel row behind the packed buffer stays
    packed = torch.full((n + 1, feat), -7.0, device="cuda")
    A._rows_gather(table.cuda(), idx, packed[:n])
    want = torch.index_select(table, 0, index)
    d_gather = int((packed[:n].cpu().view(torch.int32) != want.view(torch.int32)).sum())
    # scatter == index_copy_ into a sentinel-filled table: the rows that are not indexed keep the sentinel
    src = torch.randn(n, feat, generator=torch.Generator().manual_seed(7))
    target = torch.full((rows, feat), -7.0, device="cuda")
    A._rows_scatter(target, idx, src.cuda())
    want_t = torch.full((rows, feat), -7.0).index_copy_(0, index, src)
    d_scatter = int((target.cpu().view(torch.int32) != want_t.view(torch.int32)).sum())
    # gather, wipe the indexed rows, scatter: the table is back
    t2 = table.cuda()
    buf = torch.empty(n, feat, device="cuda")
    A._rows_gather(t2, idx, buf)
    t2[idx] = float("nan")
    A._rows_scatter(t2, idx, buf)
    d_round = int((t2.cpu().view(torch.int32) != table.view(torch.int32)).sum())
    print(f"\nrows n = {n} feat = {feat}: entries with other bits gather {d_gather}, scatter {d_scatter}, round trip {d_round}")
    assert d_gather == 0 and bool((packed[n] == -7.0).all())
    assert d_scatter == 0 and d_round == 0
    # n = 0 writes nothing (and needs no pointer)
    A._rows_gather(t2, idx[:0], packed[:0])
    A._rows_scatter(target, idx[:0], src.cuda()[:0])
    torch.cuda.synchronize()
    assert bool((packed[n] == -7.0).all()) and torch.equal(target.cpu().view(torch.int32), want_t.view(torch.int32))


def test_register_compact_single_process_round_trip(F):
    """arena.ParamArena.register_compact on the device. In a single process all_reduce_group returns before it packs anything
    (no process group, or one rank: there is nobody to exchange with), so the gradient is unchanged bit for bit, no handle comes
    back and the compact buffer is not written. The pack / unpack the exchange would run — _rows_gather into the registered
    buffer, _rows_scatter back, as _GroupHandle does — then holds the indexed rows and restores the gradient."""
    from nerfstudio_amd import arena as A

    torch.manual_seed(5)
    table = torch.nn.Parameter(torch.randn(700, 2, device="cuda"))
    other = torch.nn.Parameter(torch.randn(37, device="cuda"))
    arena = A.ParamArena({"fields": [other, table]})
    prefix = 600
    index = torch.sort(torch.randperm(prefix)[:257]).values
    arena.register_compact(table, prefix, index)
    arena.grad.normal_()
    before = arena.grad.clone()
    assert arena.all_reduce_group("fields") is None
    (off, rows, feat, idx, buf), = arena._compact.values()
    assert (rows, feat) == (prefix, 2) and idx.is_cuda and torch.equal(idx.cpu(), index)
    assert torch.equal(arena.grad.view(torch.int32), before.view(torch.int32)) and not bool(buf.any())
    view = arena.grad[off:off + rows * feat].view(rows, feat)
    assert view.data_ptr() == table.grad.data_ptr()
    A._rows_gather(view, idx, buf)
    d_pack = int((buf.cpu().view(torch.int32) != table.grad.detach().cpu()[index].view(torch.int32)).sum())
    view[idx] = 0.0
    A._GroupHandle([], [(view, idx, buf)])  # the synchronous exchange's tail: scatter the rows back
    d_back = int((arena.grad.view(torch.int32) != before.view(torch.int32)).sum())
    print(f"\nregister_compact: entries with other bits packed {d_pack}, restored {d_back}")
    assert d_pack == 0 and d_back == 0
