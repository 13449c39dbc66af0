"""The sampler and compositing FORWARD kernels through the C ABI, entry by entry against float64 references of the same
operations on the kernels' own fp32 inputs (oracle: weights64, composite64, the extended composite_bwd64, mse64,
distance_scale64), and exactly against the fp32 oracle wherever the result is or decides an integer: csrc/sampler.hip and
csrc/render.hip through csrc/ray_bodies.h (piecewise_bins_body, weights_fwd_kernel, both instantiations of pdf_resample_body,
composite_fwd_body, the d_acc / d_depth branch of composite_bwd_body) and render.hip's own depth_clip_kernel, mse_loss_kernel
and distance_gradient_scale_kernel. The shapes are the ones at which the code takes another path: the 64-sample tiles and their
carries, the fixed prefetch depths of pdf_resample_body (new edges from 128 on, previous edges from 320 on, the fused kernel's
samples from 256 on) with their clamped indices, more than 256 workgroups with a depth output (the second trip of the clip
pass over the partials), a tail workgroup with idle waves, the grid cap of the MSE kernel, and the accepted limits.

Value checks are |got - ref64| <= bound per entry (float64_check.check_entries: the bound times 1 + 2^-6 for second-order terms
and the reference's own rounding, plus 2^-140 for results in the denormals). The bounds (tests/ray_forward_cases.py) come from
the operation sequences, with u = 2^-24:

* A wave sum over S samples is ceil(S / 64) additions per lane and 6 shuffle steps: n_add(S) u of the sum of |terms|. The
  double scans count as exact to S 2^-53 of their abs sums; expf within E_EXP (test_gpu_proposal_backward.test_expf_budget);
  division and sqrt are correctly rounded.
* weights: dd = fl(fl(t1 - t0) density): 2u relative. X (double scan of the fp32 dd, cast to float): dX <= 2u sum_{i<j} |dd_i| +
  u |X| + S 2^-53 sum |dd|. T = expf(-X): relative expm1(dX) + E_EXP. e = expf(-dd): relative expm1(2u |dd|) + E_EXP.
  alpha = 1 - e: absolute de + u |alpha|. w = fl(alpha T): dalpha T + |alpha| dT + u |w|.
* compositing: acc n_add(S) u of sum |w|; a colour channel (n_add(S) + 1) u of sum |w c| (one product each); the background
  blend c + bg (1 - acc): |bg| (dacc + u |1 - acc|) + u |bg (1 - acc)| + u |result|; the eval clamp is monotonic, so the
  clamped value lies between the clamps of ref -+ bound. The loss: d = pred - target one rounding, (dr^2 + dg^2) + db^2 three
  more: sum (2 |d| dd + dd^2) + 3u sq_err; d_rgb_out = fl(2 d grad_scale): 2 grad_scale dd + u.
* expected depth: num = sum w fl(mid): (n_add(S) + 2) u of sum |w mid|; den = fl(acc + 1e-10f): dacc + u |den|; the quotient
  dnum / den + |num| dden / den^2 + u |raw|; clip is 1-Lipschitz: + u |lo|. lo / hi themselves, the median index and the median
  depth are exact.
* compositing backward: d_weights = g.c - g.bg + d_acc + g_den + g_num mid + add: 12 u of the sum of |terms| (six products, the
  additions), + the errors of g_num = gd / den (relative dden / den + u) and g_den = -gd num / den^2 (|gd| (dnum / den^2 +
  2 |num| dden / den^3) + 4u |g_den|); d_rgb as in test_gpu_proposal_backward. A ray whose float64 raw depth lies within its
  bound of lo or hi may fall on either side of the clip mask: its d_depth is zeroed on both sides (at most 2 % of the rays;
  the count is printed).
* MSE: dpred = fl(fl(p - t) 2 grad_scale), two roundings; loss_sum (ceil(n / 16384) + 6 + 4 + 64) u of the sum of squares:
  the per-thread trips of the grid-stride loop, the wave steps, the four wave partials, the atomics of at most 64 workgroups.
  The ORDER of those atomics is not fixed, so two launches over more than one workgroup (n > 256) may differ by that
  reordering: the "same bits with the other output absent" check is on bits for n <= 256 and within 64 u of the sum beyond.
* distance scale: g fl(fl(mid)^2) has three roundings, but the midpoint's enters the square twice: (2 + 1 + 1) u = 4u (a
  count of the roundings alone, 3u, is exceeded by the correctly computed fp32 expression: 3.12u seen at one entry of 1776).

tests/test_ray_forward_reference_cpu.py pins the references to float64 autograd and shows, without a GPU, that these inputs
and bounds reject a model of each defect (a dropped tile carry, a lost min / max partial, `>` for `>=`, prefetch remainders
read wrong, a missing gradient term); the PDF and median seeds are shown there to be free of double-rounding ties.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ray_forward_cases as rc
from float64_check import U, check_entries, report
from oracle import nerfacto_oracle as orc
from oracle import vanilla_oracle as vo
from test_gpu_proposal_backward import weights_bound

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -2
NAN = float("nan")
BGV = (C.c_float * 3)(*rc.BG_COLOR)


@pytest.fixture(scope="module")
def N():
    from nerfstudio_amd import _native

    _native.load()
    return _native


def dev(x):
    return None if x is None else x.cuda().contiguous()


def nanfill(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -7, dtype=dtype, device="cuda")
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def exact(got, ref, what):
    got, ref = got.detach().cpu(), torch.as_tensor(ref)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if got.dtype.is_floating_point:
        same = (got == ref.to(got.dtype)) | (torch.isnan(got) & torch.isnan(ref))
    else:
        same = got.long() == ref.long()
    assert bool(same.all()), f"{what}: {int((~same).sum())}/{same.numel()} entries differ, first at {torch.nonzero(~same)[0].tolist()}"


def untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        assert bool(torch.isnan(t).all() if t.dtype.is_floating_point else (t == -7).all()), "an output was written"


# ---------------------------------------------------------------- nsamd_piecewise_bins ----------------------------------

@pytest.mark.parametrize("S", [1, 63, 64, 65, 200])
def test_piecewise_bins_exact(N, S):
    lib, st = N.load(), N.stream()
    g = torch.Generator().manual_seed(S)
    edges = dev(torch.linspace(0.0, 1.0, S + 1))
    for uniform in (False, True):
        for n in (1, 5, 0):
            nears = (2.0 if uniform else 0.05) + torch.rand(n, 1, generator=g)
            fars = (6.0 if uniform else 1000.0) + torch.rand(n, 1, generator=g)
            for jit in (None, torch.rand(n, 1, generator=g), torch.rand(n, S + 1, generator=g)):
                so, to = vo.uniform_bins(nears, fars, S, jit) if uniform else orc.piecewise_bins(nears, fars, S, jit)
                s, t = nanfill(n, S + 1), nanfill(n, S + 1)
                nd, fd, jd = dev(nears), dev(fars), dev(jit)
                per_edge = int(jit is not None and jit.shape[-1] == S + 1)
                N.check(lib.nsamd_piecewise_bins(N.ptr(nd), N.ptr(fd), N.ptr(edges), N.ptr(jd), per_edge, n, S, int(uniform),
                                                 N.ptr(s), N.ptr(t), st), "piecewise_bins")
                exact(s, so, f"s_bins uniform={uniform} n={n}")
                exact(t, to, f"t_bins uniform={uniform} n={n}")


# ---------------------------------------------------------------- nsamd_weights_fwd -------------------------------------

@pytest.mark.parametrize("S", rc.WEIGHT_S)
def test_weights_fwd_vs_float64(N, S):
    lib, st = N.load(), N.stream()
    t, dens, plain = rc.weights_case(S)
    n = t.shape[0]
    r = orc.weights64(t, dens)
    td, dd = dev(t), dev(dens)
    w = nanfill(n, S)
    N.check(lib.nsamd_weights_fwd(N.ptr(td), N.ptr(dd), n, S, N.ptr(w), st), "weights_fwd")
    worst = {}
    check_entries("weights", w[plain.cuda()], r["w"][plain], rc.weights_fwd_bound(r)[plain], worst)
    # the NaN and +Inf rays: finite, and zero exactly where the fp32 oracle is zero
    wo = orc.weights_from_density(t, dens)
    special = ~plain
    got = w.cpu()[special]
    assert bool(torch.isfinite(got).all()) and torch.equal(got != 0, wo[special] != 0)
    # what the case is there for: exact zeros, transmittance in the denormals and at zero behind it
    assert bool((w[0] == 0).all())
    if S >= 64:
        live = r["E"][1:4]
        assert bool(((live > 0) & (live < 2.0**-126)).any()) and bool((w[1:4].cpu() == 0).any())
    report(f"weights_fwd S={S}", worst)


# ---------------------------------------------------------------- nsamd_pdf_resample ------------------------------------

def _u_base(S):
    return torch.linspace(0.0, 1.0 - (1.0 / (S + 1)), steps=S + 1)


def _pdf_launch(N, c, S, uniform=False, include_original=False, want_inds=True, anneal=1.0):
    lib, st = N.load(), N.stream()
    n, S_prev = c["w"].shape
    edges = S + 1 + (S_prev + 1 if include_original else 0)
    s, t = nanfill(n, edges), nanfill(n, edges)
    inds = nanfill(n, S + 1, dtype=torch.int32) if want_inds else None
    jit = c["jitter"]
    per_edge = int(jit is not None and jit.shape[-1] == S + 1)
    keep = [dev(c["s0"]), dev(c["w"]), dev(_u_base(S)), dev(jit), dev(c["nears"]), dev(c["fars"])]
    rc_ = lib.nsamd_pdf_resample(N.ptr(keep[0]), N.ptr(keep[1]), S_prev, N.ptr(keep[2]), N.ptr(keep[3]), N.ptr(keep[4]),
                                 N.ptr(keep[5]), anneal, None, c["hist_pad"], 1e-5, 1.0 / (2 * (S + 1)), int(uniform), per_edge,
                                 int(include_original), n, S, N.ptr(s), N.ptr(t), N.ptr(inds), st)
    torch.cuda.synchronize()
    return rc_, s, t, inds


def _pdf_check(N, S_prev, S, jitter, uniform=False, pattern=None):
    c = rc.pdf_case(S_prev, S, jitter, uniform, pattern)
    so, to, io = orc.pdf_resample(c["s0"], c["w"], S, c["jitter"], c["nears"], c["fars"], histogram_padding=c["hist_pad"],
                                  uniform=uniform)
    status, s, t, inds = _pdf_launch(N, c, S, uniform)
    N.check(status, "pdf_resample")
    what = f"({S_prev}, {S}) jitter={jitter} uniform={uniform} pattern={pattern}"
    exact(inds, io, "indices " + what)
    exact(s, so, "s_bins " + what)
    exact(t, to, "t_bins " + what)
    return io


@pytest.mark.parametrize("jitter", rc.PDF_JITTERS)
@pytest.mark.parametrize("S_prev,S", rc.PDF_PAIRS)
def test_pdf_resample_exact(N, S_prev, S, jitter):
    _pdf_check(N, S_prev, S, jitter)
    if (S_prev, S) == (321, 300):
        _pdf_check(N, S_prev, S, jitter, uniform=True)


@pytest.mark.parametrize("jitter", rc.PDF_JITTERS)
@pytest.mark.parametrize("pattern", rc.PDF_PATTERNS)
def test_pdf_resample_degenerate_histograms(N, pattern, jitter):
    io = _pdf_check(N, 96, 48, jitter, pattern=pattern)
    if jitter != "none":
        assert int((io == 97).sum()) > 0  # a draw at the end of the cdf: c1 == c0


def test_pdf_resample_limits(N):
    for S_prev, S in ((1025, 48), (96, 4097), (1025, 4097)):
        for original in (False, True):
            c = rc.pdf_case(S_prev, S, "ray")
            status, s, t, inds = _pdf_launch(N, c, S, include_original=original)
            assert status == ERR_UNSUPPORTED, (S_prev, S, original, status)
            untouched(s, t, inds)


@pytest.mark.parametrize("S_prev,S", rc.ORIGINAL_PAIRS)
def test_pdf_resample_with_original_edges(N, S_prev, S):
    """include_original keeps the S + 1 new edges of 4 rays in LDS too: 65 584 B at (1024, 1024), 114 736 B at (1024, 4096)."""
    c = rc.pdf_case(S_prev, S, "edge", uniform=True)
    sm, tm = vo.pdf_resample_with_original(c["s0"], c["w"], c["nears"], c["fars"], S, c["jitter"])
    io = orc.pdf_resample(c["s0"], c["w"], S, c["jitter"], c["nears"], c["fars"], uniform=True)[2]
    status, s, t, inds = _pdf_launch(N, c, S, uniform=True, include_original=True)
    N.check(status, f"pdf_resample(include_original) ({S_prev}, {S})")
    exact(inds, io, "indices")
    exact(s, sm, "merged s_bins")
    exact(t, tm, "merged t_bins")
    assert bool((s[:, 1:] >= s[:, :-1]).all()), "merged edges are sorted"
    # and once more without the index output, after the opt-in: the same bits
    status, s2, t2, _ = _pdf_launch(N, c, S, uniform=True, include_original=True, want_inds=False)
    N.check(status, "pdf_resample(include_original), second call")
    assert torch.equal(s2, s) and torch.equal(t2, t)


# ---------------------------------------------------------------- nsamd_proposal_resample -------------------------------

@pytest.mark.parametrize("S_prev", [1, 64, 255, 256, 257, 320, 1024])
def test_proposal_resample(N, S_prev):
    lib, st = N.load(), N.stream()
    S, n = 96, rc.PDF_RAYS
    c = rc.pdf_case(S_prev, S, "ray", seed=5000 + S_prev)
    u = dev(_u_base(S))
    u_off = 1.0 / (2 * (S + 1))

    def on_device(case):
        return {k: dev(case[k]) for k in ("s0", "t0", "dens", "jitter", "nears", "fars")}

    def fused(d, anneal, anneal_dev=None, median=True):
        w, med, s, t = nanfill(n, S_prev), nanfill(n) if median else None, nanfill(n, S + 1), nanfill(n, S + 1)
        N.check(lib.nsamd_proposal_resample(N.ptr(d["t0"]), N.ptr(d["s0"]), N.ptr(d["dens"]), S_prev, N.ptr(u),
                                            N.ptr(d["jitter"]), N.ptr(d["nears"]), N.ptr(d["fars"]), anneal, N.ptr(anneal_dev),
                                            0.01, 1e-5, u_off, 0, n, S, N.ptr(w), N.ptr(med), N.ptr(s), N.ptr(t), st),
                "proposal_resample")
        torch.cuda.synchronize()
        return w, med, s, t

    d = on_device(c)
    t0, dn = d["t0"], d["dens"]
    w, med, s, t = fused(d, 1.0)
    worst = {}
    r = orc.weights64(c["t0"], c["dens"])
    check_entries("weights", w, r["w"], rc.weights_fwd_bound(r), worst)
    # median depth: the index on the kernel's own fp32 weights, the value exact
    wc = w.cpu()
    assert np.array_equal(rc.median_index_np(wc.numpy()), orc.depth_median(wc, c["t0"])[1][:, 0].numpy())  # (no tie)
    exact(med, orc.depth_median(wc, c["t0"])[0][:, 0], "median depth")
    # bins: the bits of nsamd_weights_fwd + nsamd_pdf_resample
    w_a = nanfill(n, S_prev)
    N.check(lib.nsamd_weights_fwd(N.ptr(t0), N.ptr(dn), n, S_prev, N.ptr(w_a), st), "weights_fwd")
    assert torch.equal(w_a, w)
    status, s_a, t_a, _ = _pdf_launch(N, dict(c, w=wc), S)
    N.check(status, "pdf_resample")
    assert torch.equal(s_a, s) and torch.equal(t_a, t)
    so, to, _ = orc.pdf_resample(c["s0"], wc, S, c["jitter"], c["nears"], c["fars"])
    exact(s, so, "s_bins vs oracle")
    exact(t, to, "t_bins vs oracle")
    w2, _, s2, t2 = fused(d, 1.0, median=False)
    assert torch.equal(w2, w) and torch.equal(s2, s) and torch.equal(t2, t)
    # annealed: pow() is not bit-reproducible across libms, so on values, as test_annealed_resample_zero_and_denormal_weights
    # does (3e-6 on s, 2e-5 relative on t); the device copy of the exponent gives the host's bits. The t criterion follows from
    # the s one only while the map s -> t = 1 / (2 - 2 v) does not magnify: d t / t = d v / (1 - v), 116 x at far = 1000 but
    # <= 6 x with far = 3 (1 - v >= 1 / 6), so the value comparison runs on a case with far = 3; the bits on both.
    a_dev = torch.tensor([0.3], device="cuda")
    wh, _, sh, th = fused(d, 0.3)
    wd, _, sd, td = fused(d, 1.0, a_dev)
    assert torch.equal(wh, w) and torch.equal(wd, w) and torch.equal(sd, sh) and torch.equal(td, th)
    exact(th, orc.spacing_to_euclidean(sh.cpu(), c["nears"], c["fars"]), "annealed t_bins are the map of the annealed s_bins")
    c3 = rc.pdf_case(S_prev, S, "ray", seed=6000 + S_prev, far=3.0)
    d3 = on_device(c3)
    w3, _, sh, th = fused(d3, 0.3)
    _, _, sd, td = fused(d3, 1.0, a_dev)
    assert torch.equal(sd, sh) and torch.equal(td, th)
    sa, ta, _ = orc.pdf_resample(c3["s0"], torch.pow(w3.cpu(), 0.3), S, c3["jitter"], c3["nears"], c3["fars"])
    assert bool(torch.isfinite(sh).all())
    torch.testing.assert_close(sh.cpu(), sa, atol=3e-6, rtol=0)
    torch.testing.assert_close(th.cpu(), ta, atol=0, rtol=2e-5)
    report(f"proposal_resample S_prev={S_prev}", worst)


def test_proposal_resample_limit(N):
    lib = N.load()
    c = rc.pdf_case(1025, 96, "ray")
    n = rc.PDF_RAYS
    keep = [dev(c["t0"]), dev(c["s0"]), dev(c["dens"]), dev(_u_base(96)), dev(c["jitter"]), dev(c["nears"]), dev(c["fars"])]
    w, med, s, t = nanfill(n, 1025), nanfill(n), nanfill(n, 97), nanfill(n, 97)
    assert lib.nsamd_proposal_resample(N.ptr(keep[0]), N.ptr(keep[1]), N.ptr(keep[2]), 1025, N.ptr(keep[3]), N.ptr(keep[4]),
                                       N.ptr(keep[5]), N.ptr(keep[6]), 1.0, None, 0.01, 1e-5, 1.0 / 194, 0, n, 96, N.ptr(w),
                                       N.ptr(med), N.ptr(s), N.ptr(t), N.stream()) == ERR_UNSUPPORTED
    untouched(w, med, s, t)


# ---------------------------------------------------------------- compositing -------------------------------------------

@functools.lru_cache(maxsize=None)
def _composite_inputs(S, n=rc.COMPOSITE_RAYS):
    c = rc.composite_case(S, n)
    c["rgb_eval"] = rc.eval_colours(c["rgb"])
    c["d"] = {k: dev(c[k]) for k in ("rgb", "rgb_eval", "w", "t", "dens", "target", "bg_rays")}
    c["median_ref"] = orc.depth_median(c["w"], c["t"])
    return c


def _ws(n):
    return nanfill(2 + 2 * ((n + 3) // 4))


def _check_depth(c, ref, b, depth, ws, worst, tag):
    torch.cuda.synchronize()
    assert float(ws[0]) == float(ref["lo"]) and float(ws[1]) == float(ref["hi"]), (tag, float(ws[0]), float(ws[1]))
    check_entries(f"depth {tag}", depth, ref["depth"], b["depth"], worst)
    zero = c["zero"]
    if len(zero):
        assert bool((depth.cpu()[zero] == float(ref["lo"])).all()), f"{tag}: all-zero-weight rays must sit on lo"


@pytest.mark.parametrize("background", [0, 1, 2])
@pytest.mark.parametrize("S,n", [(S, rc.COMPOSITE_RAYS) for S in rc.COMPOSITE_S] + [(48, 5)])
def test_composite_fwd_vs_float64(N, S, n, background):
    lib, st = N.load(), N.stream()
    c = _composite_inputs(S, n)
    d = c["d"]
    bgv = BGV if background == 2 else None
    worst = {}

    def launch(rgb, outs, eval_mode=0):
        o = dict(rgb=nanfill(n, 3) if "rgb" in outs else None, acc=nanfill(n) if "acc" in outs else None,
                 depth=nanfill(n) if "depth" in outs else None, med=nanfill(n) if "med" in outs else None,
                 idx=nanfill(n, dtype=torch.int32) if "idx" in outs else None)
        o["ws"] = _ws(n) if "depth" in outs else None
        need_t = bool({"depth", "med", "idx"} & set(outs))
        N.check(lib.nsamd_composite_fwd(N.ptr(rgb), N.ptr(d["w"]), N.ptr(d["t"]) if need_t else None, n, S, background, bgv,
                                        eval_mode, N.ptr(o["rgb"]), N.ptr(o["acc"]), N.ptr(o["depth"]), N.ptr(o["med"]),
                                        N.ptr(o["idx"]), N.ptr(o["ws"]), st), f"composite_fwd {outs}")
        torch.cuda.synchronize()
        return o

    ref = orc.composite64(c["rgb"], c["w"], c["t"], background, rc.BG_COLOR)
    b = rc.composite_bounds(ref, S, background, False)
    med_ref, idx_ref = c["median_ref"]
    # all outputs
    o = launch(d["rgb"], ("rgb", "acc", "depth", "med", "idx"))
    check_entries("rgb", o["rgb"], ref["rgb"], b["rgb"], worst)
    check_entries("acc", o["acc"], ref["acc"], b["acc"], worst)
    _check_depth(c, ref, b, o["depth"], o["ws"], worst, "all")
    exact(o["idx"], idx_ref[:, 0], "median index")
    exact(o["med"], med_ref[:, 0], "median depth")
    for ray, k in c["median"].items():
        assert int(o["idx"][ray]) == k, (ray, k)
    # colour only; depth only (no colours at all); median only
    o1 = launch(d["rgb"], ("rgb",))
    check_entries("rgb (alone)", o1["rgb"], ref["rgb"], b["rgb"], worst)
    assert torch.equal(o1["rgb"], o["rgb"])
    o2 = launch(None, ("depth",))
    _check_depth(c, ref, b, o2["depth"], o2["ws"], worst, "alone")
    assert torch.equal(o2["depth"], o["depth"])
    o3 = launch(None, ("med",))
    exact(o3["med"], med_ref[:, 0], "median depth (alone)")
    o4 = launch(None, ("idx",))
    exact(o4["idx"], idx_ref[:, 0], "median index (alone)")
    # eval mode: nan_to_num on the samples' colours, clamp of the result
    if n == rc.COMPOSITE_RAYS:
        ref_e = orc.composite64(c["rgb_eval"], c["w"], c["t"], background, rc.BG_COLOR, eval_mode=True)
        b_e = rc.composite_bounds(ref_e, S, background, True)
        oe = launch(d["rgb_eval"], ("rgb", "acc", "depth"), eval_mode=1)
        check_entries("rgb (eval)", oe["rgb"], ref_e["rgb"], b_e["rgb"], worst)
        assert float(oe["rgb"].min()) >= 0 and float(oe["rgb"].max()) <= 1
        assert torch.equal(oe["depth"], o["depth"]) and torch.equal(oe["acc"], o["acc"])
    report(f"composite_fwd S={S} n={n} background={background}", worst)


@pytest.mark.parametrize("background", [0, 1, 2, 3])
@pytest.mark.parametrize("S,n", [(S, rc.COMPOSITE_RAYS) for S in rc.COMPOSITE_S] + [(48, 5)])
def test_render_train_vs_float64(N, S, n, background):
    lib, st = N.load(), N.stream()
    c = _composite_inputs(S, n)
    d = c["d"]
    bgv = BGV if background == 2 else None
    gs = 1.0 / (3 * n)
    worst = {}
    o = dict(w=nanfill(n, S), rgb=nanfill(n, 3), acc=nanfill(n), depth=nanfill(n), med=nanfill(n), ws=_ws(n), sq=nanfill(n),
             dro=nanfill(n, 3))
    N.check(lib.nsamd_render_train(N.ptr(d["rgb"]), N.ptr(d["dens"]), N.ptr(d["t"]), n, S, background, bgv, N.ptr(d["target"]),
                                   gs, N.ptr(o["w"]), N.ptr(o["rgb"]), N.ptr(o["acc"]), N.ptr(o["depth"]), N.ptr(o["med"]),
                                   N.ptr(o["ws"]), N.ptr(o["sq"]), N.ptr(o["dro"]),
                                   N.ptr(d["bg_rays"]) if background == 3 else None, st), "render_train")
    torch.cuda.synchronize()
    r = orc.weights64(c["t"], c["dens"])
    check_entries("weights", o["w"], r["w"], rc.weights_fwd_bound(r), worst)
    wk = o["w"].cpu()  # the rest is a function of the weights as stored
    ref = orc.composite64(c["rgb"], wk, c["t"], background, rc.BG_COLOR, c["bg_rays"], False, c["target"], gs)
    b = rc.composite_bounds(ref, S, background, False, c["bg_rays"], gs)
    for k, name in (("rgb", "rgb"), ("acc", "acc"), ("sq", "sq_err"), ("dro", "d_rgb_out")):
        check_entries(name, o[k], ref[name], b[name], worst)
    _check_depth(c, ref, b, o["depth"], o["ws"], worst, "train")
    med_ref, idx_ref = orc.depth_median(wk, c["t"])
    assert np.array_equal(rc.median_index_np(wk.numpy()), idx_ref[:, 0].numpy())  # (no double-rounding tie on these weights)
    exact(o["med"], med_ref[:, 0], "median depth")
    # the bits of nsamd_weights_fwd + nsamd_composite_fwd (background 3 composites without a background)
    w_a, rgb_a, acc_a, dep_a, med_a, ws_a = nanfill(n, S), nanfill(n, 3), nanfill(n), nanfill(n), nanfill(n), _ws(n)
    N.check(lib.nsamd_weights_fwd(N.ptr(d["t"]), N.ptr(d["dens"]), n, S, N.ptr(w_a), st), "weights_fwd")
    N.check(lib.nsamd_composite_fwd(N.ptr(d["rgb"]), N.ptr(w_a), N.ptr(d["t"]), n, S, background % 3, bgv, 0, N.ptr(rgb_a),
                                    N.ptr(acc_a), N.ptr(dep_a), N.ptr(med_a), None, N.ptr(ws_a), st), "composite_fwd")
    torch.cuda.synchronize()
    for a, k in ((w_a, "w"), (rgb_a, "rgb"), (acc_a, "acc"), (dep_a, "depth"), (med_a, "med")):
        assert torch.equal(a, o[k]), k
    assert torch.equal(ws_a[:2], o["ws"][:2])
    # without a target, and without the optional outputs: the same bits in what remains
    w2, rgb2 = nanfill(n, S), nanfill(n, 3)
    N.check(lib.nsamd_render_train(N.ptr(d["rgb"]), N.ptr(d["dens"]), N.ptr(d["t"]), n, S, background, bgv, None, gs, N.ptr(w2),
                                   N.ptr(rgb2), None, None, None, None, None, None,
                                   N.ptr(d["bg_rays"]) if background == 3 else None, st), "render_train (colour only)")
    torch.cuda.synchronize()
    assert torch.equal(w2, o["w"]) and torch.equal(rgb2, o["rgb"])
    report(f"render_train S={S} n={n} background={background}", worst)


def test_composite_limits(N):
    """S = 4096 passes (8 rays), S = 4097 is refused with nothing written; render_train_bwd accepts 1024 and refuses 1025."""
    lib, st = N.load(), N.stream()
    n, S = 8, 4096
    c = _composite_inputs(S, n)
    d = c["d"]
    worst = {}
    ref = orc.composite64(c["rgb"], c["w"], c["t"], 1)
    b = rc.composite_bounds(ref, S, 1, False)
    rgb, acc, depth, med, idx, ws = nanfill(n, 3), nanfill(n), nanfill(n), nanfill(n), nanfill(n, dtype=torch.int32), _ws(n)
    N.check(lib.nsamd_composite_fwd(N.ptr(d["rgb"]), N.ptr(d["w"]), N.ptr(d["t"]), n, S, 1, None, 0, N.ptr(rgb), N.ptr(acc),
                                    N.ptr(depth), N.ptr(med), N.ptr(idx), N.ptr(ws), st), "composite_fwd S=4096")
    check_entries("rgb", rgb, ref["rgb"], b["rgb"], worst)
    check_entries("acc", acc, ref["acc"], b["acc"], worst)
    _check_depth(c, ref, b, depth, ws, worst, "S=4096")
    exact(idx, c["median_ref"][1][:, 0], "median index")
    exact(med, c["median_ref"][0][:, 0], "median depth")
    w_t, rgb_t = nanfill(n, S), nanfill(n, 3)
    N.check(lib.nsamd_render_train(N.ptr(d["rgb"]), N.ptr(d["dens"]), N.ptr(d["t"]), n, S, 1, None, None, 1.0, N.ptr(w_t),
                                   N.ptr(rgb_t), None, None, None, None, None, None, None, st), "render_train S=4096")
    r = orc.weights64(c["t"], c["dens"])
    check_entries("weights (train)", w_t, r["w"], rc.weights_fwd_bound(r), worst)
    ref_t = orc.composite64(c["rgb"], w_t.cpu(), c["t"], 1)
    check_entries("rgb (train)", rgb_t, ref_t["rgb"], rc.composite_bounds(ref_t, S, 1, False)["rgb"], worst)
    # 4097
    big = 4097
    z = {k: torch.zeros(n, big + 1, device="cuda") for k in ("t", "w")}
    z3 = torch.zeros(n, big, 3, device="cuda")
    outs = [nanfill(n, 3), nanfill(n), nanfill(n), nanfill(n), nanfill(n, big)]
    assert lib.nsamd_composite_fwd(N.ptr(z3), N.ptr(z["w"]), N.ptr(z["t"]), n, big, 0, None, 0, N.ptr(outs[0]), N.ptr(outs[1]),
                                   N.ptr(outs[2]), N.ptr(outs[3]), None, N.ptr(ws), st) == ERR_UNSUPPORTED
    assert lib.nsamd_render_train(N.ptr(z3), N.ptr(z["w"]), N.ptr(z["t"]), n, big, 0, None, None, 1.0, N.ptr(outs[4]),
                                  N.ptr(outs[0]), N.ptr(outs[1]), N.ptr(outs[2]), N.ptr(outs[3]), N.ptr(ws), None, None, None,
                                  st) == ERR_UNSUPPORTED
    untouched(*outs)
    # render_train_bwd at its limit: d_rgb and d_density entry by entry, as test_gpu_proposal_backward does at S = 48
    S = 1024
    c = _composite_inputs(S, n)
    d = c["d"]
    g = torch.Generator().manual_seed(9)
    d_out = torch.randn(n, 3, generator=g) * 1e-3
    w = nanfill(n, S)
    N.check(lib.nsamd_weights_fwd(N.ptr(d["t"]), N.ptr(d["dens"]), n, S, N.ptr(w), st), "weights_fwd")
    drgb, dden, dod = nanfill(n, S, 3), nanfill(n, S), dev(d_out)
    N.check(lib.nsamd_render_train_bwd(N.ptr(d["rgb"]), N.ptr(w), N.ptr(d["dens"]), N.ptr(d["t"]), n, S, 1, None, N.ptr(dod),
                                       None, N.ptr(drgb), N.ptr(dden), None, st), "render_train_bwd S=1024")
    cb = orc.composite_bwd64(c["rgb"], w.cpu(), d_out, 1)
    b_rgb, _ = rc.composite_bwd_bounds(cb, w.cpu(), S, 1, d_out)
    check_entries("d_rgb (S=1024)", drgb, cb["d_rgb"], b_rgb, worst)
    rb = orc.weights_bwd64(c["t"], c["dens"], cb["d_weights"])
    check_entries("d_density (S=1024)", dden, rb["ddensity"], weights_bound(rb, 8 * U * cb["dw_abs"]), worst)
    z = torch.zeros(n, 1026, device="cuda")
    z3 = torch.zeros(n, 1025, 3, device="cuda")
    o3, o1 = nanfill(n, 1025, 3), nanfill(n, 1025)
    assert lib.nsamd_render_train_bwd(N.ptr(z3), N.ptr(z), N.ptr(z), N.ptr(z), n, 1025, 0, None, N.ptr(dod), None, N.ptr(o3),
                                      N.ptr(o1), None, st) == ERR_UNSUPPORTED
    untouched(o3, o1)
    report("composite limits", worst)


# ---------------------------------------------------------------- nsamd_composite_bwd -----------------------------------

@pytest.mark.parametrize("background", [0, 1, 2])
@pytest.mark.parametrize("S", rc.BWD_S)
def test_composite_bwd_vs_float64(N, S, background):
    lib, st = N.load(), N.stream()
    n = rc.BWD_RAYS
    c = rc.composite_bwd_case(S)
    bgv = BGV if background == 2 else None
    rgb, w, t = dev(c["rgb"]), dev(c["w"]), dev(c["t"])
    # the forward on the same inputs leaves the clip range in the workspace
    depth, ws = nanfill(n), _ws(n)
    N.check(lib.nsamd_composite_fwd(None, N.ptr(w), N.ptr(t), n, S, 0, None, 0, None, None, N.ptr(depth), None, None,
                                    N.ptr(ws), st), "composite_fwd")
    fwd = orc.composite64(None, c["w"], c["t"], 0)
    amb = rc.clip_ambiguous(fwd, S)
    print(f"\ncomposite_bwd S={S}: {int(amb.sum())} of {n} rays within their bound of a clip edge (d_depth zeroed)")
    assert int(amb.sum()) <= 0.02 * n and not bool(amb[c["zero"]].any())
    d_depth = c["d_depth"].clone()
    d_depth[amb] = 0.0
    g = dict(out=c["d_out"], acc=c["d_acc"], depth=d_depth)
    gd = {k: dev(v) for k, v in g.items()}
    add_d = dev(c["d_add"])
    worst = {}
    results = {}
    for mask in range(8):
        use = {k: bool(mask >> i & 1) for i, k in enumerate(("out", "acc", "depth"))}
        for with_add in (False, True):
            d_rgb, d_w = nanfill(n, S, 3), nanfill(n, S)
            N.check(lib.nsamd_composite_bwd(N.ptr(rgb), N.ptr(w), N.ptr(t) if use["depth"] else None, n, S, background, bgv,
                                            N.ptr(gd["out"]) if use["out"] else None, N.ptr(gd["acc"]) if use["acc"] else None,
                                            N.ptr(gd["depth"]) if use["depth"] else None, N.ptr(ws) if use["depth"] else None,
                                            N.ptr(add_d) if with_add else None, N.ptr(d_rgb), N.ptr(d_w), st), "composite_bwd")
            torch.cuda.synchronize()
            d_out = g["out"] if use["out"] else None
            r = orc.composite_bwd64(c["rgb"], c["w"], d_out, background, rc.BG_COLOR, None, c["d_add"] if with_add else None,
                                    g["acc"] if use["acc"] else None, g["depth"] if use["depth"] else None,
                                    c["t"] if use["depth"] else None)
            b_rgb, b_w = rc.composite_bwd_bounds(r, c["w"], S, background, d_out)
            tag = "+".join(k for k in use if use[k]) or "none"
            check_entries(f"d_weights [{tag}]", d_w, r["d_weights"], b_w, worst)
            check_entries(f"d_rgb [{tag}]", d_rgb, r["d_rgb"], b_rgb, worst)
            results[(mask, with_add)] = d_w
    # the all-zero-weight rays (raw depth 0, below lo) get exactly no depth gradient
    zero = c["zero"].cuda()
    for mask in range(4):
        for with_add in (False, True):
            assert bool((results[(mask | 4, with_add)][zero] == results[(mask, with_add)][zero]).all())
    assert not torch.equal(results[(4, False)], results[(0, False)])
    report(f"composite_bwd S={S} background={background}", worst)


# ---------------------------------------------------------------- nsamd_mse_loss ----------------------------------------

@pytest.mark.parametrize("n", rc.MSE_N)
def test_mse_loss_vs_float64(N, n):
    lib, st = N.load(), N.stream()
    g = torch.Generator().manual_seed(n)
    pred, target = torch.rand(n, generator=g), torch.rand(n, generator=g)
    gs = 1.0 / n
    r = orc.mse64(pred, target, gs)
    pd, td = dev(pred), dev(target)

    def launch(want_loss, want_grad):
        loss = torch.zeros(1, device="cuda") if want_loss else None
        dp = nanfill(n) if want_grad else None
        N.check(lib.nsamd_mse_loss(N.ptr(pd), N.ptr(td), n, gs, N.ptr(loss), N.ptr(dp), st), "mse_loss")
        torch.cuda.synchronize()
        return loss, dp

    worst = {}
    loss, dp = launch(True, True)
    check_entries("dpred", dp, r["dpred"], 2 * U * r["dpred"].abs(), worst)
    check_entries("loss_sum", loss, r["loss_sum"], torch.as_tensor(rc.mse_loss_bound(n, float(r["loss_sum"]))), worst)
    loss_only, _ = launch(True, False)
    _, grad_only = launch(False, True)
    assert torch.equal(grad_only, dp)
    if n <= 256:  # one workgroup: one atomic
        assert torch.equal(loss_only, loss)
    else:         # the order of the workgroups' atomics is not fixed
        assert abs(float(loss_only) - float(loss)) <= 64 * U * float(r["loss_sum"])
    report(f"mse_loss n={n}", worst)


# ---------------------------------------------------------------- nsamd_distance_gradient_scale -------------------------

def test_distance_gradient_scale_vs_float64(N):
    lib, st = N.load(), N.stream()
    t, d_density, d_rgb = rc.distance_case()
    n, S = d_density.shape
    td = dev(t)
    rd, rr = orc.distance_scale64(t, d_density, d_rgb)
    worst = {}
    for use_d, use_r in ((True, False), (False, True), (True, True), (False, False)):
        gd, gr = dev(d_density), dev(d_rgb)
        N.check(lib.nsamd_distance_gradient_scale(N.ptr(td), n, S, N.ptr(gd) if use_d else None, N.ptr(gr) if use_r else None,
                                                  st), "distance_gradient_scale")
        torch.cuda.synchronize()
        if use_d:
            check_entries("d_density", gd, rd, 4 * U * rd.abs(), worst)
        else:
            assert torch.equal(gd.cpu(), d_density)
        if use_r:
            check_entries("d_rgb", gr, rr, 4 * U * rr.abs(), worst)
        else:
            assert torch.equal(gr.cpu(), d_rgb)
    mids = (t[:, :-1] + t[:, 1:]) / 2
    assert float(mids.min()) < 1 < float(mids.max())
    report("distance_gradient_scale", worst)
