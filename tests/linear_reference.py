"""Float64 reference of ONE dense layer y = act(x W^T + b) and of its backward, the per-entry bounds and the case table that
tests/test_linear_reference_cpu.py (no GPU) and tests/test_gpu_linear_float64.py (nsamd_linear_fwd / nsamd_linear_bwd of
csrc/linear.hip) share.

The reference, all in float64 on the fp32 inputs:
    pre = x W^T + b        y = act(pre)        dpre = dy * act'(pre)        dx = dpre W        dW = dpre^T x        db = sum dpre
act: 0 none, 1 ReLU, 2 Sigmoid, 3 Softplus by torch's rule (v > 20 ? v : log1p(exp(v)), derivative 1 beyond 20).
The backward takes y as an INPUT at the ABI: the tests hand it `y32`, the float64 y rounded to fp32. The ReLU mask y > 0 is
then the reference's own, and no entry is excluded anywhere.

EXACT cases: x, W, b, dy are integers in [-3, 3], the activation is none or ReLU. `reference` asserts sum |term| < 2^24 for
every entry of pre, dx, dW and db (dW / db over all M points): every product and every partial sum in any order is then an
integer below 2^24, i.e. exactly representable, and the result has to EQUAL the float64 one whatever the order of the sums
(blocks, chunks, float atomics). Equality is that of fp32 numbers: the sign of a zero sum depends on the value a summation
starts from (an accumulator at +0 never ends at -0, a sum of -0 products does) and is not compared.

VALUE cases (standard-normal inputs): per entry |got - ref| <= 2 (T + 2) u A + f, u = 2^-24, T the number of terms of the
entry's sum (K for y, N for dx, M for dW / db), A the same sum over absolute values in float64: twice the textbook worst case of
an fp32 sum in any order, which also covers the fp32 store / reload of partial sums between 128-wide blocks and the one product
dy * act'. The activations are 1-Lipschitz, so the bound of pre carries to y.

f, the function-evaluation allowance of Sigmoid / Softplus and their derivatives, is MEASURED on the reference, never on the
kernel (`function_allowance`): what torch's fp32 CPU sigmoid / softplus (forward) and sigmoid_backward / softplus_backward
achieve against float64 on the case's own pre-activations rounded to fp32, in ulps of the float64 result. The kernel gets
4 x that figure and at least 4 ulp (two chained device transcendentals and a division, each documented at 1 - 2 ulp).
The derivative is taken from the fp32 y, whose rounding (<= u |y|) no implementation of this ABI can undo; that part is
derived, not measured: |d act'/dy| u |y| = |1 - 2y| u y for Sigmoid (y (1 - y)), exp(-y) u y for Softplus (1 - exp(-y)).
It is what lets a saturated Sigmoid (y rounds to 1) return 0 for 1e-13, and it is one half ulp of act' for a Softplus at
negative pre-activations, where act' ~ y: there the check is a RELATIVE one.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
NONE, RELU, SIGMOID, SOFTPLUS = 0, 1, 2, 3
ACT_NAMES = {NONE: "none", RELU: "relu", SIGMOID: "sigmoid", SOFTPLUS: "softplus"}
MIN_ULPS, ULP_MARGIN = 4.0, 4.0

Case = namedtuple("Case", "name M K N act kind spread")


def _case(stage, M, K, N, act, kind, spread=False):
    return Case(f"{stage}-{kind}-M{M}-K{K}-N{N}-{ACT_NAMES[act]}", M, K, N, act, kind, spread)


# stage 1: tile counts 1, 2, 3 (padded to 4), 5 (padded to 8) and the full block of 8: every (NT, KT) of the forward
# (NT from N, KT from K) and of the transposed kernel (NT from K, KT from N)
WIDTHS = (16, 17, 40, 65, 128)
INSTANTIATIONS = [_case("inst", 33, K, N, act, "exact") for K in WIDTHS for N in WIDTHS for act in (NONE, RELU)]
# stage 2: the grid of 128 x 128 blocks of W
BLOCK_SHAPES = ((129, 5), (5, 129), (130, 131), (132, 132), (319, 256), (256, 319))
BLOCK_GRID = ([_case("grid", 33, K, N, act, "exact") for K, N in BLOCK_SHAPES for act in (NONE, RELU)]
              + [_case("grid", 33, K, N, act, "value") for K, N in BLOCK_SHAPES for act in (NONE, RELU, SIGMOID, SOFTPLUS)])
# stage 3: point counts around the 16-point tile, the 4-wave workgroup, the dW chunking (from 2048), the 65 536 points of
# one pass of the grid-stride loop; the eval path's own layers, and the 319 x 256 layer whose `chunks` are capped
POINT_COUNTS = (1, 15, 16, 17, 63, 65, 2047, 2048, 2049, 3001, 65536, 65553)
POINT_EDGES = ([_case("points", M, 27, 64, RELU, "exact") for M in POINT_COUNTS]
               + [_case("points", M, 64, 3, NONE, "exact") for M in POINT_COUNTS]
               + [_case("points", 65553, 319, 256, RELU, "exact")])
# stage 4: pre-activations over [-30, 30]; N = 1: dx[p, :] = dpre[p] W[0, :] is one product, so dx carries act' RELATIVELY
ACTIVATIONS = [_case("act", 300, 24, 40, SIGMOID, "value", True), _case("act", 300, 24, 40, SOFTPLUS, "value", True),
               _case("act", 300, 24, 1, SOFTPLUS, "value", True), _case("act", 300, 24, 1, SIGMOID, "value", True)]
# stage 5: row strides that are multiples of 4 (bases get moved off the 16-byte alignment); 132 = a full block and a 4-wide one
ALIGNMENT = [BLOCK_GRID[i] for i, c in enumerate(BLOCK_GRID) if (c.K, c.N) == (132, 132) and (c.kind, c.act) in
             (("exact", RELU), ("value", SIGMOID))] + [_case("align", 65, 64, 16, SOFTPLUS, "value")]
CASES = INSTANTIATIONS + BLOCK_GRID + POINT_EDGES + ACTIVATIONS + ALIGNMENT[-1:]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def make_inputs(c):
    """-> dict(x [M, K], W [N, K], b [N], dy [M, N]) fp32, seeded by the case's name."""
    rs = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    if c.kind == "exact":
        draw = lambda *s: rs.randint(-3, 4, s).astype(np.float32)  # noqa: E731
        return {"x": draw(c.M, c.K), "W": draw(c.N, c.K), "b": draw(c.N), "dy": draw(c.M, c.N)}
    draw = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    x, W, b, dy = draw(c.M, c.K), draw(c.N, c.K), draw(c.N), draw(c.M, c.N)
    if c.spread:  # column 0 carries the pre-activation over [-30, 30] (both signs for every neuron), the rest is small
        x *= 0.1
        x[:, 0] = rs.permutation(np.linspace(-30.0, 30.0, c.M)).astype(np.float32)
        W[:, 0] = rs.choice([-1.0, 1.0], c.N)
        b *= 0.1
    return {"x": x, "W": W, "b": b, "dy": dy}


def act64(act, v):
    if act == RELU:
        return np.maximum(v, 0.0)
    if act == SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    if act == SOFTPLUS:
        return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))
    return v


def act_grad64(act, v):
    if act == RELU:
        return (v > 0.0).astype(np.float64)
    if act == SIGMOID:  # s (1 - s) without the cancellation in 1 - s
        return 1.0 / ((1.0 + np.exp(-v)) * (1.0 + np.exp(v)))
    if act == SOFTPLUS:
        return np.where(v > 20.0, 1.0, 1.0 / (1.0 + np.exp(-v)))
    return np.ones_like(v)


def ulp32(v):
    """The spacing of fp32 at |v| (2^-149 below FLT_MIN), as float64."""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def grad_input_rounding(act, y):
    """|d act'/dy| u |y|: what the rounding of the handed-over y to fp32 moves act'(y) by, at most (first order)."""
    if act == SIGMOID:
        return np.abs(1.0 - 2.0 * y) * U * y
    if act == SOFTPLUS:
        return np.exp(-y) * U * y
    return np.zeros_like(y)


def function_allowance(act, pre):
    """-> dict(fwd_ref, bwd_ref: torch's fp32 CPU worst case in ulps of the float64 result; fwd, bwd: the kernel's allowance in
    ulps = max(MIN_ULPS, ULP_MARGIN x that)). Zeros for none / ReLU, which evaluate no function."""
    if act in (NONE, RELU):
        return {"fwd_ref": 0.0, "bwd_ref": 0.0, "fwd": 0.0, "bwd": 0.0}
    p32 = torch.from_numpy(np.ascontiguousarray(pre.astype(np.float32)))
    p64 = p32.double().numpy()
    one = torch.ones_like(p32)
    if act == SIGMOID:
        fwd = torch.sigmoid(p32)
        y32 = torch.from_numpy(act64(act, p64).astype(np.float32))
        bwd = torch.ops.aten.sigmoid_backward(one, y32)  # from the output, as autograd saves it
        slack = grad_input_rounding(act, act64(act, p64))
    else:
        fwd = torch.nn.functional.softplus(p32)
        bwd = torch.ops.aten.softplus_backward(one, p32, 1.0, 20.0)  # from the saved input
        slack = 0.0
    ref_f, ref_b = act64(act, p64), act_grad64(act, p64)
    fwd_ref = float((np.abs(fwd.double().numpy() - ref_f) / ulp32(ref_f)).max())
    bwd_ref = float((np.maximum(np.abs(bwd.double().numpy() - ref_b) - slack, 0.0) / ulp32(ref_b)).max())
    return {"fwd_ref": fwd_ref, "bwd_ref": bwd_ref, "fwd": max(MIN_ULPS, ULP_MARGIN * fwd_ref),
            "bwd": max(MIN_ULPS, ULP_MARGIN * bwd_ref)}


def _mm(a, b):
    return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()


def reference_of(c, inp, bias=True):
    """Float64 results of the layer on `inp`, `y32` (what the backward is handed), and for a value case the per-entry bounds
    `bound_<y|dx|dW|db>` with their parts `sum_<..>` (the summation term) and `f_<..>` (the function term), `allow` (see
    function_allowance) and `grad_allow` [M, N], the absolute allowance of act' per entry. Exact cases: the bounds are None."""
    x, W, dy = (inp[k].astype(np.float64) for k in ("x", "W", "dy"))
    b = inp["b"].astype(np.float64) if bias else np.zeros(c.N)
    pre = _mm(x, W.T) + b
    y = act64(c.act, pre)
    dpre = dy * act_grad64(c.act, pre)
    r = {"pre": pre, "y": y, "y32": y.astype(np.float32), "dpre": dpre, "dy32": dy, "W32": W, "dx": _mm(dpre, W), "dW": _mm(dpre.T, x),
         "db": dpre.sum(axis=0)}
    A = {"y": _mm(np.abs(x), np.abs(W).T) + np.abs(b), "dx": _mm(np.abs(dpre), np.abs(W)),
         "dW": _mm(np.abs(dpre).T, np.abs(x)), "db": np.abs(dpre).sum(axis=0)}
    if c.kind == "exact":
        assert c.act in (NONE, RELU)
        for k, a in A.items():
            assert a.max() < 2.0 ** 24, (c.name, k, a.max())  # every partial sum in any order is an integer below 2^24
        for k in ("y", "dx", "dW", "db"):
            assert np.array_equal(r[k], r[k].astype(np.float32).astype(np.float64)), (c.name, k)
            r["bound_" + k] = None
        return r
    terms = {"y": c.K, "dx": c.N, "dW": c.M, "db": c.M}
    allow = function_allowance(c.act, pre)
    grad_allow = allow["bwd"] * ulp32(act_grad64(c.act, pre)) + grad_input_rounding(c.act, y)
    w = np.abs(dy) * grad_allow  # the allowance of dpre per entry
    f = {"y": allow["fwd"] * ulp32(y), "dx": _mm(w, np.abs(W)), "dW": _mm(w.T, np.abs(x)), "db": w.sum(axis=0)}
    for k in ("y", "dx", "dW", "db"):
        r["sum_" + k] = 2.0 * (terms[k] + 2) * U * A[k]
        r["f_" + k] = f[k]
        r["bound_" + k] = r["sum_" + k] + f[k]
    r["allow"], r["grad_allow"] = allow, grad_allow
    return r


@functools.lru_cache(maxsize=2)
def _cached(name):
    c = BY_NAME[name]
    inp = make_inputs(c)
    return inp, reference_of(c, inp)


def case_data(name):
    """(inputs, reference) of a case of the table; computed once per process for the few most recent cases. Read-only."""
    return _cached(name)


def check(c, ref, got, which=("y", "dx", "dW", "db")):
    """Assert every entry of got[k], k in `which`, against the reference: equal for an exact case, inside the bound for a value
    case. Nothing is excluded; a non-finite entry fails. -> {k: worst |got - ref| / bound} (value) or {k: 0.0} (exact)."""
    worst = {}
    for k in which:
        g, r64 = np.asarray(got[k]), ref[k]
        assert g.dtype == np.float32 and g.shape == r64.shape, (c.name, k, g.dtype, g.shape, r64.shape)
        if ref["bound_" + k] is None:
            bad = ~(g.astype(np.float64) == r64)  # (NaN compares unequal)
            if bad.any():
                at = tuple(int(i) for i in np.argwhere(bad)[0])
                raise AssertionError(f"{c.name} {k}: {int(bad.sum())} of {bad.size} entries differ from the exact result, the first "
                                     f"at {at}: got {g[at]!r} expected {r64[at]!r}")
            worst[k] = 0.0
            continue
        err = np.abs(g.astype(np.float64) - r64)
        # (a bound of 0 — every term masked by the ReLU — is met by an error of 0 only)
        ratio = np.where(np.isfinite(err), np.where(err == 0, 0.0, err / np.maximum(ref["bound_" + k], 2.0 ** -1000)), np.inf)
        at = tuple(int(i) for i in np.unravel_index(np.argmax(ratio), ratio.shape)) if ratio.ndim else ()
        worst[k] = float(ratio.max())
        if not worst[k] <= 1.0:
            raise AssertionError(f"{c.name} {k}: entry {at} got {g[at]!r} reference {r64[at]!r} error {err[at]:.3e} is "
                                 f"{ratio[at]:.2f} x its bound {ref['bound_' + k][at]:.3e}; {int((ratio > 1).sum())} of "
                                 f"{ratio.size} entries outside")
    return worst


def function_ulps(c, ref, got):
    """What of the kernel's error the measured allowance has to cover, in ulps of the float64 result: the part of |got - ref|
    above the summation term (forward: of y), and, where the derivative can be isolated (N == 1: dx is one product), the part of
    dx's error above the summation term and the rounding of the handed y. 0 = the derived terms alone cover the error.
    -> dict(fwd=, bwd= or None)."""
    out = {"fwd": None, "bwd": None}
    if "y" in got:
        out["fwd"] = float((np.maximum(np.abs(got["y"].astype(np.float64) - ref["y"]) - ref["sum_y"], 0) / ulp32(ref["y"])).max())
    if "dx" in got and c.N == 1:
        nz = ref["dx"] != 0
        derived = ref["sum_dx"] + _mm(np.abs(ref["dy32"]) * grad_input_rounding(c.act, ref["y"]),
                                      np.abs(ref["W32"]))
        e = np.maximum(np.abs(got["dx"].astype(np.float64) - ref["dx"]) - derived, 0)
        out["bwd"] = float((e[nz] / ulp32(ref["dx"][nz])).max())
    return out
