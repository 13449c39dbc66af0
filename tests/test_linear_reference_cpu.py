"""No GPU: the checker of tests/linear_reference.py on a CORRECT fp32 implementation of the dense layer's ABI and on wrong ones.

`torch_layer` is nsamd_linear_fwd / nsamd_linear_bwd restated with torch's fp32 CPU ops: F.linear for the forward, and for the
backward dpre = dy * act'(y) from the HANDED y (ReLU y > 0, Sigmoid y (1 - y), Softplus -expm1(-y)), dx = dpre W,
dW = dpre^T x, db = sum dpre. On every case of the table it has to pass the very check the kernels get: equal on the exact
cases, inside the derived bounds on the value cases. Where autograd differentiates the same thing (no activation: nothing is
taken from y) its gradients are compared too. Each deliberately wrong variant is then rejected by the case meant to catch it.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linear_reference as lr


def _act(act, v):
    return {lr.NONE: lambda t: t, lr.RELU: torch.relu, lr.SIGMOID: torch.sigmoid, lr.SOFTPLUS: F.softplus}[act](v)


def torch_layer(c, inp, y32, variant=None):
    x, W, b, dy = (torch.from_numpy(inp[k]) for k in ("x", "W", "b", "dy"))
    # forward
    if variant == "drop_last_column":
        y = _act(c.act, F.linear(x[:, :-1], W[:, :-1], b))
    elif variant in ("bias_every_block", "act_every_block"):
        acc = None
        for k0 in range(0, c.K, 128):
            part = F.linear(x[:, k0:k0 + 128], W[:, k0:k0 + 128], b if (k0 == 0 or variant == "bias_every_block") else None)
            acc = part if acc is None else acc + part
            if variant == "act_every_block":
                acc = _act(c.act, acc)
        y = acc if variant == "act_every_block" else _act(c.act, acc)
    else:
        y = _act(c.act, F.linear(x, W, b))
    if variant == "skip_last_ragged_row":
        assert c.M % 16
        y = y.clone()
        y[-1] = float("nan")  # what the test's NaN-filled output buffer keeps
    # backward, from the handed y
    yh = torch.from_numpy(y32)
    if c.act == lr.RELU:
        g = (F.linear(x, W, b) >= 0).float() if variant == "relu_mask_from_pre" else (yh > 0).float()
    elif c.act == lr.SIGMOID:
        g = yh * (1 - yh)
    elif c.act == lr.SOFTPLUS:
        g = 1.0 - torch.exp(-yh) if variant == "softplus_grad_cancels" else -torch.expm1(-yh)
    else:
        g = torch.ones_like(dy)
    dpre = dy * g
    kept = dpre
    if variant == "dw_chunk_left_out":
        assert c.M >= 2048
        kept = dpre.clone()
        kept[1024:2048] = 0
    return {"y": y.numpy(), "dx": (dpre @ W).numpy(), "dW": (kept.t() @ x).numpy(), "db": dpre.sum(0).numpy()}


@pytest.mark.parametrize("name", [c.name for c in lr.CASES])
def test_a_correct_fp32_layer_passes_every_case(name):
    c = lr.BY_NAME[name]
    inp, ref = lr.case_data(name)
    got = torch_layer(c, inp, ref["y32"])
    worst = lr.check(c, ref, got)
    if c.kind == "value":
        a = ref["allow"]
        print(f"linear-cpu {name}: worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items())
              + f"; torch's own ulps fwd {a['fwd_ref']:.2f} bwd {a['bwd_ref']:.2f}")
        assert max(worst.values()) > 0  # the sums round: a value case is not an exact one
    if c.act == lr.NONE and c.M <= 3001:  # autograd differentiates the same thing
        x, W, b = (torch.from_numpy(inp[k]).clone().requires_grad_(True) for k in ("x", "W", "b"))
        F.linear(x, W, b).backward(torch.from_numpy(inp["dy"]))
        lr.check(c, ref, {"dx": x.grad.numpy(), "dW": W.grad.numpy(), "db": b.grad.numpy()}, which=("dx", "dW", "db"))


def test_the_table_reaches_every_instantiation_and_edge():
    def pad(d):
        t, p = (d + 15) // 16, 1
        while p < t:
            p *= 2
        return p

    inst = [c for c in lr.CASES if c.name.startswith("inst")]
    pairs = {(nt, kt) for nt in (1, 2, 4, 8) for kt in (1, 2, 4, 8)}
    assert {(pad(c.N), pad(c.K)) for c in inst} == pairs == {(pad(c.K), pad(c.N)) for c in inst}
    assert {(c.K + 15) // 16 for c in inst} == {1, 2, 3, 5, 8}  # 3 and 5 tiles are the padded ones
    assert all({lr.NONE, lr.RELU} == {d.act for d in inst if (d.K, d.N) == (c.K, c.N)} for c in inst)
    big = lr.BY_NAME["points-exact-M65553-K319-N256-relu"]
    chunks = min(256, big.M // 1024)
    assert 20 * 16 * chunks > 16384  # the cap on tiles x chunks of the weight-gradient launch is in force there
    assert max(c.M for c in lr.CASES) > 65536 and all(c.M <= 300 for c in lr.CASES if c.kind == "value")
    spread = [c for c in lr.CASES if c.spread]
    assert any(c.N == 1 and c.act == lr.SOFTPLUS for c in spread)
    for c in spread:
        pre = lr.case_data(c.name)[1]["pre"]
        assert pre.min() < -29 and pre.max() > 29 and ((pre > 20).any(axis=0) & (pre < -20).any(axis=0)).all()


def test_exact_cases_hold_entries_a_wrong_relu_mask_would_flip():
    ref = lr.case_data("inst-exact-M33-K17-N16-relu")[1]
    assert (ref["pre"] == 0).sum() > 5 and (ref["pre"] < 0).any() and (ref["pre"] > 0).any()


WRONG = [("drop_last_column", "inst-exact-M33-K17-N16-none", "y"),
         ("drop_last_column", "grid-value-M33-K319-N256-none", "y"),
         ("skip_last_ragged_row", "inst-exact-M33-K16-N16-none", "y"),
         ("bias_every_block", "grid-exact-M33-K130-N131-none", "y"),
         ("bias_every_block", "grid-value-M33-K319-N256-sigmoid", "y"),
         ("act_every_block", "grid-exact-M33-K319-N256-relu", "y"),
         ("act_every_block", "grid-value-M33-K130-N131-sigmoid", "y"),
         ("act_every_block", "grid-value-M33-K132-N132-softplus", "y"),
         ("dw_chunk_left_out", "points-exact-M2048-K27-N64-relu", "dW"),
         ("dw_chunk_left_out", "points-exact-M3001-K64-N3-none", "dW"),
         ("relu_mask_from_pre", "inst-exact-M33-K17-N16-relu", "dx"),
         ("softplus_grad_cancels", "act-value-M300-K24-N1-softplus", "dx")]


@pytest.mark.parametrize("variant,name,where", WRONG)
def test_a_wrong_layer_is_rejected_by_the_case_meant_to_catch_it(variant, name, where):
    c = lr.BY_NAME[name]
    inp, ref = lr.case_data(name)
    got = torch_layer(c, inp, ref["y32"], variant)
    with pytest.raises(AssertionError, match=f"{name} {where}"):
        lr.check(c, ref, got, which=(where,))
    if where != "y":  # and only through what it gets wrong
        lr.check(c, ref, got, which=("y",))


def test_function_allowance_is_the_references_figure_with_its_margin():
    for name in ("act-value-M300-K24-N40-sigmoid", "act-value-M300-K24-N1-softplus"):
        a = lr.case_data(name)[1]["allow"]
        print(f"linear-cpu {name}: torch fp32 ulps fwd {a['fwd_ref']:.2f} bwd {a['bwd_ref']:.2f} -> allowed {a['fwd']:.2f} {a['bwd']:.2f}")
        assert 0 < a["fwd_ref"] < 8 and 0 < a["bwd_ref"] < 8  # torch itself is a few ulp from float64
        assert a["fwd"] == max(4.0, 4 * a["fwd_ref"]) and a["bwd"] == max(4.0, 4 * a["bwd_ref"])
    assert lr.case_data("grid-value-M33-K130-N131-relu")[1]["allow"]["bwd"] == 0.0
    # ulp32 at the edges it is used at
    assert lr.ulp32(1.0) == 2.0 ** -23 and lr.ulp32(-0.75) == 2.0 ** -24 and lr.ulp32(0.0) == 2.0 ** -149
