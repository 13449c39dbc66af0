"""nsamd_linear_fwd / nsamd_linear_bwd (csrc/linear.hip) ENTRY BY ENTRY against the float64 reference of one dense layer, through
the C ABI with raw pointers — as nerfstudio_amd/eval_render.py drives the predicted-normals MLP and functional._LinearFn the
stand-alone MLP and vanilla-nerf. Reference, bounds and case table: tests/linear_reference.py (tests/test_linear_reference_cpu.py
shows, without a GPU, that a correct fp32 layer passes them and that wrong ones do not).

  1. every instantiation linear_chain_kernel<NT, KT, TRANSPOSED>, exact;      4. activations over pre in [-30, 30], value;
  2. the grid of 128 x 128 blocks, exact and value;                          5. the ABI contract;
  3. point-count edges up to 65 553 (grid-stride loop, dW chunks), exact;     6. isolation of a NaN, untouched margins.

Exact cases: the result EQUALS the float64 one (integers; any summation order). Value cases: |got - ref| <= 2 (T + 2) u A + f
per entry; f is 4 x what torch's fp32 CPU functions achieve against float64 on the same pre-activations (at least 4 ulp) plus
the derived effect of handing the backward an fp32 y. No tolerance here comes from a kernel's output. Every output lies in a
buffer with a sentinel margin of MARGIN floats on both sides, y and dx are pre-filled with NaN, and `forward` / `backward`
assert after every call that the margins (and the inputs) are untouched.

Every value test prints, before it asserts, its largest error / bound per quantity and, for Sigmoid / Softplus, the ulp figures
(lines `linear-f64 ...`): torch's fp32 CPU figure, the allowance derived from it, and what of the kernel's error the allowance
has to cover. The reference's figures (from tests/test_linear_reference_cpu.py, which needs no GPU): forward 1.0 - 2.3 ulp,
derivative 0.4 - 2.1 ulp over all cases, so the kernel is allowed 4.0 - 9.3 ulp. On MI355X the
kernels' largest error / bound over all value cases is 0.20 for y, 0.50 for dx, 0.26 for dW and 0.09 for db, and in every
Sigmoid / Softplus case the part of the forward's error above the summation term is 0.00 ulp: the function allowance is not
drawn on.
"""
import numpy as np
import pytest
import torch

import linear_reference as lr

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 64          # floats = 256 B: the payload keeps the 16-byte alignment of the allocation
SENTINEL = -777.25
OK, INVALID = 0, -1


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


def _n():
    from nerfstudio_amd import _native as N

    return N


class Guarded:
    """A device array in the middle of a sentinel-filled buffer; `shift` floats off the 16-byte alignment."""

    def __init__(self, shape, fill=None, shift=0):
        self.n = int(np.prod(shape))
        self.lo = MARGIN + shift
        self.buf = torch.full((self.n + 2 * MARGIN + shift,), SENTINEL, device=DEV)
        self.t = self.buf[self.lo:self.lo + self.n].view(*shape)
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32)).view(*shape))
        elif fill is not None:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == (4 * shift) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.lo + self.n:] == SENTINEL).all())

    def numpy(self):
        return self.t.cpu().numpy().copy()


def _ptr(g):
    return None if g is None else _n().ptr(g.t)


def forward(c, inp, bias=True, shift_x=0, shift_y=0, status=OK):
    N = _n()
    x, W, b = Guarded((c.M, c.K), inp["x"], shift_x), Guarded((c.N, c.K), inp["W"]), Guarded((c.N,), inp["b"])
    y = Guarded((c.M, c.N), float("nan"), shift_y)
    s = N.load().nsamd_linear_fwd(_ptr(x), _ptr(W), _ptr(b) if bias else None, c.M, c.K, c.N, c.act, _ptr(y), N.stream())
    torch.cuda.synchronize()
    assert s == status, (c.name, s)
    assert all(g.intact() for g in (x, W, b, y)), f"{c.name}: a margin was written"
    assert np.array_equal(x.numpy(), inp["x"], equal_nan=True) and np.array_equal(W.numpy(), inp["W"])
    return y.numpy()


def backward(c, inp, y32, want="xWb", init_dW=None, init_db=None, shift_y=0, shift_dy=0, shift_dx=0):
    """-> dict of the requested gradients ("x" dx, "W" dW, "b" db); the others are passed as NULL. dW / db start from
    `init_*` (zeros by default), dx from NaN."""
    N = _n()
    x, W = Guarded((c.M, c.K), inp["x"]), Guarded((c.N, c.K), inp["W"])
    y, dy = Guarded((c.M, c.N), y32, shift_y), Guarded((c.M, c.N), inp["dy"], shift_dy)
    dx = Guarded((c.M, c.K), float("nan"), shift_dx) if "x" in want else None
    dW = Guarded((c.N, c.K), 0.0 if init_dW is None else init_dW) if "W" in want else None
    db = Guarded((c.N,), 0.0 if init_db is None else init_db) if "b" in want else None
    s = N.load().nsamd_linear_bwd(_ptr(x), _ptr(W), _ptr(y), _ptr(dy), c.M, c.K, c.N, c.act, _ptr(dx), _ptr(dW), _ptr(db),
                                  N.stream())
    torch.cuda.synchronize()
    assert s == OK, (c.name, s)
    assert all(g.intact() for g in (x, W, y, dy, dx, dW, db) if g is not None), f"{c.name}: a margin was written"
    assert np.array_equal(y.numpy(), y32, equal_nan=True) and np.array_equal(dy.numpy(), inp["dy"], equal_nan=True)
    return {k: g.numpy() for k, g in (("dx", dx), ("dW", dW), ("db", db)) if g is not None}


def run_case(name):
    """Forward and full backward of a case of the table, checked; -> (case, inputs, reference, got)."""
    c = lr.BY_NAME[name]
    inp, ref = lr.case_data(name)
    got = {"y": forward(c, inp)}
    got.update(backward(c, inp, ref["y32"]))
    if c.kind == "value":  # printed before anything is asserted
        ratios = {k: float(np.nanmax(np.abs(got[k].astype(np.float64) - ref[k]) / np.maximum(ref["bound_" + k], 2.0 ** -1000)))
                  for k in ("y", "dx", "dW", "db")}
        line = f"linear-f64 {name}: error / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items())
        if c.act in (lr.SIGMOID, lr.SOFTPLUS):
            a, k = ref["allow"], lr.function_ulps(c, ref, got)
            line += (f"; ulps forward: torch {a['fwd_ref']:.2f} allowed {a['fwd']:.2f} kernel {k['fwd']:.2f}; derivative: torch "
                     f"{a['bwd_ref']:.2f} allowed {a['bwd']:.2f}" + ("" if k["bwd"] is None else f" kernel {k['bwd']:.2f}"))
        print(line)
    lr.check(c, ref, got)
    return c, inp, ref, got


# ---------------------------------------------------------------- 1 - 4: the table --------------------------------------

@pytest.mark.parametrize("name", [c.name for c in lr.INSTANTIATIONS])
def test_every_instantiation_is_exact(F, name):
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in lr.BLOCK_GRID])
def test_block_grid_exact_and_value(F, name):
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in lr.POINT_EDGES])
def test_point_count_edges_are_exact(F, name):
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in lr.ACTIVATIONS])
def test_activations_over_the_whole_range(F, name):
    """Pre-activations over [-30, 30]: both Softplus branches, the saturated Sigmoid. With N = 1, dx[p, :] = dpre[p] W[0, :] is
    one product and its bound is 6 u |dx| + f: the derivative is checked RELATIVELY, down to v = -30 (act' = 9e-14).

    In ulps of the float64 result, torch fp32 CPU -> allowed (max(4, 4 x)): Sigmoid N = 40 forward 2.32 -> 9.30, derivative
    1.39 -> 5.57; Softplus N = 40 1.34 -> 5.36, 2.07 -> 8.28; Softplus N = 1 1.07 -> 4.26, 1.41 -> 5.63; Sigmoid N = 1
    1.29 -> 5.15, 0.75 -> 4.00. act_grad's Softplus is -expm1f(-y): the 1 - expf(-y) it replaces has an absolute error of
    2^-24 on a value of y, i.e. 2^-24 / y relative — 150 ulp at v = -5, everything by v = -17 (restated on the CPU as the
    variant `softplus_grad_cancels`, which this case rejects). On MI355X: the part of the kernel's error
    that the allowance has to cover is 0.00 ulp in all four forwards and in the Softplus N = 1 derivative; the largest relative error of dx over
    v < -5 in the Softplus N = 1 case is 1.56e-7 (2.6 u, bound 19 u). With 1 - expf(-y) the same case had 3069 of 7200 entries
    of dx outside, the worst 0.0 for 4.9e-13, and grid-value-M33-K129-N5-softplus 9 of 4257, the worst 3.55 x its bound."""
    c, inp, ref, got = run_case(name)
    if c.N == 1 and c.act == lr.SOFTPLUS:
        rel = np.abs(got["dx"].astype(np.float64) - ref["dx"]) / np.abs(ref["dx"])
        low = ref["pre"][:, 0] < -5
        assert low.sum() > 100 and ref["pre"].min() < -29.5
        print(f"linear-f64 {name}: largest relative error of dx over pre < -5: {rel[low].max():.3e}")
        assert rel[low].max() <= (6 + 2 * ref["allow"]["bwd"] + 2) * lr.U  # the bound itself, in relative form (ulp <= 2 u |v|)


# ---------------------------------------------------------------- 5: contract -------------------------------------------

@pytest.mark.parametrize("name", ["grid-exact-M33-K130-N131-relu", "points-exact-M3001-K27-N64-relu"])
def test_dw_and_db_accumulate_and_each_gradient_alone_gives_the_same_bits(F, name):
    c = lr.BY_NAME[name]
    inp, ref = lr.case_data(name)
    together = backward(c, inp, ref["y32"])
    lr.check(c, ref, together, which=("dx", "dW", "db"))
    rs = np.random.RandomState(3)
    init_dW, init_db = (rs.randint(-100, 101, s).astype(np.float32) for s in ((c.N, c.K), (c.N,)))
    acc = backward(c, inp, ref["y32"], init_dW=init_dW, init_db=init_db)
    assert np.array_equal(acc["dW"], init_dW + together["dW"]) and np.array_equal(acc["db"], init_db + together["db"])
    assert np.array_equal(acc["dx"], together["dx"])
    for want, key in (("x", "dx"), ("W", "dW"), ("b", "db")):
        alone = backward(c, inp, ref["y32"], want=want)
        assert list(alone) == [key]
        assert np.array_equal(alone[key].view(np.int32), together[key].view(np.int32)), f"{key} alone"
    both = backward(c, inp, ref["y32"], want="xb", init_db=init_db)  # what a frozen weight with a trained bias asks for
    assert np.array_equal(both["db"], init_db + together["db"]) and np.array_equal(both["dx"], together["dx"])


def test_a_single_chunk_value_case_alone_and_together(F):
    """M = 300 is one chunk: one atomic addition per dW entry, so the value case is deterministic too."""
    c = lr.BY_NAME["act-value-M300-K24-N40-sigmoid"]
    inp, ref = lr.case_data(c.name)
    together = backward(c, inp, ref["y32"])
    for want, key in (("x", "dx"), ("W", "dW"), ("b", "db")):
        assert np.array_equal(backward(c, inp, ref["y32"], want=want)[key].view(np.int32), together[key].view(np.int32)), key


def test_forward_without_a_bias(F):
    for name in ("grid-exact-M33-K130-N131-relu", "grid-value-M33-K319-N256-sigmoid"):
        c = lr.BY_NAME[name]
        inp = lr.case_data(name)[0]
        ref = lr.reference_of(c, inp, bias=False)
        lr.check(c, ref, {"y": forward(c, inp, bias=False)}, which=("y",))


def test_no_points_is_ok_and_writes_nothing_and_bad_arguments_are_refused(F):
    N = _n()
    lib = N.load()
    c = lr.BY_NAME["inst-exact-M33-K17-N16-relu"]
    inp, ref = lr.case_data(c.name)
    g = {k: Guarded(s, SENTINEL) for k, s in (("x", (33, 17)), ("W", (16, 17)), ("b", (16,)), ("y", (33, 16)), ("dy", (33, 16)),
                                                ("dx", (33, 17)), ("dW", (16, 17)), ("db", (16,)))}
    p = {k: _ptr(v) for k, v in g.items()}

    def untouched():
        torch.cuda.synchronize()
        return all(bool((v.buf == SENTINEL).all()) for v in g.values())

    assert lib.nsamd_linear_fwd(p["x"], p["W"], p["b"], 0, 17, 16, 1, p["y"], N.stream()) == OK
    assert lib.nsamd_linear_bwd(p["x"], p["W"], p["y"], p["dy"], 0, 17, 16, 1, p["dx"], p["dW"], p["db"], N.stream()) == OK
    assert untouched()
    for K, Nn, act in ((0, 16, 1), (-1, 16, 1), (17, 0, 1), (17, -3, 1), (17, 16, 4), (17, 16, -1)):
        assert lib.nsamd_linear_fwd(p["x"], p["W"], p["b"], 33, K, Nn, act, p["y"], N.stream()) == INVALID, (K, Nn, act)
        assert lib.nsamd_linear_bwd(p["x"], p["W"], p["y"], p["dy"], 33, K, Nn, act, p["dx"], p["dW"], p["db"],
                                    N.stream()) == INVALID, (K, Nn, act)
    assert lib.nsamd_linear_fwd(p["x"], p["W"], p["b"], -1, 17, 16, 1, p["y"], N.stream()) == INVALID
    assert untouched()
    # and the same pointers with valid arguments do run (the refusals above were about the arguments)
    lr.check(c, ref, {"y": forward(c, inp)}, which=("y",))


@pytest.mark.parametrize("name", [c.name for c in lr.ALIGNMENT])
def test_base_pointers_one_float_off_alignment_give_the_same_bits(F, name):
    """K and N multiples of 4 (row strides keep the alignment), bases 4 bytes off: the kernels have to take their scalar paths
    for x / y (forward) and dy / y / dx (backward). 132 = one full block plus a 4-wide one; 64 -> 16 is a single launch."""
    c = lr.BY_NAME[name]
    inp, ref = lr.case_data(name)
    bits = lambda a: a.view(np.int32)  # noqa: E731
    y = forward(c, inp)
    lr.check(c, ref, {"y": y}, which=("y",))
    for sx, sy in ((1, 0), (0, 1), (1, 1), (3, 2)):
        assert np.array_equal(bits(forward(c, inp, shift_x=sx, shift_y=sy)), bits(y)), (sx, sy)
    g = backward(c, inp, ref["y32"])
    lr.check(c, ref, g, which=("dx", "dW", "db"))
    for sy, sdy, sdx in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (2, 3, 1)):
        h = backward(c, inp, ref["y32"], shift_y=sy, shift_dy=sdy, shift_dx=sdx)
        assert all(np.array_equal(bits(h[k]), bits(g[k])) for k in ("dx", "dW", "db")), (sy, sdy, sdx)


# ---------------------------------------------------------------- 6: isolation ------------------------------------------

def test_a_nan_stays_in_its_row_and_in_the_dw_entries_it_feeds(F):
    """No activation (a NaN through a linear map is unambiguous), M = 33: point 32 is the one the dead lanes of the last tile
    are clamped to. x[32, 5] = NaN: row 32 of y, column 5 of dW. dy[32, 3] = NaN: row 32 of dx, row 3 of dW, db[3]. Every
    other entry keeps the bits of the clean run."""
    c = lr.BY_NAME["inst-exact-M33-K40-N17-none"]
    inp, ref = lr.case_data(c.name)
    clean = {"y": forward(c, inp)}
    clean.update(backward(c, inp, ref["y32"]))
    lr.check(c, ref, clean)
    p0, k0, n0 = 32, 5, 3
    bad_x = dict(inp, x=inp["x"].copy())
    bad_x["x"][p0, k0] = np.nan
    bad_dy = dict(inp, dy=inp["dy"].copy())
    bad_dy["dy"][p0, n0] = np.nan

    def only(got, clean_arr, rows=None, cols=None):
        mask = np.zeros(clean_arr.shape, bool)
        if rows is not None:
            mask[rows] = True
        if cols is not None:
            mask[:, cols] = True
        assert np.array_equal(~np.isfinite(got), mask), "the non-finite entries are not the ones the NaN feeds"
        assert np.array_equal(got[~mask].view(np.int32), clean_arr[~mask].view(np.int32))

    only(forward(c, bad_x), clean["y"], rows=p0)
    g = backward(c, bad_x, ref["y32"])
    only(g["dW"], clean["dW"], cols=k0)
    assert np.array_equal(g["dx"], clean["dx"]) and np.array_equal(g["db"], clean["db"])  # neither reads x
    g = backward(c, bad_dy, ref["y32"])
    only(g["dx"], clean["dx"], rows=p0)
    only(g["dW"], clean["dW"], rows=n0)
    only(g["db"], clean["db"], rows=n0)


# ---------------------------------------------------------------- the autograd wrapper on top ---------------------------

def test_linear_under_autograd_asks_for_the_bias_gradient_alone(F):
    """functional.linear with a frozen weight and a trained bias: nsamd_linear_bwd gets dW == NULL, db != NULL."""
    c = lr.BY_NAME["points-exact-M3001-K27-N64-relu"]
    inp, ref = lr.case_data(c.name)
    x, W, dy = (torch.from_numpy(inp[k]).to(DEV) for k in ("x", "W", "dy"))
    b = torch.from_numpy(inp["b"]).to(DEV).requires_grad_(True)
    y = F.linear(x, W, b, "relu")
    y.backward(dy)
    assert W.grad is None
    lr.check(c, ref, {"y": y.detach().cpu().numpy(), "db": b.grad.cpu().numpy()}, which=("y", "db"))
