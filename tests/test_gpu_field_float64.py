"""csrc/field_mlp.hip ENTRY BY ENTRY against the float64 reference of the main field's MLPs: nsamd_field_ray_terms,
nsamd_field_mlp_fwd and nsamd_field_mlp_bwd through the C ABI with raw pointers, so that the TEST chooses the branch of the host
code (plain or ray-terms kernels, density only, appearance from cameras / a constant row / absent, weight-gradient partials or
atomics, appearance gradient by per-tile rows / per-point rows / atomics), and nsamd_field_mlp_bwd_scatter (producer mode).
Reference, bounds and case table: tests/field_reference.py; tests/test_field_reference_cpu.py shows without a GPU that a correct
fp32 evaluation passes these bounds and that the defects they are meant for do not.

Every entry of every output goes through float64_check.check_entries: nothing is excluded (the case generator leaves no
undecided ReLU, asserted), a non-finite entry fails. Buffers the ABI says are WRITTEN (density, rgb, denc, ray_terms,
ray_inputs) start as NaN, the ACCUMULATED gradients as zeros; every output sits between sentinel margins that are checked after
the call (head layer 0's padded slots, the 3 -> 16 row padding of head layer 2 and the dead lanes of the last tile must not
reach them), the workspace starts as NaN, and the gradient rows of cameras no point uses must be exactly 0.

Each case prints, before it asserts, its worst |err| / bound per output (lines `field-f64 gpu ...`;
profiles/field_float64_ratios.txt keeps them next to the fp32 CPU evaluation's).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import field_reference as fr
from float64_check import check_entries

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 256
SENTINEL = -777.25
OK = 0


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


def _n():
    from nerfstudio_amd import _native as N

    return N


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded:
    """A device array between two sentinel margins."""

    def __init__(self, shape, fill):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * MARGIN,), SENTINEL, device=DEV)
        self.t = self.buf[MARGIN:MARGIN + self.n].view(*shape)
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32)).view(*shape))
        else:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:MARGIN] == SENTINEL).all()) and bool((self.buf[MARGIN + self.n:] == SENTINEL).all())

    def numpy(self):
        return self.t.cpu().numpy().copy()

    def bits(self):
        return self.t.view(torch.int32).clone()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Call:
    """The device inputs of one case and the three entry points on them."""

    def __init__(self, inp):
        self.inp, self.M, self.dg = inp, inp["M"], inp["dir_group"]
        self.R = inp["directions"].shape[0]
        self.ad = 32 if (inp["camera_indices"] is not None or inp["appearance_const"] is not None) else 0
        self.d = {k: _dev(inp[k]) for k in ("enc", "selector", "directions", "camera_indices", "appearance_const", "appearance",
                                            "ddensity", "drgb") + fr.W_KEYS}
        self.terms = self.inputs = None

    def mlp(self, with_terms):
        N, d = _n(), self.d
        m = N.FieldMlp(*(N.ptr(d[k]) for k in fr.W_KEYS), N.ptr(d["appearance"]), self.inp["num_images"], float(self.inp["avg"]))
        if with_terms:
            m.ray_terms, m.ray_inputs = N.ptr(self.terms.t), N.ptr(self.inputs.t)
        return m

    def ray_terms(self, keep_inputs=True):
        N, d = _n(), self.d
        self.terms = Guarded((self.R, 64), float("nan"))
        self.inputs = Guarded((self.R, 16 + self.ad), float("nan")) if keep_inputs else None
        s = N.load().nsamd_field_ray_terms(N.ptr(d["directions"]), N.ptr(d["camera_indices"]), N.ptr(d["appearance_const"]), self.R,
                                           self.mlp(False), N.ptr(self.terms.t), None if self.inputs is None else N.ptr(self.inputs.t),
                                           N.stream())
        torch.cuda.synchronize()
        assert s == OK, s
        assert self.terms.intact() and (self.inputs is None or self.inputs.intact()), "ray terms: a margin was written"
        got = {"ray_terms": self.terms.numpy()}
        if keep_inputs:
            got["ray_inputs"] = self.inputs.numpy()
        return got

    def forward(self, with_terms, rgb=True):
        N, d = _n(), self.d
        dens, col = Guarded((self.M,), float("nan")), Guarded((self.M, 3), float("nan")) if rgb else None
        s = N.load().nsamd_field_mlp_fwd(N.ptr(d["enc"]), N.ptr(d["selector"]), N.ptr(d["directions"]), N.ptr(d["camera_indices"]),
                                         N.ptr(d["appearance_const"]), self.dg, self.M, self.mlp(with_terms), N.ptr(dens.t),
                                         None if col is None else N.ptr(col.t), N.stream())
        torch.cuda.synchronize()
        assert s == OK, s
        assert dens.intact() and (col is None or col.intact()), "forward: a margin was written"
        got = {"density": dens.numpy()}
        if rgb:
            got["rgb"] = col.numpy()
        return got

    def grads(self, grad_app):
        g = {"d" + k: Guarded(self.inp[k].shape, 0.0) for k in fr.W_KEYS}
        if self.inp["camera_indices"] is not None and grad_app:
            g["dappearance"] = Guarded(self.inp["appearance"].shape, 0.0)
        g["denc"] = Guarded((32, self.M), float("nan"))
        return g

    def grads_struct(self, g):
        N = _n()
        return N.FieldMlpGrads(*(N.ptr(g["d" + k].t) for k in fr.W_KEYS), N.ptr(g["dappearance"].t) if "dappearance" in g else None)

    def workspace(self, floats):
        return None if floats == 0 else Guarded((floats,), float("nan"))

    def backward(self, with_terms, ws_floats, grad_app=True):
        """-> (outputs as numpy, their bits on the device)"""
        N, d = _n(), self.d
        g, ws = self.grads(grad_app), self.workspace(ws_floats)
        s = N.load().nsamd_field_mlp_bwd(N.ptr(d["enc"]), N.ptr(d["selector"]), N.ptr(d["directions"]), N.ptr(d["camera_indices"]),
                                         N.ptr(d["appearance_const"]), self.dg, self.M, self.mlp(with_terms), N.ptr(d["ddensity"]),
                                         N.ptr(d["drgb"]), N.ptr(g["denc"].t), self.grads_struct(g),
                                         None if ws is None else N.ptr(ws.t), ws_floats, N.stream())
        torch.cuda.synchronize()
        assert s == OK, s
        assert all(b.intact() for b in g.values()) and (ws is None or ws.intact()), "backward: a margin was written"
        assert np.array_equal(d["enc"].cpu().numpy(), self.inp["enc"])
        return {k: b.numpy() for k, b in g.items()}, {k: b.bits() for k, b in g.items()}


def _print_ratios(title, ref, got):
    """the worst |err| / bound per output, printed whether or not the assertion that follows holds"""
    line = []
    for k, g in got.items():
        err = np.abs(np.asarray(g, np.float64) - ref[k])
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / (ref["e_" + k] * (1 + 2.0 ** -6) + 2.0 ** -140))
        line.append(f"{k} {float(np.nanmax(ratio)) if np.isfinite(err).all() else float('inf'):.3f}")
    print(f"\n{title}: worst |err|/bound " + ", ".join(line))


def run_case(name):
    c = fr.BY_NAME[name]
    cus = _cus()
    inp, ref = fr.case_data(name, cus)
    assert int(ref["undecided"].sum()) == 0
    assert fr.expected_branch(c, cus) == c.expect, "the case's stated branch assumes this device's workgroup count"
    call = Call(inp)
    got = {}
    if c.ray_terms:
        got.update(call.ray_terms())
    got.update(call.forward(c.ray_terms))
    only = call.forward(c.ray_terms, rgb=False)
    back, _ = call.backward(c.ray_terms, fr.workspace_floats(c.workspace, c.M, cus), c.grad_app)
    got.update(back)
    _print_ratios(f"field-f64 gpu {fr.launch_note(c)}", ref, got)
    worst = {}
    check_entries("density (rgb == NULL)", only["density"], ref["density"], ref["e_density"], worst)
    assert np.array_equal(only["density"].view(np.int32), got["density"].view(np.int32)), "density alone: other bits than with rgb"
    fr.check(c, ref, got, worst)
    expect = set(fr.FORWARD_OUTPUTS + ("denc",) + fr.GRAD_KEYS)
    if c.app == "cams" and c.grad_app:
        expect.add("dappearance")
    if c.ray_terms:
        expect |= {"ray_terms", "ray_inputs"}
    assert set(got) == expect
    return worst


@pytest.mark.parametrize("name", [c.name for c in fr.TILE_EDGES])
def test_tile_edges(F, name):
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in fr.APP_SOURCES])
def test_appearance_sources(F, name):
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in fr.DIR_GROUPS])
def test_direction_groups_with_and_without_ray_terms(F, name):
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in fr.FORWARD_VARIANTS])
def test_selector_absent_and_with_zeros(F, name):
    c, (inp, ref) = fr.BY_NAME[name], fr.case_data(name, _cus())
    if c.selector == "zeros":  # a point with sel == 0 has density 0 and still carries its rgb gradient
        dead = inp["selector"] == 0
        assert dead.any() and (ref["density"][dead] == 0).all() and np.abs(ref["denc"][:, dead]).max() > 0
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in fr.WORKSPACES])
def test_backward_workspace_branches(F, name):
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in fr.SPREAD])
def test_trunc_exp_and_sigmoid_over_their_range(F, name):
    run_case(name)


@pytest.mark.parametrize("name", [c.name for c in fr.PERSISTENT])
def test_second_pass_of_the_persistent_workgroups(F, name):
    run_case(name)


@pytest.mark.parametrize("R,app,keep", fr.RAY_TERM_CASES)
def test_ray_terms(F, R, app, keep):
    inp = fr.draw_inputs(f"terms-{R}-{app}", R, 1, app)
    ref = fr.ray_terms64(inp)
    got = Call(inp).ray_terms(keep_inputs=keep)
    _print_ratios(f"field-f64 gpu ray terms R={R} {app}" + (" +inputs" if keep else ""), ref, got)
    worst = {}
    for k, g in got.items():
        assert g.shape == ref[k].shape
        check_entries(k, g, ref[k], ref["e_" + k], worst)


# ---- bit-level statements at small sizes -----------------------------------------------------------------------------------

def _same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


@pytest.mark.parametrize("M,dg,terms", [(17, 1, False), (96, 16, False), (96, 16, True), (272, 16, False), (272, 16, True)])
def test_two_backward_calls_on_the_workspace_path_give_the_same_bits(F, M, dg, terms):
    call = Call(fr.draw_inputs(f"bits-{M}-{dg}", M, dg, "cams"))
    if terms:
        call.ray_terms()
    ws = fr.workspace_floats("full", M, _cus())
    (_, a), (_, b) = call.backward(terms, ws), call.backward(terms, ws)
    assert _same_bits(a, b)
    assert float(a["dhead_W0"].view(torch.float32).abs().max()) > 0


@pytest.mark.parametrize("M", [17, 96, 272])
def test_inapplicable_ray_terms_do_not_change_a_bit(F, M):
    """dir_group 1: no 16-point tile lies inside one ray, so the plain kernels run whether or not terms are handed in. (With
    room for a row per point every sum has a fixed order; the appearance gradient by atomics, as dir_group 6 takes it, has not.)"""
    call = Call(fr.draw_inputs(f"bits-inapplicable-{M}", M, 1, "cams"))
    ws = fr.workspace_floats("full", M, _cus())
    f0, (_, b0) = call.forward(False), call.backward(False, ws)
    call.ray_terms()
    f1, (_, b1) = call.forward(True), call.backward(True, ws)
    only = call.forward(True, rgb=False)
    for k in f0:
        assert np.array_equal(f0[k].view(np.int32), f1[k].view(np.int32)), k
    assert np.array_equal(only["density"].view(np.int32), f0["density"].view(np.int32))
    assert _same_bits(b0, b1)


# ---- producer mode ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [17, 272])
def test_producer_mode_equals_the_plain_backward_and_the_table_scatter(F, M):
    """nsamd_field_mlp_bwd_scatter (16 levels, a 2^14 table, explicit positions): every MLP gradient and denc bit-equal to
    nsamd_field_mlp_bwd with the same workspace; its written table gradient and nsamd_hashgrid_encode_bwd_set of the plain call's
    denc both inside the per-entry bound of the float64 scatter of that denc (first-order rounding + the fixed-point truncation
    step of each call's own queue capacity, test_gpu_table_scatter._check)."""
    from oracle import nerfacto_oracle as orc
    from test_gpu_table_scatter import (_check, _level_steps, _plan, _positions, _producer_plan, _scatter, _workspace)

    N = _n()
    lib = N.load()
    L, log2_T = 16, 14
    case = _positions(F, L, 16, 2048, log2_T, M, 31 + M, N.XFORM_NONE)
    inp = fr.draw_inputs(f"producer-{M}", M, 1, "cams")
    table = torch.from_numpy((0.3 * np.random.RandomState(M).standard_normal((L << log2_T, 2))).astype(np.float32)).to(DEV)
    enc, sel = torch.empty(32, M, device=DEV), torch.empty(M, device=DEV)
    N.check(lib.nsamd_hashgrid_encode_fwd(case.pts, M, case.transform, case.box, N.ptr(table), case.spec.native(), N.ptr(enc), 1, M,
                                          N.ptr(sel), N.stream()), "hashgrid_encode_fwd")
    inp["enc"], inp["selector"] = enc.cpu().numpy(), sel.cpu().numpy()
    call = Call(inp)
    cus = _cus()
    ws_floats = fr.workspace_floats("full", M, cus)
    plain, plain_bits = call.backward(False, ws_floats)

    state = C.c_int64(0)
    words = int(lib.nsamd_field_mlp_bwd_scatter_workspace(case.spec.native(), M, C.byref(state)))
    pp = _producer_plan(case.scal, log2_T, M, cus)
    assert words > 0 and (words, int(state.value)) == (pp["words"], pp["state"]), "producer plan"
    sws = torch.empty(words, device=DEV)
    sws[:int(state.value)].zero_()
    g, ws = call.grads(True), call.workspace(ws_floats)
    dtable = Guarded((L << log2_T, 2), float("nan"))
    d = call.d
    s = lib.nsamd_field_mlp_bwd_scatter(case.pts, case.transform, case.box, case.spec.native(), N.ptr(d["enc"]), N.ptr(d["selector"]),
                                        N.ptr(d["directions"]), N.ptr(d["camera_indices"]), None, 1, M, call.mlp(False),
                                        N.ptr(d["ddensity"]), N.ptr(d["drgb"]), N.ptr(g["denc"].t), call.grads_struct(g), N.ptr(ws.t),
                                        ws_floats, N.ptr(dtable.t), N.ptr(sws), words, N.stream())
    torch.cuda.synchronize()
    assert s == OK, s
    assert all(b.intact() for b in g.values()) and ws.intact() and dtable.intact(), "producer mode: a margin was written"
    assert _same_bits({k: b.bits() for k, b in g.items()}, plain_bits)

    denc = torch.from_numpy(plain["denc"].T.copy())  # [M, 32]
    ref, ab, cnt = orc.hashgrid_scatter64(case.x, denc, torch.tensor(case.scal), case.T)
    steps, c1 = _level_steps(case, denc, Q=pp["caps"])
    worst_p = _check(f"producer M={M}", case, dtable.t, ref, ab, cnt, steps, c1)
    out = torch.full((L << log2_T, 2), float("nan"), device=DEV)
    _scatter(F, case, torch.from_numpy(plain["denc"]).to(DEV), 1, M, out, True, _workspace(F, case, True))
    torch.cuda.synchronize()
    steps2, c12 = _level_steps(case, denc, Q=_plan(case.scal, log2_T, M, True)["caps"])
    worst_s = _check(f"encode_bwd_set M={M}", case, out, ref, ab, cnt, steps2, c12)
    print(f"\nfield-f64 gpu producer M={M}: table gradient worst |err|/bound {worst_p:.3f} (nsamd_hashgrid_encode_bwd_set of the "
          f"same denc: {worst_s:.3f})")
