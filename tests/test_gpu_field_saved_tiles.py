"""The main-field backward on the forward's saved tile (include/nsamd.h, nsamd_field_mlp.saved_hb / saved_rgb) and the one-k-step
form of head layer 2's data gradient (csrc/field_mlp.hip, rows_gemm_bwd_rgb), through the C ABI with raw pointers.

1. nsamd_field_mlp_fwd with and without the buffer: density and rgb bit-equal; the stored tile, read back in the chain layout
   (lane (j, g) of tile T, register (t, r) = feature 16 t + 4 g + r of sample 16 T + j), inside the forward's bound of
   tests/field_reference.py against the float64 layers; the absent samples of a partial last tile stay as the caller zeroed them.
2. nsamd_field_mlp_bwd and nsamd_field_mlp_bwd_scatter with the saved tile against the same call with null pointers on the same
   inputs: EVERY output bit-equal (ten parameter gradients, denc, the appearance table's gradient, the written table gradient).
   The forward forms the tile with the operations of the backward's recomputation in the same order, so equality of bits is the
   statement; head layer 2's weight gradient is Dout^T X with X = the tile, so it is also the check that the tiles are equal.
3. Shapes: M = 96 (two rays of 48, ray terms), M = 40 (plain kernel, 8 live samples in the last tile), M = 16 (one tile, seven idle
   waves of the workgroup), 48 x 700 (more tiles than 256 CUs x 8 waves: a second pass of the persistent workgroups, records of
   tile k leaving during tile k + 1); appearance embedding on and off.
4. Head layer 2's data gradient issues the one k-step that holds its three outputs: the null-pointer arm's outputs are bit-equal
   to the values the kernels had before that change (tests/golden/field_bwd_bits_before_saved_tiles.json: SHA-256 of every
   output's bytes, recorded with the parent commit's library on the cases whose launch geometry does not depend on the device's CU
   count) and inside the float64 bounds of tests/field_reference.py.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import field_reference as fr
from float64_check import check_entries
from test_gpu_field_float64 import DEV, OK, Call, Guarded, _cus, _n, _same_bits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_bwd_bits_before_saved_tiles.json")

# (M, dir_group, ray terms, appearance)
SHAPES = [(96, 48, True, "cams"), (96, 48, True, "none"), (40, 1, False, "cams"), (40, 1, False, "none"), (16, 16, True, "cams"),
          (16, 1, False, "cams"), (48 * 700, 48, True, "cams")]
SMALL = [s for s in SHAPES if s[0] <= 96]  # one backward workgroup on any device


def _id(s):
    return f"M{s[0]}-g{s[1]}-{'rt' if s[2] else 'plain'}-{s[3]}"


def case_inputs(shape):
    M, dg, _, app = shape
    return fr.draw_inputs("saved-" + _id(shape), M, dg, app)


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


class SavedCall(Call):
    """Call whose nsamd_field_mlp carries the saved tile once `save()` has allocated it."""

    def __init__(self, inp):
        super().__init__(inp)
        self.hb = self.rgb = None
        self.use_saved = False

    def save(self):
        self.hb = Guarded(((self.M + 15) // 16, 4, 64, 4), 0.0)
        self.use_saved = True

    def mlp(self, with_terms):
        N = _n()
        m = super().mlp(with_terms)
        if self.use_saved:
            m.saved_hb = N.ptr(self.hb.t)
            m.saved_rgb = None if self.rgb is None else N.ptr(self.rgb)
        return m

    def tile_by_sample(self):
        """-> hb [16 tiles, 64] read back from the chain layout"""
        tiles = (self.M + 15) // 16
        return self.hb.numpy().reshape(tiles, 4, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(tiles * 16, 64)  # [T][t][g][j][r]


def forward_both(shape):
    """-> (call with the saved tile of its forward, outputs without the buffer, outputs with it)"""
    call = SavedCall(case_inputs(shape))
    if shape[2]:
        call.ray_terms()
    plain = call.forward(shape[2])
    call.save()
    saved = call.forward(shape[2])
    assert call.hb.intact(), "saved tile: a margin was written"
    call.rgb = torch.from_numpy(saved["rgb"]).to(DEV)
    return call, plain, saved


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_forward_stores_the_tile_and_leaves_its_outputs_alone(F, shape):
    call, plain, saved = forward_both(shape)
    for k in ("density", "rgb"):
        assert np.array_equal(plain[k].view(np.int32), saved[k].view(np.int32)), k
    M = shape[0]
    ref = fr.forward64(call.inp)
    hb = call.tile_by_sample()
    worst = {}
    check_entries("saved_hb", hb[:M], ref["hb"], ref["e_hb"], worst)
    print(f"\nfield saved tile {_id(shape)}: worst |err|/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not hb[M:].any(), "the absent samples of the last tile were written"
    assert float(np.abs(hb[:M]).max()) > 0
    # density only: nothing is stored (the head is not evaluated)
    call.hb.t.zero_()
    only = call.forward(shape[2], rgb=False)
    assert np.array_equal(only["density"].view(np.int32), plain["density"].view(np.int32))
    assert not call.hb.t.any()


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_backward_on_the_saved_tile_equals_the_recomputing_backward(F, shape):
    call, _, _ = forward_both(shape)
    ws = fr.workspace_floats("full", shape[0], _cus())
    call.use_saved = False
    _, null_bits = call.backward(shape[2], ws)
    call.use_saved = True
    _, saved_bits = call.backward(shape[2], ws)
    assert _same_bits(null_bits, saved_bits), [k for k in null_bits if not torch.equal(null_bits[k], saved_bits[k])]
    assert float(saved_bits["dhead_W2"].view(torch.float32).abs().max()) > 0
    # one of the two pointers: the recomputing kernels
    call.rgb = None
    _, partial_bits = call.backward(shape[2], ws)
    assert _same_bits(null_bits, partial_bits)


def _producer(call, case, with_terms, ws_floats, words, state_words):
    """nsamd_field_mlp_bwd_scatter -> the bits of every output, the table gradient among them"""
    N = _n()
    lib, d = N.load(), call.d
    L, log2_T = case.L, case.log2_T
    sws = torch.empty(words, device=DEV)
    sws[:state_words].zero_()
    g, ws = call.grads(True), call.workspace(ws_floats)
    dtable = Guarded((L << log2_T, 2), float("nan"))
    s = lib.nsamd_field_mlp_bwd_scatter(case.pts, case.transform, case.box, case.spec.native(), N.ptr(d["enc"]), N.ptr(d["selector"]),
                                        N.ptr(d["directions"]), N.ptr(d["camera_indices"]), None, call.dg, call.M,
                                        call.mlp(with_terms), N.ptr(d["ddensity"]), N.ptr(d["drgb"]), N.ptr(g["denc"].t),
                                        call.grads_struct(g), N.ptr(ws.t), ws_floats, N.ptr(dtable.t), N.ptr(sws), words, N.stream())
    torch.cuda.synchronize()
    assert s == OK, s
    assert all(b.intact() for b in g.values()) and ws.intact() and dtable.intact(), "producer mode: a margin was written"
    bits = {k: b.bits() for k, b in g.items()}
    bits["dtable"] = dtable.bits()
    return bits


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_producer_mode_on_the_saved_tile_equals_the_recomputing_one(F, shape):
    """The record-emitting backward (16 levels, a 2^14 table, explicit positions): MLP gradients, denc and the WRITTEN table
    gradient with the saved tile bit-equal to the same call with null pointers, and its MLP gradients to the plain entry point's."""
    from test_gpu_table_scatter import _positions

    N = _n()
    M = shape[0]
    case = _positions(F, 16, 16, 2048, 14, M, 77 + M, N.XFORM_NONE)
    call, _, _ = forward_both(shape)
    ws = fr.workspace_floats("full", M, _cus())
    state = C.c_int64(0)
    words = int(N.load().nsamd_field_mlp_bwd_scatter_workspace(case.spec.native(), M, C.byref(state)))
    assert words > 0
    call.use_saved = False
    null_bits = _producer(call, case, shape[2], ws, words, int(state.value))
    call.use_saved = True
    saved_bits = _producer(call, case, shape[2], ws, words, int(state.value))
    assert _same_bits(null_bits, saved_bits), [k for k in null_bits if not torch.equal(null_bits[k], saved_bits[k])]
    assert float(saved_bits["dtable"].view(torch.float32).abs().max()) > 0
    _, plain_bits = call.backward(shape[2], ws)
    assert _same_bits({k: v for k, v in saved_bits.items() if k != "dtable"}, plain_bits)


def digests(bits):
    return {k: hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for k, v in sorted(bits.items())}


@pytest.mark.parametrize("shape", SMALL, ids=_id)
def test_head_layer_2_one_k_step_gives_the_bits_of_the_sixteen_step_form(F, shape):
    M, dg, terms, app = shape
    cus = _cus()
    call = SavedCall(case_inputs(shape))
    if terms:
        call.ray_terms()
    ws = fr.workspace_floats("full", M, cus)
    got, bits = call.backward(terms, ws)
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert digests(bits) == golden[_id(shape)], "the recomputing backward no longer gives the bits it gave with 16 MFMAs in head layer 2"
    # ... and those are inside the float64 bounds (the case's branch: the bounds' summation chains)
    c = fr.Case("saved-" + _id(shape), M, dg, app, terms, "values", "full", 8 if app == "cams" else 0, True, None, None)
    c = c._replace(expect=fr.expected_branch(c, cus))
    ref = fr.reference_of(c, call.inp, cus)
    worst = fr.check(c, ref, got, {})
    print(f"\nfield head-2 k-step {_id(shape)} [{c.expect}]: worst |err|/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
