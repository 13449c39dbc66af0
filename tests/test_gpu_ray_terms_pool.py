"""nsamd_field_ray_terms with a batch pool (include/nsamd.h, nsamd_field_mlp.batch_slot / batch_slots): the main field's per-ray
terms for a batch that still lies in the pool of batches, against nsamd_select_batch followed by the plain call — the same
rows read, the same arithmetic, so `ray_terms` and `ray_inputs` must be the same BITS. trainer.HipTrainer launches it on the Adam branch of a captured iteration, where it
no longer waits for the launch that selects the batch.

Sizes: 1 / 15 / 16 / 17 rays (one ragged 16-ray tile, one exact tile, one ray past it) and 257 (17 tiles: five workgroups of 4
waves, the last with one wave at work on a one-ray tile); 1 and 3 slots; the slot -1, 0, slots - 1 and slots, so both clamps
are taken; the appearance row from the cameras' table, one constant row, or none; `ray_inputs` kept or NULL. Pools and outputs lie between NaN guards: a
read outside the selected slot's rows that reaches the result, or a write outside the outputs, shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64  # floats / indices of guard on either side of a buffer


def _guarded(x, fill):
    """-> (the buffer with GUARD elements of `fill` on either side, the view of `x`'s place in it holding `x`)."""
    flat = torch.full((x.numel() + 2 * GUARD,), fill, dtype=x.dtype, device="cuda")
    inner = flat[GUARD:GUARD + x.numel()].view(x.shape)
    inner.copy_(x)
    return flat, inner


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guards_untouched(flat):
    return bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("num_rays", [1, 15, 16, 17, 257])
def test_pool_ray_terms_are_the_bits_of_selection_then_the_plain_call(num_rays, slots):
    from nerfstudio_amd import _native as N

    lib, st = N.load(), N.stream()
    rs = np.random.RandomState(1000 * num_rays + slots)
    ncam, R = 5, num_rays
    g = lambda *shape, s=1.0: torch.from_numpy((rs.standard_normal(shape) * s).astype(np.float32)).cuda()  # noqa: E731
    emb, app_row = g(ncam + 1, 32), g(32)
    emb[ncam] = float("nan")  # the row the cameras' guards name: a camera index read outside the slot's rows shows as NaN
    d = g(slots, R, 3)
    d = (d / d.norm(dim=-1, keepdim=True)).contiguous()
    dirs_flat, dirs_pool = _guarded(d, float("nan"))
    cams_flat, cams_pool = _guarded(torch.from_numpy(rs.randint(0, ncam, (slots, R)).astype(np.int64)).cuda(), ncam)
    orig_pool, tgt_pool = g(slots, R, 3), g(slots, R, 3)
    for appearance in ("cameras", "const", "none"):
        k0 = 31 if appearance == "none" else 63
        prm = [g(64, 32, s=0.3), g(64, s=0.1), g(16, 64, s=0.2), g(16, s=0.1), g(64, k0, s=0.2), g(64, s=0.1), g(64, 64, s=0.2),
               g(64, s=0.1), g(3, 64, s=0.2), g(3, s=0.1)]
        table = emb if appearance == "cameras" else None
        fm = N.FieldMlp(*(N.ptr(p) for p in prm), N.ptr(table), ncam + 1 if table is not None else 0, 1.0)
        app_const = app_row if appearance == "const" else None
        width = 16 + (0 if appearance == "none" else 32)
        for slot_value in (-1.0, 0.0, float(slots - 1), float(slots)):
            slot = torch.tensor([slot_value], device="cuda")
            k = min(max(int(slot_value), 0), slots - 1)
            # the record: the selection's copy of the slot's rows, then the plain call on it
            o, dd, t = (torch.empty(R, 3, device="cuda") for _ in range(3))
            c = torch.empty(R, dtype=torch.int64, device="cuda")
            N.check(lib.nsamd_select_batch(N.ptr(slot), slots, R, N.ptr(orig_pool), N.ptr(dirs_pool), N.ptr(cams_pool),
                                           N.ptr(tgt_pool), N.ptr(o), N.ptr(dd), N.ptr(c), N.ptr(t), st), "select_batch")
            assert torch.equal(dd, dirs_pool[k]) and torch.equal(c, cams_pool[k])
            want_terms, want_in = torch.empty(R, 64, device="cuda"), torch.empty(R, width, device="cuda")
            N.check(lib.nsamd_field_ray_terms(N.ptr(dd), N.ptr(c) if table is not None else None, N.ptr(app_const), R, fm,
                                              N.ptr(want_terms), N.ptr(want_in), st), "field_ray_terms")
            assert bool(torch.isfinite(want_terms).all()) and bool(torch.isfinite(want_in).all())
            for keep_inputs in (True, False):
                terms_flat, terms = _guarded(torch.full((R, 64), float("nan")), float("nan"))
                in_flat, xin = _guarded(torch.full((R, width), float("nan")), float("nan"))
                fm.batch_slot, fm.batch_slots = N.ptr(slot), slots
                N.check(lib.nsamd_field_ray_terms(N.ptr(dirs_pool), N.ptr(cams_pool) if table is not None else None,
                                                  N.ptr(app_const), R, fm, N.ptr(terms), N.ptr(xin) if keep_inputs else None, st),
                        "field_ray_terms (pool)")
                fm.batch_slot, fm.batch_slots = None, 0
                torch.cuda.synchronize()
                what = (num_rays, slots, appearance, slot_value, keep_inputs)
                assert torch.equal(_bits(terms), _bits(want_terms)), what
                if keep_inputs:
                    assert torch.equal(_bits(xin), _bits(want_in)), what
                else:
                    assert bool(torch.isnan(xin).all()), what
                assert _guards_untouched(terms_flat) and _guards_untouched(in_flat), what
    assert _guards_untouched(dirs_flat) and bool((cams_flat[:GUARD] == ncam).all()) and bool((cams_flat[-GUARD:] == ncam).all())


def test_pool_ray_terms_refuse_a_pool_without_its_slot():
    """Nothing is launched (the outputs keep their fill) for a pool without `slot_dev` or with `slots` <= 0; zero rays are
    accepted as in the plain call."""
    from nerfstudio_amd import _native as N

    lib, st = N.load(), N.stream()
    R, slots = 17, 3
    g = lambda *shape: torch.randn(*shape, device="cuda")  # noqa: E731
    prm = [g(64, 32), g(64), g(16, 64), g(16), g(64, 31), g(64), g(64, 64), g(64), g(3, 64), g(3)]
    fm = N.FieldMlp(*(N.ptr(p) for p in prm), None, 0, 1.0)
    dirs, slot = g(slots, R, 3), torch.zeros(1, device="cuda")
    terms = torch.full((R, 64), -7.0, device="cuda")

    def call(slot_ptr, n_slots, rays=R):
        fm.batch_slot, fm.batch_slots = slot_ptr, n_slots
        return lib.nsamd_field_ray_terms(N.ptr(dirs), None, None, rays, fm, N.ptr(terms), None, st)

    invalid = -1  # NSAMD_ERR_INVALID_ARG
    assert call(None, slots) == invalid
    assert call(N.ptr(slot), 0) == invalid
    assert call(N.ptr(slot), -2) == invalid
    assert call(N.ptr(slot), slots, rays=0) == 0
    torch.cuda.synchronize()
    assert bool((terms == -7.0).all())
    assert call(N.ptr(slot), slots) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(terms).all()) and not bool((terms == -7.0).any())
