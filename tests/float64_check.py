"""Shared by the GPU tests that hold kernels to float64 references entry by entry (test_gpu_proposal_backward.py,
test_gpu_ray_forward.py) and by the CPU tests of those references: the rounding constants and the per-entry comparison."""
import numpy as np
import torch

U = 2.0**-24
D53 = 2.0**-53
E_EXP = 4 * U      # expf: 2 ulp = relative 2 * 2^-23 (assumed; test_expf_budget)
E_SIN = 4 * U      # sinf: 2 ulp, assumed as E_EXP is (no ULP table of the device math library ships with the toolchain to take it
                   # from); test_gpu_encoders_float64.py measures it through nsamd_nerf_encode, arguments up to ~1.6e6
SAFE = 1 + 2.0**-6
TINY = 2.0**-140


def _np(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def check_entries(name, got, ref, bound, worst):
    """Per entry |got - ref| <= bound; NaN exactly where the reference has NaN, +-Inf equal. Records the worst ratio."""
    got, ref, bound = _np(got).reshape(-1), _np(ref).reshape(-1), _np(bound).reshape(-1)
    ng, nr = np.isnan(got), np.isnan(ref)
    assert np.array_equal(ng, nr), f"{name}: NaN at {np.flatnonzero(ng != nr)[:8]} differ (got {ng.sum()}, ref {nr.sum()})"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{name}: infinite entries differ"
    fin = np.isfinite(ref) & np.isfinite(bound)
    assert np.isfinite(got[np.isfinite(ref)]).all(), f"{name}: non-finite result where the reference is finite"
    err = np.abs(got[fin] - ref[fin])
    b = bound[fin] * SAFE + TINY
    ratio = float((err / b).max()) if err.size else 0.0
    worst[name] = max(worst.get(name, 0.0), ratio)
    if not bool((err <= b).all()):
        k = int(np.argmax(err / b))
        idx = np.flatnonzero(fin)[k]
        raise AssertionError(f"{name}: {int((err > b).sum())}/{err.size} entries beyond the bound; worst at {idx}: got "
                             f"{got[idx]:.9e} ref {ref[idx]:.9e} err {err[k]:.3e} bound {b[k]:.3e} ({ratio:.1f}x)")
    return ratio


def report(title, worst):
    print(f"\n{title}: worst |err|/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
