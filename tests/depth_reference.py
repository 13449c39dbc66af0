"""Float64 restatement of the depth-supervision losses (reference: nerfstudio/model_components/losses.py:225-325 and the loop
of models/depth_nerfacto.py:94-104), the seeded inputs the depth tests share, and the CPU stand-in for nsamd_depth_loss.

`depth_loss_f64` evaluates, on fp32 inputs promoted to float64, the per-ray masked sums of every level, the loss averaged over
the levels, and its gradients in the weights of every level and in predicted_depth — the closed forms of the issue, which
tests/test_depth_cpu.py checks against torch autograd in float64.

`make_inputs(n, counts, seed)` builds what both the fixture generator (tests/golden/make_golden_depth.py) and the GPU tests
use, so the reference's fp32 error measured by the generator belongs to the very inputs the GPU tests run:
  - Euclidean bin edges in [1, 3], increasing; weights min(0.9 * Dirichlet, 0.06) (small against the Normal density of the URF
    near band, >= 0.13 at sigma = 0.1, so `w - pdf` never cancels); sigma = 0.1 and targets within 2.7 of every sample
    (exp(-(steps - target)^2 / (2 sigma)) >= 1e-16: times a short bin it stays a normal fp32 number, so no entry is zero or
    denormal in fp32 that is not in float64);
  - ray 0 (and every 7th): termination_depth == 0 — masked, loss and gradient exactly 0;
  - the last ray: all weights 0 (the DS_NERF gradient is of order 1e7 and finite);
  - ray 1 (when there is one): target in front of the first sample; ray 2: behind the last;
  - targets nudged (deterministically, by 1e-4 relative steps) until, in float64, no |steps - (target +- sigma)| is below
    1e-5 * target for either depth convention: URF's interval comparisons then cannot flip in fp32.
"""
import numpy as np
import torch

EPS = 1.0e-7
SIGMA = 0.1
GPU_COUNTS = (1, 48, 63, 64, 65, 96, 256)  # the levels of one launch in the GPU parity tests
GPU_RAYS = (1, 65, 257)
FIXTURE_COUNTS, FIXTURE_RAYS = (256, 96, 48), 33
DS_NERF, URF = 1, 2


def case_key(loss_type, n, is_euclidean):
    """Name of a case's bound in tests/golden/depth_losses.npz: the reference's fp32 error on that case's own inputs."""
    return f"e_ref_{'ds' if loss_type == DS_NERF else 'urf'}_n{n}_{'euc' if is_euclidean else 'z'}"


def boundary_clearance(t_bins, target, sigma):
    """min over samples of |steps - (target +- sigma)| / target per ray, in float64 (inf for masked rays)."""
    tb = t_bins.astype(np.float64)
    steps = (tb[:, :-1] + tb[:, 1:]) / 2
    t = target.astype(np.float64)[:, None]
    gap = np.minimum(np.abs(steps - (t + sigma)), np.abs(steps - (t - sigma))).min(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t[:, 0] > 0, gap / t[:, 0], np.inf)


def make_inputs(n, counts, seed, sigma=SIGMA):
    rs = np.random.RandomState(seed)
    t_bins, weights = [], []
    for s in counts:
        edges = np.sort(rs.uniform(1.0, 3.0, (n, s + 1)), axis=1)
        t_bins.append(edges.astype(np.float32))
        w = np.minimum(0.9 * rs.dirichlet(np.ones(s), n), 0.06)
        w[-1] = 0.0  # a ray without any weight
        weights.append(w.astype(np.float32))
    td = rs.uniform(1.2, 2.8, n)
    dn = rs.uniform(1.0, 1.1, n).astype(np.float32)
    if n > 1:
        td[1] = 0.6  # in front of every sample (also after the multiplication by directions_norm <= 1.1)
    if n > 2:
        td[2] = 3.3  # behind every sample
    td[0::7] = 0.0  # masked rays
    if n == 1:
        td[0] = 1.9  # a single ray: supervised (the masked path is covered by every larger case)
    td = td.astype(np.float32)
    for _ in range(64):  # nudge targets off the interval boundaries
        bad = np.zeros(n, bool)
        for tb in t_bins:
            for tgt in (td, (td * dn).astype(np.float32)):
                bad |= boundary_clearance(tb, tgt, sigma) < 2e-5
        if not bad.any():
            break
        td = np.where(bad, (td.astype(np.float64) * (1 + 1e-4)).astype(np.float32), td)
    else:
        raise AssertionError("could not move the targets off the interval boundaries")
    # behind both targets (td and td * directions_norm <= 1.1 td) by 0.15 at least: `target - predicted` does not cancel
    pred = (td.astype(np.float64) * 1.1 + rs.uniform(0.15, 0.45, n)).astype(np.float32)
    return {"t_bins": t_bins, "weights": weights, "termination_depth": td, "directions_norm": dn, "predicted_depth": pred,
            "sigma": np.float32(sigma)}


def depth_loss_f64(t_bins, weights, termination_depth, directions_norm, predicted_depth, sigma, is_euclidean, loss_type):
    """-> dict(per_ray [levels, n], loss, d_weights [list of [n, S]], d_predicted [n] or None), all float64; the gradients are
    those of `loss` = sum over levels of mean over rays / levels."""
    levels, n = len(weights), termination_depth.shape[0]
    td = termination_depth.astype(np.float64).reshape(-1)
    target = td if is_euclidean else td * directions_norm.astype(np.float64).reshape(-1)
    mask = target > 0
    sigma = float(np.float32(sigma))
    scale = 1.0 / (n * levels)
    per_ray, d_weights = np.zeros((levels, n)), []
    pred = None if predicted_depth is None else predicted_depth.astype(np.float64).reshape(-1)
    for lvl in range(levels):
        tb, w = t_bins[lvl].astype(np.float64), weights[lvl].astype(np.float64)
        steps, lengths = (tb[:, :-1] + tb[:, 1:]) / 2, tb[:, 1:] - tb[:, :-1]
        x = steps - target[:, None]
        if loss_type == DS_NERF:
            e = np.exp(-(x ** 2) / (2 * sigma))
            terms = -np.log(w + EPS) * e * lengths
            dw = -e * lengths / (w + EPS)
            ray = terms.sum(axis=1)
        elif loss_type == URF:
            s = sigma / 3.0
            pdf = np.exp(-(x ** 2) / (2 * s * s) - np.log(s) - np.log(np.sqrt(2 * np.pi)))
            near = (steps <= target[:, None] + sigma) & (steps >= target[:, None] - sigma)
            empty = steps < target[:, None] - sigma
            ray = (target - pred) ** 2 + (near * (w - pdf) ** 2).sum(axis=1) + (empty * w ** 2).sum(axis=1)
            dw = near * 2 * (w - pdf) + empty * 2 * w
        else:
            raise NotImplementedError(loss_type)
        per_ray[lvl] = np.where(mask, ray, 0.0)
        d_weights.append(np.where(mask[:, None], dw, 0.0) * scale)
    d_pred = None
    if loss_type == URF:
        d_pred = np.where(mask, -2 * (target - pred), 0.0) * scale * levels
    return {"per_ray": per_ray, "loss": per_ray.sum() * scale, "d_weights": d_weights, "d_predicted": d_pred}


def depth_loss_torch(t_bins, weights, termination_depth, directions_norm, predicted_depth, sigma, is_euclidean, loss_type):
    """The reference's formulas as torch ops (any dtype, differentiable): the loss averaged over the levels. What autograd in
    float64 differentiates to check `depth_loss_f64`'s closed-form gradients."""
    td = termination_depth.reshape(-1, 1)
    if not is_euclidean:
        td = td * directions_norm.reshape(-1, 1)
    mask = td > 0
    total = 0.0
    for tb, w in zip(t_bins, weights):
        steps, lengths = (tb[:, :-1] + tb[:, 1:]) / 2, tb[:, 1:] - tb[:, :-1]
        if loss_type == DS_NERF:
            loss = (-torch.log(w + EPS) * torch.exp(-((steps - td) ** 2) / (2 * sigma)) * lengths).sum(-1, keepdim=True)
        else:
            dist = torch.distributions.normal.Normal(0.0, torch.as_tensor(sigma / 3.0, dtype=steps.dtype))
            near = torch.logical_and(steps <= td + sigma, steps >= td - sigma)
            los = (near * (w - torch.exp(dist.log_prob(steps - td))) ** 2).sum(-1, keepdim=True)
            los = los + ((steps < td - sigma) * w ** 2).sum(-1, keepdim=True)
            loss = (td - predicted_depth.reshape(-1, 1)) ** 2 + los
        total = total + torch.mean(loss * mask) / len(weights)
    return total


def rel_err(x, ref):
    """Largest entrywise relative distance from `ref` over its non-zero entries; where `ref` is exactly 0 (masked rays, samples
    outside both URF intervals) `x` has to be exactly 0 as well, else inf."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    zero = ref == 0
    if (x[zero] != 0).any() or not np.isfinite(x).all():
        return float("inf")
    if zero.all():
        return 0.0
    return float((np.abs(x[~zero] - ref[~zero]) / np.abs(ref[~zero])).max())


class FakeDepthLib:
    """nsamd_depth_loss on host memory: the float64 restatement cast to fp32, behind the C signature (the CPU tests hand the
    binding numpy-backed CPU tensors; pointers are read back through ctypes)."""

    def __init__(self):
        self.calls = []

    def nsamd_depth_loss(self, levels, t_bins, weights, S, n, td, dn, pred, sigma, loss_type, scale, accumulate, per_ray,
                         d_weights, d_pred, stream):
        import ctypes as C

        def arr(p, *shape):
            if not p:
                return None
            count = int(np.prod(shape))
            return np.ctypeslib.as_array((C.c_float * count).from_address(int(p))).reshape(shape)

        counts = [int(S[i]) for i in range(levels)]
        tb = [arr(t_bins[i], n, counts[i] + 1) for i in range(levels)]
        w = [arr(weights[i], n, counts[i]) for i in range(levels)]
        r = depth_loss_f64(tb, w, arr(td, n), arr(dn, n), arr(pred, n), sigma, dn is None or not dn, loss_type)
        self.calls.append({"levels": levels, "n": n, "loss_type": loss_type, "scale": scale, "accumulate": accumulate,
                           "sigma": sigma, "grads": [bool(d_weights and d_weights[i]) for i in range(levels)]})
        unit = scale * n * levels  # the restatement's gradients carry 1 / (n * levels)
        if per_ray:
            arr(per_ray, levels, n)[...] = r["per_ray"].astype(np.float32)
        for i in range(levels):
            out = arr(d_weights[i], n, counts[i]) if d_weights else None
            if out is not None:
                g = (r["d_weights"][i] * unit).astype(np.float32)
                out[...] = out + g if accumulate else g
        if d_pred and r["d_predicted"] is not None:
            out = arr(d_pred, n)
            g = (r["d_predicted"] * unit).astype(np.float32)
            out[...] = out + g if accumulate else g
        return 0
