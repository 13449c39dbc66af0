#!/usr/bin/env python3
"""Golden fixture for the depth-supervision losses — written by THE REFERENCE ITSELF (read-only import of the reference's
model_components/losses.py through the import stubs, torch, CPU, fp32). Authoring container only:

    python tests/golden/make_golden_depth.py      ->  tests/golden/depth_losses.npz

The fixture case: 33 rays x (256, 96, 48) samples from tests/depth_reference.make_inputs (masked rays, a ray without weight, a
target in front of the first sample and one behind the last; see there). For DS_NERF and URF, with is_euclidean true and false
(`<ds|urf>_<euc|z>_...`): the reference's fp32 value of the loop of models/depth_nerfacto.py:94-104 — sum over the levels of
depth_loss(...) / levels — and its autograd gradients in the weights of every level and (URF) in predicted_depth.

It also records the reference's own fp32 distance from float64 (tests/depth_reference.depth_loss_f64 on the same fp32 inputs),
the bound the tests take, PER CASE: for every loss type, ray count (the fixture case, 33 rays, and every GPU parity case,
depth_reference.GPU_RAYS x GPU_COUNTS) and depth convention, `e_ref_<ds|urf>_n<rays>_<euc|z>` = the largest entrywise relative
error (depth_reference.rel_err) of [per-ray values (the reference evaluated ray by ray), weight gradients, predicted-depth
gradient, scalar loss], each floored at one fp32 ulp (2^-23); the unfloored figures in `..._measured`. A test takes the bound of
the very case it checks (depth_reference.case_key).

The generator asserts in float64 that no sample midpoint lies within 1e-5 * target of target +- sigma (URF's interval
comparisons cannot flip in fp32) and that no compared entry is zero in fp32 but not in float64.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402,F401  (sets up the import path of the reference and its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import depth_reference as dr  # noqa: E402

ULP = 2.0 ** -23
NAMES = {dr.DS_NERF: "ds", dr.URF: "urf"}


def reference_eval(inp, is_euclidean, loss_type, per_ray=False):
    """The reference's depth_loss over the levels as DepthNerfactoModel.get_metrics_dict calls it; fp32, autograd."""
    from nerfstudio.cameras.rays import Frustums, RaySamples
    from nerfstudio.model_components.losses import DepthLossType, depth_loss

    n = inp["termination_depth"].shape[0]
    ws = [torch.from_numpy(w.copy())[..., None].requires_grad_(True) for w in inp["weights"]]
    pred = torch.from_numpy(inp["predicted_depth"].copy())[:, None].requires_grad_(True)
    td = torch.from_numpy(inp["termination_depth"])[:, None]
    dn = torch.from_numpy(inp["directions_norm"])[:, None]
    sigma = torch.tensor([float(inp["sigma"])])
    samples = []
    for tb in inp["t_bins"]:
        tb = torch.from_numpy(tb)
        fr = Frustums(origins=torch.zeros(n, tb.shape[1] - 1, 3), directions=torch.ones(n, tb.shape[1] - 1, 3),
                      starts=tb[:, :-1, None], ends=tb[:, 1:, None], pixel_area=torch.ones(n, tb.shape[1] - 1, 1))
        samples.append(RaySamples(frustums=fr))
    kind = DepthLossType(loss_type)

    def one(rows):
        total = 0.0
        for w, rs in zip(ws, samples):
            total = total + depth_loss(weights=w[rows], ray_samples=rs[rows], termination_depth=td[rows],
                                       predicted_depth=pred[rows], sigma=sigma, directions_norm=dn[rows],
                                       is_euclidean=is_euclidean, depth_loss_type=kind) / len(ws)
        return total

    if per_ray:  # the mean over ONE ray is that ray's masked sum: [levels, n]
        out = np.zeros((len(ws), n), np.float32)
        with torch.no_grad():
            for lvl, (w, rs) in enumerate(zip(ws, samples)):
                for r in range(n):
                    rows = slice(r, r + 1)
                    out[lvl, r] = float(depth_loss(weights=w[rows], ray_samples=rs[rows], termination_depth=td[rows],
                                                   predicted_depth=pred[rows], sigma=sigma, directions_norm=dn[rows],
                                                   is_euclidean=is_euclidean, depth_loss_type=kind))
        return out
    loss = one(slice(None))
    loss.backward()
    return {"loss": np.float32(loss.item()), "d_weights": [w.grad[..., 0].numpy().copy() for w in ws],
            "d_predicted": None if pred.grad is None else pred.grad[:, 0].numpy().copy()}


def reference_errors(inp, loss_type, log, out):
    for euc in (False, True):
        f64 = dr.depth_loss_f64(inp["t_bins"], inp["weights"], inp["termination_depth"], inp["directions_norm"],
                                inp["predicted_depth"], inp["sigma"], euc, loss_type)
        tgt = inp["termination_depth"] if euc else (inp["termination_depth"] * inp["directions_norm"]).astype(np.float32)
        for tb in inp["t_bins"]:
            assert dr.boundary_clearance(tb, tgt, float(inp["sigma"])).min() >= 1e-5
        ref = reference_eval(inp, euc, loss_type)
        rays = reference_eval(inp, euc, loss_type, per_ray=True)
        e = [dr.rel_err(rays, f64["per_ray"]),
             max(dr.rel_err(a, b) for a, b in zip(ref["d_weights"], f64["d_weights"])),
             dr.rel_err(ref["d_predicted"], f64["d_predicted"]) if loss_type == dr.URF else 0.0,
             dr.rel_err(ref["loss"], f64["loss"])]
        assert np.isfinite(e).all(), e  # no entry zero in fp32 that float64 has, nothing non-finite
        log.append((NAMES[loss_type], inp["termination_depth"].shape[0], euc, *e))
        key = dr.case_key(loss_type, inp["termination_depth"].shape[0], euc)
        out[key + "_measured"] = np.array(e)
        out[key] = np.maximum(np.array(e), ULP)


def main():
    out, log = {}, []
    fx = dr.make_inputs(dr.FIXTURE_RAYS, dr.FIXTURE_COUNTS, seed=100)
    for i, (tb, w) in enumerate(zip(fx["t_bins"], fx["weights"])):
        out[f"t_bins_{i}"], out[f"weights_{i}"] = tb, w
    for k in ("termination_depth", "directions_norm", "predicted_depth", "sigma"):
        out[k] = fx[k]
    out["counts"] = np.array(dr.FIXTURE_COUNTS, np.int32)
    for lt, name in NAMES.items():
        for euc in (True, False):
            ref = reference_eval(fx, euc, lt)
            key = f"{name}_{'euc' if euc else 'z'}"
            out[f"{key}_loss"] = ref["loss"]
            for i, g in enumerate(ref["d_weights"]):
                out[f"{key}_d_weights_{i}"] = g
            if lt == dr.URF:
                out[f"{key}_d_predicted"] = ref["d_predicted"]
        reference_errors(fx, lt, log, out)
        for n in dr.GPU_RAYS:
            reference_errors(dr.make_inputs(n, dr.GPU_COUNTS, seed=n), lt, log, out)
    for row in log:
        print("%-4s n=%-4d euclidean=%-5s per_ray %.3e  d_weights %.3e  d_predicted %.3e  loss %.3e" % row)
    path = os.path.join(HERE, "depth_losses.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
