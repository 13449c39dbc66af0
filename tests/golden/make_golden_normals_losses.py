#!/usr/bin/env python3
"""Golden fixture for the two normals losses of a `predict_normals` model and their gradients — written by THE REFERENCE ITSELF
(read-only import of the reference's model_components/losses.py and field_components/field_heads.py through the import stubs,
torch, CPU, fp32). Authoring container only:

    python tests/golden/make_golden_normals_losses.py      ->  tests/golden/normals_losses.npz

Cases (rays, samples per ray) = tests/normals_loss_reference.CASES, inputs from normals_loss_reference.case_inputs (a ray
without weight, a ray whose normals all face the camera, a masked sample, a pre-activation of exactly zero). Per case `c<i>_`:
the inputs, the reference's fp32 per-ray terms — orientation_loss(weights, normals, directions) and pred_normal_loss(weights,
normals, PredNormalsFieldHead(pre-activation)), the head's linear layer set to the identity so that its input IS the
pre-activation — and the autograd gradients of the summed terms with respect to the pre-activation and the directions
(weights and normals are constants, as models/nerfacto.py:335-344 detaches them).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402,F401  (sets up the import path of the reference and its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from nerfstudio.field_components.field_heads import PredNormalsFieldHead  # noqa: E402
from nerfstudio.model_components.losses import orientation_loss, pred_normal_loss  # noqa: E402

import normals_loss_reference as nl  # noqa: E402


def reference_eval(inp):
    w = torch.from_numpy(inp["weights"])[..., None]
    nr = torch.from_numpy(inp["normals"])
    x = torch.from_numpy(inp["pred_pre"].copy()).requires_grad_(True)
    v = torch.from_numpy(inp["directions"].copy()).requires_grad_(True)
    head = PredNormalsFieldHead(in_dim=3)
    with torch.no_grad():
        head.net.weight.copy_(torch.eye(3))
        head.net.bias.zero_()
    orientation = orientation_loss(w.detach(), nr, v)
    pred = pred_normal_loss(w.detach(), nr.detach(), head(x))
    (orientation.sum() + pred.sum()).backward()
    return {"orientation_per_ray": orientation.detach().numpy(), "pred_per_ray": pred.detach().numpy(),
            "d_pred_pre": x.grad.reshape(-1, 3).numpy().copy(), "d_directions": v.grad.numpy().copy()}


def main():
    out = {"cases": np.array(nl.CASES, np.int64)}
    for i, (n, S) in enumerate(nl.CASES):
        inp = nl.case_inputs(n, S)
        ref = reference_eval(inp)
        f64 = nl.normals_losses_torch(**inp, dtype=torch.float64)
        for k, v in {**inp, **ref}.items():
            out[f"c{i}_{k}"] = np.ascontiguousarray(v, dtype=np.float32)
        print(f"case {i} ({n} x {S}): reference fp32 against float64 (largest entrywise relative error) "
              + ", ".join(f"{k} {nl.rel_err(ref[k], f64[k]):.2e}" for k in nl.OUTPUTS))
    path = os.path.join(HERE, "normals_losses.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
