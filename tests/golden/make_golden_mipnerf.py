#!/usr/bin/env python3
"""Golden fixture for mip-NeRF — written by THE REFERENCE ITSELF (read-only import of the reference's modules through the import
stubs, torch, CPU). Authoring container only:

    python tests/golden/make_golden_mipnerf.py      ->  tests/golden/mipnerf.npz

Encoding. The fixture case, 33 rays x 17 samples of tests/mipnerf_reference.make_case (a zero-width bin, directions of length
0.5 and 2, pixel areas around a pinhole's): the reference's fp32 Frustums.get_gaussian_blob (`ref_mean`, `ref_cov`) and
NeRFEncoding(...)(mean, covs=cov) with include_input for the three encodings of mipnerf_reference.ENCODINGS (`ref_enc_<name>`, with
the fp32 frequencies `freqs_<name>`; the two smaller encodings on the first mipnerf_reference.EDGE_RAYS rays only). For the fixture
case and every GPU case, `k_ref_n<n>_s<S>`: the largest value of mipnerf_reference.measure of the reference's own fp32 rows against
float64, over the three encodings — the bound a test takes is that of the case it checks.

Model. models/mipnerf.py:101-161 composed from the reference's own modules (the model class imports torchmetrics, which the
authoring container lacks): ONE NeRFField(use_integrated_encoding=True) with NeRFEncoding(3, 16, 0, 16, True) / (3, 4, 0, 4, True),
UniformSampler(64), PDFSampler(128, include_original=False), white background, median depth, MSE scaled by 0.1 / 1.0.
Parameters: oracle.vanilla_oracle.init_field_params(VanillaCfg(pos_frequencies=16, pos_max_exp=16.0), 95, "field.") — a checksum
is stored. A train pass (recorded jitters; loss and gradients as 48 seeded entries, norm and sum per tensor) and an eval pass on 12
rays, each in fp32 (`<mode>_<output>`) and with the modules cast to double: `<mode>_<output>_dist` is the largest absolute
difference of the two (gradients: `train_gdist_<name>`, of the 48 entries; `train_gnorm64_<name>`), `<mode>_<output>_zero64` the
packed mask of the entries that are exactly zero in float64.

The generator asserts in float64 that no ray's cumulative weight lies within 100 x that pass's recorded weights distance of 0.5
at a sample edge: the median depth cannot flip between two fp32 evaluations.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (sets up the import path of the reference and its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mipnerf_reference as mr  # noqa: E402

T = torch.from_numpy
PARAM_SEED, NUM_COARSE, NUM_FINE, NEAR, FAR = 95, 64, 128, 2.0, 6.0
COEFF = {"rgb_loss_coarse": 0.1, "rgb_loss_fine": 1.0}


def reference_rows(case, name, include_input=True):
    """The reference's fp32 Gaussians and integrated encoding of `case`."""
    from nerfstudio.cameras.rays import Frustums
    from nerfstudio.field_components.encodings import NeRFEncoding

    n, S = case["t_bins"].shape[0], case["t_bins"].shape[1] - 1
    tb = T(case["t_bins"])
    fr = Frustums(origins=T(case["origins"])[:, None].expand(n, S, 3), directions=T(case["directions"])[:, None].expand(n, S, 3),
                  starts=tb[:, :-1, None], ends=tb[:, 1:, None], pixel_area=T(case["pixel_area"])[:, None, None].expand(n, S, 1))
    blob = fr.get_gaussian_blob()
    F, lo, hi = mr.ENCODINGS[name]
    return blob, NeRFEncoding(3, F, lo, hi, include_input=include_input)(blob.mean, covs=blob.cov).numpy()


def k_ref(case):
    worst = 0.0
    for name in mr.ENCODINGS:
        freqs = mr.frequencies(name)
        _, rows = reference_rows(case, name)
        rows64, scale = mr.encode_f64(case, freqs, True)
        worst = max(worst, mr.measure(rows, rows64, scale))
    assert np.isfinite(worst), worst
    return worst


def gen_encoding(out):
    n, S = mr.FIXTURE_CASE
    case = mr.make_case(n, S)
    out.update(case)
    for name in mr.ENCODINGS:
        blob, rows = reference_rows(case, name)
        # (the method's own 16 frequencies on every ray; the two smaller encodings on the first EDGE_RAYS, the edge rows among them)
        out[f"ref_enc_{name}"], out[f"freqs_{name}"] = rows if name == "f16" else rows[:mr.EDGE_RAYS], mr.frequencies(name)
    out["ref_mean"], out["ref_cov"] = blob.mean.numpy(), blob.cov.numpy()
    for n, S in mr.GPU_CASES:
        out[mr.case_key(n, S)] = np.float64(k_ref(mr.make_case(n, S)))
        print(f"{mr.case_key(n, S)} = {float(out[mr.case_key(n, S)]):.3f}")


def compose(field, rb, jitters, training, dtype):
    """models/mipnerf.py:101-143 over the reference's modules -> the outputs, and the two weights."""
    from nerfstudio.field_components.field_heads import FieldHeadNames
    from nerfstudio.model_components.ray_samplers import PDFSampler, UniformSampler

    su, sp = UniformSampler(num_samples=NUM_COARSE), PDFSampler(num_samples=NUM_FINE, include_original=False)
    rgb_r, acc_r, dep_r = mg.RGBRenderer(background_color="white"), mg.AccumulationRenderer(), mg.DepthRenderer()
    for m in (su, sp, rgb_r, field):
        m.train(training)
    with mg.replay_rand([jitters[0].to(dtype)] if training else []):
        rs_u = su(rb)
    fo_c = field.forward(rs_u)
    w_c = rs_u.get_weights(fo_c[FieldHeadNames.DENSITY])
    with mg.replay_rand([jitters[1].to(dtype)] if training else []):
        rs_p = sp(rb, rs_u, w_c)
    fo_f = field.forward(rs_p)
    w_f = rs_p.get_weights(fo_f[FieldHeadNames.DENSITY])
    res = {"rgb_coarse": rgb_r(rgb=fo_c[FieldHeadNames.RGB], weights=w_c), "rgb_fine": rgb_r(rgb=fo_f[FieldHeadNames.RGB], weights=w_f),
           "accumulation_coarse": acc_r(w_c), "accumulation_fine": acc_r(w_f), "depth_coarse": dep_r(w_c, rs_u),
           "depth_fine": dep_r(w_f, rs_p), "weights_coarse": w_c[..., 0], "weights_fine": w_f[..., 0]}
    return res


def gen_model(out):
    from nerfstudio.field_components.encodings import NeRFEncoding
    from nerfstudio.fields.vanilla_nerf_field import NeRFField
    from nerfstudio.model_components.losses import MSELoss

    from oracle import vanilla_oracle as van

    cfg = van.VanillaCfg(pos_frequencies=16, pos_max_exp=16.0)
    params = van.init_field_params(cfg, PARAM_SEED, "field.")
    out["param_checksum"] = torch.stack([v.double().sum() for v in params.values()]).numpy()
    out["param_names"] = np.array(sorted(params))
    rs = np.random.RandomState(96)
    N = 12
    o = (rs.standard_normal((N, 3)) * 0.3 + np.array([0, 0, -4.0])).astype(np.float32)
    d = rs.standard_normal((N, 3)).astype(np.float32) * 0.15 + np.array([0.0, 0, 1.0], np.float32)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    area = (8.1e-7 * 2.0 ** rs.uniform(-1.0, 1.0, (N, 1))).astype(np.float32)
    tgt = rs.uniform(0, 1, (N, 3)).astype(np.float32)
    j0 = rs.uniform(0, 1, (N, NUM_COARSE + 1)).astype(np.float32)
    j1 = rs.uniform(0, 1, (N, NUM_FINE + 1)).astype(np.float32)
    out.update(m_origins=o, m_directions=d, m_pixel_area=area, m_target=tgt, j0=j0, j1=j1)
    pick = np.random.RandomState(97)
    gidx = {k: pick.randint(0, v.numel(), 48) for k, v in params.items()}
    runs = {}
    for dtype in (torch.float32, torch.float64):
        field = NeRFField(position_encoding=NeRFEncoding(3, 16, 0.0, 16.0, include_input=True),
                          direction_encoding=NeRFEncoding(3, 4, 0.0, 4.0, include_input=True), use_integrated_encoding=True)
        missing, unexpected = field.load_state_dict({k[len("field."):]: v for k, v in params.items()}, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
        field = field.to(dtype)
        for mode in ("train", "eval"):
            training = mode == "train"
            rb = mg.RayBundle(origins=T(o).to(dtype), directions=T(d).to(dtype), pixel_area=T(area).to(dtype))
            rb = mg.NearFarCollider(NEAR, FAR, reset_near_plane=False)(rb)
            rb.nears, rb.fars = rb.nears.to(dtype), rb.fars.to(dtype)
            field.zero_grad()
            with torch.set_grad_enabled(training):
                res = compose(field, rb, (T(j0), T(j1)), training, dtype)
            got = {k: v.detach().numpy() for k, v in res.items()}
            if training:
                # models/mipnerf.py:145-161 (an RGB target: the background blend for the loss is the identity)
                loss = sum(COEFF[f"rgb_loss_{p}"] * MSELoss()(T(tgt).to(dtype), res[f"rgb_{p}"]) for p in ("coarse", "fine"))
                loss.backward()
                got["loss"] = loss.detach().numpy()
                for k, p_ in field.named_parameters():
                    g_ = p_.grad.reshape(-1).double()
                    got[f"gval_field.{k}"] = g_[T(gidx["field." + k])].numpy()
                    got[f"gstat_field.{k}"] = np.array([float(g_.norm()), float(g_.sum())])
            runs[(dtype, mode)] = got
    for mode in ("train", "eval"):
        r32, r64 = runs[(torch.float32, mode)], runs[(torch.float64, mode)]
        for k in r32:
            if k.startswith("gstat_"):
                out[f"{mode}_{k}"], out[f"{mode}_gnorm64_{k[6:]}"] = r32[k], r64[k][0]
                continue
            out[f"{mode}_{k}"] = r32[k].astype(np.float32)
            dist = float(np.abs(r32[k].astype(np.float64) - r64[k]).max())
            if k.startswith("gval_"):
                out[f"{mode}_gidx_{k[5:]}"], out[f"{mode}_gdist_{k[5:]}"] = gidx[k[5:]], dist
            else:
                out[f"{mode}_{k}_zero64"], out[f"{mode}_{k}_dist"] = np.packbits(r64[k] == 0), dist
        for p in ("coarse", "fine"):  # the median depth: no cumulative weight near 0.5 at a sample edge
            cum = np.cumsum(r64[f"weights_{p}"], axis=-1)
            clear = np.abs(cum - 0.5).min()
            need = 100 * out[f"{mode}_weights_{p}_dist"]
            print(f"{mode} {p}: weights dist {out[f'{mode}_weights_{p}_dist']:.3e}, clearance of 0.5 {clear:.3e}, "
                  f"rgb dist {out[f'{mode}_rgb_{p}_dist']:.3e}, depth dist {out[f'{mode}_depth_{p}_dist']:.3e}")
            assert clear > need, (mode, p, clear, need)
    print("train loss", out["train_loss"], "dist", out["train_loss_dist"])


def main():
    out = {}
    gen_encoding(out)
    gen_model(out)
    path = os.path.join(HERE, "mipnerf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
