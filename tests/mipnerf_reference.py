"""Float64 restatement of mip-NeRF's conical frustum -> Gaussian -> integrated positional encoding (reference:
nerfstudio/cameras/rays.py:73-90, utils/math.py:42-67, :95-134, field_components/encodings.py:162-186), the seeded inputs the
mip-NeRF tests share, and the error measure. Not a test module.

`make_case(n, S)` builds what the fixture generator (tests/golden/make_golden_mipnerf.py) and the GPU tests both use, so the
reference's fp32 error the generator records (`k_ref_n<n>_s<S>`) belongs to the very inputs a test runs: origins around (0, 0, 4),
directions around -z, bin edges sorted in [2, 6], pixel areas a factor of up to 4 around a pinhole's 8.1e-7 (800 pixels). With
two rays or more, ray 0's last bin has zero width and ray 1's direction has length 0.5; with three or more, ray 2's has length 2.
The bin centres are > 0 everywhere (c = h = 0 is 0 / 0 in the reference too and is not a case).

The measure, per entry, normalised by what one fp32 ulp of the inputs does to it:

    |got - f64| / (damp64 2^-23 (w (|o_d| + |d_d| t_mean) + 2) + 2^-23),   w = 2 pi freq (1 for the appended mean, damp64 = 1)

(one ulp of o + d t, with cancellation, or of s + pi / 2, times 2 pi freq). An entry that is exactly zero in float64 must be zero.
"""
import numpy as np
import torch

ULP = 2.0 ** -23
MARGIN = 4.0
FIXTURE_CASE = (33, 17)
EDGE_RAYS = 8  # the fixture holds the two smaller encodings for the first rays only (rays 0 .. 2 are the edge rows)
# rays x samples. The kernel's guards are on the points of a 64-point tile and on the elements a tile's 256 lanes sweep: in points,
# 63 and 65 are one below and one above a tile, 256 and 640 multiples; 3 x 19 = 57 points are 513 elements at 9 columns (F = 1 with
# the input), one above two sweeps (one below is no product of a row width and a point count <= 64)
GPU_CASES = ((1, 1), (3, 5), (33, 17), (4, 64), (2, 65), (5, 128), (2, 193), (1, 63), (5, 13), (3, 19))
ENCODINGS = {"f16": (16, 0.0, 16.0), "f4": (4, 0.0, 4.0), "f1": (1, 0.0, 0.0)}  # (F, min exponent, max exponent)


def case_key(n, S):
    return f"k_ref_n{n}_s{S}"


def bound_f64(k_ref):
    """The measure an independent fp32 evaluation may reach against float64 on a case whose reference reaches `k_ref`."""
    return MARGIN * max(float(k_ref), 1.0)


def bound_ref(k_ref):
    """... and against the reference's own fp32 rows: "MARGIN + 1". Read as written that is bound_f64 + 1; the triangle inequality
    gives bound_f64 + k_ref, which is smaller where k_ref < 1 and larger where k_ref > 1. The smaller of the two is taken."""
    return bound_f64(k_ref) + min(float(k_ref), 1.0)


def frequencies(name):
    """fp32 `2 ** linspace` as NeRFEncoding evaluates it on the host (encodings.py:163)."""
    F, lo, hi = ENCODINGS[name]
    return (2 ** torch.linspace(lo, hi, F)).numpy()


def make_case(n, S):
    rs = np.random.RandomState(1000 * n + S)
    o = rs.standard_normal((n, 3)) * 0.3 + np.array([0.0, 0.0, 4.0])
    d = rs.standard_normal((n, 3)) * 0.2 + np.array([0.0, 0.0, -1.0])
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    tb = 2.0 + 4.0 * np.sort(rs.uniform(0.0, 1.0, (n, S + 1)), axis=-1)
    area = 8.1e-7 * 2.0 ** rs.uniform(-2.0, 2.0, n)
    if n >= 2:
        tb[0, -1] = tb[0, -2]
        d[1] *= 0.5
    if n >= 3:
        d[2] *= 2.0
    return {"origins": o.astype(np.float32), "directions": d.astype(np.float32), "t_bins": tb.astype(np.float32),
            "pixel_area": area.astype(np.float32)}


def gaussians(case, dtype=np.float64):
    """-> (mean [n,S,3], cov [n,S,3,3], t_mean [n,S]) of the conical frustums of `case`, evaluated in `dtype`."""
    o, d, tb, area = (case[k].astype(dtype) for k in ("origins", "directions", "t_bins", "pixel_area"))
    t0, t1 = tb[:, :-1], tb[:, 1:]
    c, h = (t0 + t1) / 2, (t1 - t0) / 2
    q = 3 * c**2 + h**2
    t_mean = c + 2 * c * h**2 / q
    var_along = h**2 / 3 - (4 / 15) * h**4 * (12 * c**2 - h**2) / q**2
    var_across = (area / np.pi)[:, None] * (c**2 / 4 + (5 / 12) * h**2 - (4 / 15) * h**4 / q)
    mean = o[:, None, :] + d[:, None, :] * t_mean[..., None]
    dd = d[:, :, None] * d[:, None, :]  # the raw d d^T; only the second projector is normalised
    across = np.eye(3, dtype=dtype) - dd / np.maximum((d**2).sum(-1), 1e-10)[:, None, None]
    cov = var_along[..., None, None] * dd[:, None] + var_across[..., None, None] * across[:, None]
    return mean, cov, t_mean


def diagonal(cov):
    return np.ascontiguousarray(np.diagonal(cov, axis1=-2, axis2=-1))


def ipe(mean, var, freqs, include_input, dtype=np.float64):
    """-> (rows [..., 6 F (+3)], damping factors [..., 3 F]) of means and covariance diagonals `[..., 3]`, in `dtype`."""
    mean, var, fr = mean.astype(dtype), var.astype(dtype), np.asarray(freqs).astype(dtype)
    s = ((2 * np.pi * mean)[..., None] * fr).reshape(*mean.shape[:-1], -1)
    damp = np.exp(-0.5 * (var[..., None] * fr**2).reshape(*mean.shape[:-1], -1))
    out = np.concatenate([damp * np.sin(s), damp * np.sin(s + np.pi / 2)], axis=-1)
    return (np.concatenate([out, mean], axis=-1) if include_input else out), damp


def encode_f64(case, freqs, include_input, explicit=None):
    """float64 rows of `case` -> (rows, per-entry scale of the measure). `explicit` = (means, variances) in fp32: the rows of
    THOSE Gaussians (what explicit mode is handed), on the scale of the rays they were formed from."""
    mean, cov, t_mean = gaussians(case)
    if explicit is None:
        explicit = (mean, diagonal(cov))
    rows, damp = ipe(explicit[0], explicit[1], freqs, include_input)
    reach = np.abs(case["origins"].astype(np.float64))[:, None, :] + np.abs(case["directions"].astype(np.float64))[:, None, :] * t_mean[..., None]
    w = 2 * np.pi * np.asarray(freqs, np.float64)
    enc = damp * ULP * ((reach[..., None] * w).reshape(*damp.shape) + 2) + ULP
    scale = np.concatenate([enc, enc] + ([ULP * (reach + 2) + ULP] if include_input else []), axis=-1)
    return rows, scale


def measure(got, rows64, scale):
    """The largest normalised error of fp32 rows `got` against the float64 rows; inf where float64 is exactly zero and got is
    not, or where got is not finite."""
    got = np.asarray(got, np.float64).reshape(rows64.shape)
    if not np.isfinite(got).all() or (got[rows64 == 0] != 0).any():
        return np.inf
    return float((np.abs(got - rows64) / scale).max())


def gaussians32(case):
    """fp32 means and covariance diagonals `[n * S, 3]` of `case`: what explicit mode is handed on the GPU."""
    mean, cov, _ = gaussians(case)
    return (np.ascontiguousarray(mean.reshape(-1, 3).astype(np.float32)),
            np.ascontiguousarray(diagonal(cov).reshape(-1, 3).astype(np.float32)))


def fake_ipe_launch(calls):
    """Stand-in for functional.ipe_encode_launch on CPU tensors: the fp32 cast of the float64 restatement, the arguments it saw
    appended to `calls`. The Points struct holds raw addresses, so the tensors are found through functional.PointSpec.native."""

    def launch(pts, M, pixel_area, variances, freqs, include_input, out):
        src = pts._tensors
        if src["positions"] is not None:
            mode, (mean, var) = "explicit", (src["positions"].numpy(), variances.numpy())
            assert pixel_area is None and mean.shape == var.shape == (M, 3)
        else:
            mode = "ray"
            case = {"origins": src["origins"].numpy(), "directions": src["directions"].numpy(), "t_bins": src["t_bins"].numpy(),
                    "pixel_area": pixel_area.numpy()}
            assert variances is None and pixel_area.shape == (case["origins"].shape[0],)
            mean, cov, _ = gaussians(case)
            mean, var = mean.reshape(-1, 3), diagonal(cov).reshape(-1, 3)
        rows, _ = ipe(mean, var, freqs.numpy(), include_input)
        out.copy_(torch.from_numpy(rows.astype(np.float32)))
        calls.append({"mode": mode, "M": M, "F": freqs.shape[0], "include_input": bool(include_input),
                      "pixel_area": None if pixel_area is None else pixel_area.clone()})

    return launch
