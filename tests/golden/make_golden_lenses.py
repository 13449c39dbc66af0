#!/usr/bin/env python3
"""Golden fixture for ray generation of distorted perspective, fisheye and equirectangular cameras — written by THE
REFERENCE ITSELF (read-only import of /root/reference, torch path, CPU). Authoring container only:

    python tests/golden/make_golden_lenses.py      ->  tests/golden/raygen_lenses.npz

Every case is the reference's own `RayGenerator(Cameras(...))` (model_components/ray_generators.py:41-56 ->
Cameras._generate_rays_from_coords, cameras/cameras.py:598-656, 781-817, 887-909; camera_utils.py:375-478) on seeded
cameras: C x 40 x 56 images, f = 40 - 60 px (normalised radius up to ~0.8), principal points off the pixel centres so that
no fisheye pixel has theta = 0 (the reference gives 0 / 0 there). Cases (`cases` in the fixture; arrays are `<case>_<name>`):

    opencv        4 perspective cameras in one Cameras: a typical COLMAP set (k1 -0.12, k2 0.03, p1 1e-3, p2 -2e-3), strong
                  barrel (k1 -0.35, k2 0.15), all six parameters non-zero, and all zeros (next to distorted rows)
    fisheye       2 fisheye cameras: with k1..k4 and without
    equirect      1 equirectangular camera (fx = fy = H, W = 2 H), no distortion parameters
    mixed         6 cameras of types 1, 2, 3, 1, 2, 3, some distorted (the equirectangular rows' parameters are ignored)
    grid_opencv   the full 24 x 32 image of one distorted perspective camera, row-major (for the grid form)
    grid_fisheye  the full 24 x 32 image of one fisheye camera with k1..k4

Sampled cases hold both corner pixels of every camera plus random pixels.

Next to the reference's fp32 arrays the fixture holds a float64 evaluation of the same formulas on the same fp32 inputs
(`<case>_f64_*`, `lens_rays_f64` below) and the reference's own distance from it, the maximum over the WHOLE fixture:
`e_ref_directions` (absolute), `e_ref_pixel_area`, `e_ref_directions_norm` (relative), each floored at one fp32 ulp of 1.0
(2^-23); the unfloored figures are `e_ref_*_measured` and per case `e_ref_by_case` (rows = cases, columns = the three
quantities). The tests take their bounds from these: 2 x e_ref against float64, 3 x e_ref against the reference's fp32.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets up the import path of the reference and its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ULP = 2.0 ** -23


def lens_rays_f64(idx, c2w, fx, fy, cx, cy, ctype, dist):
    """The reference's formulas in float64 on the fp32 inputs -> directions [N,3], pixel_area [N,1], directions_norm [N,1]."""
    cam = idx[:, 0]
    m = c2w.astype(np.float64)[cam]
    f_x, f_y, c_x, c_y = (a.astype(np.float64).reshape(-1)[cam] for a in (fx, fy, cx, cy))
    t = ctype.reshape(-1)[cam]
    k = (np.zeros((len(ctype.reshape(-1)), 6)) if dist is None else dist.astype(np.float64))[cam]
    y, x = idx[:, 1] + 0.5, idx[:, 2] + 0.5
    dirs = []
    for ox, oy in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
        xd, yd = (x - c_x + ox) / f_x, (y - c_y + oy) / f_y
        k1, k2, k3, k4, p1, p2 = (k[:, i] for i in range(6))
        u, v = xd.copy(), yd.copy()
        for _ in range(10):
            r = u * u + v * v
            d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
            f_u = d * u + 2 * p1 * u * v + p2 * (r + 2 * u * u) - xd
            f_v = d * v + 2 * p2 * u * v + p1 * (r + 2 * v * v) - yd
            d_r = k1 + r * (2.0 * k2 + r * (3.0 * k3 + r * 4.0 * k4))
            d_u, d_v = 2.0 * u * d_r, 2.0 * v * d_r
            fu_u = d + d_u * u + 2.0 * p1 * v + 6.0 * p2 * u
            fu_v = d_v * u + 2.0 * p1 * u + 2.0 * p2 * v
            fv_u = d_u * v + 2.0 * p2 * v + 2.0 * p1 * u
            fv_v = d + d_v * v + 2.0 * p2 * u + 6.0 * p1 * v
            den = fv_u * fu_v - fu_u * fv_v
            ok = np.abs(den) > 1e-3
            safe = np.where(ok, den, 1.0)
            u = u + np.where(ok, (f_u * fv_v - f_v * fu_v) / safe, 0.0)
            v = v + np.where(ok, (f_v * fu_u - f_u * fv_u) / safe, 0.0)
        u, v = np.where(t == 3, xd, u), -np.where(t == 3, yd, v)
        th = np.clip(np.sqrt(u * u + v * v), 0.0, np.pi)
        fish = np.stack([u * np.sin(th) / th, v * np.sin(th) / th, -np.cos(th)], -1)
        theta, phi = -np.pi * u, np.pi * (0.5 - v)
        equi = np.stack([-np.sin(theta) * np.sin(phi), np.cos(phi), -np.cos(theta) * np.sin(phi)], -1)
        pers = np.stack([u, v, -np.ones_like(u)], -1)
        local = np.where((t == 2)[:, None], fish, np.where((t == 3)[:, None], equi, pers))
        dirs.append(np.einsum("nij,nj->ni", m[:, :, :3], local))
    norms = [np.linalg.norm(d, axis=-1, keepdims=True) for d in dirs]
    d0, d1, d2 = (d / n for d, n in zip(dirs, norms))
    area = np.linalg.norm(d0 - d1, axis=-1, keepdims=True) * np.linalg.norm(d0 - d2, axis=-1, keepdims=True)
    return d0, area, norms[0]


def make_cameras(rs, types, dist, H, W, equirect_hw=None):
    C = len(types)
    q = rs.standard_normal((C, 3, 3))
    rot = np.stack([np.linalg.qr(m)[0] for m in q]).astype(np.float32)
    c2w = np.concatenate([rot, rs.standard_normal((C, 3, 1)).astype(np.float32)], axis=-1)
    fx = rs.uniform(40, 60, (C,)).astype(np.float32)
    fy = rs.uniform(40, 60, (C,)).astype(np.float32)
    types = np.asarray(types, np.int64)
    fx[types == 3] = H  # equirectangular: fx = fy = height = width / 2 (cameras.py:810)
    fy[types == 3] = H
    cx = np.full((C,), W / 2, np.float32) + rs.uniform(-1, 1, (C,)).astype(np.float32)
    cy = np.full((C,), H / 2, np.float32) + rs.uniform(-1, 1, (C,)).astype(np.float32)
    return dict(c2w=c2w, fx=fx, fy=fy, cx=cx, cy=cy, camera_type=types.astype(np.int32),
                distortion=None if dist is None else np.asarray(dist, np.float32), hw=np.array([H, W]))


def run_case(cam, idx):
    T = torch.from_numpy
    cams = mg.Cameras(camera_to_worlds=T(cam["c2w"]), fx=T(cam["fx"]), fy=T(cam["fy"]), cx=T(cam["cx"]), cy=T(cam["cy"]),
                      width=int(cam["hw"][1]), height=int(cam["hw"][0]),
                      distortion_params=None if cam["distortion"] is None else T(cam["distortion"]),
                      camera_type=T(cam["camera_type"].astype(np.int64)))
    rb = mg.RayGenerator(cams)(T(idx))
    ref = dict(origins=rb.origins.numpy(), directions=rb.directions.numpy(), pixel_area=rb.pixel_area.numpy(),
               directions_norm=rb.metadata["directions_norm"].numpy())
    assert all(np.isfinite(v).all() for v in ref.values()), "the reference produced a non-finite ray"
    d64, a64, n64 = lens_rays_f64(idx, cam["c2w"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["camera_type"],
                                  cam["distortion"])
    err = [float(np.abs(ref["directions"] - d64).max()), float((np.abs(ref["pixel_area"] - a64) / a64).max()),
           float((np.abs(ref["directions_norm"] - n64) / n64).max())]
    out = {k: v for k, v in cam.items() if v is not None}
    out.update(ray_indices=idx, **ref, f64_directions=d64, f64_pixel_area=a64, f64_directions_norm=n64)
    return out, err


def sample_indices(rs, C, H, W, n):
    idx = np.stack([rs.randint(0, C, n), rs.randint(0, H, n), rs.randint(0, W, n)], -1).astype(np.int64)
    corners = np.array([[c, r, col] for c in range(C) for r, col in ((0, 0), (H - 1, W - 1))], np.int64)
    return np.concatenate([corners, idx])


def full_image(H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([np.zeros_like(yy), yy, xx], -1).reshape(-1, 3).astype(np.int64)


def main():
    rs = np.random.RandomState(171)
    H, W = 40, 56
    colmap = [-0.12, 0.03, 0, 0, 1e-3, -2e-3]
    barrel = [-0.35, 0.15, 0, 0, 0, 0]
    six = [-0.2, 0.06, -0.012, 0.003, 1.5e-3, -1e-3]
    fish_k = [0.04, -0.006, 0.002, -0.0004, 0, 0]
    zeros = [0.0] * 6
    cases = {}
    cases["opencv"] = (make_cameras(rs, [1, 1, 1, 1], [colmap, barrel, six, zeros], H, W), None)
    cases["fisheye"] = (make_cameras(rs, [2, 2], [fish_k, zeros], H, W), None)
    cases["equirect"] = (make_cameras(rs, [3], None, 28, 56), None)
    cases["mixed"] = (make_cameras(rs, [1, 2, 3, 1, 2, 3], [colmap, fish_k, barrel, zeros, zeros, zeros], 28, 56), None)
    cases["grid_opencv"] = (make_cameras(rs, [1], [colmap], 24, 32), full_image(24, 32))
    cases["grid_fisheye"] = (make_cameras(rs, [2], [fish_k], 24, 32), full_image(24, 32))
    out, errs = {}, []
    for name, (cam, idx) in cases.items():
        if idx is None:
            h, w = cam["hw"]
            idx = sample_indices(rs, len(cam["fx"]), int(h), int(w), 96)
        arrs, err = run_case(cam, idx)
        errs.append(err)
        print(f"{name:13s} {idx.shape[0]:4d} rays; reference vs float64: directions {err[0]:.3e} abs, pixel_area {err[1]:.3e} rel, "
              f"directions_norm {err[2]:.3e} rel")
        out.update({f"{name}_{k}": v for k, v in arrs.items()})
    errs = np.asarray(errs)
    worst = errs.max(axis=0)
    print(f"whole fixture: directions {worst[0]:.3e}, pixel_area {worst[1]:.3e}, directions_norm {worst[2]:.3e}")
    for i, q in enumerate(("directions", "pixel_area", "directions_norm")):
        out[f"e_ref_{q}_measured"] = worst[i]
        out[f"e_ref_{q}"] = max(worst[i], ULP)
    mg.save("raygen_lenses", cases=np.array(list(cases)), e_ref_by_case=errs, **out)


if __name__ == "__main__":
    main()
