"""Float64 restatement of TSDF fusion (the reference's TSDF.integrate_tsdf, exporter/tsdf_utils.py:172-274), the seeded cases the
TSDF tests share, an fp32 torch-op restatement of the same update, and the CPU stand-in for the launch.

`integrate_f64` evaluates, on fp32 inputs promoted to float64, what one batch of views does to a volume: the state is carried in
float64 across the views, in view order. It also yields, per voxel, the two margins that say whether an fp32 evaluation can
legitimately DECIDE differently:

    pixel_margin   the smallest distance, over views and both image axes, of the unnormalised pixel coordinate
                   ((g + 1) size - 1) / 2 from a rounding tie — a half-integer, which includes the image border at -0.5 and
                   size - 0.5; coordinates more than a pixel outside the image, and non-finite ones (z == 0), are outside in
                   any arithmetic and do not count
    trunc_margin   the smallest |dist + truncation| over the views that hit a positive depth: the validity test of :245

A voxel is UNSAFE when pixel_margin < PIXEL_TIE (1e-3 px; the fp32 error of a pixel coordinate of magnitude <= 400 is ~1e-5 px,
a hundredfold margin) or trunc_margin < TRUNC_TIE (1e-4). Unsafe voxels may be at most UNSAFE_CAP = 3 % of a case; on the safe
ones weights must equal the reference's exactly, and values / colours lie within MARGIN = 4 times the reference's own fp32
distance from float64 on the same case (`e_ref_values_<case>`, `e_ref_colors_<case>` in tests/golden/tsdf.npz): an equally
long fp32 chain in another order — the 3 x 4 product, the device's inverse, the division.
"""
import numpy as np

PIXEL_TIE = 1e-3
TRUNC_TIE = 1e-4
UNSAFE_CAP = 0.03
MARGIN = 4.0
TRUNCATION_MARGIN = 5.0
CASES = ("A", "B", "C")


# ---------------------------------------------------------------- the cases ----------------------------------------------
def look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """c2w [4,4] float64 of a camera at `position` looking at `target`: the camera looks along its -z, y up."""
    p = np.asarray(position, np.float64)
    z = p - np.asarray(target, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, p
    return m


def sphere_depth(c2w, K, H, W, radius):
    """[H,W] float64: the distance along each pixel centre's ray to the sphere of `radius` about the origin, 0 where it misses."""
    iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    a = (ix + 0.5 - K[0, 2]) / K[0, 0]
    b = (iy + 0.5 - K[1, 2]) / K[1, 1]
    d = np.stack([a, -b, -np.ones_like(a)], -1) @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = c2w[:3, 3]
    od = d @ o
    disc = od * od - (o @ o - radius * radius)
    t = -od - np.sqrt(np.maximum(disc, 0.0))
    return np.where((disc > 0) & (t > 0), t, 0.0)


OUTSIDE = ((2.5, 0.3, 0.4), (-0.4, 2.4, 0.9), (0.5, -0.6, 2.6))
INSIDE = (0.2, 0.1, 0.3)


def make_case(name):
    """The fp32 inputs of a case: aabb [2,3], dims [3] int64, c2w [B,4,4], K [B,3,3], depth [B,1,H,W], color [B,3,H,W]."""
    rs = np.random.RandomState({"A": 11, "B": 12, "C": 13}[name])
    if name == "B":  # the z = 0 plane and voxels behind the camera; every coordinate exact in fp32
        aabb, dims, H, W = [[-1, -1, -1], [1, 1, 1]], (8, 8, 8), 6, 8
        K = np.array([[5.0, 0, 4.0], [0, 5.0, 3.0], [0, 0, 1]])
        c2w = np.eye(4)
        c2w[:3, 3] = (0.125, 0.125, 0.25)
        poses, depth = [c2w], [np.full((H, W), 0.9)]
    else:
        H, W = 24, 32
        K = np.array([[30.0, 0, 16.37], [0, 28.0, 11.79], [0, 0, 1]])
        if name == "A":  # 990 voxels: below one workgroup's multiple, ragged in every axis
            aabb, dims = [[-1, -1, -1], [1, 1, 1]], (9, 10, 11)
            poses = [look_at(p) for p in OUTSIDE + (INSIDE,)]
        else:  # anisotropic voxels: the truncation comes from the x size alone
            aabb, dims = [[-1, -0.5, -0.2], [1, 0.6, 0.4]], (17, 9, 5)
            poses = [look_at(p) for p in OUTSIDE[:2]]
        poses = [p.astype(np.float32).astype(np.float64) for p in poses]  # the depth belongs to the fp32 pose
        depth = [sphere_depth(p, K, H, W, 0.6) for p in poses]
        if name == "A":
            depth[3] = np.full((H, W), 0.8)  # the camera inside the box sees a constant depth
    B = len(poses)
    return {"aabb": np.asarray(aabb, np.float32), "dims": np.asarray(dims, np.int64),
            "c2w": np.stack(poses).astype(np.float32), "K": np.repeat(K[None], B, 0).astype(np.float32),
            "depth": np.stack(depth)[:, None].astype(np.float32),
            "color": rs.uniform(0, 1, (B, 3, H, W)).astype(np.float32)}


def case_inputs(g, name):
    """A case's inputs as the fixture holds them."""
    return {k: g[f"{name}_{k}"] for k in ("aabb", "dims", "c2w", "K", "depth", "color")}


def volume_geometry(aabb, dims):
    """(origin [3], voxel_size [3]) in fp32 as TSDF.from_aabb takes them (:96-97), and the truncation (:80-85)."""
    aabb = np.asarray(aabb, np.float32)
    voxel_size = ((aabb[1] - aabb[0]) / np.asarray(dims).astype(np.float32)).astype(np.float32)
    return aabb[0].copy(), voxel_size, float(voxel_size[0]) * TRUNCATION_MARGIN


def initial_state(dims):
    dims = tuple(int(d) for d in dims)
    return -np.ones(dims, np.float32), np.zeros(dims, np.float32), np.zeros(dims + (3,), np.float32)


# ---------------------------------------------------------------- float64 -------------------------------------------------
def _tie_distance(coord, size):
    """Distance of an unnormalised pixel coordinate from the nearest half-integer; inf where the coordinate is non-finite or
    more than a pixel outside [-0.5, size - 0.5]."""
    out = np.full(coord.shape, np.inf)
    near = np.isfinite(coord) & (coord > -1.5) & (coord < size + 0.5)
    c = coord[near]
    out[near] = np.abs(c - np.floor(c) - 0.5)
    return out


def integrate_f64(origin, voxel_size, truncation, values, weights, colors, c2w, K, depth, color=None):
    """-> dict(values, weights, colors (float64, same shapes), touched [X,Y,Z] bool, behind [X,Y,Z] bool: touched by a view
    that has the voxel behind it, pixel_margin, trunc_margin [X,Y,Z]). Inputs fp32 (or float64) arrays: c2w [B,4,4] or [B,3,4],
    K [B,3,3], depth [B,H,W] / [B,1,H,W], color [B,3,H,W] / [B,H,W,3] or None."""
    f8 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    dims = values.shape
    v, w, c = f8(values).reshape(-1).copy(), f8(weights).reshape(-1).copy(), f8(colors).reshape(-1, 3).copy()
    c2w, K, depth = f8(c2w), f8(K), f8(depth)
    B = c2w.shape[0]
    if depth.ndim == 4:
        depth = depth[:, 0] if depth.shape[1] == 1 else depth[..., 0]
    H, W = depth.shape[1:]
    if color is not None:
        color = f8(color)
        if color.shape[1:] != (H, W, 3):
            color = color.transpose(0, 2, 3, 1)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1).reshape(-1, 3)
    pts = f8(origin)[None] + idx * f8(voxel_size)[None]
    n = pts.shape[0]
    touched, behind = np.zeros(n, bool), np.zeros(n, bool)
    pixel_margin, trunc_margin = np.full(n, np.inf), np.full(n, np.inf)
    for b in range(B):
        m = np.eye(4)
        m[:c2w.shape[1]] = c2w[b]
        w2c = np.linalg.inv(m)
        cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
        x, y, z = cam[:, 0], -cam[:, 1], -cam[:, 2]
        voxel_depth = np.sqrt(x * x + y * y + z * z)
        with np.errstate(divide="ignore", invalid="ignore"):
            pa, pb = x / z, y / z
            u = K[b, 0, 0] * pa + K[b, 0, 1] * pb + K[b, 0, 2]
            t = K[b, 1, 0] * pa + K[b, 1, 1] * pb + K[b, 1, 2]
            cu = ((2.0 * u / W - 1.0 + 1.0) * W - 1.0) / 2.0
            cv = ((2.0 * t / H - 1.0 + 1.0) * H - 1.0) / 2.0
            ru, rv = np.rint(cu), np.rint(cv)  # ties to even
            inside = (ru >= 0) & (ru <= W - 1) & (rv >= 0) & (rv <= H - 1)  # a NaN fails every comparison
        pixel_margin = np.minimum(pixel_margin, np.minimum(_tie_distance(cu, W), _tie_distance(cv, H)))
        iu, iv = np.where(inside, ru, 0).astype(np.int64), np.where(inside, rv, 0).astype(np.int64)
        sampled = np.where(inside, depth[b][iv, iu], 0.0)
        dist = sampled - voxel_depth
        hit = sampled > 0
        trunc_margin = np.where(hit, np.minimum(trunc_margin, np.abs(dist + truncation)), trunc_margin)
        valid = (voxel_depth > 0) & hit & (dist > -truncation)
        new = np.clip(dist / truncation, -1.0, 1.0)
        total = w + 1.0
        v = np.where(valid, (v * w + new) / total, v)
        if color is not None:
            s = np.where(inside[:, None], color[b][iv, iu], 0.0)
            c = np.where(valid[:, None], (c * w[:, None] + s) / total[:, None], c)
        w = np.where(valid, np.minimum(total, 1.0), w)
        touched |= valid
        behind |= valid & (z < 0)
    shape = lambda a: a.reshape(dims)  # noqa: E731
    return {"values": shape(v), "weights": shape(w), "colors": c.reshape(*dims, 3), "touched": shape(touched),
            "behind": shape(behind), "pixel_margin": shape(pixel_margin), "trunc_margin": shape(trunc_margin)}


def safe_voxels(f64):
    return (f64["pixel_margin"] >= PIXEL_TIE) & (f64["trunc_margin"] >= TRUNC_TIE)


def distance(got, f64, key, safe):
    """Largest absolute distance of an fp32 result from float64 over the safe voxels (values lie in [-1, 1], colours in [0, 1])."""
    d = np.abs(np.asarray(got, np.float64) - f64[key])[safe]
    assert np.isfinite(d).all()
    return float(d.max()) if d.size else 0.0


def check(got, f64, e_values, e_colors, ref=None, label=""):
    """got: dict(values, weights, colors) fp32 -> prints the ratios, then asserts the rule of the module docstring; ref: the
    reference's own fp32 arrays (weights equal on safe voxels, values / colours within MARGIN + 1 bounds of each other)."""
    safe = safe_voxels(f64)
    assert 1.0 - safe.mean() <= UNSAFE_CAP, f"{label}: {100 * (1 - safe.mean()):.2f} % unsafe voxels"
    dv, dc = distance(got["values"], f64, "values", safe), distance(got["colors"], f64, "colors", safe)
    ratio = lambda d, e: d / e if e > 0 else (0.0 if d == 0 else float("inf"))  # noqa: E731
    print(f"tsdf {label}: unsafe {int((~safe).sum())}/{safe.size}  values {dv:.3e} = {ratio(dv, e_values):.2f} x e_ref "
          f"{e_values:.3e}  colors {dc:.3e} = {ratio(dc, e_colors):.2f} x e_ref {e_colors:.3e}")
    assert np.array_equal(np.asarray(got["weights"], np.float64)[safe], f64["weights"][safe]), f"{label}: weights"
    assert np.isfinite(np.asarray(got["values"])).all() and np.isfinite(np.asarray(got["colors"])).all()
    assert dv <= MARGIN * e_values, f"{label}: values {dv:.3e} > {MARGIN} x {e_values:.3e}"
    assert dc <= MARGIN * e_colors, f"{label}: colors {dc:.3e} > {MARGIN} x {e_colors:.3e}"
    if ref is not None:
        assert np.array_equal(np.asarray(got["weights"])[safe], ref["weights"][safe])
        assert np.abs(np.asarray(got["values"], np.float64) - ref["values"])[safe].max() <= (MARGIN + 1) * e_values
        assert np.abs(np.asarray(got["colors"], np.float64) - ref["colors"])[safe].max() <= (MARGIN + 1) * e_colors


# ---------------------------------------------------------------- fp32, torch ops ------------------------------------------
def integrate_torch(origin, voxel_size, truncation, values, weights, colors, c2w, K, depth, color=None):
    """The same update with fp32 torch ops over [B, voxels] temporaries, on whatever device the tensors live on — the eager form
    the kernel replaces (the GPU tests take its distance from float64 as e_ref where the fixture has no case; the export
    profile times it). values / weights / colors are updated IN PLACE. c2w [B,4,4], K [B,3,3], depth [B,1,H,W],
    color [B,3,H,W] or None; origin, voxel_size [3] tensors."""
    import torch
    import torch.nn.functional as TF

    dev, dims = values.device, values.shape
    B, (H, W) = c2w.shape[0], depth.shape[-2:]
    grid = torch.stack(torch.meshgrid([torch.arange(n, device=dev) for n in dims], indexing="ij"), 0)
    pts = (origin.to(dev).view(3, 1, 1, 1) + grid * voxel_size.to(dev).view(3, 1, 1, 1)).view(3, -1)
    hom = torch.cat([pts, torch.ones_like(pts[:1])], 0)[None].expand(B, 4, -1)
    cam = torch.bmm(torch.inverse(c2w), hom)
    x, y, z = cam[:, 0:1], -cam[:, 1:2], -cam[:, 2:3]
    voxel_depth = torch.sqrt(x * x + y * y + z * z)
    pix = torch.bmm(K, torch.cat([x, y, z], 1) / z)[:, :2].permute(0, 2, 1)
    norm = (2.0 * pix / torch.tensor([W, H], device=dev).view(1, 1, 2) - 1.0)[:, None]
    kw = dict(mode="nearest", padding_mode="zeros", align_corners=False)
    sampled = TF.grid_sample(depth, norm, **kw).squeeze(2)
    sampled_color = TF.grid_sample(color, norm, **kw).squeeze(2) if color is not None else None
    dist = sampled - voxel_depth
    new = torch.clamp(dist / truncation, min=-1.0, max=1.0)
    valid = (voxel_depth > 0) & (sampled > 0) & (dist > -truncation)
    v, w, c = values.view(-1), weights.view(-1), colors.view(-1, 3)
    for b in range(B):
        m = valid[b, 0]
        old_w = w[m]
        total = old_w + 1.0
        v[m] = (v[m] * old_w + new[b, 0][m]) / total
        if sampled_color is not None:
            c[m] = (c[m] * old_w[:, None] + sampled_color[b][:, m].permute(1, 0)) / total[:, None]
        w[m] = torch.clamp(total, max=1.0)


def fake_launch(record=None):
    """A stand-in for functional.tsdf_integrate_launch on host tensors: the float64 restatement cast to fp32. `record`
    (a list) receives the arguments of every call."""
    import torch

    def launch(origin, voxel_size, truncation, values, weights, colors, w2c, K, depth, color):
        if record is not None:
            record.append(dict(origin=origin, voxel_size=voxel_size, truncation=truncation, w2c=w2c.clone(), K=K.clone(),
                               depth=depth.clone(), color=None if color is None else color.clone()))
        B = w2c.shape[0]
        if B == 0:
            return
        hom = torch.cat([w2c.double(), torch.tensor([0.0, 0, 0, 1]).expand(B, 1, 4).double()], 1)
        K3 = torch.cat([K.double(), torch.tensor([0.0, 0, 1]).expand(B, 1, 3).double()], 1)
        r = integrate_f64(np.float32(origin), np.float32(voxel_size), truncation, values.numpy(), weights.numpy(), colors.numpy(),
                          torch.inverse(hom).numpy(), K3.numpy(), depth.numpy(), None if color is None else color.numpy())
        values.copy_(torch.from_numpy(r["values"].astype(np.float32)))
        weights.copy_(torch.from_numpy(r["weights"].astype(np.float32)))
        colors.copy_(torch.from_numpy(r["colors"].astype(np.float32)))

    return launch
