"""float64 restatements for the point-cloud export tests (tests/test_pointcloud_cpu.py, tests/test_gpu_pointcloud.py): the
selection of exporter_utils.py:155-178 with OrientedBox.within (data/scene_box.py:95-108), and Open3D's
RemoveStatisticalOutliers — the mean distance to the k nearest neighbours (the query included, as SearchKNN returns it), the
threshold and the kept indices. Open3D was not available when this was written: the outlier part restates its source and
documentation and is this project's definition. Plus the generator of the test clouds and the table of cases."""
import numpy as np

# seed, n_surf, n_out, k, std_ratio, dup -> n, removed (scipy 1.15.3's cKDTree); the smallest relative distance of any avg from
# the threshold is at least 1.2e-3 over these cases
CASES = [
    dict(seed=0, n_surf=2000, n_out=24, k=20, ratio=10.0, dup=0, n=2024, removed=8),
    dict(seed=1, n_surf=2000, n_out=24, k=20, ratio=1.0, dup=0, n=2024, removed=24),
    dict(seed=2, n_surf=4099, n_out=40, k=20, ratio=2.0, dup=0, n=4139, removed=39),
    dict(seed=3, n_surf=513, n_out=7, k=8, ratio=2.0, dup=0, n=520, removed=7),
    dict(seed=4, n_surf=2000, n_out=24, k=20, ratio=10.0, dup=25, n=2049, removed=35),  # 26 points with avg == 0, all removed
    dict(seed=5, n_surf=37, n_out=0, k=20, ratio=1.0, dup=0, n=37, removed=8),
    dict(seed=6, n_surf=15, n_out=0, k=20, ratio=1.0, dup=0, n=15, removed=2),  # n < k
]
MIN_MARGIN = 1e-6  # every avg is at least this far (relative) from the threshold: what lets a test demand the identical kept set
AVG_RTOL = 1e-12  # at most 64 terms, each a sqrt within 1 ulp plus one summation rounding: 3e-14; times 30
UNSAFE_ULPS = 4  # a box coordinate within this many fp32 ulp of |half_scale| from a face is not compared with the reference
UNSAFE_CAP = 0.01


def cloud(seed, n_surf, n_out, dup=0):
    rs = np.random.RandomState(seed)
    v = rs.normal(size=(n_surf, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    surf = 0.5 * v + rs.normal(scale=0.004, size=(n_surf, 3))
    out = rs.uniform(-3, 3, size=(n_out, 3))
    pts = np.concatenate([surf, out])
    if dup:
        pts = np.concatenate([pts, np.repeat(pts[:1], dup, axis=0)])
    return pts[rs.permutation(len(pts))].astype(np.float32)


def case_cloud(case):
    return cloud(case["seed"], case["n_surf"], case["n_out"], case["dup"])


def ascending_mean(d):
    """rows of distances -> the sequential sum of each row in ascending order, over the row's length"""
    d = np.sort(np.asarray(d, dtype=np.float64), axis=1)
    total = np.zeros(d.shape[0])
    for j in range(d.shape[1]):
        total = total + d[:, j]
    return total / d.shape[1]


def knn_mean_distance_f64(points, k):
    from scipy.spatial import cKDTree

    p = np.asarray(points).astype(np.float64)
    kk = min(k, len(p))
    d, _ = cKDTree(p).query(p, k=kk)
    return ascending_mean(d.reshape(len(p), kk))


def knn_mean_distance_brute(points, k):
    """O(n^2): differences, squares, sum, sqrt in float64"""
    p = np.asarray(points).astype(np.float64)
    diff = p[:, None, :] - p[None, :, :]
    d = np.sqrt((diff[..., 0] ** 2 + diff[..., 1] ** 2) + diff[..., 2] ** 2)
    return ascending_mean(np.sort(d, axis=1)[:, :min(k, len(p))])


def threshold_f64(avg, std_ratio):
    valid = avg > 0
    count = int(valid.sum())
    mean = 0.0
    for a in avg[valid]:
        mean += a
    mean /= count
    dev2 = 0.0
    for a in avg[valid]:
        dev2 += (a - mean) * (a - mean)
    return mean + std_ratio * np.sqrt(dev2 / (count - 1))


def kept_indices(avg, threshold):
    return np.nonzero((avg > 0) & (avg < threshold))[0].astype(np.int64)


def margin(avg, threshold):
    """the smallest relative distance of a positive avg from the threshold"""
    a = avg[avg > 0]
    return float(np.min(np.abs(a - threshold) / threshold))


def world2box_f64(R, T):
    H = np.eye(4)
    H[:3, :3] = np.asarray(R, dtype=np.float64)
    H[:3, 3] = np.asarray(T, dtype=np.float64)
    return np.linalg.inv(H)[:3]


def box_coords_f64(points, world2box):
    p = np.asarray(points, dtype=np.float64)
    return p @ np.asarray(world2box, dtype=np.float64)[:, :3].T + np.asarray(world2box, dtype=np.float64)[:, 3]


def unsafe_rows(points, world2box, half_scale):
    """rows whose box coordinate lies within UNSAFE_ULPS fp32 ulp * |half_scale| of a face"""
    h = np.asarray(half_scale, dtype=np.float64)
    q = box_coords_f64(points, world2box)
    return (np.abs(np.abs(q) - h) <= UNSAFE_ULPS * 2.0 ** -23 * np.abs(h)).any(axis=1)


def select_f64(origins, directions, depth, rgb, alpha=None, normals01=None, world2box=None, half_scale=None):
    """-> dict(keep [n] bool, points (the fp32 o + d * depth, rounded per operation), colors, view_dirs, normals, unsafe): the
    point is the fp32 one the reference forms; the box test on it is float64."""
    o, d = np.asarray(origins, np.float32), np.asarray(directions, np.float32)
    t = np.asarray(depth, np.float32).reshape(-1, 1)
    points = o + (d * t).astype(np.float32)
    n = len(points)
    keep = np.ones(n, bool)
    colors = np.asarray(rgb, np.float32)
    if alpha is not None:
        a = np.asarray(alpha, np.float32).reshape(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            keep &= a > 0.5
            colors = (colors / np.maximum(a, np.float32(1e-10))[:, None]).astype(np.float32)
    unsafe = np.zeros(n, bool)
    if world2box is not None:
        h = np.asarray(half_scale, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            q = box_coords_f64(points, world2box)
            keep &= ((q > -h) & (q < h)).all(axis=1)
        unsafe = unsafe_rows(np.nan_to_num(points), world2box, half_scale)
    out = dict(keep=keep, points=points[keep], colors=colors[keep], view_dirs=d[keep], unsafe=unsafe, normals=None)
    if normals01 is not None:
        out["normals"] = (np.asarray(normals01, np.float32) * np.float32(2.0) - np.float32(1.0))[keep]
    return out
