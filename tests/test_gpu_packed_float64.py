"""The instant-ngp packed kernels (csrc/packed.hip) ENTRY BY ENTRY against float64 references of the same operations on
the kernels' own fp32 inputs (oracle/packed_oracle.py: packed_weights64, packed_weights_bwd64, packed_visibility64,
packed_composite64, packed_composite_bwd64), through the C ABI: nsamd_packed_info, _weights_fwd (weights AND
transmittance), _weights_bwd, _visibility, _compact, _composite_fwd / _bwd, _positions.

Every output buffer is filled with NaN (masks with 0xFF, integers with a sentinel) before the launch, so an entry the kernel
does not write fails. Every check is |got - ref64| <= bound per entry (check_entries of test_gpu_proposal_backward, whose
constants are used here: u = 2^-24 per fp32 operation, the double wave scans exact to 2^-53 of their abs sum per term,
expf within E_EXP, which test_expf_budget checks). The bounds come from the operation sequence, none from a result:

* Forward (packed_weights_kernel). dd = fl(fl(te - ts) * sigma): 2u relative (the reference takes the same fp32 product,
  the term is kept as in the dense bound). X = the exclusive prefix of dd, summed in double, cast to float:
  dX <= 2u prefix_abs + u |X| + cnt 2^-53 prefix_abs with cnt the ray's OWN count. T = expf(-X): T (dX + E_EXP).
  e = expf(-dd): e (2u |dd| + E_EXP). alpha = 1 - e: de + u |alpha| (absolute; the cancellation for small dd is carried as it
  is). w = alpha T: dalpha T + |alpha| dT + u |w|. A result below FLT_MIN may be flushed: + FTZ.
* Backward (packed_weights_bwd_kernel): dsigma_j = delta_j (g_j T_j e_j - sum_{i>j} g_i w_i). The bound is written for the
  arithmetic a CORRECT kernel may use, the transmittance from the FORWARD exclusive prefix (dX as above). It holds no term
  in `total * 2^-53`: a kernel that forms the prefix as total minus suffix loses total * 2^-53 ABSOLUTE in X, which is a
  relative error of T, and must fail once that is visible (oracle: prefix_by_total_minus_suffix; CPU restatement in
  tests/test_packed_reference_cpu.py). The suffix sum (double, cast): sum_{i>j} (|g_i| dw_i + dg_i |w_i| + u |g_i w_i|) + cnt
  2^-53 suf_abs + u |suf|. The own term: |g| (dT e + T de) + dg T e + 2u |own|. The difference + u, the product with delta + 2u.
  An upstream error dg (the chained case: the compositing backward's d_weights) enters both terms.
* Visibility: the mask must equal the float64 mask wherever the float64 margins |T - eps|, |alpha - thre| exceed the forward
  bounds dT, dalpha of that sample; the other samples are "ambiguous" and left out, and at most 0.1 % of a case may be
  (asserted here, and for the same seeds from the reference alone in the CPU file). A threshold of exactly 0 is never
  ambiguous on the transmittance side: expf returns no negative number and no NaN for a finite argument, so T >= 0 holds
  identically. The inputs have dd >= 0 only: the kernel's early `break` relies on T being non-increasing along the ray.
  Kept counts, the new packed_info and the compacted arrays are compared bit for bit with numpy boolean indexing by the
  DEVICE's mask, so the ambiguous samples do not leak into that comparison.
* Compositing forward (packed_composite_fwd_kernel): each lane adds its ceil(cnt / 64) products, the xor tree 6 more: a
  chain of ceil(cnt / 64) + 6 additions, one rounding per product and one for the cast of the reference's product:
  (chain + 2) u sum |w c| (the same for the accumulation and the depth's numerator). Constant background
  c + bg (1 - acc): dacc + u |1 - acc| for the difference, u for the product, u for the sum. Depth dsum / (acc + 1e-10):
  den = fl(acc + 1e-10f) carries dacc + u |den|; the quotient ddsum / den + |dsum| dden / den^2 + u |depth| (fp32 division is
  correctly rounded in this build). clamp is 1-Lipschitz. Empty rays: EXACTLY the background, 0 and 0.
* Compositing backward: d_rgb = w g: u |d_rgb|. d_weights: 3 products + up to 4 additions: 7u of the sum of |terms|.
* nsamd_packed_positions and the marcher: bit for bit against the same fp32 operations in numpy (the library is built
  with -ffp-contract=off; o + d * (ts + te) / 2 is a multiply feeding a divide, which no compiler may contract).
Every bound is multiplied by 1 + 2^-6 and carries 2^-140 (check_entries). The sign-coherent cases (all gradients, colours and
densities positive: sum |terms| = |sum|) make a lost or doubled 64-sample chunk exceed the bound instead of hiding under
a random-sign abs sum; so does the single ray that carries gradient among thousands that carry none.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import packed_oracle as po
from test_gpu_proposal_backward import D53, E_EXP, FTZ, SAFE, TINY, U, check_entries, report

pytestmark = pytest.mark.gpu

COUNT_SET = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 1023, 1024, 1025, 4097]
GEOMETRIES = ["edges", "n1", "n3", "n4", "n5", "n1023", "n1024", "n1025", "n2049", "n4096", "empty", "zero"]
BIG = [1e2, 1e4, 1e6, 1e8, 1e9, 1e10, 1e12, 1e20, 1e30]
AMBIGUOUS_CAP = 1e-3
BG = (0.25, 0.5, 0.75)


@pytest.fixture(scope="module")
def F():
    from nerfstudio_amd import _native, functional

    _native.load()
    return functional


def _n():
    from nerfstudio_amd import _native as N

    return N


# ---------------------------------------------------------------- cases (no GPU: shared with the CPU file) ---------------

def geometry_counts(name):
    """The counts vector of a geometry of GEOMETRIES (seeded). edges: every count of COUNT_SET (the 64-sample chunk's
    multiples +- 1, 1000+, 4097 = one sample into a second block of 64 chunks); nK: K rays (the 4 waves per workgroup, the
    1024-wide loop of packed_info_kernel), the large ones with bench-like counts; empty: rays without samples; zero: no rays."""
    rs = np.random.RandomState(sum(map(ord, name)))
    if name == "edges":  # every count of the set twice, shuffled; first ray, last ray and a run of 6 rays empty
        c = np.array([v for v in COUNT_SET if v > 0] * 2 + [0])
        rs.shuffle(c)
        c = np.concatenate([[0], c[:13], np.zeros(6, np.int64), c[13:], [0]])
    elif name == "empty":
        c = np.zeros(7, np.int64)
    elif name == "zero":
        c = np.zeros(0, np.int64)
    else:
        n = int(name[1:])
        if n <= 5:
            c = rs.choice([1, 2, 63, 64, 65, 129, 193, 1025], n)
        else:  # bench-like: mean about 30, a tail to 1500, a sixth of the rays empty
            c = np.minimum(1500, np.floor(np.exp(rs.normal(2.9, 1.2, n)))).astype(np.int64)
            c[rs.uniform(size=n) < 0.16] = 0
            c[rs.randint(n)] = 1500
    return c.astype(np.int64)


def info_from_counts(counts):
    counts = np.asarray(counts, np.int64)
    return np.stack([np.cumsum(counts) - counts, counts], axis=1).reshape(-1, 2)


def samples_case(counts, seed, sigma_scale=1.0):
    """t_starts, t_ends, sigmas (lognormal(0, 1.5), as tests/test_gpu_packed.py's case) for a counts vector."""
    rs = np.random.RandomState(seed)
    n = int(np.sum(counts))
    ts = np.concatenate([np.sort(rs.uniform(0.05, 6.0, c)) for c in counts] + [np.zeros(0)]).astype(np.float32)
    te = (ts + rs.uniform(0.005, 0.05, n)).astype(np.float32)
    sig = (rs.lognormal(0.0, 1.5, n) * sigma_scale).astype(np.float32)
    return ts, te, sig


def upstream(n, seed, kind):
    rs = np.random.RandomState(seed)
    g = rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 0, n)
    return (np.abs(g) if kind == "positive" else g).astype(np.float32)


def edge_values_case(seed):
    """The `edges` geometry with one treatment per ray in turn: a run of sigma = 0, samples with dt = 0, a total optical
    depth of 1e2 / 1e3 / 1e4 (T underflows in fp32 on the way), denormal dd."""
    counts = geometry_counts("edges")
    ts, te, sig = samples_case(counts, seed)
    info = info_from_counts(counts)
    rs = np.random.RandomState(seed + 1)
    for k, (s0, c) in enumerate(info):
        sl = slice(s0, s0 + c)
        kind = k % 6
        if c == 0:
            continue
        if kind == 0:
            sig[s0 + c // 3: s0 + max(c // 3 + 1, 2 * c // 3)] = 0.0
        elif kind == 1:
            z = rs.uniform(size=c) < 0.2
            te[sl][z] = ts[sl][z]
        elif kind in (2, 3, 4):
            total = float(((te[sl] - ts[sl]).astype(np.float64) * sig[sl]).sum())
            sig[sl] = (sig[sl] * (10.0 ** kind / total)).astype(np.float32)
        else:
            sig[sl] = np.float32(1e-42) * rs.randint(1, 9, c).astype(np.float32)
    return counts, ts, te, sig


def dense_sample_case(seed):
    """For every magnitude of BIG four rays of thin samples (dd in [0.001, 0.02]) with ONE sample of optical thickness
    `big`: at the first position and the last of 40, at position 30 of 40, at position 700 of 1000."""
    rs = np.random.RandomState(seed)
    counts, where = [], []
    for _ in BIG:
        counts += [40, 40, 40, 1000]
        where += [0, 39, 30, 700]
    counts = np.array(counts, np.int64)
    info = info_from_counts(counts)
    n = int(counts.sum())
    dt = np.float32(0.005)
    ts = np.concatenate([0.05 + np.arange(c) * 0.005 for c in counts]).astype(np.float32)
    te = (ts + dt).astype(np.float32)
    sig = (rs.uniform(0.001, 0.02, n) / 0.005).astype(np.float32)
    for k, (s0, _) in enumerate(info):
        sig[s0 + where[k]] = np.float32(BIG[k // 4] / 0.005)
    return counts, ts, te, sig


def crossing_case(eps):
    """Rays on which the float64 transmittance passes `eps` at a chosen sample m with a factor 2 to spare on both sides:
    T in [2 eps, 2.3 eps] in front of samples 1..m, <= eps / 2 behind sample m. m in chunk 0, a middle chunk, the ragged
    last chunk, exactly at the chunk boundaries (last kept sample 63 / 64 / 127 / 128), and never. Returns counts, ts, te,
    sigmas and the list of m (None: never crossed)."""
    rs = np.random.RandomState(5)
    cross = [20, 150, 280, 63, 64, 127, 128, None, 299, None]
    counts = np.array([300] * 9 + [256], np.int64)
    n = int(counts.sum())
    ts = np.concatenate([0.05 + np.arange(c) * 0.01 for c in counts]).astype(np.float32)
    te = (ts + np.float32(0.01)).astype(np.float32)
    dd = rs.uniform(0.5e-4, 1e-4, n)
    for k, (s0, c) in enumerate(info_from_counts(counts)):
        if cross[k] is not None:
            dd[s0] = math.log(1.0 / (2 * eps)) - 0.1
            dd[s0 + cross[k]] = math.log(4.0) + 0.1
    sig = (dd / (te - ts).astype(np.float64)).astype(np.float32)
    return counts, ts, te, sig, cross


def march_edge_case():
    """Rays 0-3: a direction component of -0.0 / an origin exactly on a slab plane of a parallel axis, inside the other slabs;
    4: on such a plane, outside another slab; 5, 6, 11: born inside the finest level; 7 / 8: outside every level pointing in /
    away; 9: t_min > t_max; 10: t_min == t_max."""
    roi = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    rs = np.random.RandomState(3)
    levels, res = 3, 8
    B = rs.rand(levels, res, res, res) > 0.4
    lim = float(1 << (levels - 1))
    o = np.array([[0.1, 0.2, -3.0], [0.3, -3.0, 0.1], [lim, 0.2, -3.5], [-lim, 0.1, 0.3], [lim, 5.0, 0.0], [0.1, 0.1, 0.1],
                  [0.2, -0.1, 0.05], [9.0, 9.0, 9.0], [9.0, 9.0, 9.0], [0.3, 0.3, -2.0], [0.0, 0.0, -3.0], [0.5, 0.5, 0.5]], np.float32)
    d = np.array([[-0.0, 0.0, 1.0], [0.6, 0.8, -0.0], [0.0, 0.0, 1.0], [-0.0, 0.6, 0.8], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8],
                  [0.0, 1.0, 0.0], [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [-0.0, -1.0, 0.0]], np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t_min = np.full(len(o), 0.0, np.float32)
    t_max = np.full(len(o), 30.0, np.float32)
    t_min[9], t_max[9] = 3.0, 2.0     # t_min > t_max: no samples
    t_min[10], t_max[10] = 2.5, 2.5   # an empty interval
    return roi, B, o, d, t_min, t_max


# ---------------------------------------------------------------- bounds -------------------------------------------------

def _z(x):
    return np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=0.0, neginf=0.0)


def _cnt_per_sample(info):
    info = np.asarray(info).reshape(-1, 2)
    return np.repeat(info[:, 1], info[:, 1]).astype(np.float64)


def forward_bounds(r, info):
    """dT, dalpha, dw per sample from packed_weights64's quantities (module docstring)."""
    S = _cnt_per_sample(info)
    dd, X, Xabs, T, e, alpha, w = (_z(r[k]) for k in ("dd", "X", "X_abs", "T", "e", "alpha", "w"))
    dX = 2 * U * Xabs + U * np.abs(X) + S * D53 * Xabs
    dT = T * (dX + E_EXP) + FTZ
    de = e * (2 * U * np.abs(dd) + E_EXP)
    dalpha = de + U * np.abs(alpha)
    dw = dalpha * T + np.abs(alpha) * dT + U * np.abs(w) + FTZ
    return dict(dT=dT, de=de, dalpha=dalpha, dw=dw)


def backward_bound(r, info, g_err=None):
    """Per-entry bound of nsamd_packed_weights_bwd from packed_weights_bwd64's quantities: forward exclusive prefix, no
    term in the ray's total."""
    S = _cnt_per_sample(info)
    f = forward_bounds(r, info)
    T, e, w, g, suf, delta = (_z(r[k]) for k in ("T", "e", "w", "g", "suf", "delta"))
    ge = np.zeros_like(g) if g_err is None else np.asarray(g_err, np.float64)
    dgw = np.abs(g) * f["dw"] + ge * np.abs(w) + U * np.abs(g * w) + FTZ
    tail = po.segment_exclusive_suffix64(dgw, info)
    dsuf = tail + S * D53 * _z(r["suf_abs"]) + U * np.abs(suf)
    own = g * T * e
    down = np.abs(g) * (f["dT"] * e + T * f["de"]) + ge * T * e + 2 * U * np.abs(own) + FTZ
    inner = own - suf
    dinner = down + dsuf + U * np.abs(inner)
    return np.abs(delta) * dinner + 2 * U * np.abs(delta * inner) + FTZ


def _chain(info):
    cnt = np.asarray(info).reshape(-1, 2)[:, 1].astype(np.float64)
    return np.ceil(cnt / 64) + 6


def composite_bounds(c, info, bg_mode):
    ch = _chain(info) + 2
    dacc = ch * U * c["acc_abs"]
    b_rgb = ch[:, None] * U * c["rgb_abs"]
    if bg_mode == 1:
        bg = np.abs(np.asarray(BG, np.float64))[None, :]
        rem = np.abs(1.0 - c["acc"])[:, None]
        b_rgb = b_rgb + bg * (dacc[:, None] + 2 * U * rem) + U * np.abs(c["sum_wc"] + np.asarray(BG)[None, :] * (1.0 - c["acc"])[:, None])
    out = dict(rgb=b_rgb, acc=dacc)
    if "depth" in c:
        den = c["acc"] + 1e-10
        dden = dacc + U * np.abs(den)
        out["depth"] = ch * U * c["depth_abs"] / den + np.abs(c["dsum"]) * dden / den**2 + U * np.abs(c["depth"])
    return out


def visibility_ambiguous(v, info, eps, thre):
    f = forward_bounds(v, info)
    amb_T = (np.abs(v["m_T"]) <= f["dT"] * SAFE + TINY) if eps != 0.0 else np.zeros(len(v["T"]), bool)
    return amb_T | (np.abs(v["m_alpha"]) <= f["dalpha"] * SAFE + TINY)


VIS_CASES = [("edges", 1e-4, 0.01), ("n1025", 1e-4, 0.01), ("n4096", 1e-4, 0.0), ("n2049", 0.0, 0.01), ("n4", 1e-2, 0.0),
             ("empty", 1e-4, 0.01), ("zero", 1e-4, 0.01)]


def visibility_inputs(geometry):
    counts = geometry_counts(geometry)
    ts, te, sig = samples_case(counts, 70 + len(counts), sigma_scale=3.0)
    return counts, ts, te, sig


# ---------------------------------------------------------------- launches ------------------------------------------------

_SPARE = []


def _p(t):
    """Device pointer of a tensor (None -> NULL). torch gives a tensor without elements a null pointer, which the entry
    points reject: a case without samples hands the launch a small spare allocation instead (nothing is written to it)."""
    if t is None:
        return None
    if t.numel() == 0:
        if not _SPARE:
            _SPARE.append(torch.zeros(64, dtype=torch.int64, device="cuda"))
        return _SPARE[0].data_ptr()
    return _n().ptr(t)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()


def _full(shape, value, dtype):
    return torch.full(tuple(shape), value, dtype=dtype, device="cuda")


def _nan(*shape):
    return _full(shape, float("nan"), torch.float32)


def run_info(counts):
    N = _n()
    lib = N.load()
    n = len(counts)
    cd = _dev(np.asarray(counts, np.int32))
    info = _full((n, 2), -7, torch.int64)
    total = _full((1,), -7, torch.int64)
    N.check(lib.nsamd_packed_info(_p(cd), n, _p(info), _p(total), N.stream()), "packed_info")
    torch.cuda.synchronize()
    return info, int(total[0])


def run_weights(ts, te, sig, info_d, g=None):
    """-> weights, transmittance[, dsigmas] as float64 numpy; NaN-prefilled outputs."""
    N = _n()
    lib, st = N.load(), N.stream()
    n, nr = len(ts), info_d.shape[0]
    tsd, ted, sgd = _dev(ts), _dev(te), _dev(sig)
    w, T = _nan(n), _nan(n)
    N.check(lib.nsamd_packed_weights_fwd(_p(tsd), _p(ted), _p(sgd), _p(info_d), nr, _p(w), _p(T), st), "weights_fwd")
    w2 = _nan(n)  # a null transmittance pointer gives the same weights
    N.check(lib.nsamd_packed_weights_fwd(_p(tsd), _p(ted), _p(sgd), _p(info_d), nr, _p(w2), None, st), "weights_fwd")
    out = [w, T]
    if g is not None:
        gd, ds = _dev(g), _nan(n)
        N.check(lib.nsamd_packed_weights_bwd(_p(tsd), _p(ted), _p(sgd), _p(gd), _p(info_d), nr, _p(ds), st),
                "weights_bwd")
        out.append(ds)
    torch.cuda.synchronize()
    assert torch.equal(w.view(torch.int32), w2.view(torch.int32))
    return [o.cpu().double().numpy() for o in out]


def check_weights(tag, ts, te, sig, counts, g, worst, info_d=None):
    info = info_from_counts(counts)
    if info_d is None:
        info_d = _dev(info)
    w, T, ds = run_weights(ts, te, sig, info_d, g)
    r = po.packed_weights_bwd64(ts, te, sig, info, g)
    f = forward_bounds(r, info)
    check_entries(f"{tag} T", T, r["T"], f["dT"], worst)
    check_entries(f"{tag} w", w, r["w"], f["dw"], worst)
    check_entries(f"{tag} dsigma", ds, r["dsigmas"], backward_bound(r, info), worst)
    return w, T, ds, r


# ---------------------------------------------------------------- packed_info --------------------------------------------

@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_packed_info_vs_cumsum(F, geometry):
    counts = geometry_counts(geometry)
    info, total = run_info(counts)
    np.testing.assert_array_equal(info.cpu().numpy(), info_from_counts(counts))
    assert total == int(counts.sum())


def test_packed_info_total_beyond_int32(F):
    """4097 rays of 2^20 samples: the running base passes 2^31 (and 2^32) inside the second 1024-ray trip; counts only."""
    counts = np.full(4097, 1 << 20, np.int64)
    counts[::5] += np.arange(len(counts[::5]))
    info, total = run_info(counts)
    assert total == int(counts.sum()) > 2**32
    np.testing.assert_array_equal(info.cpu().numpy(), info_from_counts(counts))


# ---------------------------------------------------------------- weights forward / backward ------------------------------

@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_packed_weights_vs_float64(F, geometry):
    """Weights, transmittance and dsigmas on lognormal densities with random-sign and with all-positive upstream gradients
    (densities and steps are positive: the second is sign-coherent throughout); packed_info from the kernel itself."""
    counts = geometry_counts(geometry)
    ts, te, sig = samples_case(counts, 11 + len(counts))
    info_d, total = run_info(counts)
    assert total == len(ts)
    worst = {}
    for kind in ("random", "positive"):
        g = upstream(len(ts), 3 + len(counts), kind)
        check_weights(kind, ts, te, sig, counts, g, worst, info_d)
    report(f"packed weights {geometry}", worst)


def test_packed_weights_single_ray_with_gradient(F):
    """One ray carries gradient among 4096: every other ray's dsigmas are exactly 0."""
    counts = geometry_counts("n4096")
    info = info_from_counts(counts)
    ts, te, sig = samples_case(counts, 21)
    worst = {}
    for ray in (int(np.argmax(counts)), int(np.flatnonzero(counts == 1)[0])):
        g = np.zeros(len(ts), np.float32)
        s0, c = info[ray]
        g[s0:s0 + c] = upstream(c, ray, "positive")
        _, _, ds, _ = check_weights(f"ray {ray} ({c})", ts, te, sig, counts, g, worst)
        others = np.ones(len(ts), bool)
        others[s0:s0 + c] = False
        assert np.all(ds[others] == 0.0) and np.any(ds[~others] != 0.0)
    report("packed weights, one ray with gradient", worst)


def test_packed_weights_edge_values_vs_float64(F):
    """sigma = 0 runs, dt = 0 samples, optical depth 1e2 .. 1e4 (T underflows), denormal dd."""
    counts, ts, te, sig = edge_values_case(31)
    worst = {}
    for kind in ("random", "positive"):
        _, T, _, r = check_weights(kind, ts, te, sig, counts, upstream(len(ts), 32, kind), worst)
    assert (T == 0).sum() > 100 and ((r["dd"] > 0) & (r["dd"] < 2.0**-126)).sum() > 100 and (r["delta"] == 0).sum() > 100
    report("packed weights edge values", worst)


def test_packed_weights_one_dense_sample_vs_float64(F):
    """One sample of optical thickness 1e2 .. 1e30 among thin ones (dense_sample_case): the transmittance in front of it must
    not feel it. Checked magnitude by magnitude so the report names the first that fails."""
    counts, ts, te, sig = dense_sample_case(41)
    info = info_from_counts(counts)
    failures, worst_all = [], {}
    for kind in ("positive", "random"):
        g = upstream(len(ts), 42, kind)
        w, T, ds = run_weights(ts, te, sig, _dev(info), g)
        r = po.packed_weights_bwd64(ts, te, sig, info, g)
        f, b = forward_bounds(r, info), backward_bound(r, info)
        for k, big in enumerate(BIG):
            lo, hi = info[4 * k, 0], info[4 * k + 3, 0] + info[4 * k + 3, 1]
            worst = {}
            try:
                check_entries(f"T {big:g}", T[lo:hi], r["T"][lo:hi], f["dT"][lo:hi], worst)
                check_entries(f"w {big:g}", w[lo:hi], r["w"][lo:hi], f["dw"][lo:hi], worst)
                check_entries(f"dsigma {big:g}", ds[lo:hi], r["dsigmas"][lo:hi], b[lo:hi], worst)
            except AssertionError as exc:
                failures.append(f"[{kind}] {exc}")
            worst_all.update({f"{kind[0]}:{k_}": v for k_, v in worst.items() if k_.startswith("dsigma")})
    report("packed weights, one dense sample", worst_all)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_packed_weights_nonfinite_density_on_one_sample(F, value):
    """sigma = +Inf / NaN on ONE sample of one ray: NaN exactly where float64 has NaN, equal where it is infinite, and every
    other ray bit for bit what it is without that value."""
    counts = geometry_counts("edges")
    info = info_from_counts(counts)
    ts, te, sig = samples_case(counts, 51)
    g = upstream(len(ts), 52, "random")
    ray = int(np.flatnonzero(counts == 193)[0])
    s0, c = info[ray]
    clean = run_weights(ts, te, sig, _dev(info), g)
    sig2 = sig.copy()
    sig2[s0 + 100] = value
    worst = {}
    got = check_weights(repr(value), ts, te, sig2, counts, g, worst)[:3]
    others = np.ones(len(ts), bool)
    others[s0:s0 + c] = False
    for a, b in zip(got, clean):
        assert np.array_equal(a[others], b[others])
    report(f"packed weights sigma = {value}", worst)


# ---------------------------------------------------------------- visibility + compaction --------------------------------

def _visibility_and_compact(tag, counts, ts, te, sig, eps, thre, worst):
    N = _n()
    lib, st = N.load(), N.stream()
    info = info_from_counts(counts)
    n, nr = len(ts), len(counts)
    info_d, tsd, ted, sgd = _dev(info), _dev(ts), _dev(te), _dev(sig)
    mask = _full((n,), 0xFF, torch.uint8)
    kept = _full((nr,), -7, torch.int32)
    N.check(lib.nsamd_packed_visibility(_p(tsd), _p(ted), _p(sgd), _p(info_d), nr, eps, thre, _p(mask), _p(kept),
                                        st), "packed_visibility")
    info2 = _full((nr, 2), -7, torch.int64)
    total = _full((1,), -7, torch.int64)
    N.check(lib.nsamd_packed_info(_p(kept), nr, _p(info2), _p(total), st), "packed_info")
    torch.cuda.synchronize()
    m = mask.cpu().numpy()
    assert np.isin(m, (0, 1)).all(), f"{tag}: {int((m > 1).sum())} mask entries not written"
    m = m.astype(bool)
    v = po.packed_visibility64(ts, te, sig, info, eps, thre)
    amb = visibility_ambiguous(v, info, np.float32(eps), np.float32(thre))
    share = float(amb.mean()) if n else 0.0
    worst[f"{tag} ambiguous"] = max(worst.get(f"{tag} ambiguous", 0.0), share / AMBIGUOUS_CAP)
    assert share <= AMBIGUOUS_CAP, f"{tag}: {int(amb.sum())} of {n} samples ambiguous"
    bad = np.flatnonzero((m != v["keep"]) & ~amb)
    assert bad.size == 0, f"{tag}: mask differs from float64 at {bad[:8]} ({bad.size}); T {v['T'][bad[:4]]}, alpha {v['alpha'][bad[:4]]}"
    ri = po.packed_ray_indices(info)
    kc = np.bincount(ri[m], minlength=nr)
    np.testing.assert_array_equal(kept.cpu().numpy(), kc)
    np.testing.assert_array_equal(info2.cpu().numpy(), info_from_counts(kc))
    mk = int(total[0])
    assert mk == int(m.sum())
    ri2 = _full((mk,), -7, torch.int64)
    ts2, te2 = _nan(mk), _nan(mk)
    N.check(lib.nsamd_packed_compact(_p(mask), _p(info_d), _p(info2), nr, _p(tsd), _p(ted), _p(ri2), _p(ts2),
                                     _p(te2), st), "packed_compact")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ri2.cpu().numpy(), ri[m])
    np.testing.assert_array_equal(ts2.cpu().numpy(), ts[m])
    np.testing.assert_array_equal(te2.cpu().numpy(), te[m])
    return m, v


@pytest.mark.parametrize("geometry,eps,thre", VIS_CASES)
def test_packed_visibility_and_compaction_vs_float64(F, geometry, eps, thre):
    counts, ts, te, sig = visibility_inputs(geometry)
    worst = {}
    m, v = _visibility_and_compact(geometry, counts, ts, te, sig, eps, thre, worst)
    if len(ts) > 1000 and eps > 0:
        assert (v["T"] < eps).sum() > 100 and 0.02 < m.mean() < 0.98, "the case must exercise early termination"
    report(f"packed visibility {geometry} eps={eps} thre={thre} (share of the 0.1 % cap)", worst)


@pytest.mark.parametrize("eps", [1e-4, 1e-2])
def test_packed_visibility_threshold_crossings(F, eps):
    """The transmittance passes eps in chunk 0, a middle chunk, the ragged last chunk, exactly after sample 63 / 64 / 127 /
    128 and at the last sample, or never: the kept samples are exactly 0..m, nothing is ambiguous."""
    counts, ts, te, sig, cross = crossing_case(eps)
    worst = {}
    m, v = _visibility_and_compact("crossings", counts, ts, te, sig, eps, 0.0, worst)
    assert worst["crossings ambiguous"] == 0.0
    for k, (s0, c) in enumerate(info_from_counts(counts)):
        last = c - 1 if cross[k] is None else cross[k]
        assert np.array_equal(m[s0:s0 + c], np.arange(c) <= last), (k, cross[k])
        T = v["T"][s0:s0 + c]
        assert T[:last + 1].min() >= 2 * eps and (last == c - 1 or T[last + 1:].max() <= eps / 2)
    report(f"packed visibility crossings eps={eps}", worst)


# ---------------------------------------------------------------- compositing --------------------------------------------

def composite_inputs(counts, seed, kind):
    rs = np.random.RandomState(seed)
    ts, te, sig = samples_case(counts, seed)
    info = info_from_counts(counts)
    n, nr = len(ts), len(counts)
    w = po.packed_weights64(ts, te, sig, info)["w"].astype(np.float32)
    scale = np.where(np.arange(nr) % 5 == 1, 1e-6, 1.0).astype(np.float32)  # rays of tiny accumulation: the 1e-10 matters
    w = (w * np.repeat(scale, counts)).astype(np.float32)
    if kind == "positive":
        rgb, g_rgb, g_acc = rs.uniform(0, 1, (n, 3)), rs.uniform(0.1, 1, (nr, 3)), rs.uniform(0.1, 1, nr)
    else:
        rgb, g_rgb, g_acc = rs.uniform(-0.5, 1.5, (n, 3)), rs.standard_normal((nr, 3)), rs.standard_normal(nr)
    return ts, te, w, rgb.astype(np.float32), g_rgb.astype(np.float32), g_acc.astype(np.float32)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_packed_composite_vs_float64(F, geometry):
    """nsamd_packed_composite_fwd / _bwd: background none / a constant colour, g_accumulation present / null, depth requested /
    null, d_rgb requested / null; eval mode with NaN colours and sums clamped at both ends; empty rays exactly the
    background, 0, 0; random-sign and all-positive inputs."""
    N = _n()
    lib, st = N.load(), N.stream()
    counts = geometry_counts(geometry)
    info = info_from_counts(counts)
    nr = len(counts)
    info_d = _dev(info)
    ri_d = _dev(po.packed_ray_indices(info))
    bgv = (C.c_float * 3)(*BG)
    empty = counts == 0
    worst = {}
    for kind in ("random", "positive"):
        ts, te, w, rgb, g_rgb, g_acc = composite_inputs(counts, 60 + nr, kind)
        n = len(ts)
        tsd, ted, wd, cd, grd, gad = (_dev(a) for a in (ts, te, w, rgb, g_rgb, g_acc))
        for bg_mode in (0, 1):
            for depth in (True, False):
                o_rgb, o_acc, o_dep = _nan(nr, 3), _nan(nr), _nan(nr)
                N.check(lib.nsamd_packed_composite_fwd(_p(cd), _p(wd), _p(tsd) if depth else None,
                                                       _p(ted) if depth else None, _p(info_d), nr, bg_mode,
                                                       bgv if bg_mode else None, 0, _p(o_rgb), _p(o_acc),
                                                       _p(o_dep) if depth else None, st), "composite_fwd")
                torch.cuda.synchronize()
                c = po.packed_composite64(rgb, w, ts if depth else None, te if depth else None, info, bg_mode, BG)
                b = composite_bounds(c, info, bg_mode)
                tag = f"{kind[0]} bg{bg_mode}"
                check_entries(f"{tag} rgb", o_rgb, c["rgb"], b["rgb"], worst)
                check_entries(f"{tag} acc", o_acc, c["acc"], b["acc"], worst)
                bg_exact = np.asarray(BG, np.float32) if bg_mode else np.zeros(3, np.float32)
                assert np.array_equal(o_rgb.cpu().numpy()[empty], np.broadcast_to(bg_exact, (int(empty.sum()), 3)))
                assert np.all(o_acc.cpu().numpy()[empty] == 0.0)
                if depth:
                    check_entries(f"{tag} depth", o_dep, c["depth"], b["depth"], worst)
                    assert np.all(o_dep.cpu().numpy()[empty] == 0.0)
                else:
                    assert bool(torch.isnan(o_dep).all())  # not touched
            for with_acc in (True, False):
                for with_rgb in (True, False):
                    d_rgb, d_w = _nan(n, 3), _nan(n)
                    N.check(lib.nsamd_packed_composite_bwd(_p(cd), _p(wd), _p(ri_d), n, bg_mode, bgv if bg_mode else None,
                                                           _p(grd), _p(gad) if with_acc else None,
                                                           _p(d_rgb) if with_rgb else None, _p(d_w), st), "composite_bwd")
                    torch.cuda.synchronize()
                    cb = po.packed_composite_bwd64(rgb, w, info, bg_mode, BG, g_rgb, g_acc if with_acc else None)
                    check_entries(f"{kind[0]} bg{bg_mode} d_w", d_w, cb["d_weights"], 7 * U * cb["dw_abs"], worst)
                    if with_rgb:
                        check_entries(f"{kind[0]} bg{bg_mode} d_rgb", d_rgb, cb["d_rgb"], U * np.abs(cb["d_rgb"]) + FTZ, worst)
        # eval mode: NaN colours count as 0, the result is clamped (colours in [-0.5, 1.5]: both ends are reached)
        bad = rgb.copy()
        bad[::11] = np.nan
        badd = _dev(bad)
        for bg_mode in (0, 1):
            o_rgb, o_acc = _nan(nr, 3), _nan(nr)
            N.check(lib.nsamd_packed_composite_fwd(_p(badd), _p(wd), None, None, _p(info_d), nr, bg_mode,
                                                   bgv if bg_mode else None, 1, _p(o_rgb), _p(o_acc), None, st), "composite_fwd")
            torch.cuda.synchronize()
            c = po.packed_composite64(bad, w, None, None, info, bg_mode, BG, eval_mode=True)
            check_entries(f"{kind[0]} eval bg{bg_mode} rgb", o_rgb, c["rgb"], composite_bounds(c, info, bg_mode)["rgb"], worst)
            got = o_rgb.cpu().numpy()
            assert got.size == 0 or (got.min() >= 0.0 and got.max() <= 1.0)
            if kind == "random" and nr >= 1000:
                assert (got == 0.0).sum() > 0 and (got == 1.0).sum() > 0
    report(f"packed composite {geometry}", worst)


# ---------------------------------------------------------------- positions ------------------------------------------------

@pytest.mark.parametrize("geometry", ["edges", "n5", "n4096", "empty"])
def test_packed_positions_bit_exact(F, geometry):
    N = _n()
    lib = N.load()
    counts = geometry_counts(geometry)
    info = info_from_counts(counts)
    ts, te, _ = samples_case(counts, 80)
    rs = np.random.RandomState(81)
    o = rs.standard_normal((len(counts), 3)).astype(np.float32)
    d = rs.standard_normal((len(counts), 3)).astype(np.float32)
    ri = po.packed_ray_indices(info)
    n = len(ts)
    od, dd_, rid, tsd, ted = _dev(o), _dev(d), _dev(ri), _dev(ts), _dev(te)
    pos = _nan(n, 3)
    N.check(lib.nsamd_packed_positions(_p(od), _p(dd_), _p(rid), _p(tsd), _p(ted), n, _p(pos), N.stream()),
            "packed_positions")
    torch.cuda.synchronize()
    span = (ts + te).astype(np.float32)
    ref = (o[ri] + ((d[ri] * span[:, None]).astype(np.float32) / np.float32(2.0)).astype(np.float32)).astype(np.float32)
    np.testing.assert_array_equal(pos.cpu().numpy(), ref)


# ---------------------------------------------------------------- marcher edges ----------------------------------------------

def test_occgrid_march_edge_rays_bit_exact_vs_oracle(F):
    """Through the existing bit-exact comparison: a direction component of -0.0, an origin exactly on a slab plane of a
    parallel axis (inside and outside the other slabs: the 0 * inf branch of ray_box), t_min > t_max, near == far, a ray
    born inside the finest level, one outside every level pointing in and one pointing away."""
    roi, B, o, d, t_min, t_max = march_edge_case()
    n = len(o)
    dv = lambda a: torch.from_numpy(a).cuda()
    step = 0.05
    for near, far in ((0.05, 100.0), (1.5, 1.5)):
        ref = po.occgrid_march(o, d, B, roi, step, near_plane=near, far_plane=far, t_min=t_min, t_max=t_max)
        got = F.occgrid_march(dv(o), dv(d), dv(B.astype(np.uint8)), roi, step, near, far, dv(t_min), dv(t_max), 0.0, None)
        for a, b in zip(got[:3], ref):
            np.testing.assert_array_equal(a.cpu().numpy(), b)
        cnt = np.bincount(ref[0], minlength=n)
        np.testing.assert_array_equal(got[3].cpu().numpy()[:, 1], cnt)
        if near == far:
            assert cnt.sum() == 0
        else:
            assert cnt[[0, 1, 2, 3, 5, 6, 7, 11]].min() > 0 and cnt[[4, 8, 9, 10]].max() == 0, cnt


# ---------------------------------------------------------------- the benchmark's shape, chained -----------------------------

def test_bench_shape_packed_chain_vs_float64(F):
    """4096 rays, counts and t from the marcher on the benchmark's occupancy grid, densities = the kernels' own candidate
    densities of one NgpTrainStep.forward: visibility -> packed_info -> compact -> weights -> composite -> composite backward
    -> weights backward through the C ABI, every stage against float64 of the SAME stage on the device's own inputs of that
    stage (the compositing backward's error enters the weights backward's bound as dg)."""
    import bench
    from scripts.bench_ngp import build_ngp

    N = _n()
    lib, st = N.load(), N.stream()
    F._SCATTER_WS.clear()
    model, arena, tr, _ = build_ngp(torch.device("cuda"), bench.synthetic_rays)
    r, n = tr.runner, bench.RAYS_PER_GPU
    rs = np.random.RandomState(17)
    r.forward(torch.from_numpy(rs.uniform(0, 1, n).astype(np.float32)).cuda())
    torch.cuda.synchronize()
    mc = r.num_candidates
    counts = r.info.cpu().numpy()[:, 1]
    assert mc == counts.sum() > 20 * n and counts.max() > 64  # (rays of more than one chunk)
    ts, te, sig = (t[:mc].cpu().numpy() for t in (r.c_ts, r.c_te, r.c_sigma))
    assert np.isfinite(sig).all() and (sig >= 0).all()
    worst = {}
    m, _ = _visibility_and_compact("candidates", counts, ts, te, sig, 1e-4, min(float(model.config.alpha_thre),
                                                                               float(model.occupancy_grid._occ_mean)), worst)
    ri = po.packed_ray_indices(info_from_counts(counts))
    kc = np.bincount(ri[m], minlength=n)
    info2 = info_from_counts(kc)
    ts2, te2, sig2 = ts[m], te[m], sig[m]
    mk = len(ts2)
    assert mk > 10 * n
    # weights on the kept samples; the compositing on the device's own weights; its backward; the weights backward on the
    # device's own d_weights
    info_d, tsd, ted, sgd = _dev(info2), _dev(ts2), _dev(te2), _dev(sig2)
    w, T = _nan(mk), _nan(mk)
    N.check(lib.nsamd_packed_weights_fwd(_p(tsd), _p(ted), _p(sgd), _p(info_d), n, _p(w), _p(T), st), "weights_fwd")
    rw = po.packed_weights64(ts2, te2, sig2, info2)
    f = forward_bounds(rw, info2)
    check_entries("T", T, rw["T"], f["dT"], worst)
    check_entries("w", w, rw["w"], f["dw"], worst)
    rgb = rs.uniform(0, 1, (mk, 3)).astype(np.float32)
    g_rgb = (rs.standard_normal((n, 3)) * 1e-3).astype(np.float32)
    cd, grd, rid = _dev(rgb), _dev(g_rgb), _dev(ri[m])
    bgv = (C.c_float * 3)(*BG)
    o_rgb, o_acc, o_dep = _nan(n, 3), _nan(n), _nan(n)
    N.check(lib.nsamd_packed_composite_fwd(_p(cd), _p(w), _p(tsd), _p(ted), _p(info_d), n, 1, bgv, 0, _p(o_rgb),
                                           _p(o_acc), _p(o_dep), st), "composite_fwd")
    torch.cuda.synchronize()
    w_dev = w.cpu().numpy()
    c = po.packed_composite64(rgb, w_dev, ts2, te2, info2, 1, BG)
    b = composite_bounds(c, info2, 1)
    for k, o_ in (("rgb", o_rgb), ("acc", o_acc), ("depth", o_dep)):
        check_entries(k, o_, c[k], b[k], worst)
    d_rgb, d_w = _nan(mk, 3), _nan(mk)
    N.check(lib.nsamd_packed_composite_bwd(_p(cd), _p(w), _p(rid), mk, 1, bgv, _p(grd), None, _p(d_rgb), _p(d_w),
                                           st), "composite_bwd")
    cb = po.packed_composite_bwd64(rgb, w_dev, info2, 1, BG, g_rgb, None)
    check_entries("d_rgb", d_rgb, cb["d_rgb"], U * np.abs(cb["d_rgb"]) + FTZ, worst)
    check_entries("d_w", d_w, cb["d_weights"], 7 * U * cb["dw_abs"], worst)
    ds = _nan(mk)
    N.check(lib.nsamd_packed_weights_bwd(_p(tsd), _p(ted), _p(sgd), _p(d_w), _p(info_d), n, _p(ds), st), "weights_bwd")
    torch.cuda.synchronize()
    rb = po.packed_weights_bwd64(ts2, te2, sig2, info2, d_w.cpu().numpy())
    check_entries("dsigma", ds, rb["dsigmas"], backward_bound(rb, info2), worst)
    # ... and against float64 of the whole tail (float64 d_weights): the upstream error enters as dg
    rb2 = po.packed_weights_bwd64(ts2, te2, sig2, info2, cb["d_weights"])
    check_entries("dsigma (chained)", ds, rb2["dsigmas"], backward_bound(rb2, info2, 7 * U * cb["dw_abs"]), worst)
    report(f"bench-shape packed chain ({mc} candidates, {mk} kept)", worst)
