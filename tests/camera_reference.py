"""float64 references, per-entry error bounds and the shared inputs for the camera-pose kernels of csrc/camera.hip
(nsamd_camera_apply, nsamd_camera_backward). tests/test_camera_reference_cpu.py pins this module to csrc/camera.h as the host
compiler sees it (tests/hostcheck) and to tests/golden/camera_opt.npz; tests/test_gpu_camera_pose.py holds the kernels to it.

Reference. The package's torch mirror of the exponential maps (nerfstudio_amd.cameras.lie_groups) evaluated in double on the
fp32 pose; forward o = raw_o + t[c], d = R[c] raw_d; backward torch autograd in double through exactly that expression plus
CameraOptimizer.get_loss_dict's regulariser (with the penalties as the fp32 numbers the kernel receives). The per-ray upstream
gradient is the sum of the levels' buffers taken in fp32 in list order from 0.0f, as the kernel takes it (numpy: the same bits).
Camera indices are clamped to [0, C) as both kernels do before any read.

Branch points. The kernel decides its branches on fp32 quantities (|w|^2 against 1e-4f, |w| against 1e-2f), its backward on the
double |w|^2 against 1e-4f, the mirror in double against 1e-4 / 1e-2. Inside a window of a few 1e-12 around the branch points
these can disagree, and the two sides are then different functions (the clamp's gradient is discontinuous). `check_branches`
refuses poses closer than 1e-9 (|w|^2) / 1e-8 (|w|) to a branch point — a hundred times the window and the fp32 rounding of
those quantities; the pose set comes within a relative 1e-5 of both branch points from both sides, where the cancellation in
1 - cos and t - sin is at its worst.

Forward bound (u = 2^-24). `V` carries a float64 value with a rigorous absolute error bound through the kernel's own operation
sequence (cam_exp_map and the 3-term dot product, in the kernel's order and association):
    x (+|-) y : e_x + e_y, then one rounding                  x y : |x| e_y + |y| e_x + e_x e_y, then one rounding
    x / y     : (e_x + |x / y| e_y) / (|y| - e_y), one rounding  (division is correctly rounded)
    sqrt x    : e_x / (sqrt x + sqrt(x - e_x)), one rounding      (correctly rounded)
    max(x, c) : e_x + |c - fl32(c)| (1-Lipschitz; the mirror clamps at the double 1e-4, the kernel at 1e-4f)
    sin x     : e_x, then E_TRIG (|sin x| + e_x);   cos x : (|sin x| + e_x) e_x, then E_TRIG (|cos x| + e_x)
    a rounding adds u (|value| + error so far); constants that fp32 does not hold (1/6, 1e-4) carry |c - fl32(c)|; negation,
    halving, adding 0.0f and the reads of the inputs are exact.
E_TRIG = 2 k u for k ulp: the device's sinf / cosf are CHARGED 2 ulp each — an assumption, as E_EXP in float64_check.py; the
ratios under a 1-ulp charge are reported beside it (profiles/camera_pose_float64_ratios.txt). The cancellations are carried
by the rules themselves: just above the branch points 1 - cos t = 5e-5 carries cos's 1.2e-7 (relative 2.4e-3, into
b = (1 - cos) / t^2 and on into b w w^T, absolute ~1e-7), and t - sin t = 1.7e-7 carries sin's 1.9e-9 (relative 1e-2, into
(t - sin t) / t^3 and on into the SE3 translation, times |w|^2 |v|). The value track doubles as a check of the restatement: it
must agree with the mirror to 1e-12 relative.
SO3xR3 origins are fl(raw_o + v): no rounding precedes the sum, the bound is zero (same bits).

Backward bound. The kernel is double up to `dpose[k] += (float)dp[k] + (float)dr[k]`: fl(dp), fl(dr), fl of their sum and fl of
the sum with what dpose held — four roundings, of which those with an exactly-zero operand are exact and are not charged (zero
penalties or a zero norm: dr = 0; dpose pre-filled with zero). So
    bound = u |dp| + [dr != 0] (u |dr| + u |dp + dr|) + [old != 0] u |old + dp + dr| + 2^-40 A,
where the last term stands for the double-precision rounding of two different but equivalent closed forms (the kernel's
derivative formulas, autograd through the mirror): A = sum_ij |d out_ij / d p_k| (sum_rays |G_ij terms|) + |dr_k| is the sum of
the absolute values of the terms entering the entry, and 2^-40 is 2^13 double roundings' worth of slack, still 2^16 below the
fp32 roundings. Regulariser value `(float)(mean |v|) tp + (float)(mean |w|) rp`: five fp32 roundings on double means,
2u (|mv tp| + |mw rp|) + u |value|, plus 2^-40 of the same."""
import numpy as np
import torch

from float64_check import U

F32 = np.float32
MODES = {"SO3xR3": 1, "SE3": 2}
D40 = 2.0**-40


def trig_charge(ulp):
    return 2.0 * ulp * U


# ---------------------------------------------------------------------------------------------------------------- inputs
def special_poses():
    """The host test's set (tests/test_kernel_helpers_cpu.py) — random N(0, 0.3), |w| ~ 5e-4, |w| around both branch points,
    exact zero, pure translation, pure rotation — plus |w| = 3.1 and 5 (near and past pi), |v| = 50, and |w| within a relative
    1e-5 and 1e-3 of the branch point 1e-2 (|w|^2 = 1e-4) from both sides."""
    rs = np.random.RandomState(3)
    pose = rs.normal(0, 0.3, (40, 6)).astype(F32)
    pose[:8, 3:] *= 1e-3
    pose[8:16, 3:] *= 2e-2
    pose[16] = 0.0
    pose[17, 3:] = 0.0
    pose[18, :3] = 0.0

    def with_norm(row, part, length):
        x = pose[row, part].astype(np.float64)
        pose[row, part] = (x * (length / np.linalg.norm(x))).astype(F32)

    with_norm(19, slice(3, 6), 3.1)
    with_norm(20, slice(3, 6), 5.0)
    with_norm(21, slice(0, 3), 50.0)
    for k, rel in enumerate((1e-5, -1e-5, 1e-3, -1e-3)):
        with_norm(22 + k, slice(3, 6), 1e-2 * (1 + rel))
    pose[26, 3:] = np.array([1e-2 * (1 + 1e-5), 0, 0], F32)  # along one axis: K K has exact zeros
    pose[27, 3:] = np.array([0, 0, -1e-2 * (1 - 1e-5)], F32)
    with_norm(28, slice(3, 6), 1e-2 * (1 + 1e-5))
    with_norm(28, slice(0, 3), 50.0)  # the worst of the SE3 translation: (t - sin t) / t^3 just above the branch, times |v|
    return pose


def poses(C, seed=0):
    """[C, 6] fp32: the special poses (cyclically shifted by `seed`, so that small C sees every one of them over the seeds), then
    random N(0, 0.3)."""
    sp = np.roll(special_poses(), -seed, axis=0)
    if C <= sp.shape[0]:
        out = sp[:C].copy()
    else:
        out = np.concatenate([sp, np.random.RandomState(100 + seed).normal(0, 0.3, (C - sp.shape[0], 6)).astype(F32)])
    check_branches(out)
    return out


def check_branches(pose):
    w = pose[:, 3:].astype(np.float64)
    nrm = (w * w).sum(1)
    assert (np.abs(nrm - 1e-4) > 1e-9).all() and (np.abs(np.sqrt(nrm) - 1e-2) > 1e-8).all(), "a pose inside a branch window"
    w32 = pose[:, 3:]
    nrm32 = (w32[:, 0] * w32[:, 0] + w32[:, 1] * w32[:, 1]) + w32[:, 2] * w32[:, 2]
    assert np.array_equal(nrm32 >= F32(1e-4), nrm >= 1e-4) and np.array_equal(np.sqrt(nrm32) < F32(1e-2), np.sqrt(nrm) < 1e-2)


def rays(n, C, seed, cams=None):
    """raw origins ~ N(0, 1), unit raw directions, camera indices (random in [0, C) unless given)."""
    rs = np.random.RandomState(seed)
    o = rs.normal(0, 1, (n, 3)).astype(F32)
    d = rs.normal(0, 1, (n, 3))
    d = (d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)).astype(F32)
    c = rs.randint(0, C, n).astype(np.int64) if cams is None else np.broadcast_to(np.asarray(cams, np.int64), (n,)).copy()
    return o, d, c


def upstream_levels(n, count, seed):
    """`count` pairs of [n, 3] fp32 level buffers spanning 1e-6 .. 1e3 such that the fp32 ORDER of the level sum matters: level 1
    nearly cancels level 0 (~1e3), so in list order the ~1e-6 and ~1e-2 levels are added to a sum of order 1, in any other order
    to one of order 1e3 (ulp 6e-5)."""
    rs = np.random.RandomState(seed)

    def one():
        big = (1e3 * rs.normal(0, 1, (n, 3))).astype(F32)
        lv = [big, (-big + rs.normal(0, 1, (n, 3)).astype(F32)).astype(F32), (1e-6 * rs.normal(0, 1, (n, 3))).astype(F32),
              (1e-2 * rs.normal(0, 1, (n, 3))).astype(F32)]
        return [np.ascontiguousarray(x) for x in lv[:count]]

    return one(), one()


def level_sum32(levels, n):
    """The kernel's `so = 0.0f; for l: so += level[l]` in fp32."""
    s = np.zeros((n, 3), F32)
    for lv in levels:
        s = s + np.asarray(lv, F32)
    assert s.dtype == F32
    return s


def clamp_cams(cams, C):
    return np.clip(np.asarray(cams, np.int64), 0, C - 1)


# ------------------------------------------------------------------------------------------------------- float64 reference
def _exp_map(mode):
    from nerfstudio_amd.cameras.lie_groups import exp_map_SE3, exp_map_SO3xR3

    return exp_map_SO3xR3 if mode == "SO3xR3" else exp_map_SE3


def forward64(mode, pose, raw_o, raw_d, cams):
    """-> (origins, directions) float64 [n, 3]."""
    C = pose.shape[0]
    c = _exp_map(mode)(torch.from_numpy(pose.astype(np.float64)))[torch.from_numpy(clamp_cams(cams, C))]
    o = torch.from_numpy(raw_o.astype(np.float64)) + c[:, :, 3]
    d = torch.bmm(c[:, :, :3], torch.from_numpy(raw_d.astype(np.float64))[..., None]).squeeze(-1)
    return o.numpy(), d.numpy()


def backward64(mode, pose, raw_d, cams, d_origins, d_directions, trans_pen, rot_pen, dpose_old):
    """The kernel's outputs in double with their bounds: dict(dpose, dpose_bound, reg, reg_bound, dp, dr, jac)."""
    from nerfstudio_amd.cameras.camera_optimizers import CameraOptimizer, CameraOptimizerConfig

    C, n = pose.shape[0], raw_d.shape[0]
    tp, rp = float(F32(trans_pen)), float(F32(rot_pen))
    opt = CameraOptimizer(CameraOptimizerConfig(mode=mode, trans_l2_penalty=tp, rot_l2_penalty=rp), num_cameras=C, device="cpu").double()
    with torch.no_grad():
        opt.pose_adjustment.copy_(torch.from_numpy(pose.astype(np.float64)))
    idx = torch.from_numpy(clamp_cams(cams, C))
    go = torch.from_numpy(level_sum32(d_origins, n).astype(np.float64))
    gd = torch.from_numpy(level_sum32(d_directions, n).astype(np.float64))
    rd = torch.from_numpy(raw_d.astype(np.float64))
    # the rays' share
    c = opt(idx)
    o = c[:, :, 3]  # (+ raw_o: a constant)
    d = torch.bmm(c[:, :, :3], rd[..., None]).squeeze(-1)
    (dp,) = torch.autograd.grad((o * go).sum() + (d * gd).sum(), opt.pose_adjustment, allow_unused=True)
    dp = torch.zeros(C, 6, dtype=torch.float64) if dp is None else dp
    # the regulariser's
    ld = {}
    opt.get_loss_dict(ld)
    reg = ld["camera_opt_regularizer"]
    (dr,) = torch.autograd.grad(reg, opt.pose_adjustment)
    dp, dr, reg = dp.numpy(), dr.numpy(), float(reg.detach())
    # A: |Jacobian|^T (absolute sums of the upstream terms) + |dr|
    G_abs = np.zeros((C, 3, 4))
    np.add.at(G_abs[:, :, :3], idx.numpy(), np.abs(gd.numpy())[:, :, None] * np.abs(rd.numpy())[:, None, :])
    np.add.at(G_abs[:, :, 3], idx.numpy(), np.abs(go.numpy()))
    p = torch.from_numpy(pose.astype(np.float64)).requires_grad_(True)
    out = _exp_map(mode)(p)
    A = np.abs(dr).copy()
    jac = np.zeros((C, 3, 4, 6))  # d out_ij / d p_k per camera
    for i in range(3):
        for j in range(4):
            (J,) = torch.autograd.grad(out[:, i, j].sum(), p, retain_graph=True)
            jac[:, i, j] = J.numpy()
            A += np.abs(J.numpy()) * G_abs[:, i, j][:, None]
    old = dpose_old.astype(np.float64)
    new = old + dp + dr
    bound = U * np.abs(dp) + (dr != 0) * (U * np.abs(dr) + U * np.abs(dp + dr)) + (old != 0) * U * np.abs(new) + D40 * A
    mv = np.sqrt((pose[:, :3].astype(np.float64) ** 2).sum(1)).mean() * tp
    mw = np.sqrt((pose[:, 3:].astype(np.float64) ** 2).sum(1)).mean() * rp
    assert abs(mv + mw - reg) <= 1e-14 * max(reg, 1e-300) + 1e-300
    reg_bound = (2 * U + D40) * (abs(mv) + abs(mw)) + U * abs(reg)
    return dict(dpose=new, dpose_bound=bound, reg=reg, reg_bound=reg_bound, dp=dp, dr=dr, jac=jac)


# ---------------------------------------------------------------------------------------------------- forward error bound
class V:
    """float64 value(s) with an absolute error bound of the fp32 computation that produced them."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) + e

    def __getitem__(self, k):
        return V(self.v[k], self.e[k])

    def __neg__(self):
        return V(-self.v, self.e)

    def half(self):
        return V(0.5 * self.v, 0.5 * self.e)

    def __add__(self, o):
        o = _of(o)
        return _rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = _of(o)
        return _rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return _of(o) - self

    def __mul__(self, o):
        o = _of(o)
        return _rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _of(o)
        q = self.v / o.v
        return _rounded(q, (self.e + np.abs(q) * o.e) / (np.abs(o.v) - o.e))

    def __rtruediv__(self, o):
        return _of(o) / self


def _of(x):
    if isinstance(x, V):
        return x
    x = float(x)
    return V(x, abs(x - float(F32(x))))  # a constant as fp32 holds it


def _rounded(v, e):
    return V(v, e + U * (np.abs(v) + e))


def _sqrt(x):
    r = np.sqrt(x.v)
    den = r + np.sqrt(np.maximum(x.v - x.e, 0.0))
    return _rounded(r, np.where(x.e > 0, x.e / np.where(den > 0, den, 1.0), 0.0))


def _max(x, c):
    return V(np.maximum(x.v, c), x.e + abs(c - float(F32(c))))


def _sin(x, E):
    s = np.sin(x.v)
    return V(s, x.e + E * (np.abs(s) + x.e))


def _cos(x, E):
    c = np.cos(x.v)
    e = (np.abs(np.sin(x.v)) + x.e) * x.e
    return V(c, e + E * (np.abs(c) + e))


def _where(cond, a, b):
    return V(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))


def exp_map_tracked(mode, pose, trig_ulp=2.0):
    """cam_exp_map (csrc/camera.h) operation by operation on [C, 6] fp32 poses -> (R: 9 V of shape [C] row-major, t: 3 V)."""
    E = trig_charge(trig_ulp)
    v = [V(pose[:, k]) for k in range(3)]
    w = [V(pose[:, 3 + k]) for k in range(3)]
    zero = V(np.zeros(pose.shape[0]))
    nrm = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if mode == "SO3xR3":
        th = _sqrt(_max(nrm, 1e-4))
        inv = 1.0 / th
        a = inv * _sin(th, E)
        b = (inv * inv) * (1.0 - _cos(th, E))
        K = [zero, -w[2], w[1], w[2], zero, -w[0], -w[1], w[0], zero]
        R = []
        for i in range(3):
            for j in range(3):
                k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j]
                x = a * K[3 * i + j] + b * k2
                R.append(x + 1.0 if i == j else x)  # (+ 0.0f off the diagonal: exact)
        return R, v
    th = _sqrt(nrm)
    small = np.sqrt(nrm.v) < 1e-2
    t2 = th * th
    t3 = t2 * th
    one = V(np.ones(pose.shape[0]))
    th_s, t2_s, t3_s = _where(small, one, th), _where(small, one, t2), _where(small, one, t3)  # (the unused arm must not divide by 0)
    sn = _sin(th, E)
    cs = _where(small, 8.0 / (4.0 + t2) - 1.0, _cos(th, E))
    a = _where(small, cs.half() + 0.5, sn / th_s)
    b = _where(small, a.half(), (1.0 - cs) / t2_s)
    R = []
    for i in range(3):
        for j in range(3):
            x = (b * w[i]) * w[j]
            R.append(x + cs if i == j else x)  # (+ 0.0f off the diagonal: exact)
    s = [a * w[k] for k in range(3)]
    R[1], R[3], R[2], R[6], R[5], R[7] = R[1] - s[2], R[3] + s[2], R[2] + s[1], R[6] - s[1], R[5] - s[0], R[7] + s[0]
    at = _where(small, 1.0 - t2 / 6.0, a)
    bt = _where(small, 0.5 - t2 / 24.0, b)
    ct = _where(small, V(1.0 / 6.0, abs(1.0 / 6.0 - float(F32(1.0) / F32(6.0)))) - t2 / 120.0, (th - sn) / t3_s)
    c = [w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]]
    wv = (w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]
    t = [(at * v[k] + bt * c[k]) + ct * (w[k] * wv) for k in range(3)]
    return R, t


def forward_tracked(mode, pose, raw_o, raw_d, cams, trig_ulp=2.0):
    """camera_apply_kernel's arithmetic -> (origins value, bound, directions value, bound), each [n, 3] float64."""
    R, t = exp_map_tracked(mode, pose, trig_ulp)
    c = clamp_cams(cams, pose.shape[0])
    x, y, z = (V(raw_d[:, k]) for k in range(3))
    o, d = [], []
    for k in range(3):
        o.append(V(raw_o[:, k]) + t[k][c])
        d.append((R[3 * k][c] * x + R[3 * k + 1][c] * y) + R[3 * k + 2][c] * z)
    stack = lambda vs, f: np.stack([getattr(q, f) for q in vs], axis=1)  # noqa: E731
    return stack(o, "v"), stack(o, "e"), stack(d, "v"), stack(d, "e")
