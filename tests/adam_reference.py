"""torch/optim/adam.py's single-tensor update (no amsgrad / weight decay / maximize) in IEEE fp32 with numpy, operation by
operation in the order csrc/misc.hip's adam_kernel states, and the cases the Adam tests share (tests/test_adam_reference_cpu.py
holds this reference to torch.optim.Adam and tests/cpu_runner.cpu_adam; tests/test_gpu_adam.py holds nsamd_adam_step to it, bit
for bit). Per element, every fl() one fp32 rounding:

    gr = fl(g * grad_scale)   when grad_scale != 1, else g
    m  = fma(w1, gr - m, m)                               w1 = fl(1 - beta1)         exp_avg.lerp_(grad, 1 - beta1)
    v  = fma(fl(w2 * gr), gr, fl(v * beta2))              w2 = fl(1 - beta2)         exp_avg_sq.mul_(beta2).addcmul_(...)
    p  = fl(p + fl(fl(-step_size * m) / fl(fl(sqrt(v) / bc2_sqrt) + eps)))            param.addcdiv_(exp_avg, denom, -step_size)

with step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) from functional.adam_hyper, rounded to fp32 once.

The fused multiply-add is one rounding of the exact a b + c. It is formed in float64: the product of two fp32 numbers is exact
there (48 bits); the sum is rounded to 53 bits and would then be rounded a second time on the way to fp32, so the float64 sum is
rounded TO ODD first (its error term from the two-sum; when the sum is inexact and its last bit is even, step one float64 towards
the error) — with 53 >= 24 + 2 bits the final rounding is then the single correct one, ties included. numpy's fp32 multiply,
divide, add and sqrt are the correctly rounded hardware operations, without flush-to-zero."""
import functools

import numpy as np

from nerfstudio_amd.functional import adam_hyper

F32 = np.float32
TRIP = 256 * 3 * 256 * 4  # floats one trip of adam_kernel's grid-stride loop covers: 768 workgroups x 256 lanes x 4 = 786432
BETAS = (0.9, 0.999)


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for fp32 arrays / scalars."""
    a, b, c = (np.asarray(x, dtype=F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        s = a * b  # exact
        t = s + c
        bb = t - s
        e = (s - (t - bb)) + (c - bb)  # two-sum: s + c = t + e exactly (finite operands)
    bits = np.ascontiguousarray(t).view(np.int64)  # (t and e have the full broadcast shape)
    need = np.isfinite(t) & np.isfinite(e) & (e != 0) & ((bits & 1) == 0)
    away = (e > 0) == (t > 0)  # the error points away from zero: the magnitude (the bit pattern) grows
    bits = np.where(need, np.where(away, bits + 1, bits - 1), bits)
    with np.errstate(all="ignore"):
        return bits.view(np.float64).astype(F32)


def adam_step(p, g, m, v, step, lr, eps=1e-15, grad_scale=1.0, betas=BETAS):
    """One update of the fp32 arrays (p, m, v) with gradient g at bias-correction step `step` -> new (p, m, v)."""
    step_size, bc2_sqrt = adam_hyper(step, lr, betas)
    w1, w2, beta2 = F32(1.0 - betas[0]), F32(1.0 - betas[1]), F32(betas[1])
    neg_step, bc2_sqrt, eps, gs = -F32(step_size), F32(bc2_sqrt), F32(eps), F32(grad_scale)
    p, g, m, v = (np.asarray(x, dtype=F32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        gr = g if gs == F32(1.0) else g * gs
        m1 = fma32(w1, gr - m, m)
        v1 = fma32(w2 * gr, gr, v * beta2)
        denom = np.sqrt(v1) / bc2_sqrt + eps
        p1 = p + (neg_step * m1) / denom
    assert p1.dtype == m1.dtype == v1.dtype == F32
    return p1, m1, v1


def run(case):
    """[(p, m, v) after each of the case's steps]."""
    p, m, v = case["p"], case["m"], case["v"]
    out = []
    for k, g in enumerate(case["grads"]):
        p, m, v = adam_step(p, g, m, v, case["step"] + k, case["lr"], case["eps"], case["grad_scale"])
        out.append((p, m, v))
    return out


def same_bits(a, b):
    """Boolean array: the same fp32 bits, or NaN in both."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(p, grads, m=None, v=None, step=1, lr=1e-2, eps=1e-15, grad_scale=1.0):
    p = np.ascontiguousarray(p, dtype=F32)
    return dict(p=p, m=np.zeros_like(p) if m is None else np.ascontiguousarray(m, dtype=F32),
                v=np.zeros_like(p) if v is None else np.ascontiguousarray(v, dtype=F32),
                grads=[np.ascontiguousarray(g, dtype=F32) for g in grads], step=step, lr=lr, eps=eps, grad_scale=grad_scale)


def dense(n, seed, steps=3, **kw):
    rs = np.random.RandomState(seed)
    return _case(rs.standard_normal(n), [rs.standard_normal(n) for _ in range(steps)], **kw)


# Lane kinds of the zero-skip gradient (a lane is one float; an aligned group of four lanes is what the kernel's skip tests):
#   A  g = 0 at every step, m = v = 0: nothing may be written                          (a)
#   N  a gradient at every step
#   C  a gradient at step 1 only: g = 0 with m, v != 0 afterwards, which still decay and move p   (c)
#   D  g = -0.0 at every step (compares equal to zero)                                 (d)
#   E  g = 0 at steps 1 and 2, a gradient at step 3                                    (e)
ZERO_SKIP_GROUPS = ["AAAA", "ANAA", "NAAA", "AAAN", "CCCC", "DDDD", "EEEE", "ACDE", "DADA", "AAAA", "CAAA", "AAEA", "NNNN", "AADA"]
ZERO_SKIP_TAILS = ["ACD", "EAN", "DEC", "AN", "C", ""]  # the scalar tail has no skip: the same bits anyway


def zero_skip(tail, seed=11, **kw):
    """A table-like gradient: most aligned groups of four are zero for ever (kind A), among them the groups of
    ZERO_SKIP_GROUPS; `tail` names the lanes past the last whole group. p holds -0.0 and subnormals in A lanes."""
    rs = np.random.RandomState(seed)
    kinds = "".join(ZERO_SKIP_GROUPS[i % len(ZERO_SKIP_GROUPS)] if i % 3 == 0 else "AAAA" for i in range(3 * len(ZERO_SKIP_GROUPS)))
    kinds += tail
    k = np.frombuffer(kinds.encode(), dtype=np.uint8)
    n = k.size
    p = rs.standard_normal(n).astype(F32)
    a = np.flatnonzero(k == ord("A"))
    p[a[0::4]] = F32(-0.0)
    p[a[1::4]] = F32(1e-40) * rs.choice([-1.0, 1.0], a[1::4].size).astype(F32)  # subnormal
    p[a[2::4]] = F32(0.0)
    grads = []
    for step in (1, 2, 3):
        g = np.zeros(n, F32)
        live = (k == ord("N")) | ((k == ord("C")) & (step == 1)) | ((k == ord("E")) & (step == 3))
        g[live] = rs.standard_normal(int(live.sum())).astype(F32)
        g[live & (g == 0)] = F32(1.0)
        g[k == ord("D")] = F32(-0.0)
        grads.append(g)
    c = _case(p, grads, **kw)
    c["kinds"] = k
    return c


def magnitudes(eps, n=4099, seed=5):
    """|g| log-uniform over [1e-22, 1e18], random signs: g^2 (1 - beta2) runs from below the smallest subnormal through the
    subnormals and the normals to 1e33, just under the overflow of g g."""
    rs = np.random.RandomState(seed)
    grads = [(10.0 ** rs.uniform(-22, 18, n) * rs.choice([-1.0, 1.0], n)).astype(F32) for _ in range(3)]
    return _case(rs.standard_normal(n), grads, eps=eps)


def non_finite(seed=7):
    """+inf, -inf and NaN gradients at step 2 (ordinary ones at steps 1 and 3, so the state goes finite -> inf -> NaN), each
    inside an otherwise ordinary float4 (lanes 5, 9, 14 of 32), and all three in the tail (lanes 32 - 34)."""
    c = dense(35, seed)
    c["grads"][1][[5, 9, 14, 32, 33, 34]] = np.array([np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf], F32)
    c["special"] = np.array([5, 9, 14, 32, 33, 34])
    return c


def late(step, n=1027, seed=9):
    """Three steps from bias-correction step `step` on, from given moments (m ~ 0.1 N(0, 1), v ~ m^2 scale)."""
    rs = np.random.RandomState(seed + step % 97)
    c = dense(n, seed + 1 + step % 97, step=step)
    c["m"] = (0.1 * rs.standard_normal(n)).astype(F32)
    c["v"] = (0.01 * rs.standard_normal(n) ** 2).astype(F32)
    return c


TRIP_SIZES = [2 * TRIP + 1027, TRIP + 4, TRIP]  # two full trips + a partial third + a tail of 3; one float4 in trip 2; one trip
TAIL_SIZES = [1, 2, 3, 4, 5, 6, 7, 1021, 1022, 1023, 1024, 1025]
SCALES = [0.5, 1.0 / 3.0, 0.125]
LATE_STEPS = [1, 2, 1000, 100000]

CASES = {}
for _n in TRIP_SIZES:
    CASES[f"trips-{_n}"] = functools.partial(dense, _n, 1)
for _n in TAIL_SIZES:
    CASES[f"tail-{_n}"] = functools.partial(dense, _n, 2 + _n)
for _t in ZERO_SKIP_TAILS:
    CASES[f"zero-skip-tail{_t or '0'}"] = functools.partial(zero_skip, _t)
for _s in SCALES:
    CASES[f"scale-{_s:.3f}-dense"] = functools.partial(dense, 1027, 3, grad_scale=_s)
    CASES[f"scale-{_s:.3f}-zero-skip"] = functools.partial(zero_skip, "ACD", grad_scale=_s)
for _e in (1e-15, 1e-8):
    CASES[f"magnitudes-eps{_e:g}"] = functools.partial(magnitudes, _e)
CASES["non-finite"] = non_finite
for _s in LATE_STEPS:
    CASES[f"late-{_s}"] = functools.partial(late, _s)
