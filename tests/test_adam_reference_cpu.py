"""tests/adam_reference.py (the IEEE-fp32 restatement nsamd_adam_step is held to bit for bit in tests/test_gpu_adam.py) against
torch.optim.Adam and tests/cpu_runner.cpu_adam on the CPU, on the very cases of the GPU test: every step starts from the
reference's state, torch's result after it is compared.

* Both moments: the SAME BITS (NaN where the reference has NaN) — torch's lerp_ and mul_().addcmul_() are the two fused
  multiply-adds of the reference.
* Parameters: torch's vectorised CPU sqrt is not correctly rounded (tests/test_gpu_kernels.py::test_adam_matches_torch: ~0.6 % of
  its results are one ulp off), so they are held to that test's allowance per step: 2e-9 absolute — one ulp of an update of the
  size of lr = 1e-2, scaled up with the update where the given moments of a case make it larger — plus 3e-7 relative.
* fma32's rounding to odd is checked against exact rational arithmetic, on operands built to land on the ties where a float64 sum
  rounded a second time goes wrong."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import adam_reference as ar
import cpu_runner

F32 = np.float32


def _allowance(case, k, before, after):
    upd = np.abs(after[0].astype(np.float64) - before[0].astype(np.float64))
    return 2e-9 * np.maximum(1.0, upd / 1e-2) + 3e-7 * np.abs(after[0].astype(np.float64))


def _compare(name, what, got, ref, allowance, worst):
    (pg, mg, vg), (pr, mr, vr) = got, ref
    for label, a, b in (("exp_avg", mg, mr), ("exp_avg_sq", vg, vr)):
        same = ar.same_bits(a, b)
        assert same.all(), f"{name} {what} {label}: {int((~same).sum())}/{same.size} entries differ, first {np.flatnonzero(~same)[:5]}"
    assert np.array_equal(np.isnan(pg), np.isnan(pr)), f"{name} {what}: NaN positions of the parameters differ"
    fin = np.isfinite(pr)
    assert np.array_equal(pg[~fin & ~np.isnan(pr)], pr[~fin & ~np.isnan(pr)])
    err = np.abs(pg[fin].astype(np.float64) - pr[fin].astype(np.float64))
    ratio = float((err / allowance[fin]).max()) if err.size else 0.0
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert ratio <= 1.0, f"{name} {what}: parameters {ratio:.2f}x the allowance"


@pytest.mark.parametrize("name", list(ar.CASES))
def test_reference_matches_torch_adam_and_cpu_adam(name):
    case = ar.CASES[name]()
    states = ar.run(case)
    before = (case["p"], case["m"], case["v"])
    worst = {}
    for k, g in enumerate(case["grads"]):
        step, after = case["step"] + k, states[k]
        allowance = _allowance(case, k, before, after)
        gs = F32(case["grad_scale"])
        with np.errstate(all="ignore"):
            gr = g if gs == F32(1.0) else g * gs  # torch.optim.Adam has no grad_scale: it is handed fl(g * scale)
        # torch.optim.Adam, single tensor
        p = torch.nn.Parameter(torch.from_numpy(before[0].copy()))
        p.grad = torch.from_numpy(gr.copy())
        opt = torch.optim.Adam([p], lr=case["lr"], betas=ar.BETAS, eps=case["eps"])
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(before[1].copy()),
                        "exp_avg_sq": torch.from_numpy(before[2].copy())}
        opt.step()
        st = opt.state[p]
        assert int(st["step"]) == step
        _compare(name, "torch.optim.Adam", (p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), after, allowance, worst)
        # cpu_adam: host-derived step scalars, and the device-resident pair with the step / lr arguments wrong
        for hyper in (False, True):
            t = [torch.from_numpy(x.copy()) for x in before]
            if hyper:
                hd = torch.tensor(ar.adam_hyper(step, case["lr"], ar.BETAS), dtype=torch.float32)
                cpu_runner.cpu_adam(t[0], torch.from_numpy(g.copy()), t[1], t[2], step + 3, 123.0, ar.BETAS, case["eps"],
                                    float(gs), hd)
            else:
                cpu_runner.cpu_adam(t[0], torch.from_numpy(g.copy()), t[1], t[2], step, case["lr"], ar.BETAS, case["eps"], float(gs))
            _compare(name, "cpu_adam" + (" hyper_dev" if hyper else ""), [x.numpy() for x in t], after, allowance, worst)
        before = after
    print(f"\n{name}: worst |err| / allowance of the parameters " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_late_steps_reach_the_saturated_bias_corrections():
    """At step 100000 both bias corrections are 1 in fp32 (step_size == lr, bc2_sqrt == 1); at 1000 neither is."""
    s, b = ar.adam_hyper(100000, 1e-2, ar.BETAS)
    assert s == 1e-2 and F32(b) == F32(1.0)
    s, b = ar.adam_hyper(1000, 1e-2, ar.BETAS)
    assert F32(s) == F32(1e-2) and F32(b) < F32(1.0)  # (0.9^1000 is below fp32's resolution of 1, 0.999^1000 = 0.37 is not)
    s, b = ar.adam_hyper(2, 1e-2, ar.BETAS)
    assert F32(s) > F32(5e-2) and F32(b) < F32(0.05)


def test_zero_skip_cases_hold_what_they_claim():
    """The reference itself leaves the never-reached lanes' bits alone (what the kernel's skip relies on), moves the lanes with
    g = 0 but live moments, and every kind of lane appears both in whole groups of four and in a tail."""
    seen_body, seen_tail = set(), set()
    for tail in ar.ZERO_SKIP_TAILS:
        case = ar.zero_skip(tail)
        k = case["kinds"]
        n4 = k.size // 4 * 4
        seen_body |= set(k[:n4].tobytes().decode())
        seen_tail |= set(k[n4:].tobytes().decode())
        states = ar.run(case)
        a, c, d = k == ord("A"), k == ord("C"), k == ord("D")
        assert {0x80000000} <= set(case["p"][a].view(np.uint32).tolist()) and (np.abs(case["p"][a]) == F32(1e-40)).any()
        for p, m, v in states:
            for lanes in (a, d):
                assert ar.same_bits(p[lanes], case["p"][lanes]).all() and not m[lanes].any() and not v[lanes].any()
                assert not np.signbit(m[lanes]).any() and not np.signbit(v[lanes]).any()
        if c.any():
            assert (states[1][0][c] != states[0][0][c]).all() and (np.abs(states[1][1][c]) < np.abs(states[0][1][c])).all()
        groups = k[:n4].reshape(-1, 4)
        assert (groups == ord("A")).all(1).mean() > 0.6  # most groups are never reached
        assert ((groups == ord("N")).sum(1) == 1).any() and (groups == ord("C")).all(1).any()
    assert seen_body == set("ANCDE") and seen_tail == set("ANCDE")


def test_magnitudes_reach_the_subnormals_and_the_top():
    case = ar.magnitudes(1e-15)
    v = ar.run(case)[0][2]
    tiny = np.finfo(F32).tiny
    assert (v == 0).any() and ((v > 0) & (v < tiny)).sum() > 50 and (v > 1e30).any() and np.isfinite(v).all()


def test_fma32_rounds_once():
    rs = np.random.RandomState(0)
    n = 4000
    a = rs.standard_normal(n).astype(F32)
    b = rs.standard_normal(n).astype(F32)
    c = (rs.standard_normal(n) * 10.0 ** rs.uniform(-8, 2, n)).astype(F32)
    # near-ties: a b = 1 - 2^-46 and c an even integer in [2^24, 2^25) (ulp 2): the exact sum lies 2^-46 below the midpoint
    # c + 1, the float64 sum (ulp 2^-28 there) IS the midpoint, and its second rounding then goes to the even neighbour
    h = n // 2
    a[:h], b[:h] = F32(1.0 + 2.0**-23), F32(1.0 - 2.0**-23)
    c[:h] = (2.0 * rs.randint(1 << 23, 1 << 24, h)).astype(F32) * rs.choice([-1.0, 1.0], h).astype(F32)
    got = ar.fma32(a, b, c)
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    want = np.empty(n, F32)
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F32(float(exact))  # float(Fraction) is correctly rounded to float64; fp32 candidates around it
        cand = [lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))]
        dist = [abs(Fraction(float(x)) - exact) for x in cand]
        best = min(dist)
        tied = [x for x, d in zip(cand, dist) if d == best]
        want[i] = tied[0] if len(tied) == 1 else next(x for x in tied if (x.view(np.uint32) & 1) == 0)
    assert ar.same_bits(got, want).all()
    assert (~ar.same_bits(twice, want)).any(), "the operands were meant to include cases a second rounding gets wrong"
