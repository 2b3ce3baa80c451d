"""CPU: the domain rule of tests/gelu_domain.py on f32 restatements of the kernels' formulas, over all 65 280 finite bf16 inputs.

It shows what the rule is for: the f32 ``0.5 x (1 + erf(x / sqrt 2))`` form, which every forward site used and which the earlier tests
(one bf16 ulp of that same f32 formula plus |v| 2^-22) accepted, is rejected; the erfc / Chebyshev form of csrc/mmf_internal.h is
accepted, as is the backward's ``gelu_erf_grad``; and five planted errors are each rejected, with the number of inputs that reject them
printed.  The restatements are torch float32 on the CPU (an fma is a multiply and an add, the reciprocal a division): what they prove is
the rule's reach, the kernels themselves are held to it in tests/test_gelu_domain_gpu.py."""
import numpy as np
import torch

import gelu_domain as D
from helpers import _bf16_ulp

SQRT_HALF = np.float32(0.70710678118654752440)
INV_SQRT_2PI = np.float32(0.39894228040143267794)
CHEB = (0.17087277, -0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368, -1.26551223)


def one_plus_erf(v):
    """the f32 form every forward site had"""
    return np.float32(0.5) * v * (np.float32(1.0) + torch.erf(v * SQRT_HALF))


def erfc_cheb(v, coef=CHEB, sqrt_half=SQRT_HALF, mirror=True):
    """``gelu_erf`` of csrc/mmf_internal.h in f32; the fast exponential flushes results under the smallest normal"""
    z = v.abs() * sqrt_half
    t = (np.float32(1.0) / (np.float32(0.5) * z + np.float32(1.0))).float()
    p = torch.full_like(t, coef[0])
    for c in coef[1:]:
        p = p * t + np.float32(c)
    e = torch.exp(-z * z + p)
    e = torch.where(e < 2.0 ** -126, torch.zeros_like(e), e)
    h = np.float32(0.5) * t * e
    return v * torch.where(v < 0, h, (np.float32(1.0) - h) if mirror else h)


def grad_erfc(v):
    """``gelu_erf_grad`` of csrc/mmf_internal.h in f32"""
    return np.float32(0.5) * torch.erfc(v * -SQRT_HALF) + v * INV_SQRT_2PI * torch.exp(np.float32(-0.5) * v * v)


def _v():
    return D.domain().reshape(-1).float()


def _stored(f32):
    return f32.to(torch.bfloat16)


def test_domain_and_edge_points_hold_what_they_promise():
    d = D.domain()
    assert d.shape == (255, 256) and d.dtype == torch.bfloat16 and bool(torch.isfinite(d.float()).all())
    assert torch.unique(d.view(torch.int16)).numel() == 65280
    f = d.float().reshape(-1)
    assert int((f == 0).sum()) == 2 and int(((f != 0) & (f.abs() < 2.0 ** -126)).sum()) == 2 * 127
    tail = f[(f >= -14.0) & (f <= -4.0)]
    for n in (256, 512):
        e = D.edge_points(n)
        assert e.shape == (n,) and e.dtype == torch.float32 and torch.equal(e.to(torch.bfloat16).float(), e)
        have = set(e.view(torch.int32).tolist())
        need = torch.cat([tail, torch.tensor([0.0, -0.0, 2.0 ** -133, -2.0 ** -133, 2.0 ** -126, -2.0 ** -126, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0, 6.0,
                                              -6.0, 100.0, -100.0, D.BF16_MAX, -D.BF16_MAX, -0.75, -0.75390625])])
        assert set(need.view(torch.int32).tolist()) <= have
        assert 220 <= tail.numel() <= 240 and float(e.min()) == -D.BF16_MAX
    r = D.grad_root()
    assert -0.75390625 < r < -0.75 and abs(float(D.gelu_grad64(torch.tensor(r, dtype=torch.float64)))) < 1e-15
    assert float(D.gelu64(torch.tensor(-0.0))) == 0.0 and float(D.gelu_grad64(torch.tensor(0.0))) == 0.5


def test_one_plus_erf_forward_is_rejected_where_the_old_rule_let_it_through():
    v = _v()
    got32 = one_plus_erf(v)
    got = _stored(got32)
    ratio = D.ratio_fwd(got, v)
    w, at, fails = D.report("f32 1 + erf forward, domain rule", ratio, v)
    bad = v[ratio > 1.0]
    spacings = (got.double() - D.gelu64(v)).abs() / _bf16_ulp(D.gelu64(v))
    i = int(torch.argmax(spacings))
    print(f"  rejected on {fails} inputs in [{float(bad.min())}, {float(bad.max())}]; worst miss {float(spacings[i]):.1f} bf16 spacings at "
          f"x = {float(v[i])}; exact zero from x = {float(v[(got32 == 0) & (v < 0) & (v > -100)].max())} down")
    assert fails == 188 and float(bad.max()) < -4.0 and float(bad.min()) >= -13.5
    assert float(v[i]) == -8.625 and 254.5 <= float(spacings[i]) <= 255.5
    assert float(v[(got32 == 0) & (v < 0) & (v > -100)].max()) == -5.4375
    # the rule the suite had: one bf16 ulp of the SAME f32 formula plus |v| 2^-22
    want32 = got32.double()
    old = (got.double() - want32).abs() / (_bf16_ulp(want32) + v.double().abs() * 2.0 ** -22)
    print(f"  the old rule on the same outputs: worst error / bound = {float(old.max()):.4f}")
    assert float(old.max()) <= 1.0


def test_erfc_forward_and_backward_are_accepted():
    v = _v()
    w, at, fails = D.report("f32 erfc / Chebyshev forward", D.ratio_fwd(_stored(erfc_cheb(v)), v), v)
    assert fails == 0 and w <= 1.0
    ok = D.gelu64(v).abs() > 2.0 ** -126
    rel = ((erfc_cheb(v).double() - D.gelu64(v)).abs() / D.gelu64(v).abs())[ok]
    print(f"  worst f32 relative error on normal results {float(rel.max()):.2e}")
    assert float(rel.max()) <= 2.0 ** -15
    one = torch.ones_like(v)
    w, at, fails = D.report("f32 erfc backward, dg = 1", D.ratio_bwd(_stored(grad_erfc(v)), v, one), v)
    assert fails == 0 and w <= 1.0


def test_a_scaled_result_past_the_largest_bf16_must_be_that_infinity():
    """a dropout site multiplies kept elements by c = 1 / (1 - p): c gelu(v) of the largest inputs rounds to bf16's infinity"""
    v, c = _v(), float(np.float32(1.0) / np.float32(0.9))
    got = _stored((np.float32(c) * erfc_cheb(v)))
    n_inf = int(torch.isinf(got.float()).sum())
    w, at, fails = D.report(f"erfc forward times c = {c:.6f} ({n_inf} infinities)", D.ratio_fwd(got, v, scale=c), v)
    assert fails == 0 and 0 < n_inf < 64 and bool((torch.isinf(got.float()) == (v * c >= D.BF16_OVERFLOW)).all())
    capped = torch.where(torch.isinf(got.float()), torch.full_like(got, D.BF16_MAX), got)         # the largest finite value instead
    flipped = torch.where(torch.isinf(got.float()), -got, got)                                    # the other infinity
    early = got.clone()
    early[v == 100.0] = float("inf")                                                               # an infinity where the value is finite
    assert D.worst(D.ratio_fwd(capped, v, scale=c), v)[2] == n_inf and D.worst(D.ratio_fwd(flipped, v, scale=c), v)[2] == n_inf
    assert D.worst(D.ratio_fwd(early, v, scale=c), v)[2] == 1
    nan = got.clone()
    nan[0] = float("nan")
    assert D.worst(D.ratio_fwd(nan, v, scale=c), v)[2] == 1


def test_planted_errors_are_each_rejected():
    v = _v()
    one = torch.ones_like(v)
    coef = list(CHEB)
    coef[7] = 0.37419196                                                              # 0.37409196: the fourth significant digit
    fwd = {
        "a Chebyshev coefficient off in its fourth digit": erfc_cheb(v, coef=tuple(coef)),
        "sqrt(1/2) truncated to 0.7071": erfc_cheb(v, sqrt_half=np.float32(0.7071)),
        "Phi(x >= 0) taken as h, not 1 - h": erfc_cheb(v, mirror=False),
    }
    bwd = {
        "backward with Phi through 1 + erf": np.float32(0.5) * (np.float32(1.0) + torch.erf(v * SQRT_HALF))
                                             + v * INV_SQRT_2PI * torch.exp(np.float32(-0.5) * v * v),
        "backward without v phi(v)": np.float32(0.5) * torch.erfc(v * -SQRT_HALF),
    }
    counts = {}
    for name, got in fwd.items():
        counts[name] = D.report(f"planted: {name}", D.ratio_fwd(_stored(got), v), v)[2]
    for name, got in bwd.items():
        counts[name] = D.report(f"planted: {name}", D.ratio_bwd(_stored(got), v, one), v)[2]
    for name, n in counts.items():
        print(f"planted error rejected on {n:6d} of {v.numel()} inputs: {name}")
    assert all(n > 0 for n in counts.values()), counts
