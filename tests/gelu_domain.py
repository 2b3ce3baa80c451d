"""One rule for every exact-GELU site of the native backbones, over the whole bf16 domain, against float64.

The kernels form gelu(v) = v Phi(v) (csrc/mmf_internal.h: ``gelu_erf``) and gelu'(v) = Phi(v) + v phi(v) (``gelu_erf_grad``) in f32 and
round once to bf16.  This module holds the inputs, the float64 references and the allowance, as pure tensor functions: it needs no GPU
and no transformers, so tests/test_gelu_domain_cpu.py can prove on f32 restatements that the rule rejects the errors it is there for,
and tests/test_gelu_domain_gpu.py applies it to every kernel.

Inputs.  ``domain()`` is every finite bf16 bit pattern, both zeros and the subnormals included: 65 280 = 255 x 256 values, so one launch
covers it with a row count that is no multiple of a 256-lane block.  ``edge_points(n)`` serves the sites that reach the pre-activation
only through a per-channel f32 vector: the whole left tail, the zeros, the smallest magnitudes, the neighbours of the derivative's root,
the largest finite values, and an even grid for the rest.

Allowance.  Every term is derived, none fitted to a kernel:
  * 0.5 x _bf16_ulp(want): the one rounding of the store.
  * 2^-14 |want|: the f32 formula's own error.  Phi's exponent argument -z^2 + P(t) reaches 2^7 in magnitude before the f32 result
    underflows; its four f32 roundings (z, z^2, the fma, and the scaling inside the fast exponential) are 2^-24 of that each, 2^-15
    relative in the result, doubled for the reciprocal and the fit.
  * (1 + |v|) 2^-126 (times |dg| in the backward): Phi(v) itself falls under the smallest normal f32 near v = -13 and may flush, and so
    may any result under the smallest normal.
  * backward only, 2^-22 |dg| (Phi + |v phi|): the cancellation of the two terms at the derivative's root, which only matters when an f32
    bias moves v off the bf16 grid.
Where a kernel adds an f32 bias the caller restates v as the f32 sum ``x.float() + bias``: that is the IEEE add the kernel performs, so
v is exact and the float64 reference starts from it.  Non-finite inputs are out of scope; no other input is left out of a comparison."""
import math

import torch

from helpers import _bf16_ulp

BF16 = torch.bfloat16
F64 = torch.float64
BF16_MAX = float(torch.finfo(BF16).max)
_SQRT_HALF = 1.0 / math.sqrt(2.0)
_INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def domain():
    """(255, 256) bf16: every finite bit pattern, the positive half first"""
    x = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(BF16)
    x = x[torch.isfinite(x.float())]
    assert x.numel() == 255 * 256
    return x.reshape(255, 256).clone()


def _phi_cdf(v):
    return 0.5 * torch.erfc(-v * _SQRT_HALF)


def _v_phi(v):
    return v * torch.exp(-0.5 * v * v) * _INV_SQRT_2PI


def gelu64(v):
    """float64 v Phi(v), Phi through erfc"""
    v = v.double()
    return v * _phi_cdf(v)


def gelu_grad64(v):
    """float64 Phi(v) + v phi(v), Phi through erfc"""
    v = v.double()
    return _phi_cdf(v) + _v_phi(v)


def grad_root():
    """the negative root of gelu' (-0.7518), by bisection in float64"""
    lo, hi = -1.0, -0.5
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if float(gelu_grad64(torch.tensor(mid, dtype=F64))) < 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def edge_points(n):
    """(n,) f32, every value a bf16: the points listed in the module docstring, then an even grid on [-4, 4] (rounded to bf16)"""
    d = domain().reshape(-1).float()
    tail = d[(d >= -14.0) & (d <= -4.0)]
    r = grad_root()
    below, above = d[d < r].max(), d[d > r].min()
    named = [0.0, -0.0, 2.0 ** -133, -2.0 ** -133, 2.0 ** -126, -2.0 ** -126, float(below), float(above)]
    for a in (0.5, 1.0, 3.0, 6.0, 100.0, BF16_MAX):
        named += [a, -a]
    fixed = torch.cat([tail, torch.tensor(named, dtype=torch.float32)])
    if n < fixed.numel():
        raise ValueError(f"edge_points: n={n} is below the {fixed.numel()} points every case must hold")
    grid = torch.linspace(-4.0, 4.0, n - fixed.numel(), dtype=F64).float().to(BF16).float()
    return torch.cat([fixed, grid])


def allow_fwd(v, want):
    v, want = v.double(), want.double()
    return 0.5 * _bf16_ulp(want) + 2.0 ** -14 * want.abs() + (1.0 + v.abs()) * 2.0 ** -126


def allow_bwd(v, dg, want, stored=True):
    """``stored`` False: the result is an f32 value that was never rounded to bf16, and the store's term is left out"""
    v, dg, want = v.double(), dg.double(), want.double()
    return ((0.5 * _bf16_ulp(want) if stored else 0.0) + 2.0 ** -14 * want.abs() + dg.abs() * (1.0 + v.abs()) * 2.0 ** -126
            + 2.0 ** -22 * dg.abs() * (_phi_cdf(v) + _v_phi(v).abs()))


BF16_OVERFLOW = BF16_MAX + 2.0 ** 119               # from here up a value rounds to bf16's infinity (half a spacing past the largest)


def _ratio(got, want, allow):
    """|got - want| / allow.  A NaN is a miss.  An infinity is right (0) where the value, give or take its allowance, rounds to that
    infinity in bf16 (a dropout site's 1 / (1 - p) times the largest inputs), and a miss everywhere else"""
    g = got.double()
    r = (g - want).abs() / allow
    overflow = torch.isinf(g) & (torch.sign(g) == torch.sign(want)) & (want.abs() + allow >= BF16_OVERFLOW)
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    return torch.where(overflow, torch.zeros_like(r), r)


def ratio_fwd(got, v, scale=1.0):
    """|got - scale gelu64(v)| / allowance, elementwise; ``scale``: the f32 factor a kept element of a dropout site is multiplied by"""
    want = scale * gelu64(v)
    return _ratio(got, want, allow_fwd(v, want))


def ratio_bwd(got, v, dg, scale=1.0, stored=True):
    """|got - scale dg gelu_grad64(v)| / allowance, elementwise"""
    want = scale * dg.double() * gelu_grad64(v)
    return _ratio(got, want, allow_bwd(v, scale * dg.double(), want, stored))


def worst(ratio, v):
    """(the largest ratio, the input where it occurred, how many inputs are over 1)"""
    i = int(torch.argmax(ratio.reshape(-1)))
    return float(ratio.reshape(-1)[i]), float(v.reshape(-1)[i]), int((ratio > 1.0).sum())


def report(what, ratio, v):
    """print the worst error / allowance and its input -> (worst, at, failures)"""
    w, at, fails = worst(ratio, v.expand_as(ratio) if v.shape != ratio.shape else v)
    print(f"{what}: worst error / allowance = {w:.4f} at v = {at!r}, {fails} of {ratio.numel()} over")
    return w, at, fails
