"""The per-element bounds of the Wav2Vec2 convolution kernels' tests (tests/test_w2v_posconv_exact_gpu.py,
tests/test_w2v_posconv_elementwise_gpu.py, tests/test_w2v_conv0_kernels_gpu.py) as pure tensor functions, so that
tests/test_w2v_kernel_checks_cpu.py can prove on the CPU that each of them rejects the errors it is there for.

Exact operands.  Every operand is an integer multiple of a power of two (its ``unit``) that bf16 holds exactly.  Every product is then a
multiple of ``unit_a x unit_b`` and every partial sum, in any order, an integer number of those below ``exact_budget``; where that is
below 2^24 the f32 accumulation is exact in every order, and the kernel's result is a function of the operands alone.

Random operands.  |got - exact| <= lead(exact) + G x gamma x sum|terms|: lead is one bf16 ulp (2^-24 |exact| for an f32 output), G the
epilogue's derivative bound, sum|terms| the same contraction on the operands' magnitudes and gamma the f32 summation error relative to
it, MEASURED on the CPU in two summation orders against float64 (``gamma_conv`` / ``gamma_wgrad``) and taken four times over, the
MFMA's own order being a third we cannot restate."""
import math

import torch
import torch.nn.functional as F

import gelu_domain
import w2v_grad_ref as G
import w2v_ref
from helpers import _bf16_ulp

BF16 = torch.bfloat16
EXACT_LIMIT = 2.0 ** 24
ORDER_MARGIN = 4.0                         # measured f32 error -> bound: the margin for an order / a libm we cannot restate
_grid = torch.linspace(-8.0, 8.0, 160001, dtype=torch.float64)
_phi = lambda z: torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def gelu_grad(z):
    """gelu'(z) = Phi(z) + z phi(z) in z's own precision, Phi through erfc as the kernel forms it"""
    return 0.5 * torch.erfc(z * (-1.0 / math.sqrt(2.0))) + z * (1.0 / math.sqrt(2.0 * math.pi)) * torch.exp(-0.5 * z * z)


GELU_D1_SUP = float(gelu_grad(_grid).abs().max())                         # sup |gelu'|  = 1.1289 (at z = sqrt 2)
GELU_D2_SUP = float((_phi(_grid) * (2.0 - _grid * _grid)).abs().max())    # sup |gelu''| = 2 phi(0) = 0.7979


def kp_of(k, cg):
    return (k * cg + 31) // 32 * 32


def padded(p, Kp):
    """a packed (C, k cg) weight with its rows zero-padded to Kp columns"""
    out = torch.zeros(p.shape[0], Kp, dtype=p.dtype)
    out[:, :p.shape[1]] = p
    return out


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def exact_budget(K, a, b, unit, extra=0.0):
    """the worst partial sum of a K-term contraction of ``a`` and ``b`` (+ ``extra``), in units of ``unit`` = unit_a x unit_b: the
    accumulation is exact in every order where this is below EXACT_LIMIT"""
    return (K * float(a.abs().max()) * float(b.abs().max()) + extra) / unit


def is_multiple(t, unit):
    return bool((torch.round(t.double() / unit) * unit == t.double()).all())


def mismatches(got, want64):
    """how many elements of ``got`` (bf16 or f32) differ in their BITS from the float64 ``want64`` rounded once to got's type"""
    return int((bits(got) != bits(want64.to(got.dtype))).sum())


def worst(got, want, bound):
    """max |got - want| / bound; NaN (which fails every comparison) where ``got`` holds one"""
    return float(((got.double() - want).abs() / bound).max())


def fwd_bound(want, z):
    """y = x + gelu(z) behind an exact z, against float64: half a bf16 ulp of y (the store), 2^-24 |y| (the f32 add) and the GELU's own
    allowance without its store term (tests/gelu_domain.py: 2^-14 |gelu(z)| for the f32 formula and the flush floor)"""
    g = gelu_domain.gelu64(z)
    return 0.5 * _bf16_ulp(want) + want.abs() * 2.0 ** -24 + (gelu_domain.allow_fwd(z, g) - 0.5 * _bf16_ulp(g))


def gelu_grad_margin(z64):
    """the f32 error of gelu' over the case's z: the f32 CPU restatement of Phi(z) + z phi(z) against float64, ORDER_MARGIN times
    over for the device's erfcf / expf.  z must be exact in f32"""
    return ORDER_MARGIN * float((gelu_grad(z64.float()).double() - gelu_grad(z64)).abs().max())


def act_bound(want, dy, margin):
    """dz = dy gelu'(z) behind an exact z: one bf16 ulp of the product and |dy| times gelu's f32 error ``margin``"""
    return _bf16_ulp(want) + dy.abs() * margin


def elementwise_bound(exact, terms, gain, gamma, f32_out=False):
    lead = exact.abs() * 2.0 ** -24 if f32_out else _bf16_ulp(exact)
    return lead + gain * gamma * terms


def _rel(f32, exact, terms):
    ok = terms > 0
    return float(((f32.double() - exact).abs()[ok] / terms[ok]).max())


def gamma_conv(x, packed, cg, k, pad):
    """-> (exact, terms, gamma) of out = conv(x, packed) with ``pad`` rows of padding in front (w2v_grad_ref.conv_packed): x (N, T, C)
    and packed (C, k cg) float64.  The two f32 orders: torch's grouped conv1d, and 32-wide blocks of the (tap, channel) index
    summed from the last block to the first"""
    N, T, C = x.shape
    exact, terms = G.conv_packed(x, packed, cg, k, pad), G.conv_packed(x.abs(), packed.abs(), cg, k, pad)
    xp = F.pad(x.float().transpose(1, 2), (pad, k - 1 - pad))                                        # (N, C, T + k - 1)
    o1 = F.conv1d(xp, G.unpack(packed.float(), cg).contiguous(), groups=C // cg).transpose(1, 2)
    o2 = torch.zeros(N, T, C)
    Kb = kp_of(k, cg)
    for g in range(C // cg):
        ch = slice(g * cg, (g + 1) * cg)
        win = F.pad(w2v_ref.window(xp[:, ch].transpose(1, 2), k, 1), (0, Kb - k * cg))             # (N, T, Kb), column (j, ci)
        wg = F.pad(packed[ch].float(), (0, Kb - k * cg))
        acc = torch.zeros(N, T, cg)
        for b in reversed(range(Kb // 32)):
            acc = acc + win[..., b * 32:(b + 1) * 32] @ wg[:, b * 32:(b + 1) * 32].T
        o2[:, :, ch] = acc
    return exact, terms, ORDER_MARGIN * max(_rel(o1, exact, terms), _rel(o2, exact, terms))


def gamma_wgrad(dz, x, cg, k):
    """-> (exact, terms, gamma) of the packed weight gradient (w2v_grad_ref.conv_weight_grad), whose contraction runs over (clip,
    time).  The two f32 orders: torch's f32 contraction per tap, and 32-row blocks of time from the last clip's last block to the first"""
    N, T, C = x.shape
    exact, terms = G.conv_weight_grad(dz, x, cg, k), G.conv_weight_grad(dz.abs(), x.abs(), cg, k)
    o1 = G.conv_weight_grad(dz.float(), x.float(), cg, k)
    pad = k // 2
    xp = F.pad(x.float().transpose(1, 2), (pad, k - 1 - pad)).transpose(1, 2)                        # (N, T + k - 1, C)
    o2 = torch.zeros(C, k * cg)
    for g in range(C // cg):
        ch = slice(g * cg, (g + 1) * cg)
        win = w2v_ref.window(xp[:, :, ch], k, 1)                                                     # (N, T, k cg)
        acc = torch.zeros(cg, k * cg)
        for n in reversed(range(N)):
            for b in reversed(range((T + 31) // 32)):
                rows = slice(b * 32, min((b + 1) * 32, T))
                acc = acc + dz[n, rows, ch].float().T @ win[n, rows]
        o2[ch] = acc
    return exact, terms, ORDER_MARGIN * max(_rel(o1, exact, terms), _rel(o2, exact, terms))


def weightnorm_f32(dw, gain, v):
    """the f32 restatement of mmf_w2v_weightnorm_bwd's two reductions and its epilogue (torch's f32 sums), -> (dg, dv)"""
    dw, gain, v = dw.float(), gain.float(), v.float()
    inv = torch.rsqrt((v * v).sum(dim=(0, 1), keepdim=True))
    dg = (dw * v).sum(dim=(0, 1), keepdim=True) * inv
    return dg, gain * inv * (dw - v * inv * dg)


def scaled_err(got, ref):
    """max |got - ref| / max(|ref|, 1)"""
    return float(((got.double() - ref).abs() / ref.abs().clamp_min(1.0)).max())


# ---- layer 0 ------------------------------------------------------------------------------------------------
def conv0_expect(wave, w, mean, var, gamma, beta, s0, k1, s1, eps):
    """float64 (want, y, terms) of mmf_w2v_conv0_norm_gelu in the next layer's window form (N, T1, k1 C0), from the statistics the
    kernel is GIVEN (mean, var: (N, 1, C0)): y = gamma (conv - mean) rstd + beta, terms = |gamma| rstd (sum|w x| + |mean|) + |beta|"""
    wave, w, gamma, beta = wave.double(), w.double(), gamma.double(), beta.double()
    raw, mag = w2v_ref.conv0_raw(wave, w, s0), w2v_ref.conv0_raw(wave.abs(), w.abs(), s0)
    rstd = 1.0 / torch.sqrt(var.double() + eps)
    y = (raw - mean.double()) * rstd * gamma + beta
    terms = gamma.abs() * rstd * (mag + mean.double().abs()) + beta.abs()
    return tuple(w2v_ref.window(t, k1, s1) for t in (w2v_ref.gelu_erf(y), y, terms.expand_as(y)))
