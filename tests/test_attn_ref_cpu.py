"""CPU: the float64 attention restatement of tests/attn_ref.py that tests/test_attention_paths_gpu.py holds the kernels to.

exact() is pinned to torch autograd in float64 through a plain softmax attention (1e-12), with and without a given mask.
staged() — exact() with the kernels' rounding points — must stay within the design's own error of exact(): a trial with the
outputs rounded to bf16 as well measured 0.5 - 1.25 x BF16_TOL x max|exact| over six shapes, which bounds the unrounded form
used here from above; this file measures 0.30 - 0.92 on the same shapes (printed as GAP lines) and asserts the 1.25.  Under
a dropout mask (p = 0.3: fewer, larger terms under the same maximum) the gap is 0.23 - 1.84; the trial did not cover that, so
it is printed and not asserted.  The noise term of the GPU bounds — staged() against staged() with scores perturbed by 2^-22 —
measures 0 - 0.12 x BF16_TOL x max with and without the mask (NOISE lines; the trial with rounded outputs gave 0 - 0.41)
and is asserted below 0.41."""
import math

import numpy as np
import pytest
import torch

import attn_ref as R

F64 = torch.float64
BF16_TOL = 2 ** -8
SHAPES = [(64, 33, 31, 1.0), (96, 129, 200, 1.0), (96, 30, 512, 1.0), (64, 200, 3, 1.0), (96, 64, 97, 3.0), (64, 40, 130, 0.05)]


def operands(dh, Tq, Tk, qs, B=2, H=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda T, s: R.bf16r(torch.randn(B, T, H * dh, generator=g, dtype=F64) * s)
    return mk(Tq, qs), mk(Tk, 1.0), mk(Tk, 1.0), mk(Tq, 1.0)


def autograd(q, k, v, do, H, scale, w):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = R.heads(q, H) @ R.heads(k, H).transpose(-1, -2) * scale
    o = R.merge((torch.softmax(s, -1) * w) @ R.heads(v, H))
    o.backward(do)
    return dict(o=o.detach(), lse=torch.logsumexp(s, -1).detach(), dq=q.grad, dk=k.grad, dv=v.grad)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dh,Tq,Tk,qs", SHAPES)
def test_exact_matches_float64_autograd(dh, Tq, Tk, qs, masked):
    H, scale = 2, R.f32r_scale(1.0 / math.sqrt(dh))
    q, k, v, do = operands(dh, Tq, Tk, qs)
    keep = (torch.rand(2, H, Tq, Tk, generator=torch.Generator().manual_seed(5)) >= 0.3) if masked else None
    inv = 1.0 / 0.7 if masked else 1.0
    got = R.exact(q, k, v, do, H, scale, keep, inv)
    want = autograd(q, k, v, do, H, scale, keep.to(F64) * inv if masked else torch.ones(()).to(F64))
    for name, ref in want.items():
        err = float((got[name] - ref).abs().max() / max(1.0, float(ref.abs().max())))
        assert err < 1e-12, (name, err)
    delta = (R.heads(want["o"], H) * R.heads(do, H)).sum(-1)
    assert float((got["delta"] - delta).abs().max()) < 1e-12


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dh,Tq,Tk,qs", SHAPES)
def test_staged_stays_within_the_design_error_of_exact(dh, Tq, Tk, qs, masked):
    H, scale = 2, R.f32r_scale(1.0 / math.sqrt(dh))
    q, k, v, do = operands(dh, Tq, Tk, qs)
    thresh = R.mmf_drop_thresh(0.3) if masked else 0
    keep = R.attention_keep((7 << 32) | 99, 3, 1, 2, H, Tq, Tk, thresh) if masked else None
    inv = R.inv_keep_of(thresh)
    e = R.exact(q, k, v, do, H, scale, keep, inv)
    s = R.staged(q, k, v, do, H, scale, keep, inv)
    n = R.staged(q, k, v, do, H, scale, keep, inv, perturb=R.PERTURB, seed=1)
    for name in ("o", "dq", "dk", "dv"):
        unit = BF16_TOL * float(e[name].abs().max())
        gap, noise = float((s[name] - e[name]).abs().max()) / unit, float((s[name] - n[name]).abs().max()) / unit
        print(f"GAP {dh}-{Tq}-{Tk}-{qs}-{masked} {name} {gap:.3f}   NOISE {noise:.3f}")
        assert masked or gap <= 1.25, (name, gap)
        assert noise <= 0.41, (name, noise)
    assert float((s["lse"] - e["lse"]).abs().max()) < 1e-12 * max(1.0, float(e["lse"].abs().max()))
    # delta comes from the bf16 O: half an ulp of each O element against its dO
    o16 = R.bf16r(s["o"])
    assert bool(((s["delta"] - e["delta"]).abs() <= 1.5 * 2.0 ** -8 * R.delta_bound(o16, do, H) + 1e-6).all())


def test_staged_raises_the_running_maximum_like_the_kernel():
    """one key in the third 32-key block 5.9 / 6.1 log2 units above the first block's maximum: below DEFER the block's P
    (about 60) is rounded as it stands, above it the maximum moves and that P is exactly 1; either way O matches exact()"""
    dh, H, Tq, Tk = 64, 1, 40, 96
    for excess, rescaled in ((5.9, False), (6.1, True)):
        q = torch.zeros(1, Tq, dh, dtype=F64)
        k = torch.zeros(1, Tk, dh, dtype=F64)
        q[..., 0] = 8.0
        k[0, :, 0] = -4.0
        k[0, 3, 0] = 0.0
        k[0, 70, 0] = float(R.bf16r(torch.tensor(excess * math.log(2.0), dtype=F64)))
        g = torch.Generator().manual_seed(0)
        v, do = (R.bf16r(torch.randn(1, T, dh, generator=g, dtype=F64)) for T in (Tk, Tq))
        a = R.staged(q, k, v, do, H, 0.125)
        b = R.staged(q, k, v, do, H, 0.125, defer=1e9)
        e = R.exact(q, k, v, do, H, 0.125)
        assert float((a["o"] - e["o"]).abs().max()) <= BF16_TOL * float(e["o"].abs().max())
        assert torch.equal(a["o"], b["o"]) != rescaled
        assert float((a["lse"] - e["lse"]).abs().max()) < 1e-12


def test_hash_restatement_fixed_points():
    """the uint32 arithmetic wraps like the device's: values worked out by hand from csrc/mmf_internal.h"""
    assert int(R.mmf_mix32(0)) == 0
    x = 1
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    assert int(R.mmf_mix32(1)) == x
    assert R.mmf_drop_thresh(0.5) == 1 << 31 and R.mmf_drop_thresh(0.0) == 0 and R.mmf_drop_thresh(1e-11) == 0
    assert R.inv_keep_of(1 << 31) == 2.0 and R.inv_keep_of(0) == 1.0
    state = (0xDEADBEEF << 32) | 0x12345678
    k0, k1 = int(R.mmf_rng_key(state, 5, 0)), int(R.mmf_rng_key(state ^ (1 << 40), 5, 0))
    assert k0 ^ k1 == 1 << 8                                     # the high word enters by xor
    keep = R.attention_keep(state, 5, 2, 2, 3, 40, 50, R.mmf_drop_thresh(0.5))
    assert keep.shape == (2, 3, 40, 50) and 0.45 < float(keep.double().mean()) < 0.55
    other = R.attention_keep(state, 5, 3, 2, 3, 40, 50, R.mmf_drop_thresh(0.5))
    assert not torch.equal(keep, other)
    assert bool(np.array_equal(R.elementwise_keep(state, 5, 64, 1 << 31),
                               R.mmf_keep(R.mmf_rng_key(state, 5, 0), np.arange(64), 1 << 31)))
