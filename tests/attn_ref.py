"""float64 restatement of one fused-attention problem (csrc/attention2.hip), forward and hand-written backward, and a numpy
uint32 restatement of the counter hash that keys its dropout masks (csrc/mmf_internal.h).

Operands are (B, T, H*dh) float64 tensors holding bf16-representable values; heads are consecutive dh-column groups.
`scale` is the f32 value the kernel is handed (f32r_scale()), `keep` an optional (B, H, Tq, Tk) bool mask, `inv_keep` the factor kept probabilities are multiplied by.  Both forms
return a dict: o (B, Tq, H*dh), lse and delta (B, H, Tq), dq / dk / dv shaped like q / k / v.

exact():  softmax(Q K^T scale) V, LSE = logsumexp of the scaled scores, delta = rowsum(O * dO), dQ / dK / dV; under dropout
          the mask is applied to P in front of P.V only (nn.MultiheadAttention(dropout=p)).
staged(): the same with the kernels' rounding points and only those:
          * the forward's P — relative to the kernel's running maximum: 32-key blocks in the log2 domain, raised for a
            32-row query block only when some row's block maximum exceeds it by more than DEFER — dropped, rescaled and rounded
            to bf16 before P.V, while the row sum takes the unrounded, undropped P;
          * LSE rounded to f32; the backward's P recomputed as exp(s scale - LSE) from it;
          * delta from the bf16 O the backward is given (default: this forward's O rounded), stored as f32;
          * the dropped-and-rescaled P rounded to bf16 before dO^T.P, dS rounded to bf16 before the dQ and dK products.
          The final O / dQ / dK / dV are NOT rounded: the kernel is then half a bf16 ulp plus accumulation noise away, where a
          reference rounded the same way could differ by a whole ulp on a flip.
          `perturb` multiplies every raw score by 1 + perturb * u, u uniform in [-1, 1]: the difference between two staged()
          runs with perturb = 0 and 2^-22 is the reference's own sensitivity to f32-sized errors in the scores (flipped
          roundings of P and dS), the noise term of the GPU tests' bounds."""
import math

import numpy as np
import torch

F64 = torch.float64
DEFER = 6.0                                           # attn2_common.h
NEG_BIG = -1.0e30                                     # attn_helpers.h
LOG2E = 1.0 / math.log(2.0)
LN2 = math.log(2.0)
PERTURB = 2.0 ** -22


def bf16r(x):
    """round to bf16 the way the device does (from f32, nearest even), back in float64"""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def f32r(x):
    return x.to(torch.float32).to(F64)


def f32r_scale(x):
    return float(np.float32(x))


def heads(x, H):
    B, T, d = x.shape
    return x.reshape(B, T, H, d // H).transpose(1, 2)          # (B, H, T, dh)


def merge(x):
    B, H, T, dh = x.shape
    return x.transpose(1, 2).reshape(B, T, H * dh)


def _mask(keep, inv_keep, like):
    return torch.ones_like(like) if keep is None else keep.to(F64) * inv_keep


def _backward(p, pd16, ds_round, qh, kh, vh, doh, delta, w, scale):
    dp = (doh @ vh.transpose(-1, -2)) * w
    ds = ds_round(p * (dp - delta[..., None]))
    return merge(ds @ kh * scale), merge(ds.transpose(-1, -2) @ qh * scale), merge(pd16.transpose(-1, -2) @ doh)


def exact(q, k, v, do, H, scale, keep=None, inv_keep=1.0):
    qh, kh, vh, doh = heads(q, H), heads(k, H), heads(v, H), heads(do, H)
    s = qh @ kh.transpose(-1, -2) * scale
    p = torch.softmax(s, -1)
    w = _mask(keep, inv_keep, p)
    pd = p * w
    o = pd @ vh
    delta = (o * doh).sum(-1)
    dq, dk, dv = _backward(p, pd, lambda x: x, qh, kh, vh, doh, delta, w, scale)
    return dict(o=merge(o), lse=torch.logsumexp(s, -1), delta=delta, dq=dq, dk=dk, dv=dv)


def staged(q, k, v, do, H, scale, keep=None, inv_keep=1.0, o_bwd=None, lse_bwd=None, perturb=0.0, seed=0, defer=DEFER):
    qh, kh, vh, doh = heads(q, H), heads(k, H), heads(v, H), heads(do, H)
    B, _, Tq, dh = qh.shape
    Tk = kh.shape[2]
    s = qh @ kh.transpose(-1, -2)                                # raw scores
    if perturb:
        g = torch.Generator().manual_seed(seed)
        s = s * (1.0 + perturb * (2.0 * torch.rand(s.shape, generator=g, dtype=F64) - 1.0))
    w = _mask(keep, inv_keep, s)
    c = scale * LOG2E                                           # the kernel's exponent factor, log2 domain
    # ---- forward: online softmax over 32-key blocks, the running maximum raised per 32-row query block
    m = torch.full((B, H, Tq), NEG_BIG, dtype=F64)
    l = torch.zeros((B, H, Tq), dtype=F64)
    o = torch.zeros((B, H, Tq, dh), dtype=F64)
    qblk = torch.arange(Tq) // 32
    for k0 in range(0, Tk, 32):
        sb = s[..., k0:k0 + 32]
        mx = sb.max(-1).values * c
        over = mx > m + defer                                    # per row
        raise_blk = torch.nn.functional.pad(over, (0, -Tq % 32)).reshape(B, H, -1, 32).any(-1)
        up = raise_blk[..., qblk]                                # wave-uniform: every row of the block follows
        mnew = torch.where(up, torch.maximum(m, mx), m)
        alpha = torch.exp2(m - mnew)
        m, l, o = mnew, l * alpha, o * alpha[..., None]
        p = torch.exp2(sb * c - m[..., None])
        l = l + p.sum(-1)
        o = o + bf16r(p * w[..., k0:k0 + 32]) @ vh[:, :, k0:k0 + 32]
    o = o / l[..., None]
    lse = m * LN2 + torch.log(l)
    # ---- backward: recompute from the f32 LSE and the bf16 O it is handed
    lse32 = f32r(lse) if lse_bwd is None else lse_bwd
    o16 = bf16r(o) if o_bwd is None else heads(o_bwd, H)
    delta = f32r((o16 * doh).sum(-1))
    p = torch.exp(s * scale - lse32[..., None])
    dq, dk, dv = _backward(p, bf16r(p * w), bf16r, qh, kh, vh, doh, delta, w, scale)
    return dict(o=merge(o), lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)


def f32_noise(q, k, v, do, H, scale, o16, lse32, tol, keep=None, inv_keep=1.0):
    """What f32 summation noise in dP - delta does to dQ and dK.  dS = P (dP - delta) subtracts two f32 sums of dh products
    each; where the softmax is (nearly) one-hot the difference cancels to 0 and the sums' rounding noise is all that is left
    (Tk = 1: dS = 0 exactly, yet the kernel returns 1e-7).  With each sum held to tol x the sum of its terms' magnitudes (the
    bound the delta output itself is held to), |d dS| <= P tol (|dO|.|V|^T w + sum|O dO|); returns the largest resulting
    |d dQ| and |d dK| as dict(dq=, dk=).  Perturbing the scores (staged(perturb=)) does not model this."""
    qh, kh, vh, doh = heads(q, H), heads(k, H), heads(v, H), heads(do, H)
    p = torch.exp(qh @ kh.transpose(-1, -2) * scale - lse32[..., None])
    w = _mask(keep, inv_keep, p)
    e = p * tol * ((doh.abs() @ vh.abs().transpose(-1, -2)) * w + delta_bound(o16, do, H)[..., None])
    return dict(dq=float((e @ kh.abs()).max()) * scale, dk=float((e.transpose(-1, -2) @ qh.abs()).max()) * scale)


def delta_bound(o16, do, H):
    """sum |O * dO| per (b, h, q): the scale of the dQ kernel's delta output"""
    return (heads(o16, H) * heads(do, H)).abs().sum(-1)


# ------------------------------------------------------------------------------------------------ counter hash
M32 = np.uint64(0xFFFFFFFF)
GOLD = np.uint64(0x9E3779B9)


def _u(x):
    return np.asarray(x, dtype=np.uint64) & M32


def mmf_mix32(x):
    x = _u(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def mmf_rng_key(state, site, sub):
    state = int(state) & 0xFFFFFFFFFFFFFFFF
    lo, hi = state & 0xFFFFFFFF, state >> 32
    return mmf_mix32(lo ^ ((int(site) * 0x9E3779B9) & 0xFFFFFFFF)) ^ np.uint64(hi) ^ ((_u(sub) * np.uint64(0x85EBCA6B)) & M32)


def mmf_keep(key, idx, thresh):
    return mmf_mix32((_u(key) + ((_u(idx) * GOLD) & M32)) & M32) >= np.uint64(thresh)


def mmf_drop_thresh(p):
    t = float(np.float32(p)) * 4294967296.0
    return 4294967295 if t >= 4294967295.0 else int(t)


def inv_keep_of(thresh):
    """the f32 factor the host hands the kernels"""
    if thresh == 0:
        return 1.0
    one = np.float32(1.0)
    return float(one / (one - np.float32(thresh) * np.float32(1.0 / 4294967296.0)))


def elementwise_keep(state, site, n, thresh):
    """mmf_dropout (elementwise.hip): sub-stream 0, element index i (< 2^32 here)"""
    return mmf_keep(mmf_rng_key(state, site, 0), np.arange(n, dtype=np.uint64), thresh)


def attention_keep(state, site, problem_index, B, H, Tq, Tk, thresh):
    """(B, H, Tq, Tk) bool: stream id problem_index * 4096 + b*H + h, element index q*Tk + key (mod 2^32)"""
    bh = np.arange(B * H, dtype=np.uint64)
    key = mmf_rng_key(state, site, np.uint64(problem_index * 4096) + bh)                  # (B*H,)
    idx = (np.arange(Tq, dtype=np.uint64)[:, None] * np.uint64(Tk) + np.arange(Tk, dtype=np.uint64)[None, :]) & M32
    keep = mmf_keep(key[:, None, None], idx[None], thresh)
    return torch.from_numpy(keep.reshape(B, H, Tq, Tk))
