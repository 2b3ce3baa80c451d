"""CPU: the algebra of the uniform attention backward (csrc/attention2.hip, include/mmfusion.h: mmf_attn_bwd_grouped_uniform).
For an attention that is consumed through its mean over T only, with u[b] = g[b] / T the one output-gradient row of batch row b
and u_h a head's columns of it:

    c[k]     = V[k,:] . u_h
    delta[q] = O[q,:] . u_h
    dS[q,k]  = P[q,k] (c[k] - delta[q])
    dQ = scale dS K      dK = scale dS^T Q      dV[k,:] = (sum_q P[q,k]) u_h

restated in float64 and held against float64 autograd through softmax attention followed by the mean over T, for dQ, dK, dV
(and delta against sum_c O dO of the materialised dO).  Both sides are float64 sums of at most 96 x 65 terms of O(1) operands:
1e-12 x max|reference| is a thousand times their rounding and a million times below any slip in the formulas."""
import math

import pytest
import torch

F64 = torch.float64
B, H = 2, 2
TOL = 1e-12


def heads(x):
    b, t, d = x.shape
    return x.reshape(b, t, H, d // H).transpose(1, 2)            # (B, H, T, dh)


def merge(x):
    b, h, t, dh = x.shape
    return x.transpose(1, 2).reshape(b, t, h * dh)


def uniform_backward(q, k, v, u, scale):
    """the four formulas; u (B, d)"""
    qh, kh, vh = heads(q), heads(k), heads(v)
    uh = u.reshape(B, H, 1, -1)                                    # (B, H, 1, dh)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    o = p @ vh
    c = (vh * uh).sum(-1)                                          # (B, H, Tk)
    delta = (o * uh).sum(-1)                                       # (B, H, Tq)
    ds = p * (c[:, :, None, :] - delta[..., None])
    dq, dk = ds @ kh * scale, ds.transpose(-1, -2) @ qh * scale
    dv = p.sum(-2)[..., None] * uh
    return merge(dq), merge(dk), merge(dv), delta, merge(o)


@pytest.mark.parametrize("T", [7, 33, 65])
@pytest.mark.parametrize("dh", [64, 96])
def test_formulas_equal_autograd_through_attention_and_mean(dh, T):
    g = torch.Generator().manual_seed(100 * dh + T)
    d = H * dh
    q, k, v = (torch.randn(B, T, d, generator=g, dtype=F64).requires_grad_(True) for _ in range(3))
    gy = torch.randn(B, d, generator=g, dtype=F64)                 # gradient of the pooled (B, d) output
    scale = 1.0 / math.sqrt(dh)
    p = torch.softmax(heads(q) @ heads(k).transpose(-1, -2) * scale, -1)
    o = merge(p @ heads(v))
    o.mean(dim=1).backward(gy)
    u = gy / T
    dq, dk, dv, delta, o2 = uniform_backward(q.detach(), k.detach(), v.detach(), u, scale)
    do = u[:, None, :].expand(B, T, d)                             # what the mean's backward would materialise
    want_delta = (heads(o.detach()) * heads(do)).sum(-1)
    for name, got, want in (("dQ", dq, q.grad), ("dK", dk, k.grad), ("dV", dv, v.grad), ("delta", delta, want_delta)):
        err, ref = float((got - want).abs().max()), float(want.abs().max())
        assert err <= TOL * ref, f"{name}: {err:.3e} against max|ref| {ref:.3e}"
