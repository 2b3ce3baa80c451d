"""The gradient of the disentangled attention's position tables posQ / posK (fine-tuning: the layer's q / k weights also project
the relative embeddings) as a closed form in float64, on top of tests/deberta_grad_ref.py and in its notation.  With dS, and its
bucket sums A_ir = sum of dS_ij over {j : idx(i-j) = r}, B_jr = sum of dS_ij over {i : idx(i-j) = r}, per item and head,

    dposK[r] = sum_i A_ir Q_i        dposQ[r] = sum_j B_jr K_j        summed over all n items

because posK[r] enters s_ij through Q_i . posK[idx(i-j)] and posQ[r] through K_j . posQ[idx(i-j)].  A row no (i, j) pair maps to
gets exactly 0, and so does one that only masked pairs map to.  tests/test_deberta_wgrad_cpu.py holds it to torch autograd
through the definition."""
import torch

import deberta_grad_ref as G


def table_gradients(q, k, v, posq, posk, idx, mask, scale, dO, O=None, lse=None, f32_tol=None):
    """q, k, v, dO (n, H, T, dh); posq, posk (H, 2S, dh); idx (2T - 1,); mask (n, T) or None -> dposq, dposk (H, 2S, dh).
    ``O`` / ``lse`` given: as ``deberta_grad_ref.attention_backward`` takes them (delta from a rounded O, P = exp(s - lse)).
    ``f32_tol`` given: also -> (noise_dposq, noise_dposk), the f32 summation noise of dP - delta carried through dS and its
    bucket sums into the two gradients (``attention_backward(f32_tol=...)``'s term: where the softmax is one-hot the true
    gradient is 0 and a kernel returns that noise)."""
    n, H, T, dh = q.shape
    R = posq.shape[1]
    s, ix = G.scores(q, k, posq, posk, idx, scale)
    m = torch.ones(n, T, dtype=torch.bool) if mask is None else mask != 0
    keep = (m[:, :, None] & m[:, None, :])[:, None].expand(n, H, T, T)
    q_on = m[:, None, :, None].expand(n, H, T, T)
    if O is None or lse is None:
        O0, lse0 = G.attention_stats(q, k, v, posq, posk, idx, mask, scale)
        O, lse = O0 if O is None else O, lse0 if lse is None else lse
    zero = torch.zeros((), dtype=s.dtype)
    lse_safe = torch.where(m[:, None, :], lse, zero)
    P = torch.where(keep, torch.exp(s - lse_safe[..., None]), zero)
    P = torch.where(q_on, P, torch.full((), 1.0 / T, dtype=s.dtype))
    delta = (dO * O).sum(-1, keepdim=True)
    dS = torch.where(keep, P * (dO @ v.transpose(-1, -2) - delta), zero) / scale

    def sums(t):                                                  # -> (A [i, r], B [j, r]) of a (n, H, T, T) tensor
        a = torch.zeros(n, H, T, R, dtype=s.dtype).scatter_add_(-1, ix.expand(n, H, T, T), t)
        b = torch.zeros(n, H, T, R, dtype=s.dtype).scatter_add_(-1, ix.t().expand(n, H, T, T), t.transpose(-1, -2))
        return a, b
    A, B = sums(dS)
    dposk = torch.einsum("nhir,nhid->hrd", A, q)
    dposq = torch.einsum("nhjr,nhjd->hrd", B, k)
    if f32_tol is None:
        return dposq, dposk
    nS = torch.where(keep, P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO * O).abs().sum(-1, keepdim=True)), zero) * (f32_tol / scale)
    nA, nB = sums(nS)
    return dposq, dposk, torch.einsum("nhjr,nhjd->hrd", nB, k.abs()), torch.einsum("nhir,nhid->hrd", nA, q.abs())


def reached_rows(idx):
    """the table rows some (i, j) pair of a T-token item maps to: the values of idx (every delta in -(T-1) .. T-1 occurs)"""
    return sorted(set(int(v) for v in idx.tolist()))
