"""The backward of the disentangled attention (tests/deberta_ref.py::disentangled_attention) with respect to q, k, v as a
closed form in float64, written from the math and not from the kernel.  With c = 1 / scale:

    s_ij  = c (Q_i.K_j + Q_i.posK[idx(i-j)] + K_j.posQ[idx(i-j)]);  a masked pair (mask_i mask_j == 0) scores finfo.min
    P_ij  = exp(s_ij - lse_i) for a query with mask_i != 0;  1 / T for every key of a masked query (the uniform row)
    dS_ij = c P_ij (dO_i.V_j - delta_i) on unmasked pairs, 0 on masked pairs;  delta_i = sum_d dO_i O_i
    dV_j  = sum_i P_ij dO_i
    dQ_i  = sum_j dS_ij K_j + sum_r A_ir posK[r],   A_ir = sum of dS_ij over {j : idx(i-j) = r}
    dK_j  = sum_i dS_ij Q_i + sum_r B_jr posQ[r],   B_jr = sum of dS_ij over {i : idx(i-j) = r}

tests/test_deberta_grad_cpu.py holds it to torch autograd through the definition."""
import torch


def scores(q, k, posq, posk, idx, scale):
    """-> (s (n, H, T, T) before masking, ix (T, T) = idx(i - j))"""
    n, H, T, dh = q.shape
    ar = torch.arange(T)
    ix = idx.long()[(ar[:, None] - ar[None, :]) + T - 1]
    c2p = torch.gather(q @ posk.transpose(-1, -2), -1, ix.expand(n, H, T, T))
    p2c = torch.gather(k @ posq.transpose(-1, -2), -1, ix.t().expand(n, H, T, T)).transpose(-1, -2)
    return (q @ k.transpose(-1, -2) + c2p + p2c) / scale, ix


def attention_stats(q, k, v, posq, posk, idx, mask, scale):
    """-> (O (n, H, T, dh), lse (n, H, T)) of the masked scores; a masked query row's lse is finfo.min + log T"""
    s, _ = scores(q, k, posq, posk, idx, scale)
    if mask is not None:
        m = mask != 0
        s = s.masked_fill(~(m[:, :, None] & m[:, None, :])[:, None], torch.finfo(s.dtype).min)
    lse = torch.logsumexp(s, dim=-1)
    return torch.softmax(s, dim=-1) @ v, lse


def attention_backward(q, k, v, posq, posk, idx, mask, scale, dO, O=None, lse=None, f32_tol=None):
    """q, k, v, dO (n, H, T, dh); posq, posk (H, 2S, dh); idx (2T - 1,); mask (n, T) or None -> dq, dk, dv.
    ``O`` given: delta is taken from it (what a kernel handed a rounded O computes); ``lse`` given: P = exp(s - lse).
    ``f32_tol`` given: also -> (noise_dq, noise_dk), the f32 summation noise of dP - delta carried through dS into the two
    gradients, each of the two sums held to ``f32_tol`` x the sum of its terms' magnitudes (tests/test_attention_paths_gpu.py's
    term: where the softmax is one-hot, T = 1 for one, dP - delta cancels to 0 exactly and a kernel returns that noise)."""
    n, H, T, dh = q.shape
    R = posq.shape[1]
    s, ix = scores(q, k, posq, posk, idx, scale)
    m = torch.ones(n, T, dtype=torch.bool) if mask is None else mask != 0
    keep = (m[:, :, None] & m[:, None, :])[:, None].expand(n, H, T, T)
    q_on = m[:, None, :, None].expand(n, H, T, T)
    if O is None or lse is None:
        O0, lse0 = attention_stats(q, k, v, posq, posk, idx, mask, scale)
        O, lse = O0 if O is None else O, lse0 if lse is None else lse
    zero = torch.zeros((), dtype=s.dtype)
    lse_safe = torch.where(m[:, None, :], lse, zero)                      # a masked row's lse is not used
    P = torch.where(keep, torch.exp(s - lse_safe[..., None]), zero)
    P = torch.where(q_on, P, torch.full((), 1.0 / T, dtype=s.dtype))
    delta = (dO * O).sum(-1, keepdim=True)
    dS = torch.where(keep, P * (dO @ v.transpose(-1, -2) - delta), zero) / scale
    dv = P.transpose(-1, -2) @ dO
    A = torch.zeros(n, H, T, R, dtype=s.dtype).scatter_add_(-1, ix.expand(n, H, T, T), dS)                          # [i, r]
    B = torch.zeros(n, H, T, R, dtype=s.dtype).scatter_add_(-1, ix.t().expand(n, H, T, T), dS.transpose(-1, -2))    # [j, r]
    dq = dS @ k + A @ posk
    dk = dS.transpose(-1, -2) @ q + B @ posq
    if f32_tol is None:
        return dq, dk, dv
    nS = torch.where(keep, P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO * O).abs().sum(-1, keepdim=True)), zero) * (f32_tol / scale)
    nA = torch.zeros(n, H, T, R, dtype=s.dtype).scatter_add_(-1, ix.expand(n, H, T, T), nS)
    nB = torch.zeros(n, H, T, R, dtype=s.dtype).scatter_add_(-1, ix.t().expand(n, H, T, T), nS.transpose(-1, -2))
    return dq, dk, dv, nS @ k.abs() + nA @ posk.abs(), nS.transpose(-1, -2) @ q.abs() + nB @ posq.abs()
