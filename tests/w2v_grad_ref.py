"""The positional convolution's backward as the HIP path states it, restated as explicit tensor math in the caller's dtype: the
packed weights the kernels read, the weight gradient as a sum over time per tap, the input gradient as the FORWARD convolution on
the reversed / swapped weight with ``k - 1 - k // 2`` rows of padding in front, and the weight norm's backward in closed form.
It imports neither transformers nor the code under test; tests/test_w2v_finetune_cpu.py holds each of them to float64 autograd
through ``w2v_ref.pos_conv`` / ``w2v_ref.pos_weight``.

Shapes: activations (N, T, C) channel-last, the convolution weight ``w`` (C, cg, k) as ``torch.nn.Conv1d`` stores it, a packed
weight (C, k * cg) with row ``g cg + r`` and column ``j cg + c`` (the kernels' ``Kp`` padding columns are not modelled)."""
import torch


def pack(w):
    """(C, cg, k) -> (C, k cg): [g cg + co][j cg + ci] = w[g cg + co][ci][j], the forward's operand"""
    C, cg, k = w.shape
    return w.permute(0, 2, 1).reshape(C, k * cg)


def unpack(p, cg):
    """the inverse of ``pack``: a packed gradient (C, k cg) -> (C, cg, k)"""
    C = p.shape[0]
    return p.reshape(C, -1, cg).permute(0, 2, 1)


def pack_transposed(w):
    """(C, cg, k) -> (C, k cg): [g cg + ci][j cg + co] = w[g cg + co][ci][k - 1 - j]: taps reversed, co / ci swapped per group"""
    C, cg, k = w.shape
    return w.reshape(C // cg, cg, cg, k).flip(3).permute(0, 2, 3, 1).reshape(C, k * cg)


def conv_packed(x, packed, cg, k, pad):
    """out[n][t][g cg + r] = sum_{j, c} packed[g cg + r][j cg + c] x[n][t + j - pad][g cg + c], rows outside [0, T) zero: what
    ``mmf_w2v_posconv``'s MFMA loop computes for ``pad`` rows of padding in front"""
    N, T, C = x.shape
    xp = torch.cat([x.new_zeros(N, pad, C), x, x.new_zeros(N, k - 1 - pad, C)], dim=1)
    out = x.new_zeros(N, T, C)
    for g in range(C // cg):
        ch = slice(g * cg, (g + 1) * cg)
        for j in range(k):
            out[:, :, ch] += xp[:, j:j + T, ch] @ packed[ch, j * cg:(j + 1) * cg].T
    return out


def conv_input_grad(dz, w):
    """the gradient of ``w2v_ref.pos_conv(x, w, ...)`` with respect to x for the output gradient dz, as the forward convolution of
    dz on the reversed / swapped weight with k - 1 - k // 2 rows of padding in front"""
    C, cg, k = w.shape
    return conv_packed(dz, pack_transposed(w), cg, k, k - 1 - k // 2)


def conv_weight_grad(dz, x, cg, k):
    """packed (C, k cg): dW[g cg + co][j cg + ci] = sum_{n, t} dz[n][t][g cg + co] x[n][t + j - k // 2][g cg + ci]"""
    N, T, C = x.shape
    pad = k // 2
    xp = torch.cat([x.new_zeros(N, pad, C), x, x.new_zeros(N, k - 1 - pad, C)], dim=1)
    out = x.new_zeros(C, k * cg)
    for g in range(C // cg):
        ch = slice(g * cg, (g + 1) * cg)
        for j in range(k):
            out[ch, j * cg:(j + 1) * cg] = torch.einsum("nto,nti->oi", dz[:, :, ch], xp[:, j:j + T, ch])
    return out


def weightnorm_bwd(dw, g, v):
    """w_eff = g v / ||v||, the norm per tap over dims (0, 1); dw (C, cg, k) the gradient of w_eff -> (dg (1, 1, k), dv (C, cg, k)):
    with u = v / ||v||, dg = sum dw u and dv = (g / ||v||) (dw - u dg)"""
    norm = torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))
    u = v / norm
    dg = (dw * u).sum(dim=(0, 1), keepdim=True)
    return dg, (g / norm) * (dw - u * dg)
