"""The two-launch forms that the fused seams replaced, composed by hand from launches that exist unchanged, for the tests that hold
the fused forms bit-equal to them (test_relu_bits_gpu.py, test_ln2_add3_gpu.py, test_mult_fused_seams_gpu.py):

  * ``ffn_residual_group``: the grouped FFN whose dgrad reads the hidden tensor h through MMF_EPI_MASK_AUX (no bits written, none read);
  * ``ln2_add3_group``: ``ops.layernorm_group`` over (pre_a, pre_b) of every sum, then ``ops.add3_group`` on (x, y_a, y_b);
  * ``unpack_relu_bits``: a bit buffer as a boolean (M, N) tensor, by the layout include/mmfusion.h documents."""
from typing import List, Optional

import torch

from mmfusion import ops
from mmfusion.lib import EPI_ADD_AUX, EPI_BIAS, EPI_MASK_AUX, EPI_RELU, GEMM_NN, GEMM_NT

BF16 = torch.bfloat16


class _AuxFFN(torch.autograd.Function):
    """tensors = [x_0, W1_0, b1_0, W2_0, b2_0, x_1, ...]: y_i = x_i + W2_i dropout(relu(W1_i x_i + b1_i)) + b2_i, dH masked by h itself"""

    @staticmethod
    def forward(ctx, layers, drop, *tensors):
        n = len(layers)
        xs = [tensors[5 * i] for i in range(n)]
        hs = [torch.empty((x.shape[0], l1.weight.shape[0]), dtype=BF16, device=x.device) for x, (l1, _) in zip(xs, layers)]
        ops.gemm_group(GEMM_NT, [(x, ops.shadow(l1.weight), h, l1.bias.detach(), None)
                                 for x, h, (l1, _) in zip(xs, hs, layers)], EPI_BIAS | EPI_RELU, dropout=drop)
        ctx.keep_scale = 1.0 / (1.0 - drop[0]) if drop is not None else 1.0
        ys = [torch.empty_like(x) for x in xs]
        ops.gemm_group(GEMM_NT, [(h, ops.shadow(l2.weight), y, l2.bias.detach(), x)
                                 for x, h, y, (_, l2) in zip(xs, hs, ys, layers)], EPI_BIAS | EPI_ADD_AUX)
        ctx.layers = layers
        ctx.save_for_backward(*xs, *hs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        layers = ctx.layers
        n = len(layers)
        xs, hs = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        idx = [i for i, g in enumerate(gys) if g is not None]
        dys = {i: gys[i].contiguous() for i in idx}
        dhs = {i: torch.empty_like(hs[i]) for i in idx}
        dxs = {i: torch.empty_like(xs[i]) for i in idx}
        ops.gemm_group(GEMM_NN, [(dys[i], ops.shadow(layers[i][1].weight), dhs[i], None, hs[i]) for i in idx], EPI_MASK_AUX,
                       alpha=ctx.keep_scale)
        ops.gemm_group(GEMM_NN, [(dhs[i], ops.shadow(layers[i][0].weight), dxs[i], None, dys[i]) for i in idx], EPI_ADD_AUX)
        for i in idx:
            for l, dy_, x_ in ((layers[i][1], dys[i], hs[i]), (layers[i][0], dhs[i], xs[i])):
                if l.weight.requires_grad:
                    ops.queue_wgrad(dy_, x_, l.weight.grad, l.bias.grad)
        grads: List[Optional[torch.Tensor]] = [None] * (5 * n)
        for i in idx:
            grads[5 * i] = dxs[i]
        return (None, None, *grads)


def ffn_residual_group(items, dropout_p: float = 0.0):
    layers, tensors = [], []
    for x, l1, l2 in items:
        layers.append((l1, l2))
        tensors += [x, l1.weight, l1.bias, l2.weight, l2.bias]
    drop = (float(dropout_p), ops.next_site()) if dropout_p > 0.0 else None
    return list(_AuxFFN.apply(layers, drop, *tensors))


def ln2_add3_group(items, eps: float = 1e-5):
    ys = ops.layernorm_group([(pre, nm.weight, nm.bias) for _, pa, na, pb, nb in items for pre, nm in ((pa, na), (pb, nb))], eps)
    return ops.add3_group([(x, ys[2 * i], ys[2 * i + 1]) for i, (x, *_) in enumerate(items)])


def unpack_relu_bits(bits: torch.Tensor, M: int, N: int) -> torch.Tensor:
    """uint16 [ceil(M/32)][ceil(N/32)][64]; element (m, n) is bit 2 * ((n % 32) / 8) + (n % 4) / 2 + 8 * (n % 2) of word
    [m / 32][n / 32][32 * ((n / 4) % 2) + m % 32]"""
    mb, nb = (M + 31) // 32, (N + 31) // 32
    w = bits[:mb * nb * 128].view(torch.int16).to(torch.int32).bitwise_and(0xffff).view(mb, nb, 64)
    m = torch.arange(M, device=bits.device)[:, None]
    n = torch.arange(N, device=bits.device)[None, :]
    word = w[m // 32, n // 32, 32 * ((n // 4) % 2) + m % 32]
    return ((word >> (2 * ((n % 32) // 8) + (n % 4) // 2 + 8 * (n % 2))) & 1).bool()
