"""CPU: the closed-form backward of the disentangled attention (tests/deberta_grad_ref.py) against torch autograd through its
definition, what the restated backbone's input gradient does on padded rows, and the ABI of the backward entries."""
import math
import os
import re

import pytest
import torch

import deberta_grad_ref as G
import deberta_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mmf_deberta_attn_fwd_lse", "mmf_deberta_attn_bwd", "mmf_deberta_embed_bwd", "mmf_bias_gelu_bf16_to", "mmf_bias_gelu_bwd_bf16")
CASES = [(2, 2, 70, 8, 32, 50), (1, 2, 33, 8, 32, None), (1, 1, 200, 256, 512, 150), (1, 3, 1, 8, 32, None)]


def _case(n, H, T, S, max_pos, pad, seed=0):
    g = torch.Generator().manual_seed(100 * T + S + seed)
    q, k, v, dO = (torch.randn(n, H, T, 64, generator=g, dtype=torch.float64) for _ in range(4))
    posq, posk = (torch.randn(H, 2 * S, 64, generator=g, dtype=torch.float64) for _ in range(2))
    mask = None
    if pad is not None:
        mask = torch.ones(n, T)
        mask[n - 1, pad:] = 0
    return q, k, v, posq, posk, deberta_ref.bucket_index(T, S, max_pos), mask, dO


@pytest.mark.parametrize("n,H,T,S,max_pos,pad", CASES)
def test_closed_form_is_autograd_of_the_definition(n, H, T, S, max_pos, pad):
    q, k, v, posq, posk, idx, mask, dO = _case(n, H, T, S, max_pos, pad)
    scale = math.sqrt(3.0 * 64)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = deberta_ref.disentangled_attention(*leaves, posq, posk, idx, mask, scale)
    want = torch.autograd.grad(out, leaves, dO)
    got = G.attention_backward(q, k, v, posq, posk, idx, mask, scale, dO)
    O, lse = G.attention_stats(q, k, v, posq, posk, idx, mask, scale)
    again = G.attention_backward(q, k, v, posq, posk, idx, mask, scale, dO, O=O, lse=lse)
    for name, a, b, c in zip("qkv", got, want, again):
        err = float((a - b).abs().max())
        print(f"d{name} (n={n} H={H} T={T} S={S}): max abs error {err:.2e}")
        assert err <= 1e-12 and float((c - b).abs().max()) <= 1e-12
    if pad is not None:
        dq, dk, dv = got
        assert bool((dq[n - 1, :, pad:] == 0).all()) and bool((want[0][n - 1, :, pad:] == 0).all())       # masked query rows
        assert bool((dk[n - 1, :, pad:] == 0).all()) and bool((want[1][n - 1, :, pad:] == 0).all())       # masked keys
        uniform = dO[n - 1, :, pad:].sum(dim=1, keepdim=True) / T                                         # 1/T dO_i of the masked rows
        assert float((dv[n - 1, :, pad:] - uniform).abs().max()) <= 1e-12


def test_restated_backbone_passes_no_gradient_to_padded_rows():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(2, 40, cfg.hidden_size, generator=g, dtype=torch.float64).requires_grad_(True)
    mask = torch.ones(2, 40)
    mask[1, 25:] = 0
    out = deberta_ref.deberta_forward(sd, emb, mask, cfg)
    (grad,) = torch.autograd.grad(out, emb, torch.randn(out.shape, generator=g, dtype=torch.float64))
    assert bool((grad[1, 25:] == 0).all()) and float(grad[1, :25].abs().max()) > 0 and float(grad[0].abs().max()) > 0


def test_backward_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mmfusion.h")).read()
    declared = set(re.findall(r"\b(mmf_[a-z0-9_]+)\s*\(", header))
    from mmfusion import lib
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in lib.SYMBOLS, name
