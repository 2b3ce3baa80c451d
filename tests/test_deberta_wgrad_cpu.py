"""CPU: the closed-form gradient of the position tables (tests/deberta_wgrad_ref.py) against torch autograd through the
definition (``deberta_grad_ref.scores`` / ``attention_stats`` with posQ / posK as leaves), which rows it may touch, and the ABI
of the fine-tuning entries."""
import math
import os
import re

import pytest
import torch

import deberta_grad_ref as G
import deberta_wgrad_ref as WG
from test_deberta_grad_cpu import _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mmf_deberta_attn_bwd_pos_workspace_bytes", "mmf_deberta_attn_bwd_pos")
CASES = [(1, 3, 1, 8, 32, None), (1, 2, 33, 8, 32, None), (2, 2, 70, 8, 32, 50), (1, 2, 33, 256, 512, None)]


@pytest.mark.parametrize("n,H,T,S,max_pos,pad", CASES)
def test_table_gradients_are_autograd_of_the_definition(n, H, T, S, max_pos, pad):
    q, k, v, posq, posk, idx, mask, dO = _case(n, H, T, S, max_pos, pad)
    scale = math.sqrt(3.0 * 64)
    leaves = [t.clone().requires_grad_(True) for t in (posq, posk)]
    out, _ = G.attention_stats(q, k, v, *leaves, idx, mask, scale)
    want = torch.autograd.grad(out, leaves, dO)
    got = WG.table_gradients(q, k, v, posq, posk, idx, mask, scale, dO)
    O, lse = G.attention_stats(q, k, v, posq, posk, idx, mask, scale)
    again = WG.table_gradients(q, k, v, posq, posk, idx, mask, scale, dO, O=O, lse=lse)
    *_, nq, nk = WG.table_gradients(q, k, v, posq, posk, idx, mask, scale, dO, f32_tol=1e-5)
    for name, a, b, c, nz in zip(("posQ", "posK"), got, want, again, (nq, nk)):
        err = float((a - b).abs().max())
        print(f"d{name} (n={n} H={H} T={T} S={S}): max abs error {err:.2e}, |want| max {float(b.abs().max()):.2e}")
        assert a.shape == (H, 2 * S, 64) and err <= 1e-12 and float((c - b).abs().max()) <= 1e-12
        assert bool((nz >= 0).all()) and bool(torch.isfinite(nz).all())
    # rows no (i, j) pair maps to are exactly 0, in the closed form and in autograd; at S = 256 and T = 33 that is all but the
    # rows of the deltas -32 .. 32
    reached = WG.reached_rows(idx)
    rest = torch.ones(2 * S, dtype=torch.bool)
    rest[reached] = False
    if (S, T) == (256, 33):
        assert reached == list(range(256 - 32, 256 + 33))
    for a, b in zip(got, want):
        assert bool((a[:, rest] == 0).all()) and bool((b[:, rest] == 0).all())
    if T > 1:
        assert all(float(a[:, reached].abs().max()) > 0 for a in got)


def test_fine_tuning_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mmfusion.h")).read()
    declared = set(re.findall(r"\b(mmf_[a-z0-9_]+)\s*\(", header))
    from mmfusion import lib
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in lib.SYMBOLS, name
