"""What the three forward restatements (tests/vit_ref.py, tests/w2v_ref.py, tests/deberta_ref.py) share.  Like them it imports
neither transformers nor the code under test."""
import math

import torch


def config_kwargs(cfg):
    return dict(vars(cfg))


def _r(t, on, dtype):
    """``t`` as the HIP path stores it when ``on``: rounded to bf16, carried on in ``dtype``"""
    return t.to(torch.bfloat16).to(dtype) if on else t


def layer_norm(x, gamma, beta, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def gelu_erf(x):
    """x Phi(x), Phi through erfc: 1 + erf keeps no digit of Phi in the left tail, in float64 from x = -8.3 down"""
    return x * (0.5 * torch.erfc(x * (-1.0 / math.sqrt(2.0))))
