"""Host restatement of the keyed-dropout vocabulary of the fusion path (csrc/mmf_internal.h: every mask is
mmf_keep(mmf_rng_key(state, site, sub), idx, thresh)) — which (sub, idx) each kernel uses, stated once for the tests — and of the
GEMM epilogue's order in float64.  The hash itself is tests/attn_ref.py's; nothing here restates it.

  kernel                                               sub                     idx
  gemm2 / gemm6 / gemm7 epilogue (MMF_EPI_DROPOUT)     caller's problem index  m * N + n        (N, never ldc)
  skinny_fwd_ex / skinny_dgrad_ex                      problem index           m * N + n        (dgrad: N = N_out, the reduction)
  gat3 fwd / bwd                                       b                       (3 i + j) * heads + h
  modality dropout (draw = 1)                          0                       3 b + m; a sample left with nothing gets modality
                                                                               mmf_mix32(key ^ (0x51ed270b + b)) % 3 back
  mmf_dropout                                          0                       i                (attn_ref.elementwise_keep)
  ops: state = (seed & 0x7FFFFFFF) << 20, + 1 per begin_training_forward; sites 1, 2, ... in call order

Epilogue on the f32 accumulator, the order of the kernels' `finish` lambdas (gemm2.hip, gemm6_parts.h, gemm7.hip drain_tile):
  + bias[n] -> relu -> keep ? v * inv_keep : 0 -> (aux > 0) ? v : 0 -> * alpha -> + aux -> + C_old
Masks are numpy bool arrays, arithmetic is torch float64 on the CPU."""
import numpy as np
import torch

from attn_ref import M32, bf16r, elementwise_keep, inv_keep_of, mmf_drop_thresh, mmf_keep, mmf_mix32, mmf_rng_key  # noqa: F401

F64 = torch.float64
U24 = 2.0 ** -24                                     # unit roundoff of f32
BF16_RN = 2.0 ** -8                                  # relative error of one round-to-nearest to bf16 (8 significant bits)
FALLBACK_SALT = 0x51ED270B                           # loss.hip: modality_dropout_kernel


def gemm_keep(state, site, problem, M, N, thresh):
    """(M, N) bool: element m * N + n (mod 2^32) of sub-stream `problem`.  The skinny forward and dgrad use the same keying."""
    key = mmf_rng_key(state, site, problem)
    idx = (np.arange(M, dtype=np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]) & M32
    return mmf_keep(key, idx, thresh)


def gat3_keep(state, site, B, heads, thresh):
    """(B, 3 dst i, 3 src j, heads) bool: sub-stream b, element (3 i + j) * heads + h"""
    key = mmf_rng_key(state, site, np.arange(B, dtype=np.uint64))                       # (B,)
    return mmf_keep(key[:, None], np.arange(9 * heads, dtype=np.uint64)[None, :], thresh).reshape(B, 3, 3, heads)


def modality_keep(state, site, B, thresh):
    """((B, 3) bool with the fallback applied, (B,) bool: the rows that took it)"""
    key = mmf_rng_key(state, site, 0)
    keep = mmf_keep(key, np.arange(3 * B, dtype=np.uint64), thresh).reshape(B, 3).copy()
    fell = ~keep.any(axis=1)
    b = np.arange(B, dtype=np.uint64)
    pick = (mmf_mix32(key ^ ((np.uint64(FALLBACK_SALT) + b) & M32)) % np.uint64(3)).astype(np.int64)
    keep[fell, pick[fell]] = True
    return keep, fell


def ops_state(seed, forwards):
    """the 64-bit state after ops.seed_dropout(seed) and `forwards` calls of ops.begin_training_forward()"""
    return (((int(seed) & 0x7FFFFFFF) << 20) + int(forwards)) & 0xFFFFFFFFFFFFFFFF


def state_tensor(state, device):
    """the device int64 [1] a kernel reads `state` (an unsigned 64-bit value) from"""
    state = int(state) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([state - (1 << 64) if state >= 1 << 63 else state], dtype=torch.int64, device=device)


def _keep_t(keep, like):
    return torch.ones_like(like, dtype=torch.bool) if keep is None else torch.from_numpy(np.ascontiguousarray(keep))


def epilogue(acc, bias=None, relu=False, keep=None, inv_keep=1.0, mask_aux=None, alpha=1.0, add_aux=None, c_old=None):
    """float64: acc (M, N) the exact product of the bf16-rounded operands; bias (N,), aux / c_old (M, N) hold the values the
    kernel reads (bf16-rounded aux, f32 bias and old C).  Unrounded result."""
    v = acc if bias is None else acc + bias
    if relu:
        v = v.clamp_min(0)
    if keep is not None:
        v = torch.where(_keep_t(keep, v), v * inv_keep, torch.zeros_like(v))
    if mask_aux is not None:
        v = torch.where(mask_aux > 0, v, torch.zeros_like(v))
    v = v * alpha
    if add_aux is not None:
        v = v + add_aux
    if c_old is not None:
        v = v + c_old
    return v


def epilogue_bound(ref, abs_acc, K, out_bf16, keep=None, inv_keep=1.0, mask_aux=None, alpha=1.0):
    """Elementwise bound of |kernel - epilogue(...)|: one rounding of the result to bf16 (2^-8 |ref|, bf16 outputs only) plus the
    f32 accumulation term K 2^-24 sum|a||b| (abs_acc: |A| |B|^T, plus |bias| where the accumulator takes it as one more term),
    carried through the epilogue's factors as the accumulator's value is: times inv_keep alpha where kept, 0 where dropped or masked."""
    acc_err = K * U24 * abs_acc * (inv_keep if keep is not None else 1.0) * abs(alpha)
    if keep is not None:
        acc_err = acc_err * _keep_t(keep, ref).to(F64)
    if mask_aux is not None:
        acc_err = acc_err * (mask_aux > 0).to(F64)
    return acc_err + (BF16_RN * ref.abs() if out_bf16 else 0.0)
