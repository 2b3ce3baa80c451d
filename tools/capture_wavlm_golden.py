"""Capture tests/golden/wavlm_tiny.npz: HuggingFace ``WavLMModel`` (needs transformers; run once, on the CPU) on the tiny
configuration of tests/wavlm_ref.py (tests/w2v_ref.py's tiny sizes with num_buckets 320 / max_bucket_distance 800): weights, one
waveform of 2000 samples (99 frames: two key tiles of the attention kernel, distances past the 80 exact buckets),
``last_hidden_state``.  Data only.

The matrix and convolution entries are drawn from FOUR levels (codes -3, -1, 1, 3 times a per-tensor scale, stored as int8 + scale),
as tools/capture_w2v_golden.py does, ``gru_rel_pos_linear`` included; ``rel_attn_embed`` takes 255 levels the same way (every
bucket keeps its own value), the vectors are plain f32 and the waveform is int8 sixty-fourths, exactly, so that the file is no larger than
w2v_tiny.npz.  ``wavlm_ref.seeded_weights`` seeds the gate's parameters and ``rel_attn_embed`` away from their initial values, so
that the gate is not near constant.

    python tools/capture_wavlm_golden.py [out.npz]
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import wavlm_ref  # noqa: E402


def main(out_path: str) -> None:
    from transformers import WavLMConfig, WavLMModel
    cfg = wavlm_ref.tiny_config()
    sd = wavlm_ref.seeded_weights(cfg, seed=13)
    g = torch.Generator().manual_seed(14)
    arrays = {}
    for k, t in sd.items():
        if k.endswith("rel_attn_embed.weight"):                # 255 levels: every bucket keeps a value of its own per head
            scale = float(t.abs().max()) / 127.0
            codes = torch.round(t / scale).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        elif t.dim() >= 2 and (t.numel() > 2048 or "gru_rel_pos_linear" in k):      # GEMM, convolution and gate tensors: four levels
            rms = float(t.pow(2).mean().sqrt())                # keep the seeded scale of this tensor; codes have variance 5
            scale = rms / math.sqrt(5.0)
            codes = (torch.randint(0, 4, t.shape, generator=g) * 2 - 3).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        else:
            arrays["f:" + k] = t.numpy()
    model = WavLMModel(WavLMConfig(**wavlm_ref.config_kwargs(cfg))).eval()
    model.load_state_dict(sd)
    codes = torch.round(64.0 * (0.5 * torch.randn(1, 2000, generator=g) + 0.1)).clamp(-127, 127).to(torch.int8)
    x = codes.float() / 64.0                                                     # stored as int8 sixty-fourths, exactly
    with torch.no_grad():
        y = model(x).last_hidden_state
    arrays["input_values_q64"], arrays["last_hidden_state"] = codes.numpy(), y.numpy()
    np.savez_compressed(out_path, **arrays)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "wavlm_tiny.npz"))
