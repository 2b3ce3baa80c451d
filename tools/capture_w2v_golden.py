"""Capture tests/golden/w2v_tiny.npz: HuggingFace ``Wav2Vec2Model`` (needs transformers; run once, on the CPU) on the tiny
configuration of tests/w2v_ref.py: weights, one short waveform, ``last_hidden_state``.  Data only.

The matrix and convolution entries are drawn from FOUR levels (codes -3, -1, 1, 3 times a per-tensor scale, stored as int8 +
scale), like tools/capture_vit_golden.py, so that the compressed file stays below the largest fixture; the vectors (biases,
norm parameters, the weight-norm gain) are plain f32.

    python tools/capture_w2v_golden.py [out.npz]
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import w2v_ref  # noqa: E402


def main(out_path: str) -> None:
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    cfg = w2v_ref.tiny_config()
    sd = w2v_ref.seeded_weights(cfg, seed=11)
    g = torch.Generator().manual_seed(12)
    arrays = {}
    for k, t in sd.items():
        if t.dim() >= 2 and t.numel() > 1024:                  # GEMM and convolution tensors: four levels
            rms = float(t.pow(2).mean().sqrt())                # keep the seeded scale of this tensor; codes have variance 5
            scale = rms / math.sqrt(5.0)
            codes = (torch.randint(0, 4, t.shape, generator=g) * 2 - 3).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        else:
            arrays["f:" + k] = t.numpy()
    model = Wav2Vec2Model(Wav2Vec2Config(**w2v_ref.config_kwargs(cfg))).eval()
    model.load_state_dict(sd)
    x = 0.5 * torch.randn(1, 2000, generator=g) + 0.1
    with torch.no_grad():
        y = model(x).last_hidden_state
    arrays["input_values"], arrays["last_hidden_state"] = x.numpy(), y.numpy()
    np.savez_compressed(out_path, **arrays)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "w2v_tiny.npz"))
