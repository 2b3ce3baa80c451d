"""Capture tests/golden/vit_tiny.npz: HuggingFace ``ViTModel`` (needs transformers; run once, on the CPU) on the tiny
configuration of tests/vit_ref.py — weights, one input, ``last_hidden_state``.  Data only.

The 1.8 M matrix entries are drawn from FOUR levels (codes -3, -1, 1, 3 times a per-tensor scale, stored as int8 + scale), so
that the compressed file stays below the largest fixture; the vectors (biases, LayerNorm, cls / position) are plain f32.

    python tools/capture_vit_golden.py [out.npz]
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import vit_ref  # noqa: E402


def main(out_path: str) -> None:
    from transformers import ViTConfig, ViTModel
    cfg = vit_ref.tiny_config()
    sd = vit_ref.seeded_weights(cfg, seed=11)
    g = torch.Generator().manual_seed(12)
    arrays = {}
    for k, t in sd.items():
        if t.dim() in (2, 4):                                  # GEMM matrices: four levels
            fan_in = t[0].numel()
            scale = (1.5 if ("q_proj" in k or "k_proj" in k) else 1.0) / math.sqrt(5.0 * fan_in)      # codes have variance 5
            codes = (torch.randint(0, 4, t.shape, generator=g) * 2 - 3).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        else:
            arrays["f:" + k] = t.numpy()
    model = ViTModel(ViTConfig(**vit_ref.config_kwargs(cfg))).eval()
    model.load_state_dict(sd)
    x = torch.rand(1, cfg.num_channels, cfg.image_size, cfg.image_size, generator=g)
    with torch.no_grad():
        y = model(pixel_values=x).last_hidden_state
    arrays["pixel_values"], arrays["last_hidden_state"] = x.numpy(), y.numpy()
    np.savez_compressed(out_path, **arrays)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "vit_tiny.npz"))
