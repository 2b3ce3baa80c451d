"""Capture tests/golden/w2v_ln_tiny.npz: HuggingFace ``Wav2Vec2Model`` of the layer-norm family (``feat_extract_norm="layer"``,
``conv_bias=True``, ``do_stable_layer_norm=True``; needs transformers; run once, on the CPU) on the ``ln_tiny`` configuration of
tests/w2v_ln_ref.py: weights, one 2000-sample waveform, ``last_hidden_state``.  Data only.

The four-level int8 coding of tools/capture_w2v_golden.py: the matrix and convolution entries are codes -3, -1, 1, 3 times a
per-tensor scale (int8 + scale).  The vectors (biases, norm parameters, the weight-norm gain) are f16 here, not f32: the family has
nine more of them, and the file is to stay no larger than w2v_tiny.npz.

    python tools/capture_w2v_ln_golden.py [out.npz]
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import w2v_ln_ref  # noqa: E402


def main(out_path: str) -> None:
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    cfg = w2v_ln_ref.ln_tiny()
    sd = w2v_ln_ref.seeded_weights(cfg, seed=13)
    g = torch.Generator().manual_seed(14)
    arrays = {}
    for k, t in sd.items():
        if t.dim() >= 2 and t.numel() > 1024:                  # GEMM and convolution tensors: four levels
            rms = float(t.pow(2).mean().sqrt())                # keep the seeded scale of this tensor; codes have variance 5
            scale = rms / math.sqrt(5.0)
            codes = (torch.randint(0, 4, t.shape, generator=g) * 2 - 3).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        else:                                                  # vectors: rounded to f16 and stored so (the model gets the rounded values)
            sd[k] = t.half().float()
            arrays["h:" + k] = t.half().numpy()
    model = Wav2Vec2Model(Wav2Vec2Config(**w2v_ln_ref.config_kwargs(cfg))).eval()
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    x = 0.5 * torch.randn(1, 2000, generator=g) + 0.1
    with torch.no_grad():
        y = model(x).last_hidden_state
    arrays["input_values"], arrays["last_hidden_state"] = x.numpy(), y.numpy()
    np.savez_compressed(out_path, **arrays)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "w2v_ln_tiny.npz"))
