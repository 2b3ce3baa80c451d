"""Capture tests/golden/deberta_tiny.npz: HuggingFace ``DebertaV2Model`` (needs transformers; run once, on the CPU) on the tiny
configuration of tests/deberta_ref.py: weights, ids (2, 70) with the second item padded from token 50, the attention mask,
``last_hidden_state``, the key list, and HuggingFace's own ``build_relative_position`` tables for three geometries.  Data only.

The matrix entries are drawn from FOUR levels (codes -3, -1, 1, 3 times a per-tensor scale, stored as int8 + scale), like
tools/capture_w2v_golden.py, so that the compressed file stays below the largest fixture; the vectors are plain f32.

    python tools/capture_deberta_golden.py [out.npz]
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import deberta_ref  # noqa: E402

TABLES = ((70, 8, 32), (512, 256, 512), (530, 256, 512))       # (T, bucket_size, max_position)


def main(out_path: str) -> None:
    from transformers import DebertaV2Config, DebertaV2Model
    from transformers.models.deberta_v2.modeling_deberta_v2 import build_relative_position
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=11)
    g = torch.Generator().manual_seed(12)
    arrays = {}
    for k, t in sd.items():
        if t.dim() >= 2 and t.numel() > 1024:                  # matrices and the two embedding tables: four levels
            rms = float(t.pow(2).mean().sqrt())                # keep the seeded scale of this tensor; codes have variance 5
            scale = rms / math.sqrt(5.0)
            codes = (torch.randint(0, 4, t.shape, generator=g) * 2 - 3).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        else:
            arrays["f:" + k] = t.numpy()
    model = DebertaV2Model(DebertaV2Config(**deberta_ref.hf_config_kwargs(cfg))).eval()
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    ids = torch.randint(1, cfg.vocab_size, (2, 70), generator=g)
    mask = torch.ones(2, 70, dtype=torch.int64)
    ids[1, 50:], mask[1, 50:] = 0, 0
    with torch.no_grad():
        y = model(input_ids=ids, attention_mask=mask).last_hidden_state
    arrays["input_ids"], arrays["attention_mask"], arrays["last_hidden_state"] = ids.numpy(), mask.numpy(), y.numpy()
    arrays["keys"] = np.array(list(model.state_dict().keys()))
    for T, S, P in TABLES:
        x = torch.zeros(1, T, 1)
        arrays[f"relpos:{T}:{S}:{P}"] = build_relative_position(x, x, bucket_size=S, max_position=P)[0].numpy().astype(np.int16)
    np.savez_compressed(out_path, **arrays)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "deberta_tiny.npz"))
