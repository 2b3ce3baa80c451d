"""Capture tests/golden/bert_tiny.npz and roberta_tiny.npz: HuggingFace ``BertModel`` / ``RobertaModel`` (needs transformers; run
once, on the CPU; ``attn_implementation="eager"``, float32, randomly initialised from a seed) on the tiny configurations of
tests/bert_ref.py: weights, one batch of 3 items x 36 tokens (two 32-key blocks) with its ``attention_mask`` and ``token_type_ids``,
and ``last_hidden_state``.  Data only.

The batch: item 0 has a padded tail (25 valid tokens, pad ids behind them), item 1 a hole in the mask (tokens 10 .. 12), item 2 is
whole.  BERT's token types are 0 then 1 from the middle of each item.  In the RoBERTa batch ids and mask disagree on purpose: item
1 has a pad id under mask 1 (token 5) and its hole covers non-pad ids under mask 0, so positions taken from the mask instead of the
ids show.  No item is empty: HuggingFace's attention back ends differ there.

The matrix entries are drawn from FOUR levels (codes -3, -1, 1, 3 times a per-tensor scale, stored as int8 + scale), as
tools/capture_wavlm_golden.py does; the three embedding tables take 255 levels the same way (every row keeps values of its own), the
vectors are plain f32, so that each file is no larger than deberta_tiny.npz.

    python tools/capture_bert_golden.py [out_dir]
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import bert_ref  # noqa: E402

N, T = 3, 36


def batch(cfg, family: str, g: torch.Generator):
    pad = cfg.pad_token_id
    ids = torch.randint(2, cfg.vocab_size, (N, T), generator=g)
    mask = torch.ones(N, T, dtype=torch.int64)
    mask[0, 25:] = 0
    ids[0, 25:] = pad                                          # a padded tail
    mask[1, 10:13] = 0                                         # a hole, over non-pad ids
    types_ = torch.zeros(N, T, dtype=torch.int64)
    if family == "bert":
        types_[:, T // 2:] = 1
    else:
        ids[1, 5] = pad                                        # a pad id under mask 1
    return ids, mask, types_


def capture(family: str, out_path: str) -> None:
    import transformers
    cfg = bert_ref.tiny_config(family)
    sd = bert_ref.seeded_weights(cfg, family, seed=13)
    g = torch.Generator().manual_seed(14)
    arrays = {}
    for k, t in sd.items():
        if "embeddings" in k and t.dim() == 2:                 # 255 levels
            scale = float(t.abs().max()) / 127.0
            codes = torch.round(t / scale).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        elif t.dim() == 2:                                     # GEMM weights: four levels at the seeded scale (codes have variance 5)
            scale = float(t.pow(2).mean().sqrt()) / math.sqrt(5.0)
            codes = (torch.randint(0, 4, t.shape, generator=g) * 2 - 3).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        else:
            arrays["f:" + k] = t.numpy()
    Config, Model = {"bert": (transformers.BertConfig, transformers.BertModel),
                     "roberta": (transformers.RobertaConfig, transformers.RobertaModel)}[family]
    model = Model(Config(**bert_ref.hf_config_kwargs(cfg))).eval()
    model.load_state_dict(sd)
    ids, mask, types_ = batch(cfg, family, g)
    with torch.no_grad():
        y = model(input_ids=ids, attention_mask=mask, token_type_ids=types_).last_hidden_state
    arrays.update(input_ids=ids.to(torch.int16).numpy(), attention_mask=mask.to(torch.int8).numpy(),
                  token_type_ids=types_.to(torch.int8).numpy(), last_hidden_state=y.numpy())
    np.savez_compressed(out_path, **arrays)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden")
    for family in ("bert", "roberta"):
        capture(family, os.path.join(out_dir, f"{family}_tiny.npz"))
