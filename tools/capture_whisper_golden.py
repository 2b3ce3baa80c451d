"""Capture tests/golden/whisper_tiny.npz: HuggingFace ``WhisperFeatureExtractor`` and ``WhisperEncoder`` (needs transformers; run
once, on the CPU) on the tiny configuration of tests/whisper_ref.py (d_model 128, 2 heads, 2 layers, 80 mel bins,
max_source_positions 100: a 2 s window, 100 frames, two key tiles of the attention kernel): weights, one speech-like waveform of
20,000 samples (shorter than the window of 32,000, so the extractor's zero padding is in it), ``input_features`` and
``last_hidden_state``.  Data only.

The matrix and convolution entries are drawn from FOUR levels (codes -3, -1, 1, 3 times a per-tensor scale, stored as int8 + scale),
as tools/capture_w2v_golden.py does; the vectors and ``embed_positions`` are plain f32 and the waveform is int16 over 2^15, exactly.

    python tools/capture_whisper_golden.py [out.npz]
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import whisper_ref  # noqa: E402


def main(out_path: str) -> None:
    from transformers import WhisperConfig, WhisperFeatureExtractor
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    cfg = whisper_ref.tiny_config()
    sd = whisper_ref.seeded_weights(cfg, seed=17)
    g = torch.Generator().manual_seed(18)
    arrays = {}
    for k, t in sd.items():
        if t.dim() >= 2 and k != "embed_positions.weight":     # GEMM and convolution tensors: four levels
            scale = float(t.pow(2).mean().sqrt()) / math.sqrt(5.0)          # keep the seeded scale; the codes have variance 5
            codes = (torch.randint(0, 4, t.shape, generator=g) * 2 - 3).to(torch.int8)
            sd[k] = codes.float() * scale
            arrays["q:" + k], arrays["s:" + k] = codes.numpy(), np.float32(scale)
        else:
            arrays["f:" + k] = t.numpy()
    model = WhisperEncoder(WhisperConfig(**whisper_ref.config_kwargs(cfg))).eval()
    model.load_state_dict(sd)
    codes = np.round(32768.0 * whisper_ref.speech_like(20000, seed=19)).clip(-32767, 32767).astype(np.int16)
    wave = codes.astype(np.float32) / 32768.0
    fe = WhisperFeatureExtractor(feature_size=cfg.num_mel_bins, chunk_length=cfg.max_source_positions * 320 // 16000)
    feats = fe(wave, sampling_rate=16000, return_tensors="pt").input_features
    with torch.no_grad():
        y = model(feats).last_hidden_state
    arrays["wave_q15"], arrays["input_features"], arrays["last_hidden_state"] = codes[None], feats.numpy(), y.numpy()
    np.savez_compressed(out_path, **arrays)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "whisper_tiny.npz"))
