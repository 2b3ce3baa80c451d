"""CPU: the Wav2Vec2 restatement tests/w2v_ref.py against HuggingFace (live and through tests/golden/w2v_tiny.npz), and the
``state_dict`` surface, refusals and checkpoint loading of ``mmfusion.wav2vec2.NativeWav2Vec2`` (which needs no GPU to be
built, saved and loaded).

RESTATE_TOL = 2e-5 is the project's bound for a restatement against its reference (float32 HuggingFace against float64)."""
import os

import numpy as np
import pytest
import torch

import w2v_ref
from helpers import l2_rel

RESTATE_TOL = 2e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w2v_tiny.npz")
LARGEST_OTHER_FIXTURE = 746560


def _native(cfg, **kw):
    from mmfusion.wav2vec2 import NativeWav2Vec2
    return NativeWav2Vec2(**{**w2v_ref.config_kwargs(cfg), **kw})


def _golden():
    z = np.load(GOLDEN)
    sd = {}
    for name in z.files:
        tag, _, key = name.partition(":")
        if tag == "q":
            sd[key] = torch.from_numpy(z[name].astype(np.float32)) * float(z["s:" + key])
        elif tag == "f":
            sd[key] = torch.from_numpy(z[name])
    cfg = w2v_ref.tiny_config()
    sd = {k: sd[k] for k in w2v_ref.hf_keys(cfg)}
    return cfg, sd, torch.from_numpy(z["input_values"]), torch.from_numpy(z["last_hidden_state"])


# ---- the restatement -----------------------------------------------------------------------------------------
def test_restatement_matches_the_captured_vector_and_both_ablations_matter():
    cfg, sd, x, want = _golden()
    got = w2v_ref.w2v_forward(sd, x, cfg)
    err = l2_rel(got, want)
    no_q = l2_rel(w2v_ref.w2v_forward(sd, x, cfg, zero_q=True), want)
    no_gn = l2_rel(w2v_ref.w2v_forward(sd, x, cfg, group_norm=False), want)
    print(f"restatement vs captured HuggingFace output: {err:.3e} (bound {RESTATE_TOL}); q = 0: {no_q:.3e}; no GroupNorm: {no_gn:.3e}")
    assert got.shape == want.shape and err <= RESTATE_TOL
    assert no_q > 100 * RESTATE_TOL and no_gn > 100 * RESTATE_TOL


def test_fixture_is_no_larger_than_the_largest_beside_it():
    assert os.path.getsize(GOLDEN) <= LARGEST_OTHER_FIXTURE


@pytest.mark.parametrize("which,L", [("tiny", 4000), ("base", 16000)])
def test_restatement_matches_live_huggingface(which, L):
    transformers = pytest.importorskip("transformers")
    cfg = w2v_ref.tiny_config() if which == "tiny" else w2v_ref.base_config()
    sd = w2v_ref.seeded_weights(cfg, seed=5)
    hf = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**w2v_ref.config_kwargs(cfg))).eval()
    assert list(hf.state_dict().keys()) == list(sd.keys())
    hf.load_state_dict(sd)
    x = 0.5 * torch.randn(2, L, generator=torch.Generator().manual_seed(6)) + 0.05
    with torch.no_grad():
        want = hf(x).last_hidden_state
    got = w2v_ref.w2v_forward(sd, x, cfg)
    err = l2_rel(got, want)
    print(f"restatement vs live HuggingFace ({which}, {L} samples -> {tuple(want.shape)}): {err:.3e} (bound {RESTATE_TOL})")
    assert got.shape == want.shape and err <= RESTATE_TOL


def test_bf16_storage_switch_rounds_and_stays_close():
    cfg, sd, x, _ = _golden()
    exact = w2v_ref.w2v_forward(sd, x, cfg)
    stored = w2v_ref.w2v_forward(sd, x, cfg, bf16_storage=True)
    err = l2_rel(stored, exact)
    print(f"bf16-storage restatement vs fp64: {err:.3e}")
    assert torch.equal(stored, stored.to(torch.bfloat16).to(stored.dtype))            # the last store is a bf16 store
    assert 1e-4 < err < 2e-2


# ---- NativeWav2Vec2: the state_dict surface -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "base"])
def test_state_dict_is_huggingfaces_key_for_key(which):
    cfg = w2v_ref.tiny_config() if which == "tiny" else w2v_ref.base_config()
    m = _native(cfg)
    sd = m.state_dict()
    want = w2v_ref.hf_keys(cfg)
    assert list(sd.keys()) == list(want.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    if which == "base":
        assert len(sd) == 211
        from mmfusion.wav2vec2 import NativeWav2Vec2
        assert list(NativeWav2Vec2().state_dict().keys()) == list(want.keys())         # the defaults ARE wav2vec2-base
    assert all(not p.requires_grad for p in m.parameters())
    assert m.config.model_type == "wav2vec2" and m.config.hidden_size == cfg.hidden_size
    transformers = pytest.importorskip("transformers")
    hf = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**w2v_ref.config_kwargs(cfg)))
    assert [(k, tuple(v.shape)) for k, v in hf.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]


@pytest.mark.parametrize("legacy", [False, True])
def test_round_trip_is_bit_exact_in_both_weight_norm_spellings(legacy):
    cfg = w2v_ref.tiny_config()
    sd = w2v_ref.seeded_weights(cfg, seed=7, legacy_weight_norm=legacy)
    m = _native(cfg)
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.hf_state_dict(legacy_weight_norm=legacy)
    assert list(back.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    other = m.hf_state_dict(legacy_weight_norm=not legacy)
    assert (w2v_ref.WN_OLD[0] in other) == (not legacy) and len(other) == len(sd)
    # the fused q/k/v rows and the (C_out, k, C_in) conv storage hold what the kernels read
    d = cfg.hidden_size
    assert torch.equal(m.l0_qkv_w[:d], sd["encoder.layers.0.attention.q_proj.weight"])
    assert torch.equal(m.l0_qkv_w[d:2 * d], sd["encoder.layers.0.attention.k_proj.weight"])
    assert m.conv1_w.is_contiguous() and torch.equal(m.conv1_w, sd["feature_extractor.conv_layers.1.conv.weight"].permute(0, 2, 1))


def test_strict_loading_reports_what_is_wrong():
    cfg = w2v_ref.tiny_config()
    sd = w2v_ref.seeded_weights(cfg, seed=8)
    m = _native(cfg)
    bad = dict(sd)
    bad["encoder.layers.9.layer_norm.weight"] = torch.zeros(3)
    del bad["encoder.layer_norm.bias"]
    bad["feature_extractor.conv_layers.1.conv.weight"] = torch.zeros(256, 256, 2)
    with pytest.raises(RuntimeError) as e:
        m.load_state_dict(bad)
    msg = str(e.value)
    assert "encoder.layers.9.layer_norm.weight" in msg and "encoder.layer_norm.bias" in msg and "size mismatch" in msg
    res = m.load_state_dict({k: v for k, v in sd.items() if k != "masked_spec_embed"}, strict=False)
    assert res.missing_keys == ["masked_spec_embed"]


@pytest.mark.parametrize("legacy", [False, True])
def test_load_checkpoint_under_the_audio_encoder_prefix(tmp_path, legacy):
    import config as cfgmod
    from mmfusion.train import load_checkpoint
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.audio_hidden_size = 256, 256
    cfg.audio_backbone = "native"
    wcfg = w2v_ref.tiny_config()
    cfg.audio_backbone_kwargs = {k: v for k, v in w2v_ref.config_kwargs(wcfg).items() if k != "hidden_size"}

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.audio_encoder = AudioEncoder(cfg)

    torch.manual_seed(0)
    holder = Holder()
    assert holder.audio_encoder.hidden_size == 256
    wsd = w2v_ref.seeded_weights(wcfg, seed=9, legacy_weight_norm=legacy)
    full = {k: v.clone() for k, v in holder.state_dict().items() if not k.startswith("audio_encoder.model.")}
    full.update({"audio_encoder.model." + k: v for k, v in wsd.items()})
    path = str(tmp_path / "ckpt.pth")
    torch.save({"model_state_dict": full, "epoch": 3}, path)
    ckpt = load_checkpoint(path, holder)
    assert ckpt["epoch"] == 3
    back = holder.audio_encoder.model.hf_state_dict(legacy_weight_norm=legacy)
    for k in wsd:
        assert torch.equal(back[k], wsd[k]), k


# ---- NativeWav2Vec2: refusals --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(feat_extract_norm="layer"), dict(do_stable_layer_norm=True), dict(conv_bias=True),
    dict(num_attention_heads=8),                                        # head_dim 32
    dict(hidden_size=384, num_attention_heads=6),                       # not a LayerNorm width
    dict(conv_dim=(256, 256, 320)),                                     # conv_dim[-1] not a LayerNorm width
    dict(in_channels=2),
    dict(conv_dim=(24, 256, 256)),                                      # C_in * kernel = 72
    dict(conv_kernel=(10, 2, 2), conv_stride=(5, 3, 2)),                # kernel < stride
    dict(conv_dim=(256, 260, 256), conv_kernel=(10, 8, 8)),             # a channel count that is no multiple of 8
    dict(intermediate_size=516),
    dict(num_conv_pos_embedding_groups=64),                             # group width 4
])
def test_configurations_outside_the_base_family_are_refused(kw):
    with pytest.raises(ValueError, match="NativeWav2Vec2"):
        _native(w2v_ref.tiny_config(), **kw)


def test_forward_refusals_need_no_gpu():
    m = _native(w2v_ref.tiny_config())
    x = torch.zeros(1, 4000)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        m(x, attention_mask=torch.ones(1, 4000))
    with pytest.raises(RuntimeError, match="GPU only"):
        m(x)
    from mmfusion.wav2vec2 import NativeWav2Vec2, feat_lengths
    assert NativeWav2Vec2().frames(160000) == 499 and NativeWav2Vec2().frames(16000) == 49
    assert feat_lengths(4000, (10, 3, 2), (5, 2, 2)) == [799, 399, 199] and m.frames(20) == 0


def test_stats_slot_count_is_the_headers():
    import re
    from mmfusion import lib
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmfusion.h")
    m = re.search(r"#define\s+MMF_W2V_STATS_SLOTS\s+(\d+)", open(header).read())
    assert m and int(m.group(1)) == lib.W2V_STATS_SLOTS


def test_a_wide_last_conv_layer_fits_the_workspace():
    """conv_dim = (256, 1024) with kernels (10, 2): the feature LayerNorm's output (T x 1024) is larger than any window form"""
    m = _native(w2v_ref.tiny_config(), conv_dim=(256, 1024), conv_kernel=(10, 2), conv_stride=(5, 2))
    win, _ = m._conv_elements(4000)
    assert win >= m.frames(4000) * 1024


def test_kernel_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    from mmfusion import lib
    x = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.w2v_gelu_window(x, torch.zeros(1, 4, 128, dtype=torch.bfloat16), 1, 8, 64, 2, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.w2v_posconv(x, x, torch.zeros(64), x, 1, 8, 64, 4, 2)
