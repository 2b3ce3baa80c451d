"""CPU: the layer-norm family of Wav2Vec2 (``feat_extract_norm="layer"``, ``conv_bias=True``, ``do_stable_layer_norm=True``).  The
restatement tests/w2v_ln_ref.py against HuggingFace through tests/golden/w2v_ln_tiny.npz, with three mutants that must miss; the
``state_dict`` surface of ``NativeWav2Vec2`` on the family, the family switch and what stays refused on it; and the facts the GPU
tests' bounds rely on.

RESTATE_TOL = 2e-5 is tests/test_w2v_cpu.py's bound for a restatement against its reference (float32 HuggingFace against float64)."""
import os

import numpy as np
import pytest
import torch

import w2v_ln_ref
import w2v_ref
from helpers import l2_rel

RESTATE_TOL = 2e-5
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "w2v_ln_tiny.npz")
LN_SWITCHES = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)


def _native(cfg, **kw):
    from mmfusion.wav2vec2 import NativeWav2Vec2
    return NativeWav2Vec2(**{**w2v_ln_ref.config_kwargs(cfg), **kw})


def golden():
    """-> (cfg, state dict, waveform (1, 2000), HuggingFace's last_hidden_state); "q:" four-level int8 codes times the scale "s:",
    "h:" vectors stored as f16"""
    z = np.load(GOLDEN)
    sd = {}
    for name in z.files:
        tag, _, key = name.partition(":")
        if tag == "q":
            sd[key] = torch.from_numpy(z[name].astype(np.float32)) * float(z["s:" + key])
        elif tag == "h":
            sd[key] = torch.from_numpy(z[name].astype(np.float32))
    cfg = w2v_ln_ref.ln_tiny()
    sd = {k: sd[k] for k in w2v_ln_ref.hf_keys(cfg)}
    return cfg, sd, torch.from_numpy(z["input_values"]), torch.from_numpy(z["last_hidden_state"])


# ---- the restatement -----------------------------------------------------------------------------------------
def test_restatement_matches_the_captured_vector_and_three_mutants_miss():
    cfg, sd, x, want = golden()
    got = w2v_ln_ref.w2v_forward(sd, x, cfg)
    err = l2_rel(got, want)
    print(f"restatement vs captured HuggingFace output: {err:.3e} (bound {RESTATE_TOL})")
    assert got.shape == want.shape == (1, 99, 256) and err <= RESTATE_TOL
    for what, kw in (("the inner layers' LayerNorm dropped", dict(inner_norm=False)), ("the conv biases dropped", dict(conv_bias=False)),
                     ("the post-LN arrangement on the same weights", dict(post_ln=True))):
        miss = l2_rel(w2v_ln_ref.w2v_forward(sd, x, cfg, **kw), want)
        print(f"    {what}: {miss:.3e}")
        assert miss > 1000 * RESTATE_TOL, what


def test_fixture_is_no_larger_than_the_base_familys():
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(GOLDEN_DIR, "w2v_tiny.npz"))


def test_restatement_matches_live_huggingface():
    transformers = pytest.importorskip("transformers")
    cfg = w2v_ln_ref.ln_tiny()
    sd = w2v_ln_ref.seeded_weights(cfg, seed=5)
    hf = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**w2v_ln_ref.config_kwargs(cfg))).eval()
    assert list(hf.state_dict().keys()) == list(sd.keys())
    hf.load_state_dict(sd)
    x = 0.5 * torch.randn(2, 4000, generator=torch.Generator().manual_seed(6)) + 0.05
    with torch.no_grad():
        want = hf(x).last_hidden_state
    err = l2_rel(w2v_ln_ref.w2v_forward(sd, x, cfg), want)
    print(f"restatement vs live HuggingFace (ln_tiny, 4000 samples -> {tuple(want.shape)}): {err:.3e} (bound {RESTATE_TOL})")
    assert err <= RESTATE_TOL


def test_bf16_storage_switch_rounds_and_stays_close():
    cfg, sd, x, _ = golden()
    exact = w2v_ln_ref.w2v_forward(sd, x, cfg)
    stored = w2v_ln_ref.w2v_forward(sd, x, cfg, bf16_storage=True)
    err = l2_rel(stored, exact)
    print(f"bf16-storage restatement vs fp64: {err:.3e}")
    assert torch.equal(stored, stored.to(torch.bfloat16).to(stored.dtype))            # the last store is a bf16 store
    assert 1e-4 < err < 2e-2


# ---- NativeWav2Vec2: the state_dict surface -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["ln_tiny", "ln_wide"])
def test_state_dict_is_huggingfaces_key_for_key(which):
    cfg = getattr(w2v_ln_ref, which)()
    m = _native(cfg)
    sd = m.state_dict()
    for legacy in (False, True):
        want = w2v_ln_ref.hf_keys(cfg, legacy_weight_norm=legacy)
        have = m.hf_state_dict(legacy_weight_norm=legacy)
        assert list(have.keys()) == list(want.keys())
        assert {k: tuple(v.shape) for k, v in have.items()} == want
    fe = "feature_extractor.conv_layers."
    for i in range(len(cfg.conv_dim)):
        assert sd[f"{fe}{i}.conv.bias"].shape == sd[f"{fe}{i}.layer_norm.weight"].shape == sd[f"{fe}{i}.layer_norm.bias"].shape == (cfg.conv_dim[i],)
    assert all(not p.requires_grad for p in m.parameters())
    c = m.config
    assert (c.feat_extract_norm, c.conv_bias, c.do_stable_layer_norm) == ("layer", True, True)
    transformers = pytest.importorskip("transformers")
    kw = {k: v for k, v in vars(cfg).items() if k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "conv_dim",
                                                      "conv_kernel", "conv_stride", "num_conv_pos_embeddings", "num_conv_pos_embedding_groups")}
    with torch.device("meta"):
        hf = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**kw, **LN_SWITCHES))
    assert [(k, tuple(v.shape)) for k, v in hf.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]


@pytest.mark.parametrize("legacy", [False, True])
def test_round_trip_is_bit_exact_in_both_weight_norm_spellings(legacy):
    cfg = w2v_ln_ref.ln_tiny()
    sd = w2v_ln_ref.seeded_weights(cfg, seed=7, legacy_weight_norm=legacy)
    m = _native(cfg)
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.hf_state_dict(legacy_weight_norm=legacy)
    assert list(back.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    assert torch.equal(m.conv1_b, sd["feature_extractor.conv_layers.1.conv.bias"])
    assert torch.equal(m.conv2_ln_w, sd["feature_extractor.conv_layers.2.layer_norm.weight"])
    # a base-family checkpoint does not fill the family: its seven new keys are missing
    res = m.load_state_dict(w2v_ref.seeded_weights(w2v_ref.tiny_config(), seed=7), strict=False)
    assert len(res.missing_keys) == 7 and all(".conv.bias" in k or ".layer_norm." in k for k in res.missing_keys)


def test_the_base_familys_table_is_unchanged():
    from mmfusion.wav2vec2 import FAMILIES, NativeWav2Vec2
    cfg = w2v_ref.tiny_config()
    m = NativeWav2Vec2(**w2v_ref.config_kwargs(cfg))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == w2v_ref.hf_keys(cfg)
    assert not hasattr(m, "conv0_b") and not hasattr(m, "conv1_ln_w")
    assert [n for n, _, _ in m._ws_table(4000)][-2:] == ["stats", "partial"]
    assert set(FAMILIES) == {"base", "large", "large-lv60"}
    assert list(NativeWav2Vec2(**FAMILIES["base"]).state_dict()) == list(NativeWav2Vec2().state_dict())
    assert FAMILIES["large"] == dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)
    assert FAMILIES["large-lv60"] == dict(FAMILIES["large"], **LN_SWITCHES)


# ---- the family switch -----------------------------------------------------------------------------------------
def test_large_lv60_constructs_with_the_real_clip_length():
    from mmfusion.wav2vec2 import FAMILIES, NativeWav2Vec2
    m = NativeWav2Vec2(**FAMILIES["large-lv60"])
    c = m.config
    assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size) == (1024, 24, 16, 4096)
    assert m.frames(160000) == 499 and m.head_dim == 64 and m.pos_cg == 64
    assert "stats" not in [n for n, _, _ in m._ws_table(160000)]                        # layer 0 is one pass
    assert m.workspace_bytes_per_clip(160000) == m._bytes_per_item(m._ws_table(160000))


@pytest.mark.parametrize("on", [("feat_extract_norm",), ("conv_bias",), ("do_stable_layer_norm",), ("feat_extract_norm", "conv_bias"),
                                ("feat_extract_norm", "do_stable_layer_norm"), ("conv_bias", "do_stable_layer_norm")])
def test_mixed_settings_stay_refused(on):
    with pytest.raises(ValueError, match="NativeWav2Vec2"):
        _native(w2v_ref.tiny_config(), **{k: LN_SWITCHES[k] for k in on})


@pytest.mark.parametrize("kw", [dict(conv_dim=(96, 256, 256)),                        # 96 / 8 = 12 lanes: no power of two
                                dict(conv_dim=(256, 768, 256)),                       # 96 lanes
                                dict(feat_extract_norm="batch")])
def test_channel_counts_outside_the_kernels_are_refused(kw):
    with pytest.raises(ValueError, match="NativeWav2Vec2"):
        _native(w2v_ln_ref.ln_tiny(), **kw)
    if "conv_dim" in kw:
        _native(w2v_ref.tiny_config(), **kw)                                              # (the base family takes them)


# ---- what stays refused on the family ----------------------------------------------------------------------------
def test_fine_tune_and_regulariser_refusals():
    m = _native(w2v_ln_ref.ln_tiny())
    L = m.config.num_hidden_layers
    with pytest.raises(ValueError, match="feature encoder does not train"):
        m.set_trainable_layers(L, front=True, feature_encoder=True)
    assert m.trainable_layers == 0 and not any(p.requires_grad for p in m.parameters())
    for name, v in (("hidden_dropout", 0.1), ("attention_dropout", 0.1), ("activation_dropout", 0.1), ("feat_proj_dropout", 0.1),
                    ("layerdrop", 0.1), ("mask_time_prob", 0.05)):
        with pytest.raises(ValueError, match="layer-norm family"):
            m.set_regularisation(**{name: v})
        with pytest.raises(ValueError, match="layer-norm family"):
            _native(w2v_ln_ref.ln_tiny(), **{name: v})
    m.set_regularisation(hidden_dropout=0.0, mask_time_prob=0.0, mask_time_length=10)     # all off is what it has
    assert m.config.hidden_dropout == 0.0 and not m.config.apply_spec_augment
    with pytest.raises(ValueError, match="with all 2 layers only"):
        m.set_trainable_layers(1, front=True)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        m(torch.zeros(1, 4000), attention_mask=torch.ones(1, 4000))
    with pytest.raises(RuntimeError, match="GPU only"):
        m(torch.zeros(1, 4000))


def test_trainable_names_of_the_family():
    m = _native(w2v_ln_ref.ln_tiny())
    front = ["fp_ln_w", "fp_ln_b", "fp_w", "fp_b", "pos_b", "pos_g", "pos_v"]
    top = ["enc_ln_w", "enc_ln_b"]
    live = lambda: sorted(n for n, p in m.named_parameters() if p.requires_grad)
    m.set_trainable_layers(1)
    assert live() == sorted(m._layer_params(1) + top)                  # encoder.layer_norm sits on top: it trains from k = 1 on
    m.set_trainable_layers(2)
    assert live() == sorted(m._layer_params(0) + m._layer_params(1) + top)
    m.set_trainable_layers(2, front=True)
    assert live() == sorted(front + m._layer_params(0) + m._layer_params(1) + top) and m.trainable_front
    m.set_trainable_layers(0)
    assert live() == []


def test_audio_encoder_refuses_regularisers_on_the_family():
    import config as cfgmod
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.audio_hidden_size = 256, 768
    cfg.audio_backbone = "native"
    cfg.audio_backbone_kwargs = {k: v for k, v in w2v_ln_ref.config_kwargs(w2v_ln_ref.ln_768()).items() if k != "hidden_size"}
    cfg.audio_backbone_trainable_layers = 1
    enc = AudioEncoder(cfg)
    assert enc.model.config.do_stable_layer_norm and enc.model.trainable_layers == 1 and enc.hidden_size == 768
    cfg.audio_backbone_regularisation = True
    with pytest.raises(ValueError, match="layer-norm family"):
        AudioEncoder(cfg)
    cfg.audio_backbone_regularisation, cfg.audio_backbone_trainable_layers = 0, "full"
    with pytest.raises(ValueError, match="feature encoder does not train"):
        AudioEncoder(cfg)


def test_kernel_wrappers_refuse_cpu_tensors():
    from mmfusion import lib
    x, v = torch.zeros(1, 8, 64, dtype=torch.bfloat16), torch.zeros(64)
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.w2v_ln_gelu_window(x, v, v, torch.zeros(1, 4, 128, dtype=torch.bfloat16), 1, 8, 64, 2, 2, 1e-5)
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.w2v_conv0_ln_gelu(torch.zeros(1, 400), torch.zeros(64, 1, 10), v, v, v, x, 10, 5, 2, 2, 1e-5)


# ---- facts the GPU tests' bounds rely on --------------------------------------------------------------------------------
def _grads(sd, x, cfg, dout, keys, bf16_storage):
    leaves = {k: v.double().clone().requires_grad_(k in keys) for k, v in sd.items()}
    out = w2v_ln_ref.w2v_forward(leaves, x.double(), cfg, dtype=torch.float64, bf16_storage=bf16_storage)
    return dict(zip(keys, torch.autograd.grad(out, [leaves[k] for k in keys], dout)))


def test_rule_b_is_not_degenerate_for_any_tensor_the_backward_touches():
    """Rule (b) of tests/test_w2v_ln_finetune_gpu.py, ||got - exact|| <= 2 ||stored - exact||, needs the bf16-storage gradient to
    differ from the exact one: it does for every tensor the family's backward forms (both layers, ``encoder.layer_norm`` on top of
    them, the feature projection and the positional convolution; printed: ||stored - exact|| / ||exact|| per tensor).  The key bias is
    the one tensor held to something else: its exact gradient is zero."""
    cfg = w2v_ln_ref.ln_tiny()
    sd = w2v_ln_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 1500, generator=g)
    keys = [k for k in sd if k.startswith(("feature_projection.", "encoder."))]
    T = w2v_ln_ref.w2v_forward(sd, x.double(), cfg).shape[1]
    dout = torch.randn(2, T, cfg.hidden_size, generator=g, dtype=torch.float64)
    exact, stored = _grads(sd, x, cfg, dout, keys, False), _grads(sd, x, cfg, dout, keys, True)
    assert len(keys) == 9 + 16 * cfg.num_hidden_layers
    for k in keys:
        if k.endswith("k_proj.bias"):
            q = float(exact[k.replace("k_proj", "q_proj")].norm())
            print(f"{k}: ||exact|| = {float(exact[k].norm()):.3e} (q_proj.bias: {q:.3e})")
            assert float(exact[k].norm()) <= 1e-10 * q
            continue
        rel = float((stored[k] - exact[k]).norm() / exact[k].norm())
        print(f"{k}: ||stored - exact|| / ||exact|| = {rel:.3e}")
        assert 1e-4 < rel < 0.5, k
