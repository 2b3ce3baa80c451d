"""CPU: the WavLM restatement tests/wavlm_ref.py against HuggingFace (through tests/golden/wavlm_tiny.npz, and live where
transformers imports), its mutants, the relative-position buckets, and the ``state_dict`` surface, refusals and ``AudioEncoder``
switch of ``mmfusion.wavlm.NativeWavLM`` (which needs no GPU to be built, saved and loaded).

RESTATE_TOL = 2e-5 is the project's bound for a restatement against its reference (float32 HuggingFace against float64)."""
import os

import pytest
import torch

import wavlm_ref
from helpers import l2_rel

RESTATE_TOL = 2e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavlm_tiny.npz")
W2V_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "w2v_tiny.npz")


def _native(cfg, **kw):
    from mmfusion.wavlm import NativeWavLM
    return NativeWavLM(**{**wavlm_ref.config_kwargs(cfg), **kw})


@pytest.fixture(scope="module")
def golden():
    sd, x, want = wavlm_ref.load_golden(GOLDEN)
    cfg = wavlm_ref.tiny_config()
    return cfg, {k: sd[k] for k in wavlm_ref.hf_keys(cfg)}, x, want


# ---- the restatement -----------------------------------------------------------------------------------------
def test_restatement_matches_the_captured_vector(golden):
    cfg, sd, x, want = golden
    got = wavlm_ref.wavlm_forward(sd, x, cfg)
    err = l2_rel(got, want)
    print(f"restatement vs captured HuggingFace output {tuple(want.shape)}: {err:.3e} (bound {RESTATE_TOL})")
    assert x.shape == (1, 2000) and want.shape == (1, 99, cfg.hidden_size)
    assert got.shape == want.shape and err <= RESTATE_TOL


@pytest.mark.parametrize("mutant", wavlm_ref.MUTANTS)
def test_every_mutant_leaves_the_bound(golden, mutant):
    """gate fixed at 1, bias indexed by i - j, gate of the neighbouring head, gate from q, table index shifted by one"""
    cfg, sd, x, want = golden
    err = l2_rel(wavlm_ref.wavlm_forward(sd, x, cfg, mutant=mutant), want)
    print(f"mutant {mutant}: {err:.3e} against the captured output (bound {RESTATE_TOL})")
    assert err > 100 * RESTATE_TOL


def test_captured_gate_is_not_near_constant(golden):
    cfg, sd, x, _ = golden
    H, dh = cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads
    a = "encoder.layers.1.attention."
    rows = torch.randn(1, 50, H, dh, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    g = wavlm_ref.gate_ref(rows, sd[a + "gru_rel_pos_linear.weight"].double(), sd[a + "gru_rel_pos_linear.bias"].double(),
                           sd[a + "gru_rel_pos_const"].double().reshape(H))
    assert g.shape == (1, H, 50) and float(g.max() - g.min()) > 0.5


def test_fixture_is_data_only_and_no_larger_than_w2v_tiny():
    import numpy as np
    assert os.path.getsize(GOLDEN) <= os.path.getsize(W2V_GOLDEN)
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[n].dtype.kind in "fi" for n in z.files)


def test_restatement_matches_live_huggingface():
    transformers = pytest.importorskip("transformers")
    cfg = wavlm_ref.tiny_config()
    sd = wavlm_ref.seeded_weights(cfg, seed=5)
    hf = transformers.WavLMModel(transformers.WavLMConfig(**wavlm_ref.config_kwargs(cfg))).eval()
    assert list(hf.state_dict().keys()) == list(sd.keys())
    hf.load_state_dict(sd)
    x = 0.5 * torch.randn(2, 4000, generator=torch.Generator().manual_seed(6)) + 0.05
    with torch.no_grad():
        want = hf(x).last_hidden_state
    got = wavlm_ref.wavlm_forward(sd, x, cfg)
    err = l2_rel(got, want)
    print(f"restatement vs live HuggingFace (tiny, 4000 samples -> {tuple(want.shape)}): {err:.3e} (bound {RESTATE_TOL})")
    assert got.shape == want.shape and err <= RESTATE_TOL


def test_bf16_storage_switch_rounds_and_stays_close(golden):
    cfg, sd, x, _ = golden
    exact = wavlm_ref.wavlm_forward(sd, x, cfg)
    stored = wavlm_ref.wavlm_forward(sd, x, cfg, bf16_storage=True)
    err = l2_rel(stored, exact)
    print(f"bf16-storage restatement vs fp64: {err:.3e}")
    assert torch.equal(stored, stored.to(torch.bfloat16).to(stored.dtype))
    assert 1e-4 < err < 2e-2


def test_staged_attention_restatement_is_the_exact_one_up_to_its_roundings():
    """``relbias_staged`` (what the GPU kernel test compares against) against the direct softmax with the bias, and with a zero
    table against tests/attn_ref.py's plain staged forward, bit for bit"""
    import attn_ref as R
    B, H, T, dh = 2, 2, 77, 64
    g = torch.Generator().manual_seed(4)
    q, k, v = (R.bf16r(torch.randn(B, T, H * dh, generator=g, dtype=torch.float64)) for _ in range(3))
    gate = R.f32r(1.0 + 2.0 * torch.rand(B, H, T, generator=g, dtype=torch.float64))
    table = R.f32r(torch.randn(H, 2 * T - 1, generator=g, dtype=torch.float64))
    scale = R.f32r_scale(dh ** -0.5)
    st = wavlm_ref.relbias_staged(q, k, v, H, scale, gate, table)
    o, lse, s = wavlm_ref.relbias_attention_ref(R.heads(q, H), R.heads(k, H), R.heads(v, H), gate, table, scale)
    assert float((st["o"] - R.merge(o)).abs().max()) <= 2 ** -8 * float(o.abs().max()) and float((st["lse"] - lse).abs().max()) <= 1e-9
    one = (R.heads(q, H)[1, 1, 5] @ R.heads(k, H)[1, 1, 9]) * scale + gate[1, 1, 5] * table[1, 9 - 5 + T - 1]       # i = 5, j = 9
    assert abs(float(s[1, 1, 5, 9] - one)) <= 1e-12
    zero = wavlm_ref.relbias_staged(q, k, v, H, scale, gate, torch.zeros_like(table))
    plain = R.staged(q, k, v, torch.zeros_like(q), H, scale)
    assert torch.equal(zero["o"], plain["o"]) and torch.equal(zero["lse"], plain["lse"])


# ---- buckets -------------------------------------------------------------------------------------------------
PINNED = {79: 239, 80: 240, 799: 319, 800: 319, -800: 159}


@pytest.mark.parametrize("nb,md", [(320, 800), (32, 64)])
def test_bucket_indices_are_huggingfaces(nb, md):
    from mmfusion.wavlm import relative_buckets
    dist = torch.arange(-4095, 4096)
    mine = relative_buckets(dist, nb, md)
    assert mine.dtype == torch.int64 and torch.equal(mine, wavlm_ref.relative_buckets(dist, nb, md))
    assert int(mine.min()) >= 0 and int(mine.max()) == nb - 1 and int(mine[4095]) == 0
    if (nb, md) == (320, 800):
        assert {d: int(mine[d + 4095]) for d in PINNED} == PINNED
    transformers = pytest.importorskip("transformers")
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    att = WavLMAttention(embed_dim=64, num_heads=1, num_buckets=nb, max_distance=md)
    assert torch.equal(mine, att._relative_positions_bucket(dist))
    T = 130                                                   # compute_bias's (T, T) index is the table's, diagonal by diagonal
    i, j = torch.arange(T).view(T, 1), torch.arange(T).view(1, T)
    assert torch.equal(relative_buckets(torch.arange(-(T - 1), T), nb, md)[j - i + T - 1], att._relative_positions_bucket(j - i))


# ---- NativeWavLM: the state_dict surface ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "base"])
def test_state_dict_is_huggingfaces_key_for_key(which):
    cfg = wavlm_ref.tiny_config() if which == "tiny" else wavlm_ref.base_config()
    m = _native(cfg)
    sd = m.state_dict()
    want = wavlm_ref.hf_keys(cfg)
    assert list(sd.keys()) == list(want.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    if which == "base":
        from mmfusion.wavlm import FAMILIES, NativeWavLM
        assert list(NativeWavLM().state_dict().keys()) == list(want.keys())           # the defaults ARE wavlm-base
        assert set(FAMILIES) == {"base", "base-plus"} and FAMILIES["base"] == FAMILIES["base-plus"]
        assert list(NativeWavLM(**FAMILIES["base-plus"]).state_dict().keys()) == list(want.keys())
    assert all(not p.requires_grad for p in m.parameters())
    assert m.config.model_type == "wavlm" and (m.config.num_buckets, m.config.max_bucket_distance) == (320, 800)
    transformers = pytest.importorskip("transformers")
    hf = transformers.WavLMModel(transformers.WavLMConfig(**wavlm_ref.config_kwargs(cfg)))
    assert [(k, tuple(v.shape)) for k, v in hf.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]


@pytest.mark.parametrize("legacy", [False, True])
def test_round_trip_is_bit_exact_in_both_weight_norm_spellings(legacy):
    cfg = wavlm_ref.tiny_config()
    sd = wavlm_ref.seeded_weights(cfg, seed=7, legacy_weight_norm=legacy)
    m = _native(cfg)
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.hf_state_dict(legacy_weight_norm=legacy)
    assert list(back.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    assert torch.equal(m.rel_embed, sd["encoder.layers.0.attention.rel_attn_embed.weight"])
    assert torch.equal(m.l1_gate_c, sd["encoder.layers.1.attention.gru_rel_pos_const"]) and m.l1_gate_c.shape == (1, 4, 1, 1)
    with pytest.raises(RuntimeError, match="rel_attn_embed"):
        m.load_state_dict({k: v for k, v in sd.items() if "rel_attn_embed" not in k})


def test_huggingface_loads_the_native_state_dict_strictly():
    transformers = pytest.importorskip("transformers")
    cfg = wavlm_ref.tiny_config()
    m = _native(cfg)
    m.load_state_dict(wavlm_ref.seeded_weights(cfg, seed=17))
    hf = transformers.WavLMModel(transformers.WavLMConfig(**wavlm_ref.config_kwargs(cfg)))
    res = hf.load_state_dict(m.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    res = m.load_state_dict(hf.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


# ---- NativeWavLM: refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=False),      # wavlm-large
    dict(feat_extract_norm="layer"), dict(do_stable_layer_norm=True), dict(conv_bias=True),
    dict(num_attention_heads=8),                                                      # head_dim 32
    dict(num_buckets=30), dict(num_buckets=320, max_bucket_distance=80),
    dict(hidden_dropout=0.1), dict(layerdrop=0.1), dict(mask_time_prob=0.05),
])
def test_configurations_outside_the_base_family_are_refused(kw):
    with pytest.raises(ValueError, match="NativeWavLM"):
        _native(wavlm_ref.tiny_config(), **kw)


def test_training_surfaces_are_refused():
    m = _native(wavlm_ref.tiny_config())
    for args, kw in (((1,), {}), ((2,), dict(front=True)), ((2,), dict(front=True, feature_encoder=True)), ((True,), {})):
        with pytest.raises(ValueError, match="NativeWavLM"):
            m.set_trainable_layers(*args, **kw)
    m.set_trainable_layers(0)
    assert m.trainable_layers == 0 and all(not p.requires_grad for p in m.parameters())
    from mmfusion.wav2vec2 import REG_960H
    for settings in (dict(attention_dropout=0.1), dict(activation_dropout=0.2), dict(feat_proj_dropout=0.1), REG_960H):
        with pytest.raises(ValueError, match="NativeWavLM"):
            m.set_regularisation(**settings)
    m.set_regularisation(hidden_dropout=0.0, mask_time_length=10)


def test_forward_refusals_need_no_gpu():
    from mmfusion import ops
    m = _native(wavlm_ref.tiny_config())
    x = torch.zeros(1, 4000)
    with pytest.raises(NotImplementedError, match="NativeWavLM.*attention_mask"):
        m(x, attention_mask=torch.ones(1, 4000))
    with pytest.raises(RuntimeError, match="NativeWavLM.*GPU only"):
        m(x)
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match="NativeWavLM.*bf16 storage only"):
            m(x)
    finally:
        ops.set_precision(old)
    from mmfusion.wavlm import NativeWavLM
    assert NativeWavLM().frames(160000) == 499


def test_kernel_wrappers_check_their_operands():
    from mmfusion import lib
    x = torch.zeros(6, 128, dtype=torch.bfloat16)
    w, b, c = torch.zeros(8, 64), torch.zeros(8), torch.zeros(2)
    with pytest.raises(ValueError, match="wavlm_gate"):
        lib.wavlm_gate(x, w, b, c, torch.zeros(2 * 2 * 3 - 1), 2, 3, 2, 64)
    with pytest.raises(ValueError, match="wavlm_gate"):
        lib.wavlm_gate(x.float(), w, b, c, torch.zeros(12), 2, 3, 2, 64)
    p = lib.AttnProblem(None, None, None, None, None, None, None, None, None, None, 2, 2, 3, 3, 128, 128, 128, 128)
    with pytest.raises(ValueError, match="attn_fwd_relbias"):
        lib.attn_fwd_relbias(p, 64, 0.125, torch.zeros(12), torch.zeros(2, 4))


# ---- AudioEncoder ------------------------------------------------------------------------------------------------
def _encoder_config(**extra):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.audio_hidden_size = 256, 256
    cfg.audio_backbone = "native-wavlm"
    wcfg = wavlm_ref.tiny_config()
    cfg.audio_backbone_kwargs = {k: v for k, v in wavlm_ref.config_kwargs(wcfg).items() if k != "hidden_size"}
    for k, v in extra.items():
        setattr(cfg, k, v)
    return cfg, wcfg


def test_audio_encoder_switch_builds_the_native_wavlm():
    from mmfusion.wav2vec2 import NativeWav2Vec2
    from mmfusion.wavlm import NativeWavLM
    from models.encoders import AudioEncoder
    cfg, wcfg = _encoder_config()
    enc = AudioEncoder(cfg)
    assert type(enc.model) is NativeWavLM and enc.hidden_size == 256 and enc._native
    assert list(enc.model.state_dict().keys()) == list(wavlm_ref.hf_keys(wcfg).keys())
    assert "model.encoder.layers.0.attention.rel_attn_embed.weight" in enc.state_dict()
    cfg.audio_backbone = "native"                              # "native" is what it was
    cfg.audio_backbone_kwargs = {k: v for k, v in cfg.audio_backbone_kwargs.items() if k not in ("num_buckets", "max_bucket_distance")}
    assert type(AudioEncoder(cfg).model) is NativeWav2Vec2


@pytest.mark.parametrize("extra", [dict(audio_backbone_trainable_layers=1), dict(audio_backbone_trainable_layers="all"),
                                   dict(audio_backbone_trainable_layers="full"), dict(audio_backbone_regularisation=True),
                                   dict(audio_backbone_regularisation=dict(hidden_dropout=0.1))])
def test_audio_encoder_refuses_training_this_backbone(extra):
    from models.encoders import AudioEncoder
    cfg, _ = _encoder_config(**extra)
    with pytest.raises(ValueError, match="NativeWavLM"):
        AudioEncoder(cfg)
