"""CPU: the float64 restatement tests/whisper_ref.py against HuggingFace (the captured tests/golden/whisper_tiny.npz, and live where
transformers is installed), the package's own tables against HuggingFace's, every named mutant, and the host side of
``mmfusion.whisper.NativeWhisperEncoder``: the ``state_dict`` surface, the refusals, the ``AudioEncoder`` route's refusals and the
entry points' argument checks (which run before anything is launched, so they need no GPU).

Bounds.  The log-mel restatement against ``WhisperFeatureExtractor``: 1e-4 absolute (both are float64 up to the extractor's float32
result; measured: 2e-6 on the captured clip, at most 3e-5 over noise, a half-silent clip, a short clip and a speech-like clip).  The
encoder restatement against the captured float32 output: relative L2 1e-5 (measured 4e-7).  A mutant must leave the bound the true
restatement meets."""
import os

import numpy as np
import pytest
import torch

import whisper_ref as R
from helpers import l2_rel
from mmfusion import lib
from mmfusion import whisper as W
from mmfusion.whisper import NativeWhisperEncoder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "whisper_tiny.npz")
LOGMEL_BOUND, ENCODER_BOUND = 1e-4, 1e-5
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
BASE = 0x7F0000000000                        # addresses are only looked at (null, alignment), never followed
WHO = "NativeWhisperEncoder"


@pytest.fixture(scope="module")
def golden():
    sd, wave, feats, out = R.load_golden(GOLDEN)
    return R.tiny_config(), sd, wave, feats, out


def _clips(n_samples: int):
    rng = np.random.default_rng(0)
    half = 0.3 * rng.standard_normal(n_samples)
    half[n_samples // 2:] = 0.0
    return {"noise": 0.3 * rng.standard_normal(n_samples), "half_silent": half, "short": 0.3 * rng.standard_normal(9001),
            "speech": R.speech_like(n_samples, seed=1).astype(np.float64)}


def test_the_fixture_is_small_and_whole(golden):
    cfg, sd, wave, feats, out = golden
    assert os.path.getsize(GOLDEN) <= 750_000
    assert list(sd) == list(R.hf_keys(cfg)) and all(tuple(sd[k].shape) == s for k, s in R.hf_keys(cfg).items())
    assert wave.shape == (1, 20000) and feats.shape == (1, 80, 200) and out.shape == (1, 100, 128)
    assert len(sd) == 5 + 15 * cfg.encoder_layers + 2 and not any("k_proj.bias" in k for k in sd)


def test_restatement_against_the_captured_huggingface_output(golden):
    cfg, sd, wave, feats, out = golden
    f = R.log_mel(wave.numpy(), cfg.num_mel_bins, cfg.max_source_positions)
    err_f = float(np.abs(f - feats.numpy()).max())
    err_e = l2_rel(R.encoder_forward(sd, feats, cfg), out)
    err_w = l2_rel(R.whisper_forward(sd, wave.numpy(), cfg), out)
    print(f"restatement vs captured: log-mel max abs {err_f:.3e}, encoder {err_e:.3e}, from the waveform {err_w:.3e}")
    assert err_f <= LOGMEL_BOUND and err_e <= ENCODER_BOUND and err_w <= ENCODER_BOUND


@pytest.mark.parametrize("mutant", R.LOGMEL_MUTANTS)
def test_every_log_mel_mutant_leaves_the_bound(golden, mutant):
    cfg, sd, wave, feats, out = golden
    quiet = 1e-3 * np.random.default_rng(5).standard_normal(20000)            # 50 dB under the captured clip: a batch-wide maximum clamps it
    waves = [wave.numpy()[0].astype(np.float64), quiet]
    true = R.log_mel(waves, cfg.num_mel_bins, cfg.max_source_positions)
    assert float(np.abs(true[:1] - feats.numpy()).max()) <= LOGMEL_BOUND
    err = float(np.abs(R.log_mel(waves, cfg.num_mel_bins, cfg.max_source_positions, mutant=mutant) - true).max())
    print(f"mutant {mutant}: log-mel max abs {err:.3e}")
    assert err > 10 * LOGMEL_BOUND


@pytest.mark.parametrize("mutant", R.ENCODER_MUTANTS)
def test_every_encoder_mutant_leaves_the_bound(golden, mutant):
    cfg, sd, wave, feats, out = golden
    err = l2_rel(R.encoder_forward(sd, feats, cfg, mutant=mutant), out)
    print(f"mutant {mutant}: encoder relative L2 {err:.3e}")
    assert err > 100 * ENCODER_BOUND


def test_bf16_storage_mode_is_close_and_not_equal(golden):
    cfg, sd, wave, feats, out = golden
    err = l2_rel(R.whisper_forward(sd, wave.numpy(), cfg, bf16_storage=True), out)
    assert 1e-4 < err < 2e-2


# ---- live against transformers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,T", [(80, 100), (128, 50)])
def test_log_mel_restatement_against_the_feature_extractor(n_mels, T):
    transformers = pytest.importorskip("transformers")
    n_samples = 320 * T
    fe = transformers.WhisperFeatureExtractor(feature_size=n_mels, chunk_length=n_samples // 16000)
    for name, clip in _clips(n_samples).items():
        want = fe(clip.astype(np.float32), sampling_rate=16000, return_tensors="np").input_features[0]
        got = R.log_mel([clip.astype(np.float32)], n_mels, T)[0]
        err = float(np.abs(got - want).max())
        print(f"log-mel restatement vs WhisperFeatureExtractor, {n_mels} bins, {name}: max abs {err:.3e}")
        assert got.shape == want.shape == (n_mels, 2 * T) and err <= LOGMEL_BOUND


def test_encoder_restatement_against_live_huggingface():
    transformers = pytest.importorskip("transformers")
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    cfg = R.tiny_config(max_source_positions=50)
    hf = WhisperEncoder(transformers.WhisperConfig(**R.config_kwargs(cfg))).eval()
    sd = R.seeded_weights(cfg, seed=7)
    hf.load_state_dict(sd)
    assert list(hf.state_dict()) == list(R.hf_keys(cfg))
    feats = torch.from_numpy(R.log_mel([R.speech_like(16000, seed=8)], 80, 50)).float()
    with torch.no_grad():
        want = hf(feats).last_hidden_state
    assert l2_rel(R.encoder_forward(sd, feats, cfg), want) <= ENCODER_BOUND


def test_package_tables_against_huggingface():
    transformers = pytest.importorskip("transformers")
    from transformers.audio_utils import window_function
    from transformers.models.whisper.modeling_whisper import sinusoids
    for n_mels in (80, 128):
        want = transformers.WhisperFeatureExtractor(feature_size=n_mels).mel_filters
        got = W.mel_filter_bank(n_mels)
        assert got.shape == want.shape == (201, n_mels) and float(np.abs(got - want).max()) <= 1e-15
    assert float(np.abs(W.hann_window() - window_function(400, "hann")).max()) <= 1e-15
    for T, d in ((100, 128), (1500, 768)):
        assert torch.equal(W.sinusoids(T, d), sinusoids(T, d))


def test_package_tables_against_the_restatement():
    for n_mels in (80, 128):
        assert float(np.abs(W.mel_filter_bank(n_mels) - R.filter_bank(n_mels)).max()) <= 1e-14
    assert float(np.abs(W.hann_window() - R.hann()).max()) <= 1e-15
    assert torch.equal(W.sinusoids(100, 128), R.sinusoids(100, 128))
    t = W.dft_table()
    k, b = 37, 113
    assert t.shape == (400, 2 * lib.WHISPER_DFT_COLS) and not t[:, 201:224].any() and not t[:, 224 + 201:].any()
    assert abs(t[k, b] - np.cos(2 * np.pi * k * b / 400)) <= 1e-13 and abs(t[k, 224 + b] - np.sin(2 * np.pi * k * b / 400)) <= 1e-13
    assert abs(t[100, 1]) <= 1e-16 and t[100, 224 + 1] == 1.0 and t[399, 1] == t[1, 1]      # the angle is reduced in integers first


# ---- the module's host side ---------------------------------------------------------------------------------------------
def test_state_dict_surface_is_huggingfaces(golden):
    cfg, sd, *_ = golden
    m = NativeWhisperEncoder(**R.config_kwargs(cfg))
    own = m.state_dict()
    assert list(own) == list(R.hf_keys(cfg)) and all(tuple(own[k].shape) == s for k, s in R.hf_keys(cfg).items())
    assert torch.equal(own["embed_positions.weight"], R.sinusoids(100, 128))            # built from sizes: the sinusoid table
    assert m.config.d_model == m.config.hidden_size == 128 and all(not p.requires_grad for p in m.parameters())
    m.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert not m.l0_qkv_b[128:256].any() and torch.equal(m.l0_qkv_b[:128], sd["layers.0.self_attn.q_proj.bias"])
    with pytest.raises(RuntimeError, match="Unexpected key.*k_proj.bias"):
        m.load_state_dict({**sd, "layers.0.self_attn.k_proj.bias": torch.zeros(128)})
    with pytest.raises(RuntimeError, match="Missing key.*layer_norm.bias"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "layer_norm.bias"})
    with pytest.raises(RuntimeError, match="size mismatch for conv1.weight"):
        m.load_state_dict({**sd, "conv1.weight": torch.zeros(128, 3, 80)})


def test_families_build_from_sizes():
    assert sorted(W.FAMILIES) == ["base", "large", "medium", "small", "tiny"]
    m = NativeWhisperEncoder(**{**W.FAMILIES["tiny"], "max_source_positions": 50})
    assert m.config.d_model == 384 and m.head_dim == 64 and len(m.state_dict()) == 5 + 15 * 4 + 2
    m = NativeWhisperEncoder(**{**W.FAMILIES["large"], "encoder_layers": 1, "max_source_positions": 50})
    assert m.config.num_mel_bins == 128 and m.head_dim == 64 and m.state_dict()["conv1.weight"].shape == (1280, 128, 3)
    import inspect
    d = {k: v.default for k, v in inspect.signature(NativeWhisperEncoder.__init__).parameters.items() if k in W.FAMILIES["small"]}
    assert d == W.FAMILIES["small"]


def test_refusals_name_the_class():
    tiny = R.config_kwargs(R.tiny_config())
    for kw in (dict(activation_function="gelu_new"), dict(dropout=0.1), dict(attention_dropout=0.1), dict(activation_dropout=0.1),
               dict(encoder_layerdrop=0.1), dict(apply_spec_augment=True), dict(encoder_attention_heads=1), dict(encoder_attention_heads=4),
               dict(num_mel_bins=64), dict(max_source_positions=0), dict(d_model=132, encoder_attention_heads=2)):
        with pytest.raises(ValueError, match=WHO):
            NativeWhisperEncoder(**{**tiny, **kw})
    m = NativeWhisperEncoder(**tiny)
    m.set_trainable_layers(0)
    for k in (1, 2, True):
        with pytest.raises(ValueError, match=WHO + ".*frozen"):
            m.set_trainable_layers(k)
    with pytest.raises(ValueError, match=WHO + ".*frozen"):
        m.set_trainable_layers(0, front=True)
    with pytest.raises(ValueError, match=WHO):
        m.set_regularisation(dropout=0.1)
    with pytest.raises(RuntimeError, match=WHO + ".*GPU only"):
        m(torch.zeros(1, 4000))
    with pytest.raises(RuntimeError, match=WHO + ".*GPU only"):
        m.features(torch.zeros(1, 4000))
    with pytest.raises(RuntimeError, match=WHO + ".*GPU only"):
        m(input_features=torch.zeros(1, 80, 200))
    with pytest.raises(NotImplementedError, match=WHO):
        m(torch.zeros(1, 4000), attention_mask=torch.ones(1, 100))
    with pytest.raises(ValueError, match=WHO):
        m()
    from mmfusion import ops
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match=WHO + ".*bf16 storage only"):
            m(torch.zeros(1, 4000))
    finally:
        ops.set_precision(old)


def test_audio_encoder_route_builds_and_refuses():
    import config as cfgmod
    from models.encoders import AudioEncoder

    def cfg(**kw):
        c = cfgmod.ModelConfig()
        c.fusion_hidden_size, c.audio_hidden_size, c.audio_backbone = 256, 512, "native-whisper"
        c.audio_backbone_kwargs = dict(encoder_layers=1, encoder_attention_heads=8, encoder_ffn_dim=256, max_source_positions=50)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    enc = AudioEncoder(cfg())
    assert type(enc.model) is NativeWhisperEncoder and enc.hidden_size == 512 and enc.model.trainable_layers == 0
    assert "model.layers.0.self_attn.k_proj.weight" in enc.state_dict() and "model.layers.0.self_attn.k_proj.bias" not in enc.state_dict()
    for kw in (dict(audio_backbone_trainable_layers=1), dict(audio_backbone_trainable_layers="all"), dict(audio_backbone_trainable_layers="full"),
               dict(audio_backbone_regularisation=True), dict(audio_backbone_regularisation=dict(hidden_dropout=0.1))):
        with pytest.raises(ValueError, match=WHO):
            AudioEncoder(cfg(**kw))


# ---- the entry points' argument checks (host only) ---------------------------------------------------------------------------
def test_entry_points_refuse_before_they_launch():
    L = lib.load()
    A = [BASE + 0x1000 * i for i in range(1, 9)]
    sb = L.mmf_whisper_logmel_scratch_bytes(2, 16000, 80)
    assert sb == (2 * 100 * 80 + 2 * 2) * 4 and L.mmf_whisper_logmel_scratch_bytes(0, 16000, 80) == 0

    def logmel(wave=A[0], ld=9001, win=A[1], dft=A[2], fb=A[3], f=A[4], w=A[5], sc=A[6], sbytes=sb, N=2, Ln=9001, ns=16000, M=80, Kw=240):
        return L.mmf_whisper_logmel(wave, ld, win, dft, fb, f, w, sc, sbytes, N, Ln, ns, M, Kw, None)
    for kw, code in [(dict(wave=None), E_SHAPE), (dict(win=None), E_SHAPE), (dict(dft=None), E_SHAPE), (dict(fb=None), E_SHAPE),
                     (dict(sc=None), E_SHAPE), (dict(f=None, w=None), E_SHAPE), (dict(N=0), E_SHAPE), (dict(Ln=0), E_SHAPE),
                     (dict(Ln=16001, ld=16001), E_SHAPE), (dict(ns=16100), E_SHAPE), (dict(ns=0), E_SHAPE), (dict(ld=9000), E_SHAPE),
                     (dict(Kw=232), E_SHAPE), (dict(Kw=244), E_SHAPE), (dict(sbytes=sb - 4), E_SHAPE),
                     (dict(M=40), E_UNSUPPORTED), (dict(M=96, Kw=288), E_UNSUPPORTED), (dict(N=65536), E_UNSUPPORTED),
                     (dict(wave=A[0] + 2), E_ALIGN), (dict(f=A[4] + 1), E_ALIGN), (dict(w=A[5] + 8), E_ALIGN), (dict(sc=A[6] + 4), E_ALIGN)]:
        assert logmel(**kw) == code, kw
        assert b"mmf_whisper_logmel" in L.mmf_last_error()
    assert L.mmf_whisper_gelu_window(A[0], A[1], A[0], 1, 10, 128, 3, 2, 1, None) == E_UNSUPPORTED
    assert L.mmf_whisper_gelu_window(A[0], A[1], A[2], 1, 10, 128, 3, 2, 3, None) == E_SHAPE
    assert L.mmf_whisper_gelu_window(A[0], A[1] + 4, A[2], 1, 10, 128, 3, 2, 1, None) == E_ALIGN
    assert L.mmf_whisper_stem_out(A[0], A[1], A[2], A[0], 21, 10, 128, None) == E_SHAPE
    assert L.mmf_whisper_stem_out(A[0], A[1], A[2], A[0], 20, 10, 132, None) == E_UNSUPPORTED
    assert L.mmf_whisper_stem_out(A[0], A[1], A[2] + 4, A[0], 20, 10, 128, None) == E_ALIGN
    assert L.mmf_whisper_feature_window(A[0], A[1], 1, 80, 100, 232, None) == E_SHAPE
