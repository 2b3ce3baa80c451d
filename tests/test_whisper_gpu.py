"""GPU: ``mmfusion.whisper.NativeWhisperEncoder`` against the captured HuggingFace output (tests/golden/whisper_tiny.npz) and the
explicit restatement tests/whisper_ref.py, which needs neither the reference nor transformers.  Tiny model: d_model 128, 2 heads,
2 layers, ``max_source_positions`` 100, so that T crosses the attention kernel's 64-key tile.

Bounds (tests/test_wavlm_gpu.py's).  (a) against the restatement with bf16 storage: relative L2 <= BOUND_A, the project's bound for a
kernel against an oracle with the same storage format.  (b) against the exact restatement (and the captured output, which the
restatement meets to 1e-6): 2 x the error of the bf16-storage restatement against the exact one on the same inputs, computed here
on the CPU."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import whisper_ref as R  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "whisper_tiny.npz")


def _native(cfg, sd, **kw):
    from mmfusion.whisper import NativeWhisperEncoder
    m = NativeWhisperEncoder(**{**R.config_kwargs(cfg), **kw})
    m.load_state_dict(sd)
    return m.cuda().eval()


def _waves(n: int, L: int, seed: int) -> torch.Tensor:
    return torch.from_numpy(np.stack([R.speech_like(L, seed=seed + i) * (0.5 + i) for i in range(n)]))


def _setup(n: int, L: int, seed: int = 21, **kw):
    cfg = R.tiny_config()
    sd = R.seeded_weights(cfg, seed=seed)
    return cfg, sd, _native(cfg, sd, **kw), _waves(n, L, seed + 1)


@pytest.fixture(scope="module")
def golden():
    """the captured case with the restatement's two forms of it, computed once"""
    sd, wave, feats, want = R.load_golden(GOLDEN)
    cfg = R.tiny_config()
    return cfg, sd, wave, feats, want, R.whisper_forward(sd, wave.numpy(), cfg), R.whisper_forward(sd, wave.numpy(), cfg, bf16_storage=True)


def test_tiny_model_against_the_captured_output_and_the_restatement(golden):
    cfg, sd, wave, feats, want, exact, stored = golden
    m = _native(cfg, sd)
    got = m(wave.cuda()).last_hidden_state
    assert got.dtype == torch.float32 and got.shape == want.shape == (1, 100, cfg.d_model) and not got.requires_grad
    a, model_err = l2_rel(got, stored), l2_rel(stored, exact)
    b, h = l2_rel(got, exact), l2_rel(got, want)
    print(f"NativeWhisperEncoder tiny 1 x 20000: (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A}); (b) vs exact restatement "
          f"{b:.3e}, vs captured HuggingFace {h:.3e} (bound {2 * model_err:.3e})")
    assert a <= BOUND_A and b <= 2 * model_err and h <= 2 * model_err
    f = m.features(wave.cuda())
    err = float((f.cpu() - feats).abs().max())
    print(f"features vs the captured input_features: max abs {err:.3e}")
    assert f.shape == feats.shape and err <= 1e-4
    from_feats = m(input_features=feats.cuda()).last_hidden_state
    assert l2_rel(from_feats, stored) <= BOUND_A and l2_rel(from_feats, want) <= 2 * model_err


def test_waveform_and_its_own_features_agree_bit_for_bit():
    cfg, sd, m, x = _setup(3, 32000)
    xd = x.cuda()
    by_wave = m(xd).last_hidden_state
    by_feats = m(input_features=m.features(xd)).last_hidden_state
    assert torch.equal(by_wave, by_feats)
    short = m(xd[:, :9001]).last_hidden_state                       # a shorter clip is the zero-padded one
    padded = torch.zeros_like(xd)
    padded[:, :9001] = xd[:, :9001]
    assert torch.equal(short, m(padded).last_hidden_state) and not torch.equal(short, by_wave)


def test_results_do_not_depend_on_chunk():
    cfg, sd, m1, x = _setup(3, 20000, chunk=1)
    m2 = _native(cfg, sd, chunk=2)
    xd = x.cuda()
    f1, f2 = m1(xd).last_hidden_state, m2(xd).last_hidden_state
    assert torch.equal(f1, f2)
    assert torch.equal(m2(xd).last_hidden_state, f2)
    assert torch.equal(m1.features(xd), m2.features(xd))
    held = sum(v.numel() * v.element_size() for v in m2._ws.values() if isinstance(v, torch.Tensor))
    assert held == 2 * m2.workspace_bytes_per_clip()
    stored = R.whisper_forward(sd, x.numpy(), cfg, bf16_storage=True)
    assert l2_rel(f2, stored) <= BOUND_A


def test_forward_replays_from_a_captured_graph():
    cfg, sd, m, x = _setup(3, 20000, chunk=2)
    xd = x.cuda()
    eager = m(xd).last_hidden_state.clone()
    static = xd.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(static)                                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(static).last_hidden_state
    new = 0.3 * torch.randn_like(static)
    static.copy_(new)
    graph.replay()
    other = out.clone()
    static.copy_(xd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(other, m(new).last_hidden_state) and not torch.equal(other, eager)


def test_state_dict_round_trips_and_refreshes_what_is_derived():
    cfg, sd, m, x = _setup(2, 20000)
    xd = x.cuda()
    first = m(xd).last_hidden_state.clone()
    back = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert list(back) == list(R.hf_keys(cfg)) and all(torch.equal(back[k], sd[k]) for k in sd)
    sd2 = R.seeded_weights(cfg, seed=99)
    m.load_state_dict(sd2)
    second = m(xd).last_hidden_state
    want2 = R.whisper_forward(sd2, x.numpy(), cfg, bf16_storage=True)
    assert l2_rel(second, want2) <= BOUND_A and l2_rel(second, first) > 3 * BOUND_A
    m.load_state_dict(back)
    assert torch.equal(m(xd).last_hidden_state, first)


def test_huggingface_state_dict_to_native_output():
    transformers = pytest.importorskip("transformers")
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    cfg = R.tiny_config()
    hf = WhisperEncoder(transformers.WhisperConfig(**R.config_kwargs(cfg))).eval()
    hf.load_state_dict(R.seeded_weights(cfg, seed=41))
    sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    m = _native(cfg, sd)
    x = _waves(2, 32000, 42)
    fe = transformers.WhisperFeatureExtractor(feature_size=cfg.num_mel_bins, chunk_length=2)
    feats = fe([w for w in x.numpy()], sampling_rate=16000, return_tensors="pt").input_features
    with torch.no_grad():
        want = hf(feats).last_hidden_state
    model_err = l2_rel(R.whisper_forward(sd, x.numpy(), cfg, bf16_storage=True), R.whisper_forward(sd, x.numpy(), cfg))
    err = l2_rel(m(x.cuda()).last_hidden_state, want)
    print(f"NativeWhisperEncoder vs HuggingFace fp32 (tiny): {err:.3e} (bound {2 * model_err:.3e})")
    assert err <= 2 * model_err


def test_a_1280_wide_layer_runs_on_every_kernel_of_the_path():
    """``FAMILIES["large"]`` is offered because every kernel takes d = 1280 (head_dim 64, the LayerNorm forward's chunk form, 128 mel
    bins): one layer of that width at a 1 s window against the restatement"""
    cfg = R.tiny_config(d_model=1280, encoder_attention_heads=20, encoder_layers=1, encoder_ffn_dim=512, num_mel_bins=128, max_source_positions=50)
    sd = R.seeded_weights(cfg, seed=51)
    m = _native(cfg, sd)
    x = _waves(1, 16000, 52)
    a = l2_rel(m(x.cuda()).last_hidden_state, R.whisper_forward(sd, x.numpy(), cfg, bf16_storage=True))
    print(f"NativeWhisperEncoder d_model 1280, 128 mel bins: (a) {a:.3e} (bound {BOUND_A})")
    assert a <= BOUND_A


def test_audio_encoder_native_whisper_against_reference_backbone():
    """``config.audio_backbone = "native-whisper"`` at width 512 against the same encoder given the restatement as its ``backbone=``;
    the tail (temporal attention, projection) is the same HIP code on both sides.  Tolerance:
    ``test_audio_encoder_native_backbone_against_reference_backbone``'s 1e-2 scaled by max(1, |want|max)."""
    import config as cfgmod
    from mmfusion.whisper import NativeWhisperEncoder
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 512      # the tail's 8 heads need a head_dim of 64 / 96
    cfg.audio_backbone = "native-whisper"
    cfg.audio_backbone_kwargs = dict(encoder_layers=2, encoder_attention_heads=8, encoder_ffn_dim=512, max_source_positions=50)
    torch.manual_seed(3)
    enc = AudioEncoder(cfg)
    assert type(enc.model) is NativeWhisperEncoder and enc.model.config.d_model == 512
    wcfg = R.tiny_config(d_model=512, encoder_layers=2, encoder_attention_heads=8, encoder_ffn_dim=512, max_source_positions=50)
    sd = R.seeded_weights(wcfg, seed=31)
    enc.model.load_state_dict(sd)
    cfg_ref = cfgmod.ModelConfig()
    cfg_ref.fusion_hidden_size, cfg_ref.fusion_dropout = 256, 0.0
    ref = AudioEncoder(cfg_ref, backbone=R.RefWhisper(sd, wcfg))
    tail = {k: v for k, v in enc.state_dict().items() if not k.startswith("model.")}
    assert len(tail) < len(enc.state_dict()) and "model.layers.0.self_attn.k_proj.weight" in enc.state_dict()
    ref.load_state_dict(tail)
    wave = _waves(2, 12000, 32).cuda()
    enc, ref = enc.cuda().eval(), ref.cuda().eval()
    with torch.no_grad():
        got, want = enc(wave), ref(wave)
    for k in ("features", "sequence_output"):
        err = float((got[k] - want[k]).abs().max())
        scale = max(1.0, float(want[k].abs().max()))
        print(f"AudioEncoder native-whisper vs reference backbone, {k}: abs err {err:.3e} (scale {scale:.2f})")
        assert got[k].shape == want[k].shape and err <= 1e-2 * scale, k


def test_forward_refusals():
    from mmfusion import ops
    cfg, sd, m, x = _setup(1, 4000)
    xd, who = x.cuda(), "NativeWhisperEncoder"
    feats = m.features(xd)
    with pytest.raises(RuntimeError, match=who):
        m(x)                                                           # a CPU tensor
    with pytest.raises(RuntimeError, match=who):
        m(input_features=feats.cpu())
    with pytest.raises(ValueError, match=who):
        m(xd, input_features=feats)
    with pytest.raises(ValueError, match=who):
        m()
    with pytest.raises(NotImplementedError, match=who):
        m(xd, attention_mask=torch.ones(1, 100, device="cuda"))
    with pytest.raises(ValueError, match=who):
        m(torch.zeros(1, 32001, device="cuda"))                        # over the window
    with pytest.raises(ValueError, match=who):
        m(torch.zeros(1, 0, device="cuda"))
    with pytest.raises(ValueError, match=who):
        m(input_features=feats[:, :, :-1])
    with pytest.raises(TypeError, match=who):
        m(xd.double())
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match=who + ".*bf16 storage only"):
            m(xd)
        with pytest.raises(RuntimeError, match=who + ".*bf16 storage only"):
            m.features(xd)
    finally:
        ops.set_precision(old)
