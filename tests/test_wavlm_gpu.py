"""GPU: ``mmfusion.wavlm.NativeWavLM`` against the captured HuggingFace output (tests/golden/wavlm_tiny.npz) and the explicit
restatement tests/wavlm_ref.py, which needs neither the reference nor transformers.

Bounds (tests/test_w2v_gpu.py's).  (a) against the restatement with bf16 storage: relative L2 <= BOUND_A, the project's bound for a
kernel against an oracle with the same storage format.  (b) against the exact restatement (and the captured output, which the
restatement meets to 2e-5): 2 x the error of the bf16-storage restatement against the exact one on the same inputs, computed here
on the CPU."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import wavlm_ref  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavlm_tiny.npz")


def _native(cfg, sd, **kw):
    from mmfusion.wavlm import NativeWavLM
    m = NativeWavLM(**{**wavlm_ref.config_kwargs(cfg), **kw})
    m.load_state_dict(sd)
    return m.cuda().eval()


def _setup(n: int, L: int, seed: int = 21, **kw):
    cfg = wavlm_ref.tiny_config()
    sd = wavlm_ref.seeded_weights(cfg, seed=seed)
    x = 0.5 * torch.randn(n, L, generator=torch.Generator().manual_seed(seed + 1)) + 0.1
    return cfg, sd, _native(cfg, sd, **kw), x


@pytest.fixture(scope="module")
def golden():
    """the captured case with the restatement's two forms of it, computed once"""
    sd, x, want = wavlm_ref.load_golden(GOLDEN)
    cfg = wavlm_ref.tiny_config()
    return cfg, sd, x, want, wavlm_ref.wavlm_forward(sd, x, cfg), wavlm_ref.wavlm_forward(sd, x, cfg, bf16_storage=True)


def test_tiny_model_against_the_captured_output_and_the_restatement(golden):
    cfg, sd, x, want, exact, stored = golden
    got = _native(cfg, sd)(x.cuda()).last_hidden_state
    assert got.dtype == torch.float32 and got.shape == want.shape == (1, 99, cfg.hidden_size) and not got.requires_grad
    a, model_err = l2_rel(got, stored), l2_rel(stored, exact)
    b, h = l2_rel(got, exact), l2_rel(got, want)
    print(f"NativeWavLM tiny 1 x 2000: (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A}); (b) vs exact restatement {b:.3e}, "
          f"vs captured HuggingFace {h:.3e} (bound {2 * model_err:.3e})")
    assert a <= BOUND_A and b <= 2 * model_err and h <= 2 * model_err


def test_a_long_clip_reaches_clamped_buckets_and_several_query_chunks():
    """16,400 samples -> 819 frames: distances past max_bucket_distance (the clamped last bucket), seven query chunks per head,
    thirteen key tiles.  Bound (a)."""
    cfg, sd, m, x = _setup(1, 16400)
    assert m.frames(16400) == 819 > cfg.max_bucket_distance
    stored = wavlm_ref.wavlm_forward(sd, x, cfg, bf16_storage=True, dtype=torch.float32)
    got = m(x.cuda()).last_hidden_state
    a = l2_rel(got, stored)
    print(f"NativeWavLM tiny 1 x 16400 (819 frames): (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A})")
    assert got.shape == stored.shape and a <= BOUND_A


def test_results_do_not_depend_on_chunk():
    cfg, sd, m1, x = _setup(3, 4000, chunk=1)
    m2 = _native(cfg, sd, chunk=2)
    xd = x.cuda()
    f1, f2 = m1(xd).last_hidden_state, m2(xd).last_hidden_state
    assert torch.equal(f1, f2)
    assert torch.equal(m2(xd).last_hidden_state, f2)
    T, H = m2.frames(4000), cfg.num_attention_heads
    assert m2._ws["gate"].numel() == 2 * H * T
    held = sum(v.numel() * v.element_size() for v in m2._ws.values() if isinstance(v, torch.Tensor))
    assert held == 2 * m2.workspace_bytes_per_clip(4000)


def test_forward_replays_from_a_captured_graph():
    cfg, sd, m, x = _setup(3, 4000, chunk=2)
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
    new = torch.randn_like(static)
    static.copy_(new)
    graph.replay()
    other = out.clone()
    static.copy_(xd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(other, m(new).last_hidden_state) and not torch.equal(other, eager)


def test_load_state_dict_refreshes_the_derived_tables():
    cfg, sd, m, x = _setup(2, 4000)
    xd = x.cuda()
    first = m(xd).last_hidden_state.clone()
    want = wavlm_ref.wavlm_forward(sd, x, cfg, bf16_storage=True)
    assert l2_rel(first, want) <= BOUND_A
    other = wavlm_ref.seeded_weights(cfg, seed=99)
    sd2 = dict(sd)
    for k in sd:
        if "rel_attn_embed" in k or "gru_rel_pos" in k:
            sd2[k] = other[k]
    m.load_state_dict(sd2)
    second = m(xd).last_hidden_state
    want2 = wavlm_ref.wavlm_forward(sd2, x, cfg, bf16_storage=True)
    moved = l2_rel(want2, want)
    print(f"new rel_attn_embed / gate weights: restatement moved by {moved:.3e}; native vs new {l2_rel(second, want2):.3e}, vs old "
          f"{l2_rel(second, want):.3e}")
    assert l2_rel(second, want2) <= BOUND_A and moved > 3 * BOUND_A and l2_rel(second, want) > BOUND_A
    sd3 = dict(sd2)                                                                   # the embedding alone: only the table changes
    sd3["encoder.layers.0.attention.rel_attn_embed.weight"] = sd["encoder.layers.0.attention.rel_attn_embed.weight"]
    m.load_state_dict(sd3)
    third = m(xd).last_hidden_state
    want3 = wavlm_ref.wavlm_forward(sd3, x, cfg, bf16_storage=True)
    assert l2_rel(third, want3) <= BOUND_A and l2_rel(want3, want2) > 3 * BOUND_A and l2_rel(third, want2) > BOUND_A


def test_huggingface_state_dict_to_native_output():
    transformers = pytest.importorskip("transformers")
    cfg = wavlm_ref.tiny_config()
    hf = transformers.WavLMModel(transformers.WavLMConfig(**wavlm_ref.config_kwargs(cfg))).eval()
    hf.load_state_dict(wavlm_ref.seeded_weights(cfg, seed=41))
    sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    m = _native(cfg, sd)
    x = 0.5 * torch.randn(2, 4000, generator=torch.Generator().manual_seed(42))
    with torch.no_grad():
        want = hf(x).last_hidden_state
    model_err = l2_rel(wavlm_ref.wavlm_forward(sd, x, cfg, bf16_storage=True), wavlm_ref.wavlm_forward(sd, x, cfg))
    err = l2_rel(m(x.cuda()).last_hidden_state, want)
    print(f"NativeWavLM vs HuggingFace fp32 (tiny): {err:.3e} (bound {2 * model_err:.3e})")
    assert err <= 2 * model_err


def test_audio_encoder_native_wavlm_against_reference_backbone():
    """``config.audio_backbone = "native-wavlm"`` against the same encoder given the restatement as its ``backbone=``; the tail
    (temporal attention, projection) is the same HIP code on both sides.  Tolerance:
    ``test_audio_encoder_native_backbone_against_reference_backbone``'s 1e-2 scaled by max(1, |want|max)."""
    import config as cfgmod
    from mmfusion.wavlm import NativeWavLM
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 768     # the tail's 8 heads need a head_dim of 64 / 96
    cfg.audio_backbone = "native-wavlm"
    cfg.audio_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=512, conv_dim=(256, 256, 256), conv_kernel=(10, 3, 2),
                                     conv_stride=(5, 2, 2), num_conv_pos_embeddings=16)
    torch.manual_seed(3)
    enc = AudioEncoder(cfg)
    assert type(enc.model) is NativeWavLM
    wcfg = enc.model.config
    sd = wavlm_ref.seeded_weights(wcfg, seed=31)
    enc.model.load_state_dict(sd)
    cfg_ref = cfgmod.ModelConfig()
    cfg_ref.fusion_hidden_size, cfg_ref.fusion_dropout = 256, 0.0
    ref = AudioEncoder(cfg_ref, backbone=wavlm_ref.RefWavLM(sd, wcfg))
    tail = {k: v for k, v in enc.state_dict().items() if not k.startswith("model.")}
    assert len(tail) < len(enc.state_dict()) and "model.encoder.layers.0.attention.rel_attn_embed.weight" in enc.state_dict()
    ref.load_state_dict(tail)
    wave = (0.5 * torch.randn(2, 4000, generator=torch.Generator().manual_seed(32))).cuda()
    enc, ref = enc.cuda().eval(), ref.cuda().eval()
    with torch.no_grad():
        got, want = enc(wave), ref(wave)
    for k in ("features", "sequence_output"):
        err = float((got[k] - want[k]).abs().max())
        scale = max(1.0, float(want[k].abs().max()))
        print(f"AudioEncoder native-wavlm vs reference backbone, {k}: abs err {err:.3e} (scale {scale:.2f})")
        assert got[k].shape == want[k].shape and err <= 1e-2 * scale, k
