"""GPU: the Wav2Vec2 kernels (csrc/wav2vec2.hip) against float64, and ``mmfusion.wav2vec2.NativeWav2Vec2`` against the
explicit restatement tests/w2v_ref.py, which needs neither the reference nor transformers.

Bounds.  (a) against the restatement with bf16 storage: relative L2 <= 2e-2, the project's bound for a kernel against an
oracle with the same storage format.  (b) against the exact restatement: 2 x the error of the bf16-storage restatement
against the exact one on the same inputs, computed here on the CPU: the error of an L-layer bf16 residual stream is
modelled by the storage format, not by the code under test, with a factor 2 for summation order."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gelu_domain  # noqa: E402
import w2v_ref  # noqa: E402
from helpers import BOUND_A, _lib, l2_rel  # noqa: E402

BF16 = torch.bfloat16
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5


# ---- kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T_in,C,k,s", [(3, 41, 256, 3, 2), (2, 40, 512, 3, 2), (3, 37, 64, 2, 2), (1, 38, 8, 2, 2)])
def test_gelu_window_within_one_bf16_ulp_of_f32_erf_gelu(N, T_in, C, k, s):
    lib = _lib()
    x = (3.0 * torch.randn(N, T_in, C, generator=torch.Generator().manual_seed(T_in + C))).to(BF16)
    T_out = (T_in - k) // s + 1
    out = torch.full((N, T_out, k * C), float("nan"), dtype=BF16, device="cuda")
    lib.w2v_gelu_window(x.cuda(), out, N, T_in, C, k, s)
    v = w2v_ref.window(x.float(), k, s)
    worst = float(gelu_domain.ratio_fwd(out.cpu(), v).max())                           # float64, the allowance of tests/gelu_domain.py
    print(f"gelu_window N={N} T_in={T_in} C={C} k={k} s={s}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("N,L,C0,k1,s1,dc", [(2, 4000, 256, 3, 2, 0.5), (3, 4003, 512, 3, 2, 0.0), (1, 1237, 64, 2, 2, 0.5),
                                                (2, 4000, 256, 3, 2, 20.0)])
def test_conv0_two_passes_against_float64(N, L, C0, k1, s1, dc):
    """Statistics at 1e-4 relative: the variance relative to itself; the mean relative to itself on every channel with
    |mean| > std, and relative to |mean| + std on all channels (a mean near zero has no relative accuracy in any arithmetic;
    what the normalisation needs is the mean to a fraction of the spread).  The offset of 20 puts |mean| / std at 10 to 100
    on most channels: a bare f32 E[x^2] - mean^2 loses (mean / std)^2 x 6e-8, i.e. 1e-5 to 1e-3, of the variance there, so
    that case holds only with a shifted or Welford accumulation."""
    lib = _lib()
    g = torch.Generator().manual_seed(L)
    wave = 0.5 * torch.randn(N, L, generator=g) + dc
    w = 0.4 * torch.randn(C0, 1, 10, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(C0, generator=g), 0.1 * torch.randn(C0, generator=g)
    raw = w2v_ref.conv0_raw(wave.double(), w.double(), 5)
    mean, var = w2v_ref.conv0_stats(raw)
    stats = torch.full((N, 2, C0), float("nan"), device="cuda")
    partial = torch.empty(N * lib.W2V_STATS_SLOTS * 2 * C0, device="cuda")
    lib.w2v_conv0_stats(wave.cuda(), w.cuda(), stats, partial, 10, 5)
    got = stats.cpu().double()
    std = var.sqrt()
    e_mean = float(((got[:, 0:1] - mean).abs() / (mean.abs() + std)).max())
    e_var = float(((got[:, 1:2] - var).abs() / var).max())
    big = mean.abs() > std
    e_rel = float(((got[:, 0:1] - mean).abs() / mean.abs())[big].max()) if bool(big.any()) else 0.0
    print(f"conv0 stats N={N} L={L} C0={C0} dc={dc}: mean err / (|mean| + std) {e_mean:.2e}, variance rel err {e_var:.2e} (bound 1e-4); "
          f"largest |mean| / std {float((mean.abs() / std).max()):.2f}")
    print(f"    mean rel err on the {int(big.sum())} channels with |mean| > std: {e_rel:.2e}")
    assert e_mean <= 1e-4 and e_var <= 1e-4 and e_rel <= 1e-4
    T0 = raw.shape[1]
    T1 = (T0 - k1) // s1 + 1
    out = torch.full((N, T1, k1 * C0), float("nan"), dtype=BF16, device="cuda")
    lib.w2v_conv0_norm_gelu(wave.cuda(), w.cuda(), stats, gamma.cuda(), beta.cuda(), out, 10, 5, k1, s1, 1e-5)
    act = w2v_ref.gelu_erf((raw - mean) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double())
    want = w2v_ref.window(act.to(BF16).double(), k1, s1)
    err = l2_rel(out.cpu(), want)
    print(f"conv0 norm+gelu window form: rel L2 {err:.3e} (bound {BOUND_A})")
    assert not torch.isnan(out).any() and err <= BOUND_A


@pytest.mark.parametrize("N,T,groups,cg,k", [(2, 499, 16, 48, 128), (3, 199, 4, 64, 16), (2, 77, 4, 48, 15), (1, 130, 2, 16, 5)])
def test_posconv_against_float64(N, T, groups, cg, k):
    lib = _lib()
    C = groups * cg
    g = torch.Generator().manual_seed(T + k)
    x = torch.randn(N, T, C, generator=g).to(BF16)
    w = (torch.randn(C, cg, k, generator=g) * math.sqrt(2.0 / (cg * k))).to(BF16)
    bias = 0.1 * torch.randn(C, generator=g)
    Kp = (k * cg + 31) // 32 * 32
    packed = torch.zeros(C, Kp, dtype=BF16)
    packed[:, :k * cg] = w.permute(0, 2, 1).reshape(C, k * cg)
    y = torch.full((N, T, C), float("nan"), dtype=BF16, device="cuda")
    lib.w2v_posconv(x.cuda(), packed.cuda(), bias.cuda(), y, N, T, C, groups, k)
    xd = x.double()
    want = xd + w2v_ref.gelu_erf(w2v_ref.pos_conv(xd, w.double(), bias.double(), groups))
    ref_conv = torch.nn.functional.conv1d(xd.transpose(1, 2), w.double(), bias.double(), padding=k // 2, groups=groups)[:, :, :T]
    assert l2_rel(w2v_ref.pos_conv(xd, w.double(), bias.double(), groups), ref_conv.transpose(1, 2)) < 1e-12
    got = y.cpu().double()
    h = k // 2
    edge = torch.cat([torch.arange(0, h), torch.arange(T - h, T)])
    err, err_edge = l2_rel(got, want), l2_rel(got[:, edge], want[:, edge])
    print(f"posconv cg={cg} k={k} T={T}: rel L2 {err:.3e}, boundary frames {err_edge:.3e} (bound {BOUND_A})")
    assert not torch.isnan(got).any() and err <= BOUND_A and err_edge <= BOUND_A


def test_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    nan32 = torch.full((1 << 14,), float("nan"), device="cuda")
    f = torch.zeros(1 << 14, device="cuda")
    b = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    cases = [
        ("mmf_w2v_gelu_window", lambda: L.mmf_w2v_gelu_window(p(b), p(nan16), 1, 40, 60, 3, 2, s), E_UNSUPPORTED),
        ("mmf_w2v_gelu_window", lambda: L.mmf_w2v_gelu_window(p(b), p(nan16), 1, 2, 64, 3, 2, s), E_SHAPE),
        ("mmf_w2v_gelu_window", lambda: L.mmf_w2v_gelu_window(p(b, 2), p(nan16), 1, 40, 64, 3, 2, s), E_ALIGN),
        ("mmf_w2v_gelu_window", lambda: L.mmf_w2v_gelu_window(None, p(nan16), 1, 40, 64, 3, 2, s), E_SHAPE),
        ("mmf_w2v_conv0_stats", lambda: L.mmf_w2v_conv0_stats(p(f), p(f), p(nan32), p(f), 1, 400, 60, 10, 5, s), E_UNSUPPORTED),
        ("mmf_w2v_conv0_stats", lambda: L.mmf_w2v_conv0_stats(p(f), p(f), p(nan32), p(f), 1, 8, 64, 10, 5, s), E_SHAPE),
        ("mmf_w2v_conv0_stats", lambda: L.mmf_w2v_conv0_stats(p(f), p(f), p(nan32, 4), p(f), 1, 400, 64, 10, 5, s), E_ALIGN),
        ("mmf_w2v_conv0_norm_gelu", lambda: L.mmf_w2v_conv0_norm_gelu(p(f), p(f), p(f), p(f), p(f), p(nan16), 1, 400, 64, 17, 5, 3, 2, 1e-5, s), E_UNSUPPORTED),
        ("mmf_w2v_conv0_norm_gelu", lambda: L.mmf_w2v_conv0_norm_gelu(p(f), p(f), p(f), p(f), p(f), p(nan16), 1, 400, 64, 10, 5, 0, 2, 1e-5, s), E_SHAPE),
        ("mmf_w2v_conv0_norm_gelu", lambda: L.mmf_w2v_conv0_norm_gelu(p(f), p(f), p(f), p(f), p(f), p(nan16, 2), 1, 400, 64, 10, 5, 3, 2, 1e-5, s), E_ALIGN),
        ("mmf_w2v_posconv", lambda: L.mmf_w2v_posconv(p(b), p(b), p(f), p(nan16), 1, 20, 96, 4, 16, s), E_UNSUPPORTED),      # cg 24
        ("mmf_w2v_posconv", lambda: L.mmf_w2v_posconv(p(b), p(b), p(f), p(nan16), 1, 20, 128, 2, 512, s), E_UNSUPPORTED),    # LDS
        ("mmf_w2v_posconv", lambda: L.mmf_w2v_posconv(p(b), p(b), p(f), p(nan16), 1, 20, 100, 3, 16, s), E_SHAPE),
        ("mmf_w2v_posconv", lambda: L.mmf_w2v_posconv(p(b), p(b), p(f, 4), p(nan16), 1, 20, 128, 2, 16, s), E_ALIGN),
    ]
    for name, call, want in cases:
        rc = call()
        assert rc == want, (name, rc, want)
        assert name.encode() in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all())            # nothing was launched


# ---- module ------------------------------------------------------------------------------------------------
def _setup(which: str, n: int, L: int, seed: int = 21, chunk=None):
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg = w2v_ref.tiny_config() if which == "tiny" else w2v_ref.base_config()
    sd = w2v_ref.seeded_weights(cfg, seed=seed)
    kw = w2v_ref.config_kwargs(cfg)
    if chunk is not None:
        kw["chunk"] = chunk
    m = NativeWav2Vec2(**kw)
    m.load_state_dict(sd)
    x = 0.5 * torch.randn(n, L, generator=torch.Generator().manual_seed(seed + 1)) + 0.1
    return cfg, sd, m.cuda().eval(), x


def _check_against_restatement(which, n, L, dt, both_bounds=True):
    cfg, sd, m, x = _setup(which, n, L)
    stored = w2v_ref.w2v_forward(sd, x, cfg, bf16_storage=True, dtype=dt)
    got = m(x.cuda()).last_hidden_state
    assert got.dtype == torch.float32 and got.shape == stored.shape and not got.requires_grad
    a = l2_rel(got, stored)
    print(f"NativeWav2Vec2 {which} {n} x {L}: (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A})")
    assert a <= BOUND_A
    if both_bounds:
        exact = w2v_ref.w2v_forward(sd, x, cfg, dtype=dt)
        model_err = l2_rel(stored, exact)
        b = l2_rel(got, exact)
        print(f"    (b) vs exact restatement {b:.3e} (bound {2 * model_err:.3e})")
        assert b <= 2 * model_err


def test_forward_against_restatement_tiny():
    _check_against_restatement("tiny", 3, 4000, torch.float64)


def test_forward_against_restatement_base():
    _check_against_restatement("base", 2, 16000, torch.float32)


def test_forward_base_at_the_real_clip_length():
    """One 10 s clip (160000 samples -> 499 frames) against the fp32 restatement with bf16 storage, bound (a).  On the CPU the
    bf16-storage restatement itself is 9.4e-3 from the fp32 one at this length (seed 21), inside bound (a)."""
    _check_against_restatement("base", 1, 160000, torch.float32, both_bounds=False)


def test_chunking_repeatability_and_workspace():
    cfg, sd, m2, x = _setup("tiny", 5, 4000, chunk=2)
    _, _, m5, _ = _setup("tiny", 5, 4000, chunk=5)
    xd = x.cuda()
    f2, f5 = m2(xd).last_hidden_state, m5(xd).last_hidden_state
    assert l2_rel(f2, f5) <= BOUND_A
    assert torch.equal(m2(xd).last_hidden_state, f2) and torch.equal(m5(xd).last_hidden_state, f5)
    T = m2.frames(4000)
    assert m2._ws["x"].numel() == 2 * T * cfg.hidden_size and m5._ws["x"].numel() == 5 * T * cfg.hidden_size
    held = sum(v.numel() * v.element_size() for v in m2._ws.values() if isinstance(v, torch.Tensor))
    assert held == 2 * m2.workspace_bytes_per_clip(4000)
    with pytest.raises(ValueError, match="receptive field"):
        m2(torch.zeros(1, 20, device="cuda"))
    with pytest.raises(TypeError):
        m2(xd.double())


def test_forward_replays_from_a_captured_graph():
    cfg, sd, m, x = _setup("tiny", 3, 4000, chunk=2)
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
    static.copy_(torch.randn_like(static))
    graph.replay()
    other = out.clone()
    static.copy_(xd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert not torch.equal(other, eager)


def test_load_state_dict_refreshes_what_the_kernels_read():
    cfg, sd, m, x = _setup("tiny", 2, 4000)
    xd = x.cuda()
    first = m(xd).last_hidden_state.clone()
    sd2 = w2v_ref.seeded_weights(cfg, seed=99)
    m.load_state_dict(sd2)
    second = m(xd).last_hidden_state.clone()
    want = w2v_ref.w2v_forward(sd2, x, cfg, bf16_storage=True)
    assert l2_rel(second, want) <= BOUND_A and l2_rel(first, want) > 10 * BOUND_A
    # a second weight-norm gain alone: the folded positional weight follows it
    sd3 = dict(sd2)
    sd3[w2v_ref.WN_NEW[0]] = sd2[w2v_ref.WN_NEW[0]] * torch.linspace(0.2, 3.0, cfg.num_conv_pos_embeddings).view(1, 1, -1)
    m.load_state_dict(sd3)
    third = m(xd).last_hidden_state
    want3 = w2v_ref.w2v_forward(sd3, x, cfg, bf16_storage=True)
    moved = l2_rel(want3, want)
    print(f"new weight-norm gain: restatement moved by {moved:.3e}; native vs new {l2_rel(third, want3):.3e}, vs old {l2_rel(third, want):.3e}")
    assert l2_rel(third, want3) <= BOUND_A and moved > 3 * BOUND_A and l2_rel(third, want) > BOUND_A


def test_fp32_parity_mode_is_refused():
    from mmfusion import ops
    cfg, sd, m, x = _setup("tiny", 1, 4000)
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match="bf16 storage only"):
            m(x.cuda())
    finally:
        ops.set_precision(old)


def test_huggingface_state_dict_to_native_output():
    transformers = pytest.importorskip("transformers")
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg = w2v_ref.tiny_config()
    hf = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**w2v_ref.config_kwargs(cfg))).eval()
    hf.load_state_dict(w2v_ref.seeded_weights(cfg, seed=41))
    sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    m = NativeWav2Vec2(**w2v_ref.config_kwargs(cfg))
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = 0.5 * torch.randn(3, 4000, generator=torch.Generator().manual_seed(42))
    with torch.no_grad():
        want = hf(x).last_hidden_state
    model_err = l2_rel(w2v_ref.w2v_forward(sd, x, cfg, bf16_storage=True), w2v_ref.w2v_forward(sd, x, cfg))
    err = l2_rel(m(x.cuda()).last_hidden_state, want)
    print(f"NativeWav2Vec2 vs HuggingFace fp32 (tiny): {err:.3e} (bound {2 * model_err:.3e})")
    assert err <= 2 * model_err


def test_audio_encoder_native_backbone_against_reference_backbone():
    """``config.audio_backbone = "native"`` against the same encoder given the restatement as its ``backbone=``; the tail
    (temporal attention, projection) is the same HIP code on both sides.  Tolerance: tests/test_encoders_gpu.py's 1e-2 scaled
    by max(1, |want|max)."""
    import config as cfgmod
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 768     # the tail's 8 heads need a head_dim of 64 / 96
    cfg.audio_backbone = "native"
    cfg.audio_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=512, conv_dim=(256, 256, 256), conv_kernel=(10, 3, 2),
                                     conv_stride=(5, 2, 2), num_conv_pos_embeddings=16)
    torch.manual_seed(3)
    enc = AudioEncoder(cfg)
    wcfg = enc.model.config
    sd = w2v_ref.seeded_weights(wcfg, seed=31)
    enc.model.load_state_dict(sd)
    cfg_ref = cfgmod.ModelConfig()
    cfg_ref.fusion_hidden_size, cfg_ref.fusion_dropout = 256, 0.0
    ref = AudioEncoder(cfg_ref, backbone=w2v_ref.RefWav2Vec2(sd, wcfg))
    tail = {k: v for k, v in enc.state_dict().items() if not k.startswith("model.")}
    assert len(tail) < len(enc.state_dict()) and "model.encoder.layers.0.layer_norm.weight" in enc.state_dict()
    ref.load_state_dict(tail)
    wave = (0.5 * torch.randn(2, 4000, generator=torch.Generator().manual_seed(32))).cuda()
    enc, ref = enc.cuda().eval(), ref.cuda().eval()
    with torch.no_grad():
        got, want = enc(wave), ref(wave)
    for k in ("features", "sequence_output"):
        err = float((got[k] - want[k]).abs().max())
        scale = max(1.0, float(want[k].abs().max()))
        print(f"AudioEncoder native vs reference backbone, {k}: abs err {err:.3e} (scale {scale:.2f})")
        assert got[k].shape == want[k].shape and err <= 1e-2 * scale, k
