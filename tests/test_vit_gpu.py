"""GPU: the ViT streaming kernels (csrc/vit.hip) bit for bit / within one bf16 ulp, and ``mmfusion.vit.NativeViT`` against
the explicit restatement tests/vit_ref.py — which needs neither the reference nor transformers.

Bounds.  (a) against the restatement with bf16 storage: relative L2 <= 2e-2, the project's bound for a kernel against an
oracle with the same storage format.  (b) against the fp32 restatement: 2 x the error of the bf16-storage restatement
against the fp32 one on the same inputs, computed here on the CPU — the error of an L-layer bf16 residual stream is modelled
by the storage format, not by the code under test, with a factor 2 for summation order."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gelu_domain  # noqa: E402
import vit_ref  # noqa: E402
from helpers import BOUND_A, _lib, l2_rel  # noqa: E402

BF16 = torch.bfloat16


# ---- kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W,P", [(3, 3, 64, 64, 16), (2, 3, 224, 224, 16), (5, 1, 48, 80, 8), (1, 2, 96, 32, 32)])
def test_patchify_is_unfold_with_one_rounding(N, C, H, W, P):
    lib = _lib()
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(N + H)).cuda()
    out = torch.full((N * (H // P) * (W // P), C * P * P), float("nan"), dtype=BF16, device="cuda")
    lib.vit_patchify(x, out, N, C, H, W, P)
    want = vit_ref.patchify(x.cpu(), P).to(BF16)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    unfold = torch.nn.functional.unfold(x.cpu(), kernel_size=P, stride=P).transpose(1, 2).reshape(-1, C * P * P).to(BF16)
    assert torch.equal(want.view(torch.int16), unfold.view(torch.int16))


def test_patchify_refuses_unsupported_shapes():
    lib = _lib()
    L = lib.load()
    x = torch.zeros(1, 3, 60, 64, device="cuda")
    out = torch.zeros(3 * 60 * 64, dtype=BF16, device="cuda")
    for (H, W, P) in ((60, 64, 16), (64, 60, 16), (64, 64, 12), (60, 60, 12)):
        rc = L.mmf_vit_patchify(x.data_ptr(), out.data_ptr(), 1, 3, H, W, P, lib.stream_ptr())
        assert rc == -5 and b"mmf_vit_patchify" in L.mmf_last_error()               # MMF_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(out.float().abs().max()) == 0.0                                      # nothing was launched


@pytest.mark.parametrize("N,T,d", [(3, 17, 256), (2, 197, 768), (7, 5, 8)])
def test_embed_tokens_is_f32_add_with_one_rounding(N, T, d):
    lib = _lib()
    g = torch.Generator().manual_seed(T)
    pe = torch.randn(N * (T - 1), d, generator=g).to(BF16)
    cls, pos = torch.randn(d, generator=g), torch.randn(T, d, generator=g)
    tok = torch.full((N * T, d), float("nan"), dtype=BF16, device="cuda")
    lib.vit_embed_tokens(pe.cuda(), cls.cuda(), pos.cuda(), tok, N, T, d)
    want = (torch.cat([cls.expand(N, 1, d), pe.float().view(N, T - 1, d)], dim=1) + pos).to(BF16).view(N * T, d)
    assert torch.equal(tok.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("rows,cols,ld,bias", [(37, 1024, 1024, True), (301, 72, 128, True), (5, 3072, 3080, False)])
def test_bias_gelu_within_one_bf16_ulp_of_f32_erf_gelu(rows, cols, ld, bias):
    """A grid over |x| <= 8 with both zeros, a row count that is no multiple of the 256-lane block, a row stride above
    the row.  The reference is float64 and the bound the allowance of tests/gelu_domain.py (half a bf16 ulp for the store,
    2^-14 of the value for the f32 formula, the flush floor): the kernel forms Phi through erfc, so the left tail holds
    it too.  v is the f32 sum the kernel forms, restated exactly."""
    lib = _lib()
    n = rows * cols
    grid = torch.linspace(-8.0, 8.0, n - 2, dtype=torch.float64).float()
    vals = torch.cat([grid, torch.tensor([0.0, -0.0])])[torch.randperm(n, generator=torch.Generator().manual_seed(rows))]
    buf = torch.full((rows, ld), 777.0, dtype=BF16)
    buf[:, :cols] = vals.view(rows, cols).to(BF16)
    b = 0.25 * torch.randn(cols, generator=torch.Generator().manual_seed(cols)) if bias else None
    dev = buf.cuda()
    lib.bias_gelu(dev[:, :cols], b.cuda() if bias else None)
    got = dev.cpu()
    assert torch.equal(got[:, cols:], buf[:, cols:])                                   # the padding columns are untouched
    v = buf[:, :cols].float() + b if bias else buf[:, :cols].float()
    worst = float(gelu_domain.ratio_fwd(got[:, :cols], v).max())
    print(f"bias_gelu rows={rows} cols={cols} ld={ld}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    if not bias:
        z = got[:, :cols][buf[:, :cols] == 0]
        assert z.numel() >= 2 and float(z.float().abs().max()) == 0.0


def test_bias_gelu_refuses_unsupported_shapes():
    lib = _lib()
    L = lib.load()
    x = torch.zeros(4, 64, dtype=BF16, device="cuda")
    assert L.mmf_bias_gelu_bf16(x.data_ptr(), None, 4, 60, 64, lib.stream_ptr()) == -5
    assert L.mmf_bias_gelu_bf16(x.data_ptr(), None, 4, 64, 60, lib.stream_ptr()) == -5
    assert b"mmf_bias_gelu_bf16" in L.mmf_last_error()


# ---- module ------------------------------------------------------------------------------------------------
def _setup(which: str, n_images: int, seed: int = 21, chunk=None):
    from mmfusion.vit import NativeViT
    cfg = vit_ref.tiny_config() if which == "tiny" else vit_ref.base_config()
    sd = vit_ref.seeded_weights(cfg, seed=seed)
    kw = vit_ref.config_kwargs(cfg)
    if chunk is not None:
        kw["chunk"] = chunk
    m = NativeViT(**kw)
    m.load_state_dict(sd)
    x = torch.rand(n_images, cfg.num_channels, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(seed + 1))
    return cfg, sd, m.cuda().eval(), x


@pytest.mark.parametrize("which", ["tiny", "base"])
def test_forward_and_cls_features_against_restatement(which):
    cfg, sd, m, x = _setup(which, 4)
    dt = torch.float64 if which == "tiny" else torch.float32
    exact = vit_ref.vit_forward(sd, x, cfg, dtype=dt)
    stored = vit_ref.vit_forward(sd, x, cfg, bf16_storage=True, dtype=dt)
    model_err = l2_rel(stored, exact)
    model_err_cls = l2_rel(stored[:, 0], exact[:, 0])
    full = m(x.cuda()).last_hidden_state
    cls = m.cls_features(x.cuda())
    assert full.dtype == torch.float32 and full.shape == exact.shape and cls.shape == (4, cfg.hidden_size)
    assert not full.requires_grad and not cls.requires_grad
    a_full, a_cls = l2_rel(full, stored), l2_rel(cls, stored[:, 0])
    b_full, b_cls = l2_rel(full, exact), l2_rel(cls, exact[:, 0])
    both = l2_rel(cls, full[:, 0])
    print(f"NativeViT {which}: (a) vs bf16-storage restatement: forward {a_full:.3e}, cls_features {a_cls:.3e} (bound {BOUND_A}); "
          f"(b) vs fp32 restatement: forward {b_full:.3e} (bound {2 * model_err:.3e}), cls_features {b_cls:.3e} "
          f"(bound {2 * model_err_cls:.3e}); cls_features vs forward[:, 0] {both:.3e}")
    assert a_full <= BOUND_A and a_cls <= BOUND_A
    assert b_full <= 2 * model_err and b_cls <= 2 * model_err_cls
    assert both <= BOUND_A


def test_chunking_and_repeatability():
    cfg, sd, m2, x = _setup("tiny", 5, chunk=2)
    _, _, m5, _ = _setup("tiny", 5, chunk=5)
    xd = x.cuda()
    f2, f5 = m2(xd).last_hidden_state, m5(xd).last_hidden_state
    c2, c5 = m2.cls_features(xd), m5.cls_features(xd)
    assert l2_rel(f2, f5) <= BOUND_A and l2_rel(c2, c5) <= BOUND_A
    assert torch.equal(m2(xd).last_hidden_state, f2) and torch.equal(m2.cls_features(xd), c2)
    assert torch.equal(m5(xd).last_hidden_state, f5) and torch.equal(m5.cls_features(xd), c5)
    assert m2._ws["x"].numel() == 2 * m2.T * cfg.hidden_size                           # the workspace is the chunk's, not the batch's


def test_cls_features_replays_from_a_captured_graph():
    cfg, sd, m, x = _setup("tiny", 5, chunk=2)
    xd = x.cuda()
    eager = m.cls_features(xd).clone()
    static = xd.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.cls_features(static)                                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.cls_features(static)
    static.copy_(torch.rand_like(static))
    graph.replay()
    other = out.clone()
    static.copy_(xd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert not torch.equal(other, eager)


def test_load_state_dict_refreshes_what_the_kernels_read():
    cfg, sd, m, x = _setup("tiny", 2)
    xd = x.cuda()
    first = m.cls_features(xd).clone()
    sd2 = vit_ref.seeded_weights(cfg, seed=99)
    m.load_state_dict(sd2)
    second = m.cls_features(xd)
    want = vit_ref.vit_forward(sd2, x, cfg, bf16_storage=True, dtype=torch.float64)[:, 0]
    assert l2_rel(second, want) <= BOUND_A and l2_rel(first, want) > 10 * BOUND_A


def test_fp32_parity_mode_is_refused():
    from mmfusion import ops
    cfg, sd, m, x = _setup("tiny", 1)
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match="bf16 storage only"):
            m(x.cuda())
    finally:
        ops.set_precision(old)


def test_video_encoder_native_backbone_against_reference_backbone():
    """``config.video_backbone = "native"`` against the same encoder given the restatement as its ``backbone=``; the tail
    (BiLSTM, facial attention, projection) is the same HIP code on both sides.  Tolerance: tests/test_encoders_gpu.py's
    1e-2 scaled by max(1, |want|max)."""
    import config as cfgmod
    from models.encoders import VideoEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout = 256, 0.0
    cfg.video_hidden_size, cfg.video_frame_size = 768, (64, 64)
    cfg.video_backbone = "native"
    cfg.video_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=1024)
    torch.manual_seed(3)
    enc = VideoEncoder(cfg)
    vcfg = enc.vit.config
    sd = vit_ref.seeded_weights(vcfg, seed=31)
    enc.vit.load_state_dict(sd)
    cfg_ref = cfgmod.ModelConfig()
    cfg_ref.fusion_hidden_size, cfg_ref.fusion_dropout = 256, 0.0
    ref = VideoEncoder(cfg_ref, backbone=vit_ref.RefViT(sd, vcfg))
    tail = {k: v for k, v in enc.state_dict().items() if not k.startswith("vit.")}
    assert len(tail) < len(enc.state_dict()) and "vit.layers.0.mlp.fc1.weight" in enc.state_dict()
    ref.load_state_dict(tail)
    frames = torch.rand(2, 6, 3, 64, 64, generator=torch.Generator().manual_seed(32)).cuda()
    enc, ref = enc.cuda().eval(), ref.cuda().eval()
    with torch.no_grad():
        got, want = enc(frames), ref(frames)
    for k in ("features", "sequence_output"):
        err = float((got[k] - want[k]).abs().max())
        scale = max(1.0, float(want[k].abs().max()))
        print(f"VideoEncoder native vs reference backbone, {k}: abs err {err:.3e} (scale {scale:.2f})")
        assert got[k].shape == want[k].shape and err <= 1e-2 * scale, k


def test_huggingface_state_dict_to_native_output():
    transformers = pytest.importorskip("transformers")
    cfg = vit_ref.tiny_config()
    hf = transformers.ViTModel(transformers.ViTConfig(**vit_ref.config_kwargs(cfg))).eval()
    hf.load_state_dict(vit_ref.seeded_weights(cfg, seed=41))
    sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    from mmfusion.vit import NativeViT
    m = NativeViT(**vit_ref.config_kwargs(cfg))
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(42))
    with torch.no_grad():
        want = hf(pixel_values=x).last_hidden_state
    model_err = l2_rel(vit_ref.vit_forward(sd, x, cfg, bf16_storage=True, dtype=torch.float64), vit_ref.vit_forward(sd, x, cfg))
    got = m(x.cuda()).last_hidden_state
    err = l2_rel(got, want)
    print(f"NativeViT vs HuggingFace fp32 (tiny): {err:.3e} (bound {2 * model_err:.3e})")
    assert err <= 2 * model_err
