"""GPU: fine-tuning the native ViT.  The weight gradients of ``NativeViT.set_trainable_layers(k[, embeddings=True])`` on both
routes (``forward`` and ``cls_features``, whose last layer runs, forward and backward, for the CLS rows only) against float64
autograd through the restatement tests/vit_ref.py, the arena's accumulation protocol, both input kinds, graph capture, and the
optimiser step through ``VideoEncoder``.

Bounds.  Rule (b) per parameter tensor in absolute form, ||got - exact|| <= 2 ||stored - exact||, ``exact`` / ``stored`` the
autograd gradients of ``vit_ref.vit_forward`` without / with ``bf16_storage`` on the state dict's tensors as leaves (tests/
test_deberta_finetune_gpu.py's rule and helpers); both sides are computed here and printed per tensor.  The key bias is the one
tensor held to something else: its exact gradient is zero (tests/test_vit_finetune_cpu.py) and the backward adds nothing to it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vit_ref  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402
from test_deberta_finetune_gpu import _frozen_grads_are_empty, _hf_grads, _rule_b  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402

_EMB = ("embeddings.cls_token", "embeddings.position_embeddings", "embeddings.patch_embeddings.projection.weight",
        "embeddings.patch_embeddings.projection.bias")
_ref_cache = {}


def _cfg(which):
    cfg = vit_ref.base_config() if which == "base" else vit_ref.tiny_config()
    if which == "tiny192":                                  # T = 145: past one 128-row query chunk and two 64-key tiles, and odd
        cfg.image_size = 192
    return cfg


def _setup(which, n_images, seed=21, chunk=2):
    from mmfusion.vit import NativeViT
    cfg = _cfg(which)
    sd = vit_ref.seeded_weights(cfg, seed=seed)
    m = NativeViT(**{**vit_ref.config_kwargs(cfg), "chunk": chunk})
    m.load_state_dict(sd)
    x = torch.rand(n_images, cfg.num_channels, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(seed + 1))
    return cfg, sd, m.cuda().eval(), x


def _keys(cfg, k, embeddings=False):
    L = cfg.num_hidden_layers
    keys = [key for key in vit_ref.hf_keys(cfg) if any(key.startswith(f"layers.{i}.") for i in range(L - k, L))]
    return (list(_EMB) if embeddings else []) + keys + ["layernorm.weight", "layernorm.bias"]


def _ref_grads(tag, sd, x, cfg, dout, dtype, bf16_storage, keys, cls):
    """autograd through the restatement with the state dict's tensors as leaves of ``dtype`` -> {key: gradient}; kept per
    ``tag`` so that the tests that share a case compute it once"""
    key_ = (tag, str(dtype), bf16_storage, cls, tuple(keys))
    if key_ not in _ref_cache:
        leaves = {key: v.to(dtype).clone().requires_grad_(key in keys) for key, v in sd.items()}
        out = vit_ref.vit_forward(leaves, x.to(dtype), cfg, bf16_storage=bf16_storage, dtype=dtype, cls_last_only=cls)
        _ref_cache[key_] = dict(zip(keys, torch.autograd.grad(out, [leaves[key] for key in keys], dout.to(dtype))))
    return _ref_cache[key_]


def _native_grads(m, x, dout, keys, cls, zero=True, aug=None):
    from mmfusion import arena
    ar = arena.ensure(m)
    if zero:
        ar.zero_grad()
    out = m.cls_features(x, aug=aug) if cls else m(x, aug=aug).last_hidden_state
    assert out.requires_grad and out.dtype == torch.float32
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    return _hf_grads(m, keys), out.detach()


def _douts(cfg, n, T, cls, seed):
    """a random gradient of the result and, for the full route, one that is non-zero on row 0 of each image only"""
    g = torch.Generator().manual_seed(seed)
    if cls:
        return [("random", torch.randn(n, cfg.hidden_size, generator=g))]
    dout = torch.randn(n, T, cfg.hidden_size, generator=g)
    row0 = torch.zeros_like(dout)
    row0[:, 0] = dout[:, 0]
    return [("random", dout), ("CLS-row", row0)]


def _without_key_bias(keys):
    return [k for k in keys if not k.endswith("k_proj.bias")]


def _check_key_bias(m, keys):
    for key in keys:
        if key.endswith("k_proj.bias"):
            name, rows, _ = m._hf[key]
            assert not bool(getattr(m, name).grad[rows[0]:rows[1]].any()), f"{key} received a gradient"


@pytest.mark.parametrize("cls", [False, True], ids=["forward", "cls_features"])
@pytest.mark.parametrize("k,emb", [(1, False), (2, False), (2, True)], ids=["k1", "k2", "all"])
@pytest.mark.parametrize("which", ["tiny", "tiny192"])
def test_weight_gradients_against_float64_autograd(which, k, emb, cls):
    """2 layers, d 256, 4 heads; 3 images in chunks of 2"""
    cfg, sd, m, x = _setup(which, 3)
    T = m.T
    with torch.no_grad():
        plain = (m.cls_features(x.cuda()) if cls else m(x.cuda()).last_hidden_state).clone()
    m.set_trainable_layers(k, embeddings=emb)
    keys = _keys(cfg, k, emb)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted({m._hf[key][0] for key in keys})
    for tag, dout in _douts(cfg, 3, T, cls, 51):
        case = (which, cls, tag)
        exact = _ref_grads(case, sd, x, cfg, dout, torch.float64, False, keys, cls)
        stored = _ref_grads(case, sd, x, cfg, dout, torch.float64, True, keys, cls)
        got, out = _native_grads(m, x.cuda(), dout, keys, cls)
        assert torch.equal(_bits(out), _bits(plain)), "the differentiable forward's bits are not the inference call's"
        kept = _without_key_bias(keys)
        _rule_b(f"NativeViT {which} 3 images, k={k}{' + embeddings' if emb else ''}, {'cls_features' if cls else 'forward'}, {tag} dO,",
                {key: got[key] for key in kept}, {key: exact[key] for key in kept}, {key: stored[key] for key in kept})
        _check_key_bias(m, keys)
        _frozen_grads_are_empty(m)


def test_weight_gradients_against_autograd_base_sizes():
    """ViT-base sizes (12 layers, d 768, 12 heads, T 197: the real GEMM shapes and the LayerNorm lane form), 2 images through
    ``cls_features``, the top layer trainable, float32 references.  The worst error / bound is in profiles/vit_finetune.txt.

    The case that pins ``mmf_vit_cls_attn_bwd``: with the CLS query's attention backward on ``mmf_attn_bwd_grouped`` (``Tq = 1``)
    ``q_proj.weight`` was 0.861 from the exact gradient against a bound of 0.230 (3.74 of it), ``q_proj.bias`` 3.85 and
    ``k_proj.weight`` 4.08 of theirs.  That kernel takes delta = dO . O from the bf16 O, so a row of dS sums to
    dO . (O - bf16(O)) instead of zero, and with these weights the CLS row's exact dQ / dK are small (||d q_proj.weight|| 3.0 beside
    269 for v_proj): the residue was 29 % of them (the float64 restatement with that one change gives 0.62, the storage model 0.11).
    With delta = sum_j p_j dp_j all seventeen tensors are at 0.49 to 0.55 of their bounds."""
    cfg, sd, m, x = _setup("base", 2, chunk=2)
    m.set_trainable_layers(1)
    keys = _keys(cfg, 1)
    (_, dout), = _douts(cfg, 2, m.T, True, 53)
    exact = _ref_grads("base", sd, x, cfg, dout, torch.float32, False, keys, True)
    stored = _ref_grads("base", sd, x, cfg, dout, torch.float32, True, keys, True)
    got, _ = _native_grads(m, x.cuda(), dout, keys, True)
    kept = _without_key_bias(keys)
    _rule_b("NativeViT base 2 images, k=1, cls_features,", {key: got[key] for key in kept}, {key: exact[key] for key in kept},
            {key: stored[key] for key in kept})
    _check_key_bias(m, keys)
    _frozen_grads_are_empty(m)


@pytest.mark.parametrize("cls", [False, True], ids=["forward", "cls_features"])
def test_frames_with_an_aug_give_the_pixel_routes_gradients(cls):
    """uint8 frames with an ``aug`` against the f32 pixels ``prepare_video`` makes of them: the patch matrices are bit-equal, so
    every gradient is, the patch projection's (whose backward rebuilds the patch matrix) included.  Bit for bit but for the
    LayerNorm parameters: ``mmf_layernorm_bwd_grouped``'s finalize pass adds the workgroups' column sums with one f32 atomic per
    slice, in the order the slices arrive, so the last bits of a dgamma / dbeta differ between two runs of the SAME call (measured:
    ``layers.0.layernorm_before.weight`` differed between the two routes, whose inputs to that launch are bit-equal); those are
    held to ``F32_TOL``, the bound of a change of summation order"""
    from mmfusion import prep
    cfg, sd, m, _ = _setup("tiny", 3)
    g = torch.Generator().manual_seed(7)
    frames = torch.randint(0, 256, (3, 48, 80, 3), generator=g, dtype=torch.uint8).cuda()
    aug = prep.VideoAug(bgr=True, brightness=torch.tensor([1.1, 0.9, 1.0]).cuda(), flip=torch.tensor([1, 0, 1], dtype=torch.uint8).cuda())
    pixels = prep.prepare_video(frames, (cfg.image_size, cfg.image_size), bgr=aug.bgr, live=aug.live, brightness=aug.brightness, flip=aug.flip)
    L = cfg.num_hidden_layers
    m.set_trainable_layers(L, embeddings=True)
    keys = _keys(cfg, L, True)
    (_, dout), *_ = _douts(cfg, 3, m.T, cls, 57)
    a, out_a = _native_grads(m, frames, dout, keys, cls, aug=aug)
    b, out_b = _native_grads(m, pixels, dout, keys, cls)
    assert torch.equal(_bits(out_a), _bits(out_b))
    for key in keys:
        if "layernorm" in key:
            assert l2_rel(a[key], b[key]) <= F32_TOL, key
        else:
            assert torch.equal(_bits(a[key]), _bits(b[key])), key
    assert float(a["embeddings.patch_embeddings.projection.weight"].norm()) > 0


def test_chunking_changes_only_the_summation_order():
    got = {}
    for chunk in (2, 3):
        cfg, sd, m, x = _setup("tiny", 3, chunk=chunk)
        L = cfg.num_hidden_layers
        m.set_trainable_layers(L, embeddings=True)
        keys = _without_key_bias(_keys(cfg, L, True))
        (_, dout), *_ = _douts(cfg, 3, m.T, True, 58)
        got[chunk], _ = _native_grads(m, x.cuda(), dout, keys, True)
    for key in keys:
        e = l2_rel(got[2][key], got[3][key])
        print(f"chunk 2 vs chunk 3, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key


def test_gradients_accumulate_and_honour_the_lazy_zero_protocol():
    from mmfusion import arena
    cfg, sd, m, x = _setup("tiny", 3)
    L = cfg.num_hidden_layers
    m.set_trainable_layers(L, embeddings=True)
    keys = _without_key_bias(_keys(cfg, L, True))
    (_, dout), *_ = _douts(cfg, 3, m.T, True, 60)
    once, _ = _native_grads(m, x.cuda(), dout, keys, True)
    twice, _ = _native_grads(m, x.cuda(), dout, keys, True, zero=False)
    for key in keys:
        e = l2_rel(twice[key], 2 * once[key])
        print(f"two backwards vs 2 x one, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    ar = arena.ensure(m)
    ar.zero_grad(lazy=True)
    _native_grads(m, x.cuda(), dout, keys, True, zero=False)
    ar.finalize_grads()
    torch.cuda.synchronize()
    again = _hf_grads(m, keys)
    for key in keys:
        e = l2_rel(again[key], once[key])
        print(f"after zero_grad(lazy=True), {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    _frozen_grads_are_empty(m)


def test_forward_and_backward_replay_from_a_captured_graph():
    from mmfusion import arena
    cfg, sd, m, x = _setup("tiny", 3)
    m.set_trainable_layers(1)
    keys = _without_key_bias(_keys(cfg, 1))
    (_, dout), *_ = _douts(cfg, 3, m.T, True, 63)
    eager, _ = _native_grads(m, x.cuda(), dout, keys, True)
    ar = arena.ensure(m)
    static, dO = x.cuda().clone(), dout.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        m.cls_features(static).backward(dO)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.cls_features(static).backward(dO)
    with torch.no_grad():
        static.copy_(torch.rand_like(static))
    ar.zero_grad()
    graph.replay()
    torch.cuda.synchronize()
    other = _hf_grads(m, keys)
    with torch.no_grad():
        static.copy_(x.cuda())
    ar.zero_grad()
    graph.replay()
    torch.cuda.synchronize()
    got = _hf_grads(m, keys)
    for key in keys:
        e = l2_rel(got[key], eager[key])
        print(f"captured forward + backward, {key}: rel L2 vs eager {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    assert any(l2_rel(other[key], eager[key]) > 1e-2 for key in keys)


def test_video_encoder_steps_the_trainable_layer_and_serves_the_new_weights():
    import config as cfgmod
    from mmfusion import arena
    from mmfusion.train import finetune_optimizer
    from models.encoders import VideoEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout = 256, 0.0
    cfg.video_hidden_size, cfg.video_frame_size = 768, (64, 64)          # (the facial attention's 8 heads need a head_dim of 96)
    cfg.video_backbone = "native"
    cfg.video_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=1024)
    cfg.video_backbone_trainable_layers = 1
    torch.manual_seed(3)
    enc = VideoEncoder(cfg)
    vcfg = enc.vit.config
    assert enc.vit.trainable_layers == 1
    enc.vit.load_state_dict(vit_ref.seeded_weights(vcfg, seed=31))
    enc = enc.cuda().train()
    frames = torch.rand(2, 3, 3, 64, 64, generator=torch.Generator().manual_seed(32)).cuda()
    flat = frames.reshape(-1, 3, 64, 64)
    ar = arena.ensure(enc)
    opt = finetune_optimizer(enc, ar, lr=1e-2, weight_decay=0.01)
    with torch.no_grad():
        first = enc.vit.cls_features(flat).clone()
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    before_sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    for _ in range(2):
        ar.zero_grad()
        feats = enc(frames)["features"]
        assert feats.requires_grad
        feats.sum().backward()
        opt.advance()
        opt.launch()
    torch.cuda.synchronize()
    trainable = sorted(enc.vit._layer_params(vcfg.num_hidden_layers - 1) + ["ln_w", "ln_b"])
    assert sorted(n for n, p in enc.vit.named_parameters() if p.requires_grad) == trainable
    for n, p in enc.named_parameters():
        same = torch.equal(_bits(p.detach()), _bits(before[n]))
        if n.startswith("vit."):
            assert same != p.requires_grad, f"{n}: {'did not move' if same else 'is frozen and moved'}"
        elif not p.requires_grad:
            assert same, f"the frozen {n} moved"
    # what the kernels read now is the stepped weights
    sd = {k: v.detach().cpu().clone() for k, v in enc.vit.state_dict().items()}
    assert list(sd) == list(vit_ref.hf_keys(vcfg))
    with torch.no_grad():
        got = enc.vit.cls_features(flat)
    want = vit_ref.vit_forward(sd, flat.cpu(), vcfg, bf16_storage=True, dtype=torch.float64, cls_last_only=True)
    err, moved = l2_rel(got, want), l2_rel(got, first)
    print(f"VideoEncoder, 2 AdamW steps on the top layer: no_grad cls_features vs the restatement on the new state_dict {err:.3e} "
          f"(bound {BOUND_A}); the output moved by {moved:.3e}")
    assert err <= BOUND_A and moved > 3 * BOUND_A
    # frozen again under the old weights: the first output's bits
    enc.vit.load_state_dict({k[len("vit."):]: v for k, v in before_sd.items() if k.startswith("vit.")})
    enc.vit.set_trainable_layers(0)
    back = enc.vit.cls_features(flat)
    assert not back.requires_grad and torch.equal(_bits(back), _bits(first))


def test_refusals_and_the_frozen_default():
    from mmfusion import ops
    cfg, sd, m, x = _setup("tiny", 2)
    xd = x.cuda()
    assert m.trainable_layers == 0 and not any(p.requires_grad for p in m.parameters())
    out = m.cls_features(xd)                                                           # grad mode on, nothing trainable
    full = m(xd).last_hidden_state
    assert not out.requires_grad and not full.requires_grad
    m.set_trainable_layers(2)
    assert m.cls_features(xd).requires_grad and m(xd).last_hidden_state.requires_grad
    with torch.no_grad():
        assert not m.cls_features(xd).requires_grad
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match="bf16 storage only"):
            m.cls_features(xd)
    finally:
        ops.set_precision(old)
    m.set_trainable_layers(0)
    again, again_full = m.cls_features(xd), m(xd).last_hidden_state
    assert not again.requires_grad and torch.equal(again, out) and torch.equal(again_full, full)
    assert not any(p.requires_grad for p in m.parameters())
