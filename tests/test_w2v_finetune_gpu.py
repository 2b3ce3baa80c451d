"""GPU: fine-tuning the native Wav2Vec2.  The weight gradients of ``NativeWav2Vec2.set_trainable_layers(k[, front=True])`` against
float64 autograd through the restatement tests/w2v_ref.py, the arena's accumulation protocol, graph capture, and the optimiser
step through ``AudioEncoder``.

Bounds.  Rule (b) per parameter tensor in absolute form, ||got - exact|| <= 2 ||stored - exact||, ``exact`` / ``stored`` the
autograd gradients of ``w2v_ref.w2v_forward`` without / with ``bf16_storage`` on the state dict's tensors as leaves (tests/
test_deberta_finetune_gpu.py's rule and helpers); both sides are computed here and printed per tensor.  The rule is not degenerate
for any tensor of the front end, the weight norm's g / v and the feature projection included: tests/test_w2v_finetune_cpu.py
(``test_rule_b_is_not_degenerate_for_the_front_end``) measures ||stored - exact|| / ||exact|| between 1e-4 and 0.5 for each, so none
needs the fallback to BOUND_A.  The key bias is the one tensor held to something else: its exact gradient is zero (the same file)
and the backward adds nothing to it."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_ref  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402
from test_deberta_finetune_gpu import _frozen_grads_are_empty, _hf_grads, _rule_b  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402

_FRONT = ("feature_projection.", "encoder.pos_conv_embed.", "encoder.layer_norm.")
_ref_cache = {}


def wide_config():
    """d 768 in 12 heads and 16 positional groups (group width 48, the shipped form) of 15 taps (odd), 2 layers, the tiny conv stack"""
    return types.SimpleNamespace(hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=512,
                                 conv_dim=(256, 256, 256), conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2), conv_bias=False,
                                 num_conv_pos_embeddings=15, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
                                 feat_extract_norm="group", do_stable_layer_norm=False)


def _cfg(which):
    return {"tiny": w2v_ref.tiny_config, "wide": wide_config, "base": w2v_ref.base_config}[which]()


def _setup(which, n, L, seed=21, chunk=2):
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg = _cfg(which)
    sd = w2v_ref.seeded_weights(cfg, seed=seed)
    m = NativeWav2Vec2(**{**w2v_ref.config_kwargs(cfg), "chunk": chunk})
    m.load_state_dict(sd)
    x = 0.5 * torch.randn(n, L, generator=torch.Generator().manual_seed(seed + 1)) + 0.1
    return cfg, sd, m.cuda().eval(), x


def _keys(cfg, k, front=False):
    L = cfg.num_hidden_layers
    keys = [key for key in w2v_ref.hf_keys(cfg) if any(key.startswith(f"encoder.layers.{i}.") for i in range(L - k, L))]
    return ([key for key in w2v_ref.hf_keys(cfg) if key.startswith(_FRONT)] if front else []) + keys


def _ref_grads(tag, sd, x, cfg, dout, dtype, bf16_storage, keys):
    """autograd through the restatement with the state dict's tensors as leaves of ``dtype`` -> {key: gradient}; kept per ``tag``
    so that the tests that share a case compute it once"""
    key_ = (tag, str(dtype), bf16_storage, tuple(keys))
    if key_ not in _ref_cache:
        leaves = {key: v.to(dtype).clone().requires_grad_(key in keys) for key, v in sd.items()}
        out = w2v_ref.w2v_forward(leaves, x.to(dtype), cfg, bf16_storage=bf16_storage, dtype=dtype)
        _ref_cache[key_] = dict(zip(keys, torch.autograd.grad(out, [leaves[key] for key in keys], dout.to(dtype))))
    return _ref_cache[key_]


def _native_grads(m, x, dout, keys, zero=True):
    from mmfusion import arena
    ar = arena.ensure(m)
    if zero:
        ar.zero_grad()
    out = m(x).last_hidden_state
    assert out.requires_grad and out.dtype == torch.float32
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    return _hf_grads(m, keys), out.detach()


def _douts(cfg, n, T, seed):
    """a random gradient of the result and one that is non-zero on frame 0 of each clip only"""
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(n, T, cfg.hidden_size, generator=g)
    row0 = torch.zeros_like(dout)
    row0[:, 0] = dout[:, 0]
    return [("random", dout), ("frame-0", row0)]


def _without_key_bias(keys):
    return [k for k in keys if not k.endswith("k_proj.bias")]


def _check_key_bias(m, keys):
    for key in keys:
        if key.endswith("k_proj.bias"):
            name, rows, _ = m._hf[key]
            assert not bool(getattr(m, name).grad[rows[0]:rows[1]].any()), f"{key} received a gradient"


def _pick(d, keys):
    return {key: d[key] for key in keys}


@pytest.mark.parametrize("k,front", [(1, False), (2, False), (2, True)], ids=["k1", "k2", "all"])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_weight_gradients_against_float64_autograd(which, k, front):
    """2 layers; 3 clips of 3000 samples in chunks of 2: T = 149, odd and past one 128-row block"""
    cfg, sd, m, x = _setup(which, 3, 3000)
    T = m.frames(3000)
    assert T == 149
    with torch.no_grad():
        plain = m(x.cuda()).last_hidden_state.clone()
    m.set_trainable_layers(k, front=front)
    keys = _keys(cfg, k, front)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted({m._hf[key][0] for key in keys})
    every = _keys(cfg, 2, True)                                     # one autograd pass serves the three parametrisations
    for tag, dout in _douts(cfg, 3, T, 51):
        exact = _ref_grads((which, tag), sd, x, cfg, dout, torch.float64, False, every)
        stored = _ref_grads((which, tag), sd, x, cfg, dout, torch.float64, True, every)
        got, out = _native_grads(m, x.cuda(), dout, keys)
        assert torch.equal(_bits(out), _bits(plain)), "the differentiable forward's bits are not the inference call's"
        kept = _without_key_bias(keys)
        _rule_b(f"NativeWav2Vec2 {which} 3 x 3000, k={k}{' + front end' if front else ''}, {tag} dO,", _pick(got, kept), _pick(exact, kept),
                _pick(stored, kept))
        _check_key_bias(m, keys)
        _frozen_grads_are_empty(m)


@pytest.mark.parametrize("all_", [False, True], ids=["k1", "all"])
def test_weight_gradients_against_autograd_base_sizes(all_):
    """wav2vec2-base sizes (12 layers, d 768, 12 heads, 7 conv layers, 16 groups of 48 channels and 128 taps: the real GEMM shapes,
    the LayerNorm lane forms at 768 and 512 and the positional kernels' real form), 2 clips of 16000 samples (T = 49), float32
    references; the top layer, and every layer with the front end.  The worst error / bound is in profiles/w2v_finetune.txt.

    The case that pins the attention backward's delta (``mmf_attn_delta_f32`` + ``mmf_attn_bwd_grouped_delta``).  With
    ``mmf_attn_bwd_grouped``, whose delta = dO . O reads the bf16 O, layer 11's ``k_proj.weight`` was 14.11 from the exact gradient
    against a bound of 0.370 (38 times it), ``q_proj.weight`` 14.00 against 0.381 and ``q_proj.bias`` 0.494 against 0.0134, and in
    the "all" case every layer's q / k tensors missed, from 1.04 of the bound at layer 0 to 38 at layer 11, while the error stayed
    near 10: the exact gradients halve from layer to layer (||d k_proj.weight|| 811 at layer 0, 0.77 at layer 11: the frames of a
    clip grow alike in a deep network of seeded weights, and dS vanishes with them), the residue dO . (O - bf16(O)) does not.  With
    delta = sum_j p_ij dp_ij in f32 the worst tensor of either case is at 0.53 of its bound."""
    cfg, sd, m, x = _setup("base", 2, 16000)
    L = cfg.num_hidden_layers
    m.set_trainable_layers(L if all_ else 1, front=all_)
    keys = _keys(cfg, L if all_ else 1, all_)
    (_, dout), _ = _douts(cfg, 2, m.frames(16000), 53)
    every = _keys(cfg, L, True)
    exact = _ref_grads("base", sd, x, cfg, dout, torch.float32, False, every)
    stored = _ref_grads("base", sd, x, cfg, dout, torch.float32, True, every)
    got, _ = _native_grads(m, x.cuda(), dout, keys)
    kept = _without_key_bias(keys)
    _rule_b(f"NativeWav2Vec2 base 2 x 16000, {'all' if all_ else 'k=1'},", _pick(got, kept), _pick(exact, kept), _pick(stored, kept))
    _check_key_bias(m, keys)
    _frozen_grads_are_empty(m)


def test_gradients_accumulate_and_honour_the_lazy_zero_protocol():
    """two backward calls without zeroing give twice the gradient, to rule (b) on the doubled reference; a first touch after
    ``zero_grad(lazy=True)`` overwrites"""
    from mmfusion import arena
    cfg, sd, m, x = _setup("tiny", 3, 3000)
    L = cfg.num_hidden_layers
    m.set_trainable_layers(L, front=True)
    keys = _without_key_bias(_keys(cfg, L, True))
    (tag, dout), _ = _douts(cfg, 3, m.frames(3000), 51)
    every = _keys(cfg, 2, True)
    exact = _ref_grads(("tiny", tag), sd, x, cfg, dout, torch.float64, False, every)
    stored = _ref_grads(("tiny", tag), sd, x, cfg, dout, torch.float64, True, every)
    once, _ = _native_grads(m, x.cuda(), dout, keys)
    twice, _ = _native_grads(m, x.cuda(), dout, keys, zero=False)
    _rule_b("NativeWav2Vec2 tiny, two backwards without zeroing against 2 x the reference,", twice, {k: 2 * exact[k] for k in keys},
            {k: 2 * stored[k] for k in keys})
    for key in keys:
        e = l2_rel(twice[key], 2 * once[key])
        print(f"two backwards vs 2 x one, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    ar = arena.ensure(m)
    ar.zero_grad(lazy=True)
    _native_grads(m, x.cuda(), dout, keys, zero=False)
    ar.finalize_grads()
    torch.cuda.synchronize()
    again = _hf_grads(m, keys)
    for key in keys:
        e = l2_rel(again[key], once[key])
        print(f"after zero_grad(lazy=True), {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    _frozen_grads_are_empty(m)


def test_forward_and_backward_replay_from_a_captured_graph():
    """k = 2 with the front end, a fixed shape, one stream: the replayed gradients are the eager call's bits, but for the tensors
    whose sums go through f32 atomics in an order that differs between two runs of the same call (the LayerNorm parameters:
    ``mmf_layernorm_bwd_grouped``'s finalize pass; the biases: the TN GEMM's fused column sum and ``mmf_colsum_grouped``), which
    are held to ``F32_TOL``, the bound of a change of summation order"""
    from mmfusion import arena
    cfg, sd, m, x = _setup("tiny", 3, 3000)
    m.set_trainable_layers(2, front=True)
    keys = _without_key_bias(_keys(cfg, 2, True))
    (_, dout), _ = _douts(cfg, 3, m.frames(3000), 63)
    eager, _ = _native_grads(m, x.cuda(), dout, keys)
    ar = arena.ensure(m)
    static, dO = x.cuda().clone(), dout.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        m(static).last_hidden_state.backward(dO)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m(static).last_hidden_state.backward(dO)
    with torch.no_grad():
        static.copy_(torch.randn_like(static))
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
        if key.endswith(".bias") or "layer_norm" in key:
            e = l2_rel(got[key], eager[key])
            print(f"captured forward + backward, {key}: rel L2 vs eager {e:.3e} (bound {F32_TOL})")
            assert e <= F32_TOL, key
        else:
            assert torch.equal(_bits(got[key]), _bits(eager[key])), key
    assert any(l2_rel(other[key], eager[key]) > 1e-2 for key in keys)


@pytest.mark.parametrize("k", [1, "all"])
def test_audio_encoder_steps_the_trainable_parameters(k):
    """one ``finetune_optimizer`` step changes exactly the trainable backbone parameters and the encoder's own, and the loss
    gradient of a top-layer weight matches the float64 route (the restatement in front of the encoder's tail in float64) to
    rule (b)"""
    import config as cfgmod
    from mmfusion import arena
    from mmfusion.train import finetune_optimizer
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 768     # the tail's 8 heads need a head_dim of 64 / 96
    cfg.audio_backbone = "native"
    cfg.audio_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=512, conv_dim=(256, 256, 256), conv_kernel=(10, 3, 2),
                                     conv_stride=(5, 2, 2), num_conv_pos_embeddings=16)
    cfg.audio_backbone_trainable_layers = k
    cfg.encoder_attention_weights = False
    torch.manual_seed(3)
    enc = AudioEncoder(cfg)
    wcfg = enc.model.config
    L = wcfg.num_hidden_layers
    assert enc.model.trainable_layers == (L if k == "all" else k) and enc.model.trainable_front == (k == "all")
    sd = w2v_ref.seeded_weights(wcfg, seed=31)
    enc.model.load_state_dict(sd)
    enc = enc.cuda().train()
    wave = (0.5 * torch.randn(2, 3000, generator=torch.Generator().manual_seed(32))).cuda()
    ar = arena.ensure(enc)
    opt = finetune_optimizer(enc, ar, lr=1e-2, weight_decay=0.01)
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    ar.zero_grad()
    feats = enc(wave)["features"]
    assert feats.requires_grad
    feats.sum().backward()
    torch.cuda.synchronize()
    top = f"encoder.layers.{L - 1}.feed_forward.output_dense.weight"
    got = _hf_grads(enc.model, [top])
    opt.advance()
    opt.launch()
    torch.cuda.synchronize()
    names = enc.model._layer_params(L - 1) if k == 1 else [n for n, _ in enc.model.named_parameters() if n.startswith(("l0_", "l1_"))] \
        + list(enc.model._FRONT_PARAMS)
    assert sorted(n for n, p in enc.model.named_parameters() if p.requires_grad) == sorted(names)
    for n, p in enc.named_parameters():
        same = torch.equal(_bits(p.detach()), _bits(before[n]))
        if n.startswith("model."):
            key_bias = "_qkv_b" in n                                                   # (a third of it, the key bias, has no gradient)
            assert same != p.requires_grad or key_bias, f"{n}: {'did not move' if same else 'is frozen and moved'}"
        elif p.requires_grad and n.startswith(("temporal_attention.", "projection.")):
            assert not same, f"{n} did not move"
        elif not p.requires_grad:
            assert same, f"the frozen {n} moved"

    # the float64 route: the restatement, then the tail (self-attention over T in 8 heads, mean over T, projection), summed
    def loss(bf16_storage):
        leaves = {key: v.double().clone().requires_grad_(key == top) for key, v in sd.items()}
        seq = w2v_ref.w2v_forward(leaves, wave.cpu().double(), wcfg, bf16_storage=bf16_storage, dtype=torch.float64)
        ta = {n: before["temporal_attention." + n].cpu().double() for n in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")}
        B, T, d = seq.shape
        q, kk, v = ((seq @ ta["in_proj_weight"].T + ta["in_proj_bias"]).reshape(B, T, 3, 8, d // 8).permute(2, 0, 3, 1, 4))
        att = (torch.softmax(q @ kk.transpose(-1, -2) / (d // 8) ** 0.5, dim=-1) @ v).transpose(1, 2).reshape(B, T, d)
        pooled = (att @ ta["out_proj.weight"].T + ta["out_proj.bias"]).mean(dim=1)
        out = pooled @ before["projection.weight"].cpu().double().T + before["projection.bias"].cpu().double()
        return torch.autograd.grad(out.sum(), leaves[top])[0]
    _rule_b(f"AudioEncoder, audio_backbone_trainable_layers={k!r}, d loss / d", got, {top: loss(False)}, {top: loss(True)})


def test_refusals_and_the_frozen_default():
    from mmfusion import ops
    cfg, sd, m, x = _setup("tiny", 2, 3000)
    xd = x.cuda()
    assert m.trainable_layers == 0 and not any(p.requires_grad for p in m.parameters())
    out = m(xd).last_hidden_state                                                      # grad mode on, nothing trainable
    assert not out.requires_grad
    m.set_trainable_layers(2, front=True)
    live = m(xd).last_hidden_state
    assert live.requires_grad
    with torch.no_grad():
        assert not m(xd).last_hidden_state.requires_grad
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match="bf16 storage only"):
            m(xd)
        with pytest.raises(RuntimeError, match="bf16 storage only"):                   # ... and in the backward, as in the forward
            live.backward(torch.ones_like(live))
    finally:
        ops.set_precision(old)
    m.set_trainable_layers(0)
    again = m(xd).last_hidden_state
    assert not again.requires_grad and torch.equal(again, out) and not any(p.requires_grad for p in m.parameters())
    assert BOUND_A > 0
