"""GPU: the launch sequence of the three frozen backbones (``mmfusion.vit.NativeViT``, ``mmfusion.wav2vec2.NativeWav2Vec2``,
``mmfusion.deberta.NativeDeberta``) is the one their module docstrings list: every launch that ``mmfusion.lib`` records while ``lib.PROFILE`` is a list, in
order, with the shapes it records.

The expected lists are written out here from the configuration's sizes alone; nothing below asks the modules under test
for a size.  GEMM labels are reduced to layout and output dtype (which kernel generation the dispatch chose is not this
test's business).  Launches that are not recorded (the widening cast into the result, the bf16 shadow cast of the
weights) are not expected.  One full chunk and one short chunk each.  The same for a differentiable forward and its backward
with the top two layers trainable: Wav2Vec2's and DeBERTa's backward lists are one function of what each model supplies."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_ref  # noqa: E402
import vit_ref  # noqa: E402
import w2v_ref  # noqa: E402

N, CHUNK, SAMPLES = 3, 2, 4000
_GEMM = re.compile(r"^gemm\d*_grouped_kernel<(\w+),(\w+)>$")


def _recorded(fn):
    from mmfusion import lib
    fn()                                                                              # warm-up: workspace, shadow casts
    torch.cuda.synchronize()
    lib.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        recs = lib.PROFILE
    finally:
        lib.PROFILE = None
    out = []
    for label, _flops, _e0, _e1, detail in recs:
        m = _GEMM.match(label)
        out.append((f"gemm<{m.group(1)},{m.group(2)}>" if m else label, tuple(tuple(int(v) for v in d) for d in detail)))
    return out


def _assert_same(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i}: recorded {g}, expected {w}"
    k = min(len(got), len(want))
    assert len(got) == len(want), f"{len(got)} launches recorded, {len(want)} expected; the first one over: {(got[k:] + want[k:])[0]}"


def gemm(*mnk):
    return ("gemm<NT,bf16>", tuple(mnk))


def ln(rows, width):
    return ("ln_fwd_kernel", ((rows, width),))


def gelu(rows, cols):
    return ("bias_gelu_kernel", ((rows, cols),))


def attn(head_dim, Tq, Tk):
    return (f"attn_fwd_kernel<{head_dim}>", ((Tq, Tk),))


def _chunks():
    return [min(CHUNK, N - n0) for n0 in range(0, N, CHUNK)]


# ---- the backward: one differentiable forward plus ``backward`` with the top two layers trainable and nothing else.  At these
# sizes every chunk has fewer than 1024 rows, so the K-slab rule gives 1 on any device: every weight gradient is one TN launch
def dgrad(*mnk):
    return ("gemm<NN,bf16>", tuple(mnk))


def wgrad(*mnk):
    return ("gemm<TN,f32>", tuple(mnk))


def ln_bwd(rows, width):
    return ("ln_bwd_kernel", ((rows, width),))


def _mlp_backward(m, d, I):
    """fc2 wgrad, dgrad; GELU backward; fc1 wgrad, dgrad: on the ``m`` rows of a gradient"""
    return [wgrad((d, I, m)), dgrad((m, I, d)), ("bias_gelu_bwd_kernel", ((m, I),)), wgrad((I, d, m)), dgrad((m, d, I))]


def _post_ln_layer(rows, d, I, attend):
    return [gemm((rows, 3 * d, d)), attend, gemm((rows, d, d)), ln(rows, d), gemm((rows, I, d)), gelu(rows, I), gemm((rows, d, I)), ln(rows, d)]


def _post_ln_layer_grad(rows, d, I, attend, attn_bwd, qkv_wgrad, below):
    """the rows of ``_post_ln_layer_grad`` in mmfusion/backbone.py: what a model supplies is ``attend``, ``attn_bwd`` (a list) and
    ``qkv_wgrad``"""
    return (_post_ln_layer(rows, d, I, attend) + [ln_bwd(rows, d)] + _mlp_backward(rows, d, I) + [ln_bwd(rows, d), wgrad((d, d, rows)), dgrad((rows, d, d))]
            + attn_bwd + [qkv_wgrad] + ([dgrad((rows, d, 3 * d))] if below else []))


def _backward_recorded(run):
    def step():
        out = run()
        out.backward(torch.ones_like(out))
    return _recorded(step)


# ---- ViT ---------------------------------------------------------------------------------------------------
def _vit_expected(cfg, cls_only):
    d, I, H, C, S, P = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_channels, cfg.image_size, cfg.patch_size
    NP = (S // P) ** 2
    T, hd = NP + 1, d // H
    want = []
    for n in _chunks():
        rows = n * T
        want += [("vit_patchify_kernel", ((n, C * S * S),)), gemm((n * NP, d, C * P * P)), ("vit_embed_tokens_kernel", ((rows, d),))]
        full = [ln(rows, d), gemm((rows, 3 * d, d)), attn(hd, T, T), gemm((rows, d, d)),
                ln(rows, d), gemm((rows, I, d)), gelu(rows, I), gemm((rows, d, I))]
        if not cls_only:
            want += full * cfg.num_hidden_layers + [ln(rows, d)]
            continue
        want += full * (cfg.num_hidden_layers - 1)
        # the last layer: K / V for every token and Q for row 0 of each image in one grouped launch, the rest on n rows
        want += [ln(rows, d), gemm((rows, 2 * d, d), (n, d, d)), attn(hd, 1, T), gemm((n, d, d)),
                 ln(n, d), gemm((n, I, d)), gelu(n, I), gemm((n, d, I)), ln(n, d)]
    return want


@pytest.fixture(scope="module")
def vit_case():
    from mmfusion.vit import NativeViT
    cfg = vit_ref.tiny_config()
    m = NativeViT(**vit_ref.config_kwargs(cfg), chunk=CHUNK)
    m.load_state_dict(vit_ref.seeded_weights(cfg, seed=21))
    x = torch.rand(N, cfg.num_channels, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(22))
    return cfg, m.cuda().eval(), x.cuda()


def test_vit_forward_launches_are_the_documented_sequence(vit_case):
    cfg, m, x = vit_case
    _assert_same(_recorded(lambda: m(x)), _vit_expected(cfg, cls_only=False))


def test_vit_cls_features_launches_are_the_documented_sequence(vit_case):
    cfg, m, x = vit_case
    _assert_same(_recorded(lambda: m.cls_features(x)), _vit_expected(cfg, cls_only=True))


def _vit_backward_expected(cfg, cls_only):
    """after the forward of every chunk, per chunk: the final LayerNorm again and its backward, then the top two layers top down,
    each again up to the GELU output and then its pre-LN backward; on the ``cls_features`` route the last layer in its CLS form
    (``m = n`` rows behind the attention) and the layer below on every row"""
    d, I, H, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_hidden_layers
    T, hd = (cfg.image_size // cfg.patch_size) ** 2 + 1, d // H
    want = _vit_expected(cfg, cls_only)
    for n in _chunks():
        rows = n * T
        m = n if cls_only else rows
        want += [ln(m, d), ln_bwd(m, d)]
        for i in (L - 1, L - 2):
            m = n if cls_only and i == L - 1 else rows
            if m == n:
                want += [ln(rows, d), gemm((rows, 2 * d, d), (n, d, d)), attn(hd, 1, T), gemm((n, d, d))]
            else:
                want += [ln(rows, d), gemm((rows, 3 * d, d)), attn(hd, T, T), gemm((rows, d, d))]
            want += [ln(m, d), gemm((m, I, d)), gelu(m, I)] + _mlp_backward(m, d, I) + [ln_bwd(m, d), wgrad((d, d, m)), dgrad((m, d, d))]
            if m == n:
                # dQ of row 0 and dK | dV of every row; the Q rows of the weight over n rows and the K | V rows over all in one
                # launch; the Q input gradient of row 0, then the K | V one of every row
                want += [("vit_cls_attn_bwd_kernel", ((rows, 2 * d),)), wgrad((d, d, n)), wgrad((d, d, rows), (d, d, rows)),
                         dgrad((n, d, d)), dgrad((rows, d, 2 * d)), ln_bwd(rows, d)]
            else:
                want += [(f"attn_bwd_kernels<{hd}>", ((T, T),)), wgrad((d, d, rows), (d, d, rows), (d, d, rows)), dgrad((rows, d, 3 * d)),
                         ln_bwd(rows, d)]
    return want


@pytest.mark.parametrize("cls_only", [False, True], ids=["forward", "cls_features"])
def test_vit_backward_launches_are_the_documented_sequence(cls_only):
    from mmfusion.vit import NativeViT
    cfg = vit_ref.tiny_config()
    m = NativeViT(**vit_ref.config_kwargs(cfg), chunk=CHUNK)
    m.load_state_dict(vit_ref.seeded_weights(cfg, seed=21))
    m = m.cuda().eval()
    m.set_trainable_layers(2)
    x = torch.rand(N, cfg.num_channels, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(22)).cuda()
    got = _backward_recorded((lambda: m.cls_features(x)) if cls_only else (lambda: m(x).last_hidden_state))
    _assert_same(got, _vit_backward_expected(cfg, cls_only))


# ---- Wav2Vec2 ----------------------------------------------------------------------------------------------
def _w2v_expected(cfg, L):
    d, I, H = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
    dims, ks, ss = cfg.conv_dim, cfg.conv_kernel, cfg.conv_stride
    Ts, t = [], L
    for k, s in zip(ks, ss):
        t = (t - k) // s + 1
        Ts.append(t)
    T, hd, last = Ts[-1], d // H, len(dims) - 1
    cg = d // cfg.num_conv_pos_embedding_groups
    want = []
    for n in _chunks():
        rows = n * T
        want += [("w2v_conv0_stats_kernels", ((n, L),)), ("w2v_conv0_norm_gelu_kernel", ((n, L),))]
        for i in range(1, last + 1):
            want.append(gemm((n * Ts[i], dims[i], ks[i] * dims[i - 1])))
            if i < last:
                want.append(("w2v_gelu_window_kernel", ((n * Ts[i + 1], ks[i + 1] * dims[i]),)))
            else:
                want.append(gelu(rows, dims[i]))
        want += [ln(rows, dims[-1]), gemm((rows, d, dims[-1])),
                 ("w2v_posconv_kernel", ((rows, d, cfg.num_conv_pos_embeddings * cg),)), ln(rows, d)]
        want += [gemm((rows, 3 * d, d)), attn(hd, T, T), gemm((rows, d, d)), ln(rows, d),
                 gemm((rows, I, d)), gelu(rows, I), gemm((rows, d, I)), ln(rows, d)] * cfg.num_hidden_layers
    return want


def test_w2v_forward_launches_are_the_documented_sequence():
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg = w2v_ref.tiny_config()
    m = NativeWav2Vec2(**w2v_ref.config_kwargs(cfg), chunk=CHUNK)
    m.load_state_dict(w2v_ref.seeded_weights(cfg, seed=21))
    m = m.cuda().eval()
    x = (0.5 * torch.randn(N, SAMPLES, generator=torch.Generator().manual_seed(22))).cuda()
    _assert_same(_recorded(lambda: m(x)), _w2v_expected(cfg, SAMPLES))


def test_w2v_backward_launches_are_the_documented_sequence():
    """the shared post-LN walk with the fused attention: its backward is the f32 delta pass and the MFMA backward, the Q/K/V
    weight gradient one launch of the three row blocks (the key bias's column sum is sent aside); the lowest walked layer
    launches no input gradient"""
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg = w2v_ref.tiny_config()
    m = NativeWav2Vec2(**w2v_ref.config_kwargs(cfg), chunk=CHUNK)
    m.load_state_dict(w2v_ref.seeded_weights(cfg, seed=21))
    m = m.cuda().eval()
    m.set_trainable_layers(2)
    x = (0.5 * torch.randn(N, SAMPLES, generator=torch.Generator().manual_seed(22))).cuda()
    d, I, L, hd = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.hidden_size // cfg.num_attention_heads
    T = SAMPLES
    for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
        T = (T - k) // s + 1
    want = _w2v_expected(cfg, SAMPLES)
    for n in _chunks():
        rows = n * T
        for i in (L - 1, L - 2):
            want += _post_ln_layer_grad(rows, d, I, attn(hd, T, T), [(f"attn_delta_kernel<{hd}>", ((T, T),)), (f"attn_bwd_kernels<{hd}>", ((T, T),))],
                                        wgrad((d, d, rows), (d, d, rows), (d, d, rows)), below=i > L - 2)
    _assert_same(_backward_recorded(lambda: m(x).last_hidden_state), want)


# ---- DeBERTa -----------------------------------------------------------------------------------------------
def test_deberta_backward_launches_are_the_documented_sequence():
    """the shared post-LN walk with the disentangled attention, from ids: its backward also forms the position tables' gradient,
    the Q/K/V weight gradient is one plain launch on the fused weight.  Both layers train, so both position tables are computed
    in front of the forward and behind the walk each layer's q and k rows take their position-path term"""
    from mmfusion.deberta import NativeDeberta
    T = 70
    cfg = deberta_ref.tiny_config()
    m = NativeDeberta(**deberta_ref.config_kwargs(cfg), chunk=CHUNK)
    m.load_state_dict(deberta_ref.seeded_weights(cfg, seed=21))
    m = m.cuda().eval()
    m.set_trainable_layers(2)
    ids = torch.randint(1, cfg.vocab_size, (N, T), generator=torch.Generator().manual_seed(22))
    mask = torch.ones(N, T, dtype=torch.int64)
    ids[N - 1, 50:], mask[N - 1, 50:] = 0, 0
    i, k = ids.cuda(), mask.cuda()
    d, I, L, S2 = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, 2 * cfg.position_buckets
    attend = ("deberta_attn_fwd_kernel<64>", ((T, T),))
    want = [gemm((S2, 2 * d, d))] * 2
    for n in _chunks():
        want += [("deberta_embed_kernel", ((n * T, d),))] + _post_ln_layer(n * T, d, I, attend) * L
    for n in _chunks():
        for layer in (L - 1, L - 2):
            want += _post_ln_layer_grad(n * T, d, I, attend, [("deberta_attn_bwd_pos_kernels<64>", ((T, T),))], wgrad((3 * d, d, n * T)),
                                        below=layer > L - 2)
    want += [wgrad((d, d, S2)), wgrad((d, d, S2))] * 2
    _assert_same(_backward_recorded(lambda: m(input_ids=i, attention_mask=k).last_hidden_state), want)


def test_deberta_forward_launches_are_the_documented_sequence():
    """the widening cast and the once-per-weight-version position tables are not recorded in a warmed-up forward"""
    from mmfusion.deberta import NativeDeberta
    T = 70
    cfg = deberta_ref.tiny_config()
    m = NativeDeberta(**deberta_ref.config_kwargs(cfg), chunk=CHUNK)
    m.load_state_dict(deberta_ref.seeded_weights(cfg, seed=21))
    m = m.cuda().eval()
    ids = torch.randint(1, cfg.vocab_size, (N, T), generator=torch.Generator().manual_seed(22))
    mask = torch.ones(N, T, dtype=torch.int64)
    ids[N - 1, 50:], mask[N - 1, 50:] = 0, 0
    i, k = ids.cuda(), mask.cuda()
    got = _recorded(lambda: m(input_ids=i, attention_mask=k))
    d, I = cfg.hidden_size, cfg.intermediate_size
    want = []
    for n in (2, 1):
        rows = n * T
        want.append(("deberta_embed_kernel", ((rows, d),)))
        want += [gemm((rows, 3 * d, d)), ("deberta_attn_fwd_kernel<64>", ((T, T),)), gemm((rows, d, d)), ln(rows, d),
                 gemm((rows, I, d)), gelu(rows, I), gemm((rows, d, I)), ln(rows, d)] * cfg.num_hidden_layers
    _assert_same(got, want)
    assert len(got) == len(want) == 2 * (1 + 8 * cfg.num_hidden_layers)
