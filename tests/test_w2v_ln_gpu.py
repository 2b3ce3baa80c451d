"""GPU: the layer-norm family of Wav2Vec2.  Its two kernels (``mmf_w2v_conv0_ln_gelu``, ``mmf_w2v_ln_gelu_window``) against float64,
and ``NativeWav2Vec2`` on the family against the explicit restatement tests/w2v_ln_ref.py and the captured HuggingFace output.

Bounds.  Kernels: every output within one bf16 ulp of the float64 value rounded to bf16, as the issue sets it, and relative L2 <=
BOUND_A.  The one-ulp rule is asserted bare on every output but those of the CANCELLING SET, where no f32 arithmetic can hold it (the
issue asks for f32; it wants amending there): the pre-activation y = gamma (v - mean) rstd + beta is formed in f32, so its error is
relative to its TERMS, terms = |gamma| rstd (|v| + |mean|) + |beta| (|v| = sum |w x| + |b| for the convolution), at most
F32_TERMS = 2^-20 of them (16 roundings of 2^-24: the convolution's taps and bias, the two reductions, the normalisation).  gelu(y)
~ y / 2 near 0 carries that error over while the ulp shrinks with the result, so the output can leave its ulp only where
2^-20 terms / |y| reaches bf16's 2^-8: the cancelling set is |y| < CANCEL x terms, CANCEL = 2^-12.  Everywhere else, the left tail
included (where gelu's condition number is y^2: 25 x 2^-20 terms / |y| is still far below 2^-8), the bare rule holds or the test
fails.  Inside the set the error is capped in size, ulp + 0.51 x F32_TERMS x terms (gelu' is within 0.5 +- 0.01 there), and the set
in count: y is spread over about terms / 4 or more, so |y| < 2^-12 terms takes about 2^-9 of the outputs; the cap is 2^-8 of them
(at least 8 for the tiny cases).  A further case puts every pre-activation into the left tail (y in about -6 .. -4, beta = -5),
where nothing cancels and the bare rule holds throughout: a GELU formed as 1 + erf would miss it there by 20 ulps.  Module: tests/test_w2v_gpu.py's two,
(a) <= BOUND_A against the restatement with bf16 storage, (b) <= 2 x the bf16-storage restatement's own error against the exact one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_ln_ref  # noqa: E402
import w2v_ref  # noqa: E402
from helpers import BOUND_A, _bf16_ulp, _lib, l2_rel  # noqa: E402
from test_w2v_ln_ref_cpu import golden  # noqa: E402

BF16 = torch.bfloat16
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
EPS = 1e-5
GUARD = 4096                               # NaN elements behind every output: what a kernel must leave alone
F32_TERMS = 2.0 ** -20                     # the f32 budget of the pre-activation, relative to its terms (module docstring)
CANCEL = 2.0 ** -12                        # |y| < CANCEL x terms: where that budget reaches a bf16 ulp of the result


def _out(numel):
    return torch.full((numel + GUARD,), float("nan"), dtype=BF16, device="cuda")


def _check(what, buf, want, y, terms, tail=False):
    """``buf``: the NaN-filled output with its guard; ``want``: float64, the exact result; ``y`` / ``terms``: the exact pre-activation
    and the magnitude of its terms, laid out as ``want``.  ``tail``: a left-tail case, whose cancelling set must be empty"""
    n = want.numel()
    got = buf[:n].cpu().double().view(want.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: NaN left in the output"
    assert bool(torch.isnan(buf[n:]).all()), f"{what}: the guard behind the output was written"
    rounded = want.to(BF16).double()
    diff, ulp = (got - rounded).abs(), _bf16_ulp(rounded)
    cancel = y.abs() < CANCEL * terms
    bare = diff / ulp
    outside = float(bare[~cancel].max())
    inside = float((diff / (ulp + 0.51 * F32_TERMS * terms))[cancel].max()) if bool(cancel.any()) else 0.0
    count, cap = int(cancel.sum()), 0 if tail else max(8, n >> 8)
    err = l2_rel(got, want)
    print(f"{what}: worst |got - bf16(exact)| / ulp outside the cancelling set {outside:.3f} (bound 1); the set: {count} of {n} outputs (cap {cap}), "
          f"{int((bare[cancel] > 1.0).sum())} of them above one ulp, worst {float(bare[cancel].max()) if count else 0.0:.1f} ulps, worst / its bound {inside:.3f}; "
          f"rel L2 {err:.3e} (bound {BOUND_A}); y in {float(y.min()):.2f} .. {float(y.max()):.2f}")
    assert outside <= 1.0 and inside <= 1.0 and count <= cap and err <= BOUND_A


def _ln_gelu(x, gamma, beta, mag=None):
    """-> (gelu(y), y, terms): y the LayerNorm over the last dim of x, terms the magnitude of its terms; ``mag``: |x| where x is
    itself a sum"""
    g, b = gamma.double(), beta.double()
    mean = x.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + EPS)
    terms = g.abs() * rstd * ((x.abs() if mag is None else mag) + mean.abs()) + b.abs()
    y = w2v_ref.layer_norm(x, g, b, EPS)
    return w2v_ref.gelu_erf(y), y, terms.expand_as(y)


def _affine(C, g, tail):
    """gamma, beta of a case: spread around 1 and 0, or (``tail``) 0.25 and -5, which puts every y into the left tail"""
    if tail:
        return 0.25 + 0.02 * torch.randn(C, generator=g), -5.0 + 0.1 * torch.randn(C, generator=g)
    return 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


# ---- kernels -----------------------------------------------------------------------------------------------
def _conv0_case(N, L, C0, k0, s0, k1, s1, with_bias, tail=False):
    lib = _lib()
    g = torch.Generator().manual_seed(L + C0 + k0)
    wave = 0.5 * torch.randn(N, L, generator=g) + 0.5
    w = 0.4 * torch.randn(C0, 1, k0, generator=g)
    bias = 0.3 * torch.randn(C0, generator=g) if with_bias else None
    gamma, beta = _affine(C0, g, tail)
    raw = w2v_ref.conv0_raw(wave.double(), w.double(), s0) + (bias.double() if with_bias else 0.0)
    mag = w2v_ref.conv0_raw(wave.double().abs(), w.double().abs(), s0) + (bias.double().abs() if with_bias else 0.0)
    T1 = (raw.shape[1] - k1) // s1 + 1
    want, y, terms = (w2v_ref.window(t, k1, s1) for t in _ln_gelu(raw, gamma, beta, mag))
    buf = _out(N * T1 * k1 * C0)
    lib.w2v_conv0_ln_gelu(wave.cuda(), w.cuda(), bias.cuda() if with_bias else None, gamma.cuda(), beta.cuda(), buf, k0, s0, k1, s1, EPS)
    _check(f"conv0_ln_gelu N={N} L={L} C0={C0} k0={k0} k1={k1} s1={s1} bias={with_bias}{' left tail' if tail else ''}", buf, want, y, terms, tail)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("N,L,C0,k1,s1", [(2, 4000, 256, 3, 2), (3, 4003, 512, 3, 2), (1, 1237, 64, 2, 2), (1, 1237, 8, 2, 2),
                                          (1, 2000, 1024, 3, 2)])
def test_conv0_ln_gelu_against_float64(N, L, C0, k1, s1, with_bias):
    """sub-wave (256, 64), one-wave (512), one-lane (8) and two-wave (1024) frames; the waveform has a DC offset of 0.5"""
    _conv0_case(N, L, C0, 10, 5, k1, s1, with_bias)


def test_conv0_ln_gelu_sixteen_tap_form():
    """k0 = 12: the kernel's 16-tap instantiation (k0 above 10)"""
    _conv0_case(1, 1237, 64, 12, 5, 2, 2, True)


def test_conv0_ln_gelu_left_tail():
    _conv0_case(2, 2000, 512, 10, 5, 3, 2, True, tail=True)


def _window_case(N, T_in, C, k, s, tail=False, in_place=False):
    """``k = 0``: the last layer's form, (T_in, C) out"""
    lib = _lib()
    g = torch.Generator().manual_seed(T_in + C)
    x = (3.0 * torch.randn(N, T_in, C, generator=g) + 0.5).to(BF16)
    gamma, beta = _affine(C, g, tail)
    want, y, terms = ((w2v_ref.window(t, k, s) if k else t) for t in _ln_gelu(x.double(), gamma, beta))
    buf = _out(want.numel())
    src = buf if in_place else x.cuda()
    if in_place:
        buf[:x.numel()].copy_(x.reshape(-1))
    lib.w2v_ln_gelu_window(src, gamma.cuda(), beta.cuda(), buf, N, T_in, C, k, s if k else 1, EPS)
    _check(f"ln_gelu_window N={N} T_in={T_in} C={C} k={k} s={s}{' in place' if in_place else ''}{' left tail' if tail else ''}", buf, want, y,
           terms, tail)


@pytest.mark.parametrize("N,T_in,C,k,s", [(3, 41, 256, 3, 2), (2, 40, 512, 3, 2), (3, 37, 64, 2, 2), (1, 38, 8, 2, 2), (1, 20, 1024, 2, 2)])
def test_ln_gelu_window_against_float64(N, T_in, C, k, s):
    """(3, 37, 64, 2, 2): the last input row is read by no window"""
    _window_case(N, T_in, C, k, s)


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
def test_ln_gelu_window_last_layer_form(in_place):
    """k = 0: (T_in, C) out, no window form; 33 rows in passes of 4: the last pass has lanes past the end"""
    _window_case(2, 33, 512, 0, 0, in_place=in_place)


@pytest.mark.parametrize("C", [512, 1024])
def test_ln_gelu_window_left_tail(C):
    _window_case(2, 40, C, 3, 2, tail=True)


def test_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    f = torch.zeros(1 << 14, device="cuda")
    b = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    win, c0 = L.mmf_w2v_ln_gelu_window, L.mmf_w2v_conv0_ln_gelu
    cases = [
        ("mmf_w2v_ln_gelu_window", lambda: win(p(b), p(f), p(f), p(nan16), 1, 40, 24, 3, 2, EPS, s), E_UNSUPPORTED),          # C = 24
        ("mmf_w2v_ln_gelu_window", lambda: win(p(b, 2), p(f), p(f), p(nan16), 1, 40, 64, 3, 2, EPS, s), E_ALIGN),
        ("mmf_w2v_ln_gelu_window", lambda: win(p(b), p(f), p(f), p(nan16, 2), 1, 40, 64, 3, 2, EPS, s), E_ALIGN),
        ("mmf_w2v_ln_gelu_window", lambda: win(p(b), p(f), p(f), p(nan16), 1, 40, 64, 2, 3, EPS, s), E_UNSUPPORTED),          # k < s
        ("mmf_w2v_ln_gelu_window", lambda: win(p(nan16), p(f), p(f), p(nan16), 1, 40, 64, 3, 2, EPS, s), E_UNSUPPORTED),      # in place with k > 0
        ("mmf_w2v_ln_gelu_window", lambda: win(p(b), p(f), p(f), p(nan16), 1, 2, 64, 3, 2, EPS, s), E_SHAPE),
        ("mmf_w2v_ln_gelu_window", lambda: win(p(b), None, p(f), p(nan16), 1, 40, 64, 3, 2, EPS, s), E_SHAPE),
        ("mmf_w2v_conv0_ln_gelu", lambda: c0(p(f), p(f), p(f), p(f), p(f), p(nan16), 1, 400, 24, 10, 5, 3, 2, EPS, s), E_UNSUPPORTED),   # C0 = 24
        ("mmf_w2v_conv0_ln_gelu", lambda: c0(p(f), p(f), p(f), p(f), p(f), p(nan16, 2), 1, 400, 64, 10, 5, 3, 2, EPS, s), E_ALIGN),
        ("mmf_w2v_conv0_ln_gelu", lambda: c0(p(f), p(f), p(f), p(f), p(f), p(nan16), 1, 400, 64, 10, 5, 2, 3, EPS, s), E_UNSUPPORTED),   # k1 < s1
        ("mmf_w2v_conv0_ln_gelu", lambda: c0(p(f), p(f), p(f), p(f), p(f), p(nan16), 1, 400, 64, 17, 5, 3, 2, EPS, s), E_UNSUPPORTED),
        ("mmf_w2v_conv0_ln_gelu", lambda: c0(p(f), p(f), p(f), p(f), p(f), p(nan16), 1, 8, 64, 10, 5, 3, 2, EPS, s), E_SHAPE),
    ]
    for name, call, want in cases:
        rc = call()
        assert rc == want, (name, rc, want)
        assert name.encode() in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all())                                               # nothing was launched


# ---- module ------------------------------------------------------------------------------------------------
_CFG = {"tiny": w2v_ln_ref.ln_tiny, "wide": w2v_ln_ref.ln_wide}
_ref_cache = {}


def _setup(which: str, n: int, L: int, seed: int = 21, chunk=None):
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg = _CFG[which]()
    sd = w2v_ln_ref.seeded_weights(cfg, seed=seed)
    kw = w2v_ln_ref.config_kwargs(cfg)
    if chunk is not None:
        kw["chunk"] = chunk
    m = NativeWav2Vec2(**kw)
    m.load_state_dict(sd)
    x = 0.5 * torch.randn(n, L, generator=torch.Generator().manual_seed(seed + 1)) + 0.1
    return cfg, sd, m.cuda().eval(), x


def _restatement(which, n, L, seed, bf16_storage):
    """the float64 restatement of ``_setup(which, n, L, seed)``'s case, computed once"""
    key = (which, n, L, seed, bf16_storage)
    if key not in _ref_cache:
        cfg = _CFG[which]()
        x = 0.5 * torch.randn(n, L, generator=torch.Generator().manual_seed(seed + 1)) + 0.1
        _ref_cache[key] = w2v_ln_ref.w2v_forward(w2v_ln_ref.seeded_weights(cfg, seed=seed), x, cfg, bf16_storage=bf16_storage)
    return _ref_cache[key]


@pytest.mark.parametrize("which,n,chunk", [("tiny", 3, 2), ("wide", 2, None)])
def test_forward_against_restatement(which, n, chunk):
    cfg, sd, m, x = _setup(which, n, 4000, chunk=chunk)
    stored, exact = _restatement(which, n, 4000, 21, True), _restatement(which, n, 4000, 21, False)
    got = m(x.cuda()).last_hidden_state
    assert got.dtype == torch.float32 and got.shape == stored.shape and not got.requires_grad
    a, b, model_err = l2_rel(got, stored), l2_rel(got, exact), l2_rel(stored, exact)
    print(f"NativeWav2Vec2 ln_{which} {n} x 4000: (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A})")
    print(f"    (b) vs exact restatement {b:.3e} (bound {2 * model_err:.3e})")
    assert a <= BOUND_A and b <= 2 * model_err


def test_captured_huggingface_output():
    """the fixture's HuggingFace ``last_hidden_state`` on ``ln_tiny``, under bound (b)"""
    from mmfusion.wav2vec2 import NativeWav2Vec2
    cfg, sd, x, want = golden()
    m = NativeWav2Vec2(**w2v_ln_ref.config_kwargs(cfg))
    m.load_state_dict(sd)
    got = m.cuda().eval()(x.cuda()).last_hidden_state
    model_err = l2_rel(w2v_ln_ref.w2v_forward(sd, x, cfg, bf16_storage=True), w2v_ln_ref.w2v_forward(sd, x, cfg))
    err = l2_rel(got, want)
    print(f"NativeWav2Vec2 vs captured HuggingFace fp32 (ln_tiny): {err:.3e} (bound {2 * model_err:.3e})")
    assert got.shape == want.shape and err <= 2 * model_err


def test_chunking_repeatability_and_workspace():
    cfg, sd, m2, x = _setup("tiny", 5, 4000, chunk=2)
    _, _, m5, _ = _setup("tiny", 5, 4000, chunk=5)
    xd = x.cuda()
    f2, f5 = m2(xd).last_hidden_state, m5(xd).last_hidden_state
    e = l2_rel(f2, f5)
    print(f"chunk 2 vs chunk 5: rel L2 {e:.3e} (bound {BOUND_A}); bitwise equal: {torch.equal(f2, f5)}")
    assert e <= BOUND_A
    assert torch.equal(m2(xd).last_hidden_state, f2) and torch.equal(m5(xd).last_hidden_state, f5)
    held = sum(v.numel() * v.element_size() for v in m2._ws.values() if isinstance(v, torch.Tensor))
    assert held == 2 * m2.workspace_bytes_per_clip(4000) and "stats" not in m2._ws


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


def test_load_state_dict_refreshes_the_new_parameters():
    """new conv biases and conv LayerNorm weights alone: the output follows them"""
    cfg, sd, m, x = _setup("tiny", 2, 4000)
    xd = x.cuda()
    first = m(xd).last_hidden_state.clone()
    g = torch.Generator().manual_seed(99)
    sd2 = dict(sd)
    for k in sd:
        if k.startswith("feature_extractor.") and (k.endswith(".conv.bias") or k.endswith(".layer_norm.weight")):
            sd2[k] = sd[k] + 0.5 * torch.randn(sd[k].shape, generator=g)
    m.load_state_dict(sd2)
    second = m(xd).last_hidden_state
    old, new = w2v_ln_ref.w2v_forward(sd, x, cfg, bf16_storage=True), w2v_ln_ref.w2v_forward(sd2, x, cfg, bf16_storage=True)
    moved = l2_rel(new, old)
    print(f"new conv biases / LayerNorm weights: restatement moved by {moved:.3e}; native vs new {l2_rel(second, new):.3e}, vs old {l2_rel(second, old):.3e}")
    assert l2_rel(first, old) <= BOUND_A and l2_rel(second, new) <= BOUND_A and moved > 3 * BOUND_A and l2_rel(second, old) > BOUND_A


def test_audio_encoder_native_backbone_against_reference_backbone():
    """``AudioEncoder`` at width 768 over a layer-norm-family backbone against the same encoder given the restatement as its
    ``backbone=``; tests/test_w2v_gpu.py's tolerance, 1e-2 scaled by max(1, |want|max)"""
    import config as cfgmod
    from models.encoders import AudioEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.audio_hidden_size = 256, 0.0, 768
    cfg.audio_backbone = "native"
    cfg.audio_backbone_kwargs = {k: v for k, v in w2v_ln_ref.config_kwargs(w2v_ln_ref.ln_768()).items() if k != "hidden_size"}
    torch.manual_seed(3)
    enc = AudioEncoder(cfg)
    wcfg = enc.model.config
    assert wcfg.do_stable_layer_norm and wcfg.hidden_size == 768
    sd = w2v_ln_ref.seeded_weights(wcfg, seed=31)
    enc.model.load_state_dict(sd)
    cfg_ref = cfgmod.ModelConfig()
    cfg_ref.fusion_hidden_size, cfg_ref.fusion_dropout = 256, 0.0
    ref = AudioEncoder(cfg_ref, backbone=w2v_ln_ref.RefWav2Vec2(sd, wcfg))
    tail = {k: v for k, v in enc.state_dict().items() if not k.startswith("model.")}
    assert "model.feature_extractor.conv_layers.1.layer_norm.weight" in enc.state_dict()
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
