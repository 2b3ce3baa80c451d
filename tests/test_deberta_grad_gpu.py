"""GPU: the input-gradient path of the native DeBERTa (prompt tuning through the frozen layers).  The backward kernels of
csrc/deberta.hip and csrc/vit.hip against float64, then ``NativeDeberta`` / ``TextEncoder`` gradients against float64 autograd
through the restatement tests/deberta_ref.py.

Bounds.  (a) a kernel against a float64 reference with the same storage: relative L2 <= BOUND_A (2e-2).  The attention backward
is handed the REFERENCE's O (rounded to bf16) and lse (f32), and the reference takes delta from that same O, so a forward
error can neither hide nor mimic a backward one.  (b) a gradient through the whole backbone against the exact float64 one: 2 x
the error of the ``bf16_storage=True`` autograd gradient against the exact one on the same inputs, computed here on the CPU
(``_r`` rounds the gradient in its backward where it rounds the activation in its forward, so that function is the storage
model of the backward too; tests/test_w2v_gpu.py's rule).  lse: tests/test_attention_paths_gpu.py's rule, F32_TOL x
max(|ref|, 1) absolute.

Where the true dQ / dK are 0 a relative bound has no scale: at T = 1 the softmax is one-hot, dP - delta cancels exactly, the
reference gives 1e-16 and a kernel returns the rounding noise of its two 64-term f32 sums (1e-7 here).  So the bound on
||got - want|| is BOUND_A ||want|| + ||N||, N = the f32 summation noise of dP - delta carried through dS into dQ / dK
(deberta_grad_ref.attention_backward(f32_tol=F32_TOL); tests/test_attention_paths_gpu.py's term for its one-hot cases).  On
the other cases ||N|| is 1e-3 ||want|| or less (it adds a few percent to the bound), and each line prints it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_grad_ref as G  # noqa: E402
import deberta_ref  # noqa: E402
from helpers import BOUND_A, _bf16_ulp, _lib, l2_rel  # noqa: E402
from test_deberta_gpu import _attn_case, _model  # noqa: E402

BF16 = torch.bfloat16
F32_TOL = 1e-5                     # tests/test_kernel_forms_gpu.py's, the figure the attention tests' lse rule uses
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
SCALE = math.sqrt(3.0 * 64)
ATTN_CASES = [
    (1, 3, 1, 8, 32, None),              # T = 1
    (1, 2, 33, 8, 32, None),             # one key past a tile
    (2, 2, 70, 8, 32, 50),               # both clamps, ragged, padded item
    (2, 2, 200, 256, 512, None),         # linear and log region, four query blocks and seven key tiles
    (1, 1, 530, 256, 512, None),         # the clamp binds
]
_cache = {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _heads(t, n, T, H):
    return t.reshape(n, T, H, 64).transpose(1, 2)


def _rows(t, n, T, H):
    return t.transpose(1, 2).reshape(n * T, H * 64)


def _attn_bwd_case(n, H, T, S, max_pos, pad):
    """operands, the reference's O (bf16) / lse (f32) and the float64 dq, dk, dv for them; computed once per case"""
    key = (n, H, T, S, max_pos, pad)
    if key not in _cache:
        qkv, posq, posk, idx, mask = _attn_case(n, H, T, S, max_pos, pad)
        d = H * 64
        g = torch.Generator().manual_seed(7 * T + S)
        dout = torch.randn(n * T, d, generator=g).to(BF16)
        q, k, v = (_heads(qkv.double()[:, i * d:(i + 1) * d], n, T, H) for i in range(3))
        pq, pk = (t.double().reshape(2 * S, H, 64).transpose(0, 1) for t in (posq, posk))
        O, lse = G.attention_stats(q, k, v, pq, pk, idx, mask, SCALE)
        o16 = _rows(O, n, T, H).to(BF16)
        lse32 = lse.float()
        *want, ndq, ndk = G.attention_backward(q, k, v, pq, pk, idx, mask, SCALE, _heads(dout.double(), n, T, H),
                                               O=_heads(o16.double(), n, T, H), lse=lse32.double(), f32_tol=F32_TOL)
        _cache[key] = dict(qkv=qkv, posq=posq, posk=posk, idx=idx, mask=mask, dout=dout, o16=o16, lse32=lse32, lse64=lse,
                           O64=_rows(O, n, T, H), want=[_rows(t, n, T, H) for t in want],
                           noise=[float(ndq.norm()), float(ndk.norm()), 0.0])
    return _cache[key]


def _attn_bwd_run(c, n, H, T, S, mask_dtype=torch.float32):
    lib = _lib()
    dev = {k: c[k].cuda() for k in ("qkv", "posq", "posk", "idx", "dout", "o16", "lse32")}
    m = None if c["mask"] is None else c["mask"].to(mask_dtype).cuda()
    before = {k: _bits(dev[k]) for k in ("qkv", "o16", "lse32", "dout")}
    dqkv = torch.full((n * T, 3 * H * 64), float("nan"), dtype=BF16, device="cuda")
    delta = torch.empty(n * H * T, device="cuda")
    lib.deberta_attn_bwd(dev["qkv"], dev["posq"], dev["posk"], dev["idx"], m, dev["o16"], dev["lse32"].reshape(-1), dev["dout"], delta, dqkv,
                         n, H, T, S, SCALE)
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(_bits(dev[k]), b), f"{k} was written"
    return dqkv.cpu()


def _check_attn_bwd(n, H, T, S, max_pos, pad, mask_dtype=torch.float32):
    c = _attn_bwd_case(n, H, T, S, max_pos, pad)
    got = _attn_bwd_run(c, n, H, T, S, mask_dtype)
    again = _attn_bwd_run(c, n, H, T, S, mask_dtype)
    assert not torch.isnan(got.float()).any(), "an element of dqkv was not written"
    assert torch.equal(_bits(got), _bits(again)), "two runs differ"
    d = H * 64
    parts = [got[:, i * d:(i + 1) * d].double() for i in range(3)]
    errs = [float((p - w).norm()) for p, w in zip(parts, c["want"])]
    bounds = [BOUND_A * float(w.norm()) + nz for w, nz in zip(c["want"], c["noise"])]
    print(f"deberta attention backward n={n} H={H} T={T} S={S} max_pos={max_pos} pad={pad} ({mask_dtype}): error / bound dQ "
          f"{errs[0] / bounds[0]:.3e} dK {errs[1] / bounds[1]:.3e} dV {errs[2] / bounds[2]:.3e}; rel L2 "
          + " ".join(f"{l2_rel(p, w):.3e}" for p, w in zip(parts, c["want"]))
          + "; f32 noise term / BOUND_A ||want|| " + " ".join(f"{nz / max(BOUND_A * float(w.norm()), 1e-300):.1e}" for w, nz in zip(c["want"][:2], c["noise"])))
    assert all(e <= b for e, b in zip(errs, bounds)), (errs, bounds)
    return c, parts


@pytest.mark.parametrize("n,H,T,S,max_pos,pad", [c for c in ATTN_CASES if c[5] is None])
def test_attention_backward_against_float64(n, H, T, S, max_pos, pad):
    _check_attn_bwd(n, H, T, S, max_pos, pad)


@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.uint8, torch.bool])
def test_attention_backward_with_a_padded_item(mask_dtype):
    n, H, T, S, max_pos, pad = ATTN_CASES[2]
    c, (dq, dk, dv) = _check_attn_bwd(n, H, T, S, max_pos, pad, mask_dtype)
    masked = torch.arange(T + pad, 2 * T)
    assert bool((dq[masked] == 0).all()), "dQ of a masked query row"
    assert bool((dk[masked] == 0).all()), "dK of a masked key"
    uniform = c["dout"].double()[masked].sum(dim=0, keepdim=True) / T                      # 1/T dO_i of the masked query rows
    e = l2_rel(dv[masked], uniform.expand(T - pad, -1))
    print(f"dV of the masked keys against 1/T sum of the masked rows' dO: {e:.3e} (bound {BOUND_A})")
    assert e <= BOUND_A


@pytest.mark.parametrize("n,H,T,S,max_pos,pad", ATTN_CASES)
def test_attention_forward_with_lse(n, H, T, S, max_pos, pad):
    lib = _lib()
    c = _attn_bwd_case(n, H, T, S, max_pos, pad)
    qkv, posq, posk, idx = (c[k].cuda() for k in ("qkv", "posq", "posk", "idx"))
    m = None if c["mask"] is None else c["mask"].cuda()
    plain = torch.full((n * T, H * 64), float("nan"), dtype=BF16, device="cuda")
    out = plain.clone()
    lse = torch.full((n, H, T), float("nan"), device="cuda")
    lib.deberta_attn_fwd(qkv, posq, posk, idx, m, plain, n, H, T, S, SCALE)
    lib.deberta_attn_fwd(qkv, posq, posk, idx, m, out, n, H, T, S, SCALE, lse=lse)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(plain))
    on = torch.ones(n, T, dtype=torch.bool) if c["mask"] is None else c["mask"] != 0
    sel = on[:, None, :].expand(n, H, T)
    ref, got = c["lse64"][sel], lse.cpu().double()[sel]
    bound = F32_TOL * max(float(ref.abs().max()), 1.0)
    err = float((got - ref).abs().max())
    print(f"deberta lse n={n} H={H} T={T} S={S}: max abs error {err:.3e} (bound {bound:.3e})")
    assert bool(torch.isfinite(got).all()) and err <= bound
    assert not torch.isnan(lse).any()


# ---- streaming kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("rows,cols", [(70, 512), (9, 3072)])
def test_gelu_out_of_place_and_backward(rows, cols, has_bias):
    lib = _lib()
    g = torch.Generator().manual_seed(rows + cols)
    h = (2.0 * torch.randn(rows, cols, generator=g)).to(BF16)
    dg = torch.randn(rows, cols, generator=g).to(BF16)
    bias = 0.3 * torch.randn(cols, generator=g) if has_bias else None
    hd, dgd, bd = h.cuda(), dg.cuda(), None if bias is None else bias.cuda()
    inplace = hd.clone()
    lib.bias_gelu(inplace, bd)
    out = torch.full_like(hd, float("nan"))
    lib.bias_gelu_to(hd, bd, out)
    assert torch.equal(_bits(out), _bits(inplace)) and torch.equal(_bits(hd), _bits(h))
    v64 = (h.float() + bias if has_bias else h.float()).double()               # the f32 sum the kernel forms, exactly
    Phi64, vphi64 = 0.5 * torch.erfc(-v64 / math.sqrt(2.0)), v64 * torch.exp(-0.5 * v64 * v64) / math.sqrt(2.0 * math.pi)
    want64 = dg.double() * (Phi64 + vphi64)
    # one bf16 ulp of the float64 value plus four f32 ulps of the formula's two terms: near v = -0.7518 they cancel (gelu' = 0) and an
    # f32 v comes arbitrarily close to that root.  The kernel forms Phi through erfc, so the left tail needs no term of its own
    # (tests/test_gelu_domain_gpu.py holds it to half an ulp over every finite bf16 input).
    bound = _bf16_ulp(want64) + 2.0 ** -22 * dg.double().abs() * (Phi64 + vphi64.abs())
    dh = torch.full_like(hd, float("nan"))
    lib.bias_gelu_bwd(dgd, hd, bd, dh)
    alias = dgd.clone()
    lib.bias_gelu_bwd(alias, hd, bd, alias)
    torch.cuda.synchronize()
    got = dh.cpu().float()
    worst = float(((got.double() - want64).abs() / bound).max())
    print(f"gelu backward ({rows}, {cols}) bias={has_bias}: worst error / bound against float64 = {worst:.3f}")
    assert not torch.isnan(got).any() and worst <= 1.0
    assert torch.equal(_bits(alias), _bits(dh)) and torch.equal(_bits(dgd), _bits(dg))


@pytest.mark.parametrize("rows,d", [(70, 256), (9, 768), (5, 1024)])
def test_embed_backward_against_float64(rows, d):
    lib = _lib()
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * 2.0 + 0.3
    gamma, beta = 1.0 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    mask = (torch.rand(rows, generator=g) > 0.3).float()
    mask[0], mask[-1] = 1.0, 0.0
    dy = torch.randn(rows, d, generator=g).to(BF16)
    leaf = x.double().requires_grad_(True)
    y = deberta_ref.layer_norm(leaf, gamma.double(), beta.double(), 1e-7) * mask.double().unsqueeze(-1)
    (want,) = torch.autograd.grad(y, leaf, dy.double())
    for m in (mask.cuda(), mask.bool().cuda()):
        got = torch.full((rows, d), float("nan"), device="cuda")
        lib.deberta_embed_bwd(x.cuda(), gamma.cuda(), 1e-7, m, dy.cuda(), got)
        err = l2_rel(got.double().cpu(), want)
        print(f"deberta embed backward rows={rows} d={d} ({m.dtype}): rel L2 {err:.3e} (bound 1e-5)")
        assert not torch.isnan(got).any() and err <= 1e-5
        assert bool((got.cpu()[mask == 0] == 0).all())


# ---- refusals -----------------------------------------------------------------------------------------------
def test_backward_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    nan32 = torch.full((1 << 14,), float("nan"), device="cuda")
    f = torch.zeros(1 << 14, device="cuda")
    b = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    idx = torch.zeros(4096, dtype=torch.int32, device="cuda")
    u8 = torch.ones(4096, dtype=torch.uint8, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    fwd = lambda qkv, ld, ix, mask, kind, lse, n, H, T, S, hd, scale=SCALE: L.mmf_deberta_attn_fwd_lse(
        qkv, p(b), p(b), ld, ix, mask, kind, p(nan16), lse, n, H, T, S, hd, scale, s)
    bwd = lambda qkv, ld, ix, mask, kind, lse, dout, delta, dqkv, n, H, T, S, hd, scale=SCALE: L.mmf_deberta_attn_bwd(
        qkv, p(b), p(b), ld, ix, mask, kind, p(b), lse, dout, delta, dqkv, n, H, T, S, hd, scale, s)
    gelu_to = lambda h, bias, g_, rows, cols, ld: L.mmf_bias_gelu_bf16_to(h, bias, g_, rows, cols, ld, s)
    gelu_bwd = lambda dg, h, dh, rows, cols, ld: L.mmf_bias_gelu_bwd_bf16(dg, h, p(f), dh, rows, cols, ld, s)
    emb = lambda e, mask, kind, dout, dx, rows, d: L.mmf_deberta_embed_bwd(e, p(f), 1e-7, mask, kind, dout, dx, rows, d, s)
    A, B_ = "mmf_deberta_attn_fwd_lse", "mmf_deberta_attn_bwd"
    cases = [
        (A, lambda: fwd(p(b), 128, p(idx), None, 0, None, 1, 2, 16, 8, 64), E_SHAPE),                       # no lse
        (A, lambda: fwd(p(b), 128, p(idx), None, 0, p(nan32), 1, 2, 16, 8, 96), E_UNSUPPORTED),
        (A, lambda: fwd(p(b), 128, p(idx), None, 0, p(nan32), 1, 2, 1025, 8, 64), E_UNSUPPORTED),
        (A, lambda: fwd(p(b), 64, p(idx), None, 0, p(nan32), 1, 2, 16, 8, 64), E_SHAPE),
        (A, lambda: fwd(p(b), 128, p(idx), None, 0, p(nan32, 2), 1, 2, 16, 8, 64), E_ALIGN),
        (A, lambda: fwd(p(b, 2), 128, p(idx), None, 0, p(nan32), 1, 2, 16, 8, 64), E_ALIGN),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, None, p(b), p(nan32), p(nan16), 1, 2, 16, 8, 64), E_SHAPE),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), None, p(nan32), p(nan16), 1, 2, 16, 8, 64), E_SHAPE),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b), None, p(nan16), 1, 2, 16, 8, 64), E_SHAPE),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b), p(nan32), None, 1, 2, 16, 8, 64), E_SHAPE),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b), p(nan32), p(nan16), 1, 2, 0, 8, 64), E_SHAPE),
        (B_, lambda: bwd(p(b), 128, p(idx), p(u8), 0, p(f), p(b), p(nan32), p(nan16), 1, 2, 16, 8, 64), E_SHAPE),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b), p(nan32), p(nan16), 1, 2, 16, 8, 64, 0.0), E_SHAPE),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b), p(nan32), p(nan16), 1, 2, 16, 8, 96), E_UNSUPPORTED),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b), p(nan32), p(nan16), 1, 2, 1025, 8, 64), E_UNSUPPORTED),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b), p(nan32), p(nan16), 1, 2, 16, 257, 64), E_UNSUPPORTED),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b, 2), p(nan32), p(nan16), 1, 2, 16, 8, 64), E_ALIGN),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f), p(b), p(nan32), p(nan16, 2), 1, 2, 16, 8, 64), E_ALIGN),
        (B_, lambda: bwd(p(b), 128, p(idx), None, 0, p(f, 2), p(b), p(nan32), p(nan16), 1, 2, 16, 8, 64), E_ALIGN),
        (B_, lambda: bwd(p(b), 132, p(idx), None, 0, p(f), p(b), p(nan32), p(nan16), 1, 2, 16, 8, 64), E_ALIGN),
        ("mmf_bias_gelu_bf16_to", lambda: gelu_to(None, p(f), p(nan16), 8, 64, 64), E_SHAPE),
        ("mmf_bias_gelu_bf16_to", lambda: gelu_to(p(b), p(f), p(nan16), 0, 64, 64), E_SHAPE),
        ("mmf_bias_gelu_bf16_to", lambda: gelu_to(p(b), p(f), p(nan16), 8, 60, 64), E_UNSUPPORTED),
        ("mmf_bias_gelu_bf16_to", lambda: gelu_to(p(b), p(f), p(nan16), 8, 64, 56), E_UNSUPPORTED),
        ("mmf_bias_gelu_bf16_to", lambda: gelu_to(p(b), p(f), p(nan16, 2), 8, 64, 64), E_ALIGN),
        ("mmf_bias_gelu_bwd_bf16", lambda: gelu_bwd(p(b), None, p(nan16), 8, 64, 64), E_SHAPE),
        ("mmf_bias_gelu_bwd_bf16", lambda: gelu_bwd(p(b), p(b), p(nan16), 8, 60, 64), E_UNSUPPORTED),
        ("mmf_bias_gelu_bwd_bf16", lambda: gelu_bwd(p(b, 2), p(b), p(nan16), 8, 64, 64), E_ALIGN),
        ("mmf_deberta_embed_bwd", lambda: emb(None, None, 0, p(b), p(nan32), 8, 256), E_SHAPE),
        ("mmf_deberta_embed_bwd", lambda: emb(p(f), None, 1, p(b), p(nan32), 8, 256), E_SHAPE),             # mask_kind without a mask
        ("mmf_deberta_embed_bwd", lambda: emb(p(f), None, 0, p(b), p(nan32), 8, 2048), E_UNSUPPORTED),
        ("mmf_deberta_embed_bwd", lambda: emb(p(f), None, 0, p(b), p(nan32), 8, 250), E_UNSUPPORTED),
        ("mmf_deberta_embed_bwd", lambda: emb(p(f, 4), None, 0, p(b), p(nan32), 8, 256), E_ALIGN),
        ("mmf_deberta_embed_bwd", lambda: emb(p(f), None, 0, p(b, 2), p(nan32), 8, 256), E_ALIGN),
    ]
    for name, call, want in cases:
        rc = call()
        assert rc == want, (name, rc, want, L.mmf_last_error())
        assert name.encode() in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all())                 # nothing was launched


# ---- NativeDeberta: the gradient with respect to inputs_embeds ------------------------------------------------------
PROMPT = 10


def _grad_inputs(cfg, n, text, pad_from, seed):
    """n items of PROMPT + text tokens as unit-variance input embeddings; the last item padded from token ``pad_from`` of its
    text, the prompt's mask ones prepended; a random gradient of the result and one that is non-zero on row 0 of each item only"""
    g = torch.Generator().manual_seed(seed)
    T = PROMPT + text
    emb = torch.randn(n, T, cfg.hidden_size, generator=g)
    mask = torch.ones(n, T, dtype=torch.int64)
    mask[n - 1, PROMPT + pad_from:] = 0
    dout = torch.randn(n, T, cfg.hidden_size, generator=g)
    cls = torch.zeros_like(dout)
    cls[:, 0] = dout[:, 0]
    return emb, mask, dout, cls


def _ref_grad(sd, emb, mask, cfg, dout, dtype, bf16_storage):
    leaf = emb.to(dtype).requires_grad_(True)
    out = deberta_ref.deberta_forward(sd, leaf, mask, cfg, bf16_storage=bf16_storage, dtype=dtype)
    return torch.autograd.grad(out, leaf, dout.to(dtype))[0]


def _native_grad(m, emb, mask, dout):
    leaf = emb.cuda().requires_grad_(True)
    out = m(inputs_embeds=leaf, attention_mask=mask.cuda()).last_hidden_state
    assert out.requires_grad and out.dtype == torch.float32
    (grad,) = torch.autograd.grad(out, leaf, dout.cuda())
    torch.cuda.synchronize()
    return grad.cpu()


def _check_grad(m, sd, cfg, emb, mask, douts, dtype, what):
    padded = mask == 0
    for tag, dout in douts:
        exact = _ref_grad(sd, emb, mask, cfg, dout, dtype, False)
        stored = _ref_grad(sd, emb, mask, cfg, dout, dtype, True)
        got = _native_grad(m, emb, mask, dout)
        model_err, err = l2_rel(stored, exact), l2_rel(got, exact)
        print(f"NativeDeberta d inputs_embeds, {what}, {tag} dO: vs exact {err:.3e} (bound (b) 2 x {model_err:.3e} = {2 * model_err:.3e}); "
              f"vs the bf16-storage gradient {l2_rel(got, stored):.3e}")
        assert got.dtype == torch.float32 and not torch.isnan(got).any()
        assert err <= 2 * model_err
        assert bool((got[padded] == 0).all()) and bool((exact[padded] == 0).all())


def test_input_gradient_against_float64_autograd_tiny():
    """2 layers, d 256, 4 heads, S 8; 2 items of 10 + 70 tokens, the last padded from token 50 of its text.  Bound (b); the
    storage model itself is 1.3e-2 to 1.5e-2 from the exact gradient here."""
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    emb, mask, dout, cls = _grad_inputs(cfg, 2, 70, 50, seed=40)
    _check_grad(_model(cfg, sd), sd, cfg, emb, mask, [("random", dout), ("CLS-row", cls)], torch.float64, "tiny 2 x (10 + 70)")


def test_input_gradient_against_autograd_base_sizes():
    """deberta-v3-base sizes (12 layers, d 768, 12 heads, S 256: the LayerNorm lane form and the real GEMM shapes), one item of
    10 + 54 tokens padded from token 40 of its text, float32 references.  Bound (b); the storage model is 3.0e-2 to 3.2e-2 here."""
    cfg = deberta_ref.base_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    emb, mask, dout, _ = _grad_inputs(cfg, 1, 54, 40, seed=41)
    _check_grad(_model(cfg, sd), sd, cfg, emb, mask, [("random", dout)], torch.float32, "base 1 x (10 + 54)")


def test_gradient_is_bit_repeatable_and_chunking_does_not_change_it():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    emb, mask, dout, _ = _grad_inputs(cfg, 5, 60, 30, seed=42)
    m2, m5 = _model(cfg, sd, chunk=2), _model(cfg, sd, chunk=5)
    g2, g2b, g5 = _native_grad(m2, emb, mask, dout), _native_grad(m2, emb, mask, dout), _native_grad(m5, emb, mask, dout)
    assert torch.equal(_bits(g2), _bits(g2b))
    print(f"chunk 2 vs chunk 5 gradients: rel L2 {l2_rel(g2, g5):.3e}, bit-equal {torch.equal(_bits(g2), _bits(g5))}")
    assert torch.equal(_bits(g2), _bits(g5))
    # the forward workspace is still the tables; the backward's is its own
    held = sum(v.numel() * v.element_size() for v in m2._ws.values() if isinstance(v, torch.Tensor))
    assert held == 2 * m2.workspace_bytes_per_item(70)
    mine = sum(m2._gws[name].numel() * m2._gws[name].element_size() for name, _, _ in m2._grad_table(70))
    assert mine == 2 * m2.grad_workspace_bytes_per_item(70)


def test_forward_and_backward_replay_from_a_captured_graph():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    emb, mask, dout, _ = _grad_inputs(cfg, 3, 60, 30, seed=43)
    m = _model(cfg, sd, chunk=2)
    eager = _native_grad(m, emb, mask, dout)
    static = emb.cuda().requires_grad_(True)
    k, dO = mask.cuda(), dout.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        torch.autograd.grad(m(inputs_embeds=static, attention_mask=k).last_hidden_state, static, dO)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(inputs_embeds=static, attention_mask=k).last_hidden_state
        (grad,) = torch.autograd.grad(out, static, dO)
    with torch.no_grad():
        static.copy_(torch.randn_like(static))
    graph.replay()
    other = grad.clone()
    with torch.no_grad():
        static.copy_(emb.cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(grad), _bits(eager))
    assert not torch.equal(_bits(other), _bits(eager))


def test_every_other_call_is_the_inference_path():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    emb, mask, dout, _ = _grad_inputs(cfg, 2, 70, 50, seed=44)
    ids = torch.randint(1, cfg.vocab_size, (2, 80), generator=torch.Generator().manual_seed(5)).cuda()
    fresh, used = _model(cfg, sd), _model(cfg, sd)
    _native_grad(used, emb, mask, dout)                                                 # `used` has taken the differentiable path
    e, k = emb.cuda(), mask.cuda()
    leaf = emb.cuda().requires_grad_(True)
    with torch.no_grad():
        a, b = used(inputs_embeds=leaf, attention_mask=k).last_hidden_state, fresh(inputs_embeds=e, attention_mask=k).last_hidden_state
    assert torch.equal(a, b) and not a.requires_grad
    a = used(inputs_embeds=e, attention_mask=k).last_hidden_state                       # grad mode on, embeds that do not require grad
    assert torch.equal(a, b) and not a.requires_grad
    a, b = used(input_ids=ids, attention_mask=k).last_hidden_state, fresh(input_ids=ids, attention_mask=k).last_hidden_state
    assert torch.equal(a, b) and not a.requires_grad
    # the differentiable forward returns the same bits
    assert torch.equal(used(inputs_embeds=leaf, attention_mask=k).last_hidden_state.detach(), fresh(inputs_embeds=e, attention_mask=k).last_hidden_state)
    from mmfusion import ops
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match="bf16 storage only"):
            used(inputs_embeds=leaf, attention_mask=k)
    finally:
        ops.set_precision(old)


# ---- TextEncoder: prompt tuning through the native backbone ---------------------------------------------------------
def test_text_encoder_prompt_embeddings_train_through_the_native_backbone():
    import config as cfgmod
    from models.encoders import TextEncoder
    tcfg = deberta_ref.tiny_config()
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.text_hidden_size = 256, 0.0, 256
    cfg.text_backbone = "native"
    cfg.text_backbone_kwargs = {k: v for k, v in deberta_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
    torch.manual_seed(3)
    enc = TextEncoder(cfg)
    sd = deberta_ref.seeded_weights(tcfg, seed=31)
    enc.model.load_state_dict(sd)
    g = torch.Generator().manual_seed(32)
    ids = torch.randint(1, tcfg.vocab_size, (2, 70), generator=g)
    mask = torch.ones(2, 70, dtype=torch.int64)
    ids[1, 50:], mask[1, 50:] = 0, 0
    P = cfg.prompt_length
    full = torch.cat([torch.ones(2, P, dtype=torch.int64), mask], dim=1)
    W_, b_ = enc.projection.weight.detach().double(), enc.projection.bias.detach().double()

    def ref_grad(bf16_storage):
        pe = enc.prompt_embeddings.detach().double().requires_grad_(True)
        x = torch.cat([pe.unsqueeze(0).expand(2, -1, -1), sd["embeddings.word_embeddings.weight"].double()[ids]], dim=1)
        out = deberta_ref.deberta_forward(sd, x, full, tcfg, bf16_storage=bf16_storage)
        (out[:, 0] @ W_.T + b_).sum().backward()
        return pe.grad
    exact, stored = ref_grad(False), ref_grad(True)
    enc = enc.cuda().eval()
    out = enc(ids.cuda(), mask.cuda(), use_prompt=True)
    assert out["features"].requires_grad
    out["features"].sum().backward()
    torch.cuda.synchronize()
    got = enc.prompt_embeddings.grad
    assert got is not None and float(got.abs().max()) > 0
    model_err, err = l2_rel(stored, exact), l2_rel(got, exact)
    print(f"TextEncoder prompt_embeddings.grad through the native backbone: vs exact {err:.3e} (bound (b) 2 x {model_err:.3e})")
    assert err <= 2 * model_err
    assert enc.projection.weight.grad is not None and float(enc.projection.weight.grad.abs().max()) > 0
    assert enc.projection.bias.grad is not None
    # without the prompt nothing requires grad through the backbone, and the output is the inference one
    plain = enc(ids.cuda(), mask.cuda(), use_prompt=False)
    assert not plain["sequence_output"].requires_grad
    with torch.no_grad():
        again = enc(ids.cuda(), mask.cuda(), use_prompt=False)
    assert torch.equal(plain["sequence_output"], again["sequence_output"])
