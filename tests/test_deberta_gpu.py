"""GPU: the DeBERTa kernels (csrc/deberta.hip) against float64, and ``mmfusion.deberta.NativeDeberta`` against the explicit
restatement tests/deberta_ref.py, which needs neither the reference nor transformers.

Bounds.  (a) against a float64 / restatement reference with the same storage format (bf16-rounded inputs, bf16 stores):
relative L2 <= 2e-2, the project's bound for a kernel against such an oracle.  (b) against the exact restatement: 2 x the
error of the bf16-storage restatement against the exact one on the same inputs, computed here on the CPU: the error of an
L-layer bf16 residual stream is modelled by the storage format, not by the code under test, with a factor 2 for summation
order (tests/test_w2v_gpu.py's rule)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_ref  # noqa: E402
from helpers import BOUND_A, _bf16_ulp, _lib, l2_rel  # noqa: E402

BF16 = torch.bfloat16
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deberta_tiny.npz")


# ---- the attention kernel ------------------------------------------------------------------------------------
def _attn_case(n, H, T, S, max_pos, pad_from=None, seed=0):
    """bf16-rounded operands: fused qkv rows, the two position tables, the index table, and a mask padding the LAST item from
    ``pad_from`` (None: no mask)"""
    g = torch.Generator().manual_seed(1000 * T + 10 * S + H + seed)
    d = H * 64
    qkv = (1.5 * torch.randn(n * T, 3 * d, generator=g)).to(BF16)
    posq, posk = (1.2 * torch.randn(2 * S, d, generator=g)).to(BF16), (1.2 * torch.randn(2 * S, d, generator=g)).to(BF16)
    idx = deberta_ref.bucket_index(T, S, max_pos)
    mask = None
    if pad_from is not None:
        mask = torch.ones(n, T)
        mask[n - 1, pad_from:] = 0
    return qkv, posq, posk, idx, mask


def _attn_ref(qkv, posq, posk, idx, mask, n, H, T, S):
    d = H * 64
    q, k, v = (qkv.double()[:, i * d:(i + 1) * d].reshape(n, T, H, 64).transpose(1, 2) for i in range(3))
    pq, pk = (t.double().reshape(2 * S, H, 64).transpose(0, 1) for t in (posq, posk))
    out = deberta_ref.disentangled_attention(q, k, v, pq, pk, idx, mask, math.sqrt(3.0 * 64))
    return out.transpose(1, 2).reshape(n * T, d)


def _attn_run(qkv, posq, posk, idx, mask, n, H, T, S, mask_dtype=torch.float32):
    lib = _lib()
    out = torch.full((n * T, H * 64), float("nan"), dtype=BF16, device="cuda")
    m = None if mask is None else mask.to(mask_dtype).cuda()
    lib.deberta_attn_fwd(qkv.cuda(), posq.cuda(), posk.cuda(), idx.cuda(), m, out, n, H, T, S, math.sqrt(3.0 * 64))
    torch.cuda.synchronize()
    return out.cpu().double()


@pytest.mark.parametrize("n,H,T,S,max_pos,pad_from", [
    (1, 3, 1, 8, 32, None),              # T = 1
    (1, 2, 33, 8, 32, None),             # ragged T: one key past a 32-key tile
    (2, 2, 200, 256, 512, None),         # real geometry: linear and log region, four query blocks
    (1, 1, 512, 256, 512, None),         # full length
    (1, 1, 530, 256, 512, None),         # T > max_position: the clamp binds
    (2, 2, 70, 8, 32, None),             # both clamps, ragged T, mask NULL
])
def test_attention_against_float64(n, H, T, S, max_pos, pad_from):
    case = _attn_case(n, H, T, S, max_pos, pad_from)
    want = _attn_ref(*case, n, H, T, S)
    got = _attn_run(*case, n, H, T, S)
    err = l2_rel(got, want)
    print(f"deberta attention n={n} H={H} T={T} S={S} max_pos={max_pos}: rel L2 {err:.3e} (bound {BOUND_A})")
    assert not torch.isnan(got).any() and err <= BOUND_A


@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.uint8, torch.bool])
def test_attention_with_a_padded_item_row_set_by_row_set(mask_dtype):
    """(2, 2, 70, 8, 32), item 1 padded from token 50.  Masked-query rows (uniform over all 70 keys), real rows, and a copy whose
    padded keys carry K = V = 50: its real rows must be the first run's."""
    n, H, T, S, max_pos, pad = 2, 2, 70, 8, 32, 50
    qkv, posq, posk, idx, mask = _attn_case(n, H, T, S, max_pos, pad)
    want = _attn_ref(qkv, posq, posk, idx, mask, n, H, T, S)
    got = _attn_run(qkv, posq, posk, idx, mask, n, H, T, S, mask_dtype)
    padded = torch.arange(T + pad, 2 * T)
    real = torch.cat([torch.arange(0, T + pad)])
    e_pad, e_real = l2_rel(got[padded], want[padded]), l2_rel(got[real], want[real])
    d = H * 64
    loud = qkv.clone()
    loud[T + pad:, d:] = 50.0
    got2 = _attn_run(loud, posq, posk, idx, mask, n, H, T, S, mask_dtype)
    e_loud = l2_rel(got2[real], want[real])
    print(f"padded item ({mask_dtype}): masked-query rows {e_pad:.3e}, real rows {e_real:.3e}, real rows with K = V = 50 on the padded keys "
          f"{e_loud:.3e} (bound {BOUND_A}); bit-equal to the first run: {torch.equal(got2[real], got[real])}")
    assert not torch.isnan(got).any() and not torch.isnan(got2).any()
    assert e_pad <= BOUND_A and e_real <= BOUND_A and e_loud <= BOUND_A
    # the masked-query rows are the plain mean of V over all T keys of that item
    v1 = qkv.double()[T:, 2 * d:]
    assert l2_rel(got[padded], v1.mean(dim=0, keepdim=True).expand(T - pad, -1)) <= BOUND_A


# ---- the embedding kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["ids", "embeds"])
@pytest.mark.parametrize("rows,d,vocab", [(70, 256, 300), (9, 768, 50), (5, 1024, 7)])
def test_embed_within_one_bf16_ulp_of_f32_layernorm(route, rows, d, vocab):
    lib = _lib()
    g = torch.Generator().manual_seed(rows + d)
    table = torch.randn(vocab, d, generator=g) * 2.0 + 0.3
    gamma, beta = 1.0 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    ids = torch.randint(0, vocab, (rows,), generator=g)
    ids[0], ids[-1] = 0, vocab - 1
    mask = (torch.rand(rows, generator=g) > 0.3).float()
    x = table[ids]
    want = deberta_ref.layer_norm(x.double(), gamma.double(), beta.double(), 1e-7) * mask.double().unsqueeze(-1)
    out = torch.full((rows, d), float("nan"), dtype=BF16, device="cuda")
    if route == "ids":
        lib.deberta_embed(out, table.cuda(), gamma.cuda(), beta.cuda(), 1e-7, ids=ids.cuda(), mask=mask.cuda())
    else:
        lib.deberta_embed(out, None, gamma.cuda(), beta.cuda(), 1e-7, embeds=x.cuda(), mask=mask.bool().cuda())
    got = out.cpu().double()
    worst = float(((got - want).abs() / _bf16_ulp(want.float()).double()).max())
    print(f"deberta embed ({route}) rows={rows} d={d}: worst error / bf16 ulp = {worst:.3f}")
    assert not torch.isnan(got).any() and worst <= 1.0
    assert bool((got[mask == 0] == 0).all())


# ---- refusals -----------------------------------------------------------------------------------------------
def test_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    f = torch.zeros(1 << 14, device="cuda")
    b = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    idx = torch.zeros(4096, dtype=torch.int32, device="cuda")
    u8 = torch.ones(4096, dtype=torch.uint8, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    sc = math.sqrt(192.0)
    embed = lambda ids_, emb, tab, mask, kind, out, rows, d, vocab: L.mmf_deberta_embed(ids_, emb, tab, p(f), p(f), 1e-7, mask, kind, out, rows, d, vocab, s)
    attn = lambda qkv, pq, ld, ix, mask, kind, out, n, H, T, S, hd, scale=sc: L.mmf_deberta_attn_fwd(qkv, pq, pq, ld, ix, mask, kind, out, n, H, T, S, hd, scale, s)
    cases = [
        ("mmf_deberta_embed", lambda: embed(p(ids), p(f), p(f), None, 0, p(nan16), 8, 256, 16), E_SHAPE),          # both ids and embeds
        ("mmf_deberta_embed", lambda: embed(None, None, p(f), None, 0, p(nan16), 8, 256, 16), E_SHAPE),            # neither
        ("mmf_deberta_embed", lambda: embed(p(ids), None, None, None, 0, p(nan16), 8, 256, 16), E_SHAPE),          # ids without a table
        ("mmf_deberta_embed", lambda: embed(p(ids), None, p(f), None, 0, p(nan16), 0, 256, 16), E_SHAPE),
        ("mmf_deberta_embed", lambda: embed(p(ids), None, p(f), None, 1, p(nan16), 8, 256, 16), E_SHAPE),          # mask_kind without a mask
        ("mmf_deberta_embed", lambda: embed(p(ids), None, p(f), None, 0, p(nan16), 8, 2048, 4), E_UNSUPPORTED),
        ("mmf_deberta_embed", lambda: embed(p(ids), None, p(f), None, 0, p(nan16), 8, 250, 16), E_UNSUPPORTED),
        ("mmf_deberta_embed", lambda: embed(None, p(f, 4), None, None, 0, p(nan16), 8, 256, 0), E_ALIGN),
        ("mmf_deberta_embed", lambda: embed(p(ids), None, p(f), None, 0, p(nan16, 2), 8, 256, 16), E_ALIGN),
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 128, p(idx), None, 0, p(nan16), 1, 2, 16, 8, 96), E_UNSUPPORTED),   # head_dim 96
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 128, p(idx), None, 0, p(nan16), 1, 2, 1025, 8, 64), E_UNSUPPORTED),
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 128, p(idx), None, 0, p(nan16), 1, 2, 16, 257, 64), E_UNSUPPORTED),
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 128, p(idx), None, 0, p(nan16), 1, 2, 0, 8, 64), E_SHAPE),
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 64, p(idx), None, 0, p(nan16), 1, 2, 16, 8, 64), E_SHAPE),          # ld_pos < H * 64
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 128, None, None, 0, p(nan16), 1, 2, 16, 8, 64), E_SHAPE),
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 128, p(idx), p(u8), 0, p(nan16), 1, 2, 16, 8, 64), E_SHAPE),        # a mask with mask_kind 0
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 128, p(idx), None, 0, p(nan16), 1, 2, 16, 8, 64, 0.0), E_SHAPE),
        ("mmf_deberta_attn_fwd", lambda: attn(p(b, 2), p(b), 128, p(idx), None, 0, p(nan16), 1, 2, 16, 8, 64), E_ALIGN),
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 132, p(idx), None, 0, p(nan16), 1, 2, 16, 8, 64), E_ALIGN),
        ("mmf_deberta_attn_fwd", lambda: attn(p(b), p(b), 128, p(idx), p(u8, 2), 1, p(nan16), 1, 2, 16, 8, 64), E_ALIGN),     # f32 mask off 4 bytes
    ]
    for name, call, want in cases:
        rc = call()
        assert rc == want, (name, rc, want, L.mmf_last_error())
        assert name.encode() in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all())                                                # nothing was launched


# ---- module ------------------------------------------------------------------------------------------------
def _inputs(cfg, n, T, seed, pad_from=None):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, cfg.vocab_size, (n, T), generator=g)
    mask = torch.ones(n, T, dtype=torch.int64)
    if pad_from is not None:
        ids[n - 1, pad_from:], mask[n - 1, pad_from:] = 0, 0
    return ids, mask


def _model(cfg, sd, chunk=None):
    from mmfusion.deberta import NativeDeberta
    kw = deberta_ref.config_kwargs(cfg)
    if chunk is not None:
        kw["chunk"] = chunk
    m = NativeDeberta(**kw)
    m.load_state_dict(sd)
    return m.cuda().eval()


def _setup(n, T, seed=21, chunk=None, pad_from=None):
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=seed)
    ids, mask = _inputs(cfg, n, T, seed + 1, pad_from)
    return cfg, sd, _model(cfg, sd, chunk), ids, mask


@pytest.fixture(scope="module")
def base_case():
    cfg = deberta_ref.base_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    return cfg, sd, _model(cfg, sd)


def test_forward_against_restatement_tiny():
    """(3, 70) with the last item padded from token 50: bound (a) against the bf16-storage restatement, bound (b) against the exact
    one; all rows, padded ones included"""
    cfg, sd, m, ids, mask = _setup(3, 70, pad_from=50)
    stored = deberta_ref.deberta_forward(sd, ids, mask, cfg, bf16_storage=True)
    exact = deberta_ref.deberta_forward(sd, ids, mask, cfg)
    got = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    assert got.dtype == torch.float32 and got.shape == stored.shape and not got.requires_grad
    a, b, model_err = l2_rel(got, stored), l2_rel(got, exact), l2_rel(stored, exact)
    a_pad = l2_rel(got[2, 50:], stored[2, 50:])
    print(f"NativeDeberta tiny 3 x 70: (a) vs bf16-storage restatement {a:.3e}, padded rows {a_pad:.3e} (bound {BOUND_A}); "
          f"(b) vs exact restatement {b:.3e} (bound {2 * model_err:.3e})")
    assert a <= BOUND_A and a_pad <= BOUND_A and b <= 2 * model_err
    # the inputs_embeds route on the same inputs is the ids route
    emb = m.embeddings.word_embeddings(ids.cuda())
    got2 = m(inputs_embeds=emb, attention_mask=mask.cuda().bool()).last_hidden_state
    assert torch.equal(got2, got)


def test_forward_against_restatement_base(base_case):
    """deberta-v3-base sizes, (2, 128) with the second item padded from token 100, fp32 restatement with bf16 storage: bound (a)"""
    cfg, sd, m = base_case
    ids, mask = _inputs(cfg, 2, 128, 23, pad_from=100)
    stored = deberta_ref.deberta_forward(sd, ids, mask, cfg, bf16_storage=True, dtype=torch.float32)
    got = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    a = l2_rel(got, stored)
    print(f"NativeDeberta base 2 x 128: (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A})")
    assert got.shape == stored.shape and a <= BOUND_A


def test_forward_base_at_full_length(base_case):
    """One item of 512 tokens (padded from 480) against the fp32 restatement with bf16 storage, bound (a).  On the CPU the
    bf16-storage restatement itself is 8.5e-3 from the fp32 one at this size (weights seed 21, ids seed 22), inside
    bound (a), so all twelve layers are kept."""
    cfg, sd, m = base_case
    ids, mask = _inputs(cfg, 1, 512, 22)
    mask[0, 480:] = 0
    stored = deberta_ref.deberta_forward(sd, ids, mask, cfg, bf16_storage=True, dtype=torch.float32)
    got = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    a = l2_rel(got, stored)
    print(f"NativeDeberta base 1 x 512: (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A})")
    assert got.shape == stored.shape and a <= BOUND_A


# ---- behaviour -----------------------------------------------------------------------------------------------
def test_chunking_is_bit_repeatable_and_the_workspace_is_the_tables():
    cfg, sd, m2, ids, mask = _setup(5, 70, chunk=2, pad_from=40)
    m5 = _model(cfg, sd, chunk=5)
    i, k = ids.cuda(), mask.cuda()
    f2, f5 = m2(input_ids=i, attention_mask=k).last_hidden_state, m5(input_ids=i, attention_mask=k).last_hidden_state
    assert torch.equal(f2, f5)
    assert torch.equal(m2(input_ids=i, attention_mask=k).last_hidden_state, f2)
    assert m2._ws["x"].numel() == 2 * 70 * cfg.hidden_size and m5._ws["x"].numel() == 5 * 70 * cfg.hidden_size
    held = sum(v.numel() * v.element_size() for v in m2._ws.values() if isinstance(v, torch.Tensor))
    assert held == 2 * m2.workspace_bytes_per_item(70)
    short = m2(input_ids=i[:, :33].contiguous(), attention_mask=k[:, :33].contiguous()).last_hidden_state     # a shorter sequence: the same workspace
    assert tuple(short.shape) == (5, 33, cfg.hidden_size) and m2._ws["x"].numel() == 2 * 70 * cfg.hidden_size
    with pytest.raises(ValueError, match="1 .. 1024"):
        m2(input_ids=torch.zeros(1, 1025, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        m2(input_ids=i.int())
    with pytest.raises(TypeError):
        m2(inputs_embeds=torch.zeros(1, 8, cfg.hidden_size, dtype=torch.float64, device="cuda"))


def test_forward_replays_from_a_captured_graph():
    cfg, sd, m, ids, mask = _setup(3, 70, chunk=2, pad_from=50)
    i, k = ids.cuda(), mask.cuda()
    eager = m(input_ids=i, attention_mask=k).last_hidden_state.clone()
    static = i.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(input_ids=static, attention_mask=k)                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(input_ids=static, attention_mask=k).last_hidden_state
    static.copy_(torch.randint_like(static, 1, cfg.vocab_size))
    graph.replay()
    other = out.clone()
    static.copy_(i)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert not torch.equal(other, eager)


def test_load_state_dict_refreshes_what_the_kernels_read():
    cfg, sd, m, ids, mask = _setup(2, 70, pad_from=60)
    i, k = ids.cuda(), mask.cuda()
    first = m(input_ids=i, attention_mask=k).last_hidden_state.clone()
    sd2 = deberta_ref.seeded_weights(cfg, seed=99)
    m.load_state_dict(sd2)
    second = m(input_ids=i, attention_mask=k).last_hidden_state.clone()
    want = deberta_ref.deberta_forward(sd2, ids, mask, cfg, bf16_storage=True)
    assert l2_rel(second, want) <= BOUND_A and l2_rel(first, want) > 10 * BOUND_A
    # new relative embeddings alone: the cached LayerNorm(rel) and every layer's posQ / posK follow them
    sd3 = dict(sd2)
    sd3["encoder.rel_embeddings.weight"] = deberta_ref.seeded_weights(cfg, seed=5)["encoder.rel_embeddings.weight"]
    m.load_state_dict(sd3)
    third = m(input_ids=i, attention_mask=k).last_hidden_state
    want3 = deberta_ref.deberta_forward(sd3, ids, mask, cfg, bf16_storage=True)
    moved = l2_rel(want3, want)
    print(f"new relative embeddings: restatement moved by {moved:.3e}; native vs new {l2_rel(third, want3):.3e}, vs old {l2_rel(third, want):.3e}")
    assert l2_rel(third, want3) <= BOUND_A and moved > 3 * BOUND_A and l2_rel(third, want) > BOUND_A


def test_fp32_parity_mode_is_refused():
    from mmfusion import ops
    cfg, sd, m, ids, mask = _setup(1, 16)
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match="bf16 storage only"):
            m(input_ids=ids.cuda())
        with pytest.raises(RuntimeError, match="bf16 storage only"):
            m(inputs_embeds=torch.zeros(1, 16, cfg.hidden_size, device="cuda"))
    finally:
        ops.set_precision(old)


def test_huggingface_state_dict_to_native_output():
    """the golden weights through a live ``DebertaV2Model``'s ``state_dict`` into the native model: the golden output, bound (a)"""
    transformers = pytest.importorskip("transformers")
    z = np.load(GOLDEN)
    cfg = deberta_ref.tiny_config()
    sd = {}
    for name in z.files:
        tag, _, key = name.partition(":")
        if tag == "q":
            sd[key] = torch.from_numpy(z[name].astype(np.float32)) * float(z["s:" + key])
        elif tag == "f":
            sd[key] = torch.from_numpy(z[name])
    hf = transformers.DebertaV2Model(transformers.DebertaV2Config(**deberta_ref.hf_config_kwargs(cfg))).eval()
    hf.load_state_dict(sd)
    m = _model(cfg, {k: v.detach().clone() for k, v in hf.state_dict().items()})
    ids, mask, want = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"]), torch.from_numpy(z["last_hidden_state"])
    got = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    err, err_pad = l2_rel(got, want), l2_rel(got[1, 50:], want[1, 50:])
    print(f"NativeDeberta vs the captured HuggingFace output (tiny): {err:.3e}, padded rows {err_pad:.3e} (bound {BOUND_A})")
    assert err <= BOUND_A and err_pad <= BOUND_A


@pytest.mark.parametrize("use_prompt", [False, True])
def test_text_encoder_native_backbone_against_restatement_backbone(use_prompt):
    """``config.text_backbone = "native"`` against the same encoder given the bf16-storage restatement as its ``backbone=``; the
    tail (CLS pooling, projection) is the same HIP code on both sides, so bound (a) applies to both outputs."""
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
    cfg_ref = cfgmod.ModelConfig()
    cfg_ref.fusion_hidden_size, cfg_ref.fusion_dropout = 256, 0.0
    ref = TextEncoder(cfg_ref, backbone=deberta_ref.RefDeberta(sd, tcfg, bf16_storage=True))
    tail = {k: v for k, v in enc.state_dict().items() if not k.startswith("model.")}
    assert len(tail) < len(enc.state_dict()) and "model.encoder.rel_embeddings.weight" in enc.state_dict()
    ref.load_state_dict(tail)
    ids, mask = _inputs(tcfg, 2, 70, 32, pad_from=50)
    enc, ref = enc.cuda().eval(), ref.cuda().eval()
    with torch.no_grad():
        got, want = enc(ids.cuda(), mask.cuda(), use_prompt=use_prompt), ref(ids.cuda(), mask.cuda(), use_prompt=use_prompt)
    T = 70 + (cfg.prompt_length if use_prompt else 0)
    assert tuple(got["sequence_output"].shape) == (2, T, 256) and torch.equal(got["attention_mask"], want["attention_mask"])
    for k in ("features", "sequence_output"):
        err = l2_rel(got[k], want[k])
        print(f"TextEncoder native vs restatement backbone (use_prompt={use_prompt}), {k}: rel L2 {err:.3e} (bound {BOUND_A})")
        assert got[k].shape == want[k].shape and err <= BOUND_A, k
