"""GPU: ``mmfusion.bert.NativeBert`` / ``NativeRoberta`` against the captured HuggingFace outputs (tests/golden/bert_tiny.npz,
roberta_tiny.npz) and the explicit restatement tests/bert_ref.py, which needs neither the reference nor transformers.

Bounds (tests/test_wavlm_gpu.py's).  (a) against the restatement with bf16 storage: relative L2 <= BOUND_A, the project's bound for a
kernel against an oracle with the same storage format.  (b) against the exact restatement (and the captured output, which the
restatement meets to 2e-5): 2 x the error of the bf16-storage restatement against the exact one on the same inputs, computed here
on the CPU."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import bert_ref  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402

FAMILIES = ("bert", "roberta")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = {f: os.path.join(HERE, "golden", f"{f}_tiny.npz") for f in FAMILIES}


def _class(family):
    from mmfusion.bert import NativeBert, NativeRoberta
    return {"bert": NativeBert, "roberta": NativeRoberta}[family]


def _native(family, cfg, sd, **kw):
    m = _class(family)(**{**bert_ref.config_kwargs(cfg), **kw})
    m.load_state_dict(sd)
    return m.cuda().eval()


def _setup(family, n, T, seed=21, max_pos=None, **kw):
    """a seeded tiny model with a position table for ``T`` tokens, ids without pads, and token types"""
    cfg = bert_ref.tiny_config(family, max_position_embeddings=max_pos or T + 4)
    sd = bert_ref.seeded_weights(cfg, family, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    ids = torch.randint(2, cfg.vocab_size, (n, T), generator=g)
    tt = torch.randint(0, cfg.type_vocab_size, (n, T), generator=g)
    return cfg, sd, _native(family, cfg, sd, **kw), ids, tt


@pytest.fixture(scope="module")
def golden():
    """the captured cases with the restatement's two forms of them, computed once"""
    out = {}
    for f in FAMILIES:
        sd, ids, mask, tt, want = bert_ref.load_golden(GOLDEN[f])
        cfg = bert_ref.tiny_config(f)
        run = lambda **kw: bert_ref.bert_forward(sd, ids, mask, cfg, f, token_type_ids=tt, **kw)
        out[f] = (cfg, sd, ids, mask, tt, want, run(), run(bf16_storage=True))
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_tiny_model_against_the_captured_output_and_the_restatement(golden, family):
    cfg, sd, ids, mask, tt, want, exact, stored = golden[family]
    m = _native(family, cfg, sd)
    got = m(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=tt.cuda()).last_hidden_state
    assert got.dtype == torch.float32 and got.shape == want.shape == (3, 36, cfg.hidden_size) and not got.requires_grad
    a, model_err = l2_rel(got, stored), l2_rel(stored, exact)
    b, h = l2_rel(got, exact), l2_rel(got, want)
    print(f"{_class(family).__name__} tiny 3 x 36: (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A}); (b) vs exact restatement "
          f"{b:.3e}, vs captured HuggingFace {h:.3e} (bound {2 * model_err:.3e})")
    assert a <= BOUND_A and b <= 2 * model_err and h <= 2 * model_err
    for dtype in (torch.bool, torch.float32, torch.uint8, torch.int32):              # the mask in any dtype: the same launches
        again = m(input_ids=ids.cuda(), attention_mask=mask.to(dtype).cuda(), token_type_ids=tt.cuda()).last_hidden_state
        assert torch.equal(again, got), dtype


@pytest.mark.parametrize("family", FAMILIES)
def test_a_padded_item_over_several_query_chunks_and_skipped_tiles(family):
    """2 items x 200 tokens, one padded to 70 valid tokens: two query chunks per head, four key tiles of which the padded item stages
    two and computes 70 keys.  Bound (a)."""
    cfg, sd, m, ids, tt = _setup(family, 2, 200)
    mask = torch.ones(2, 200, dtype=torch.int64)
    mask[1, 70:] = 0
    ids[1, 70:] = cfg.pad_token_id
    stored = bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt, bf16_storage=True, dtype=torch.float32)
    got = m(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=tt.cuda()).last_hidden_state
    a = l2_rel(got, stored)
    unmasked = l2_rel(bert_ref.bert_forward(sd, ids, None, cfg, family, token_type_ids=tt, bf16_storage=True, dtype=torch.float32), stored)
    print(f"{_class(family).__name__} tiny 2 x 200 (70 valid): (a) vs bf16-storage restatement {a:.3e} (bound {BOUND_A}); the mask moves "
          f"the restatement by {unmasked:.3e}")
    assert got.shape == stored.shape and a <= BOUND_A and unmasked > 3 * BOUND_A


@pytest.mark.parametrize("family", FAMILIES)
def test_an_empty_item_beside_a_full_one_is_finite_and_within_the_bound(family):
    cfg, sd, m, ids, tt = _setup(family, 2, 50)
    mask = torch.ones(2, 50, dtype=torch.int64)
    mask[0] = 0
    stored = bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt, bf16_storage=True, dtype=torch.float32)
    got = m(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=tt.cuda()).last_hidden_state
    a = l2_rel(got, stored)
    plain = l2_rel(bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt, bf16_storage=True, dtype=torch.float32,
                                         mutant="empty_item_plain_softmax"), stored)
    print(f"{_class(family).__name__} tiny 2 x 50, item 0 empty: (a) {a:.3e} (bound {BOUND_A}); the plain-softmax mutant is at {plain:.3e}")
    assert bool(torch.isfinite(got).all()) and a <= BOUND_A and plain > 3 * BOUND_A


@pytest.mark.parametrize("family", FAMILIES)
def test_results_do_not_depend_on_chunk(family):
    cfg, sd, m1, ids, tt = _setup(family, 3, 70, chunk=1)
    m2 = _native(family, cfg, sd, chunk=2)
    mask = torch.ones(3, 70, dtype=torch.int64)
    mask[1, 33:], mask[2, 5] = 0, 0
    a = dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=tt.cuda())
    f1, f2 = m1(**a).last_hidden_state, m2(**a).last_hidden_state
    assert torch.equal(f1, f2)
    assert torch.equal(m2(**a).last_hidden_state, f2)
    held = sum(v.numel() * v.element_size() for v in m2._ws.values() if isinstance(v, torch.Tensor))
    assert held == 2 * m2.workspace_bytes_per_item(70)


@pytest.mark.parametrize("family", FAMILIES)
def test_forward_replays_from_a_captured_graph_with_other_ids_and_another_mask(family):
    cfg, sd, m, ids, tt = _setup(family, 3, 70, chunk=2)
    mask = torch.ones(3, 70, dtype=torch.int64)
    mask[0, 40:] = 0
    ids_d, mask_d, tt_d = ids.cuda(), mask.cuda(), tt.cuda()
    eager = m(input_ids=ids_d, attention_mask=mask_d, token_type_ids=tt_d).last_hidden_state.clone()
    s_ids, s_mask = ids_d.clone(), mask_d.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(input_ids=s_ids, attention_mask=s_mask, token_type_ids=tt_d)                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(input_ids=s_ids, attention_mask=s_mask, token_type_ids=tt_d).last_hidden_state
    new_ids = torch.randint(2, cfg.vocab_size, (3, 70), generator=torch.Generator().manual_seed(5)).cuda()
    new_ids[2, 60:] = cfg.pad_token_id                                                # RoBERTa: other positions too
    new_mask = torch.ones_like(mask_d)
    new_mask[1, :8], new_mask[2, 60:] = 0, 0
    s_ids.copy_(new_ids), s_mask.copy_(new_mask)
    graph.replay()
    other = out.clone()
    s_ids.copy_(ids_d), s_mask.copy_(mask_d)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    want = m(input_ids=new_ids, attention_mask=new_mask, token_type_ids=tt_d).last_hidden_state
    assert torch.equal(other, want) and not torch.equal(other, eager)
    only_mask = m(input_ids=new_ids, attention_mask=mask_d, token_type_ids=tt_d).last_hidden_state
    assert not torch.equal(only_mask, want)                                           # the replay took the new mask, not only the new ids


@pytest.mark.parametrize("family", FAMILIES)
def test_inputs_embeds_match_ids_bit_for_bit_where_the_positions_agree(family):
    """without a pad id among them RoBERTa's positions from the ids are pad + 1 + place, the ``inputs_embeds`` rule"""
    cfg, sd, m, ids, tt = _setup(family, 2, 40)
    assert not bool((ids == cfg.pad_token_id).any())
    mask = torch.ones(2, 40, dtype=torch.int64)
    mask[1, 30:] = 0
    a = dict(attention_mask=mask.cuda(), token_type_ids=tt.cuda())
    by_ids = m(input_ids=ids.cuda(), **a).last_hidden_state
    emb = m.embeddings.word_embeddings(ids.cuda())
    assert emb.dtype == torch.float32 and torch.equal(emb.cpu(), sd["embeddings.word_embeddings.weight"][ids])
    assert torch.equal(m(inputs_embeds=emb, **a).last_hidden_state, by_ids)
    stored = bert_ref.bert_forward(sd, emb.cpu(), mask, cfg, family, token_type_ids=tt, bf16_storage=True, dtype=torch.float32)
    assert l2_rel(by_ids, stored) <= BOUND_A
    none = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state      # token_type_ids None: type 0
    zero = m(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=torch.zeros_like(tt).cuda()).last_hidden_state
    assert torch.equal(none, zero)
    assert torch.equal(m(input_ids=ids.cuda()).last_hidden_state, m(input_ids=ids.cuda(), attention_mask=torch.ones(2, 40).cuda()).last_hidden_state)


@pytest.mark.parametrize("family", FAMILIES)
def test_forward_refusals_on_the_gpu(family):
    cfg, sd, m, ids, tt = _setup(family, 1, 8, max_pos=16)
    who, d = _class(family).__name__, cfg.hidden_size
    room = 16 - (0 if family == "bert" else cfg.pad_token_id + 1)
    long_ids = torch.zeros(1, room + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match=who + ".*tokens"):
        m(input_ids=long_ids)
    assert m(input_ids=long_ids[:, :room]).last_hidden_state.shape == (1, room, d)   # the longest it takes
    emb = torch.zeros(1, 8, d, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match=who + ".*requires a gradient"):
        m(inputs_embeds=emb)
    with torch.no_grad():
        assert not m(inputs_embeds=emb).last_hidden_state.requires_grad
    with pytest.raises(ValueError, match=who + ".*attention_mask"):
        m(input_ids=ids.cuda(), attention_mask=torch.ones(1, 9).cuda())
    with pytest.raises(ValueError, match=who + ".*token_type_ids"):
        m(input_ids=ids.cuda(), token_type_ids=tt.int().cuda())
    with pytest.raises(TypeError, match=who + ".*input_ids"):
        m(input_ids=ids.int().cuda())


@pytest.mark.parametrize("family", FAMILIES)
def test_huggingface_state_dict_to_native_output(family):
    transformers = pytest.importorskip("transformers")
    cfg = bert_ref.tiny_config(family)
    Config, Model = {"bert": (transformers.BertConfig, transformers.BertModel),
                     "roberta": (transformers.RobertaConfig, transformers.RobertaModel)}[family]
    hf = Model(Config(**bert_ref.hf_config_kwargs(cfg))).eval()
    hf.load_state_dict(bert_ref.seeded_weights(cfg, family, seed=41))
    sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    m = _native(family, cfg, sd)
    g = torch.Generator().manual_seed(42)
    ids = torch.randint(0, cfg.vocab_size, (2, 36), generator=g)
    mask = torch.ones(2, 36, dtype=torch.int64)
    mask[0, 21:], mask[1, 4] = 0, 0
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask).last_hidden_state
    run = lambda **kw: bert_ref.bert_forward(sd, ids, mask, cfg, family, **kw)
    model_err = l2_rel(run(bf16_storage=True), run())
    err = l2_rel(m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state, want)
    print(f"{_class(family).__name__} vs HuggingFace fp32 eager (tiny): {err:.3e} (bound {2 * model_err:.3e})")
    assert err <= 2 * model_err


@pytest.mark.parametrize("use_prompt", [False, True])
def test_text_encoder_native_roberta_against_reference_backbone(use_prompt):
    """``config.text_backbone = "native-roberta"`` against the same encoder given the restatement as its ``backbone=``; the tail
    (CLS pooling, projection) is the same HIP code on both sides.  With ``use_prompt`` (under no_grad: the backbone is frozen) the
    prompt rows go in front through ``inputs_embeds``.  The restatement has bf16 storage, so bound (a) applies to both outputs, as in
    tests/test_deberta_gpu.py's encoder test."""
    import config as cfgmod
    from mmfusion.bert import NativeRoberta
    from models.encoders import TextEncoder
    bcfg = bert_ref.tiny_config("roberta", max_position_embeddings=64)
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.text_hidden_size = 256, 0.0, 256
    cfg.text_backbone = "native-roberta"
    cfg.text_backbone_kwargs = {k: v for k, v in bert_ref.config_kwargs(bcfg).items() if k != "hidden_size"}
    torch.manual_seed(3)
    enc = TextEncoder(cfg)
    assert type(enc.model) is NativeRoberta
    sd = bert_ref.seeded_weights(bcfg, "roberta", seed=31)
    enc.model.load_state_dict(sd)
    cfg_ref = cfgmod.ModelConfig()
    cfg_ref.fusion_hidden_size, cfg_ref.fusion_dropout = 256, 0.0
    ref = TextEncoder(cfg_ref, backbone=bert_ref.RefBert(sd, bcfg, "roberta", bf16_storage=True))
    tail = {k: v for k, v in enc.state_dict().items() if not k.startswith("model.")}
    assert len(tail) < len(enc.state_dict()) and "prompt_embeddings" in tail
    ref.load_state_dict(tail)
    g = torch.Generator().manual_seed(32)
    ids = torch.randint(2, bcfg.vocab_size, (3, 40), generator=g)
    mask = torch.ones(3, 40, dtype=torch.int64)
    mask[1, 25:] = 0
    ids[1, 25:] = bcfg.pad_token_id
    enc, ref = enc.cuda().eval(), ref.cuda().eval()
    with torch.no_grad():
        got = enc(ids.cuda(), mask.cuda(), use_prompt=use_prompt)
        want = ref(ids.cuda(), mask.cuda(), use_prompt=use_prompt)
    T = 40 + (cfg.prompt_length if use_prompt else 0)
    assert T + 2 <= bcfg.max_position_embeddings
    assert tuple(got["sequence_output"].shape) == (3, T, 256) and torch.equal(got["attention_mask"], want["attention_mask"])
    for k in ("features", "sequence_output"):
        err = l2_rel(got[k], want[k])
        print(f"TextEncoder native-roberta vs restatement backbone (use_prompt={use_prompt}), {k}: rel L2 {err:.3e} (bound {BOUND_A})")
        assert got[k].shape == want[k].shape and err <= BOUND_A, k
    if use_prompt:                                                                     # in grad mode the frozen backbone refuses
        with pytest.raises(RuntimeError, match="NativeRoberta.*requires a gradient"):
            enc(ids.cuda(), mask.cuda(), use_prompt=True)
