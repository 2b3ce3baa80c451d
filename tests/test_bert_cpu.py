"""CPU: the BERT / RoBERTa restatement tests/bert_ref.py against HuggingFace (through tests/golden/bert_tiny.npz and
roberta_tiny.npz, and live where transformers imports), its mutants, RoBERTa's position ids, the staged restatement of the key-masked
attention, and the ``state_dict`` surface, refusals and ``TextEncoder`` switch of ``mmfusion.bert.NativeBert`` / ``NativeRoberta``
(which need no GPU to be built, saved and loaded).

RESTATE_TOL = 2e-5 is the project's bound for a restatement against its reference (float32 HuggingFace against float64), the one
tests/test_wavlm_cpu.py uses for its fixture."""
import math
import os

import pytest
import torch

import bert_ref
from helpers import l2_rel

RESTATE_TOL = 2e-5
FAMILIES = ("bert", "roberta")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = {f: os.path.join(HERE, "golden", f"{f}_tiny.npz") for f in FAMILIES}
DEBERTA_GOLDEN = os.path.join(HERE, "golden", "deberta_tiny.npz")


def _class(family):
    from mmfusion.bert import NativeBert, NativeRoberta
    return {"bert": NativeBert, "roberta": NativeRoberta}[family]


def _native(family, cfg=None, **kw):
    cfg = bert_ref.tiny_config(family) if cfg is None else cfg
    return _class(family)(**{**bert_ref.config_kwargs(cfg), **kw})


def _hf(family, cfg):
    import transformers
    Config, Model = {"bert": (transformers.BertConfig, transformers.BertModel),
                     "roberta": (transformers.RobertaConfig, transformers.RobertaModel)}[family]
    return Model(Config(**bert_ref.hf_config_kwargs(cfg))).eval()


@pytest.fixture(scope="module")
def golden():
    out = {}
    for f in FAMILIES:
        sd, ids, mask, tt, want = bert_ref.load_golden(GOLDEN[f])
        cfg = bert_ref.tiny_config(f)
        out[f] = (cfg, {k: sd[k] for k in bert_ref.hf_keys(cfg, f)}, ids, mask, tt, want)
    return out


def _with_empty_item(ids, mask, tt):
    """the captured batch with item 2's mask cleared: the case the empty-item mutant needs"""
    mask = mask.clone()
    mask[2] = 0
    return ids, mask, tt


# ---- the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_matches_the_captured_vector(golden, family):
    cfg, sd, ids, mask, tt, want = golden[family]
    got = bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt)
    err = l2_rel(got, want)
    print(f"{family}: restatement vs captured HuggingFace output {tuple(want.shape)}: {err:.3e} (bound {RESTATE_TOL})")
    assert ids.shape == (3, 36) and want.shape == (3, 36, cfg.hidden_size)
    assert got.shape == want.shape and err <= RESTATE_TOL


@pytest.mark.parametrize("family", FAMILIES)
def test_captured_case_has_what_the_mutants_need(golden, family):
    cfg, sd, ids, mask, tt, _ = golden[family]
    pad = cfg.pad_token_id
    assert int(mask[0].sum()) == 25 and bool((mask[0, 25:] == 0).all())           # a padded tail
    assert bool((mask[1, 10:13] == 0).all()) and int(mask[1].sum()) == 33          # a hole
    assert bool(mask.any(dim=1).all())                                            # no empty item
    if family == "bert":
        assert bool((tt != 0).any()) and bool((tt == 0).any())
    else:
        assert bool(((ids == pad) & (mask == 1)).any()) and bool(((ids != pad) & (mask == 0)).any())    # ids and mask disagree


@pytest.mark.parametrize("family,mutant", [(f, m) for f in FAMILIES for m in bert_ref.MUTANTS
                                           if f == "roberta" or m not in bert_ref.ROBERTA_ONLY])
def test_every_mutant_leaves_the_bound(golden, family, mutant):
    """mask ignored, padded query rows zeroed, RoBERTa positions from the mask / without the pad offset, token types dropped, pre-LN
    layers against the captured output; the empty item as a plain softmax against the true restatement on the captured batch with
    one item's mask cleared (HuggingFace's back ends differ on an empty item, so none is captured)"""
    cfg, sd, ids, mask, tt, want = golden[family]
    if mutant in bert_ref.NEEDS_EMPTY_ITEM:
        ids, mask, tt = _with_empty_item(ids, mask, tt)
        want = bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt)
        assert bool(torch.isfinite(want).all())
    err = l2_rel(bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt, mutant=mutant), want)
    print(f"{family} mutant {mutant}: {err:.3e} (bound {RESTATE_TOL})")
    assert err > 100 * RESTATE_TOL


def test_empty_item_is_the_uniform_row_as_float32_gives_it(golden):
    """score + finfo.min in float32 is finfo.min for every key, so the softmax row is uniform over all T keys: HuggingFace's eager
    arithmetic, written out"""
    cfg, sd, ids, mask, tt, _ = golden["bert"]
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(1, 2, 9, 16, generator=g) for _ in range(3))
    s = (q @ k.transpose(-1, -2)) * 0.25 + torch.finfo(torch.float32).min
    want = torch.softmax(s, dim=-1) @ v
    got, lse = bert_ref.masked_attention_ref(q.double(), k.double(), v.double(), torch.zeros(1, 9, dtype=torch.bool), 0.25)
    assert float((got - want).abs().max()) <= 1e-6 and float((lse - math.log(9.0)).abs().max()) <= 1e-12
    assert float((got - v.double().mean(dim=2, keepdim=True)).abs().max()) <= 1e-12


@pytest.mark.parametrize("family", FAMILIES)
def test_fixture_is_data_only_and_no_larger_than_deberta_tiny(family):
    import numpy as np
    assert os.path.getsize(GOLDEN[family]) <= os.path.getsize(DEBERTA_GOLDEN)
    z = np.load(GOLDEN[family], allow_pickle=False)
    assert all(z[n].dtype.kind in "fi" for n in z.files)


@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_matches_live_huggingface(family):
    pytest.importorskip("transformers")
    cfg = bert_ref.tiny_config(family)
    sd = bert_ref.seeded_weights(cfg, family, seed=5)
    hf = _hf(family, cfg)
    assert list(hf.state_dict().keys()) == list(sd.keys())
    hf.load_state_dict(sd)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, cfg.vocab_size, (2, 33), generator=g)
    mask = torch.ones(2, 33, dtype=torch.int64)
    mask[0, 20:], mask[1, 0] = 0, 0
    tt = torch.randint(0, cfg.type_vocab_size, (2, 33), generator=g)
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask, token_type_ids=tt).last_hidden_state
        emb = hf.embeddings.word_embeddings(ids)
        want_e = hf(inputs_embeds=emb, attention_mask=mask, token_type_ids=tt).last_hidden_state
    got = bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt)
    got_e = bert_ref.bert_forward(sd, emb, mask, cfg, family, token_type_ids=tt)
    err, err_e = l2_rel(got, want), l2_rel(got_e, want_e)
    print(f"{family}: restatement vs live HuggingFace (tiny, 2 x 33): ids {err:.3e}, inputs_embeds {err_e:.3e} (bound {RESTATE_TOL})")
    assert got.shape == want.shape and err <= RESTATE_TOL and err_e <= RESTATE_TOL


@pytest.mark.parametrize("family", FAMILIES)
def test_bf16_storage_switch_rounds_and_stays_close(golden, family):
    cfg, sd, ids, mask, tt, _ = golden[family]
    exact = bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt)
    stored = bert_ref.bert_forward(sd, ids, mask, cfg, family, token_type_ids=tt, bf16_storage=True)
    err = l2_rel(stored, exact)
    print(f"{family}: bf16-storage restatement vs fp64: {err:.3e}")
    assert torch.equal(stored, stored.to(torch.bfloat16).to(stored.dtype))
    assert 1e-4 < err < 2e-2


def test_staged_attention_restatement_is_the_exact_one_up_to_its_roundings():
    """``keymask_staged`` (what the GPU kernel test compares against) against the exact masked softmax; with all ones against
    tests/attn_ref.py's plain staged forward, bit for bit; masked rows of K and V never enter"""
    import attn_ref as R
    B, H, T, dh = 3, 2, 77, 64
    g = torch.Generator().manual_seed(4)
    q, k, v = (R.bf16r(torch.randn(B, T, H * dh, generator=g, dtype=torch.float64)) for _ in range(3))
    valid = torch.ones(B, T, dtype=torch.bool)
    valid[0, 40:], valid[1, 32:64], valid[1, 3], valid[2] = False, False, False, False        # a tail, a whole block + a hole, empty
    scale = R.f32r_scale(dh ** -0.5)
    st = bert_ref.keymask_staged(q, k, v, H, scale, valid)
    o, lse = bert_ref.masked_attention_ref(R.heads(q, H), R.heads(k, H), R.heads(v, H), valid, scale)
    assert float((st["o"] - R.merge(o)).abs().max()) <= 2 ** -8 * float(o.abs().max()) and float((st["lse"] - lse).abs().max()) <= 1e-9
    assert float((st["lse"][2] - math.log(T)).abs().max()) <= 1e-12
    big = torch.where(valid[..., None] | ~valid.any(1)[:, None, None], k, torch.full_like(k, 3.0e4))
    bigv = torch.where(valid[..., None] | ~valid.any(1)[:, None, None], v, torch.full_like(v, 3.0e4))
    leak = bert_ref.keymask_staged(q, big, bigv, H, scale, valid)
    assert torch.equal(leak["o"], st["o"]) and torch.equal(leak["lse"], st["lse"])
    ones = bert_ref.keymask_staged(q, k, v, H, scale, torch.ones(B, T, dtype=torch.bool))
    plain = R.staged(q, k, v, torch.zeros_like(q), H, scale)
    assert torch.equal(ones["o"], plain["o"]) and torch.equal(ones["lse"], plain["lse"])


# ---- RoBERTa's position ids ------------------------------------------------------------------------------------
def test_roberta_position_ids_are_huggingfaces():
    pad = 1
    ids = torch.tensor([[1, 1, 5, 6, 7, 8], [5, 6, 1, 1, 7, 8], [5, 6, 7, 1, 1, 1], [1, 1, 1, 1, 1, 1], [5, 1, 6, 1, 7, 1]])
    mine = bert_ref.position_ids(ids, "roberta", pad)
    assert mine.tolist() == [[1, 1, 2, 3, 4, 5], [2, 3, 1, 1, 4, 5], [2, 3, 4, 1, 1, 1], [1] * 6, [2, 1, 3, 1, 4, 1]]
    assert bert_ref.embeds_position_ids(1, 4, "roberta", pad).tolist() == [[2, 3, 4, 5]]
    assert bert_ref.position_ids(ids, "bert", 0).tolist() == [list(range(6))] * 5
    pytest.importorskip("transformers")
    from transformers.models.roberta import modeling_roberta as mr
    fn = getattr(mr.RobertaEmbeddings, "create_position_ids_from_input_ids", None) or mr.create_position_ids_from_input_ids
    g = torch.Generator().manual_seed(8)
    for p in (0, 1, 3):
        rnd = torch.randint(0, 6, (7, 130), generator=g)
        assert torch.equal(bert_ref.position_ids(rnd, "roberta", p), fn(rnd, p))
        assert torch.equal(bert_ref.position_ids(ids, "roberta", p), fn(ids, p))


def test_pack_restatement_and_the_loader_agree_on_the_row_length():
    from mmfusion import lib
    for T in (1, 31, 32, 33, 64, 65, 128, 129, 193, 512):
        assert lib.mask_pack_words(T) == bert_ref.pack_words(T) == lib.load().mmf_mask_pack_words(T)
    m = torch.zeros(2, 70)
    m[0, 3], m[0, 33], m[0, 69] = 1, 2.5, -1
    p = bert_ref.pack_ref(m, 2, 70)
    assert p.shape == (2, 6) and p[0].tolist() == [70, 3, 1 << 3, 1 << 1, 1 << 5, 0] and p[1].tolist() == [0] * 6
    assert bert_ref.pack_ref(None, 1, 33)[0].tolist() == [33, 33, 0xffffffff, 1, ]


# ---- the state_dict surface ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "base"])
@pytest.mark.parametrize("family", FAMILIES)
def test_state_dict_is_huggingfaces_key_for_key(family, which):
    from mmfusion.bert import FAMILIES as SIZES
    cfg = bert_ref.tiny_config(family) if which == "tiny" else bert_ref.base_config(family)
    if which == "base":
        cfg.num_hidden_layers = 2                             # (base widths; two of its twelve layers keep the test quick)
    m = _native(family, cfg)
    sd = m.state_dict()
    want = bert_ref.hf_keys(cfg, family)
    assert list(sd.keys()) == list(want.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(not p.requires_grad for p in m.parameters())
    assert m.config.model_type == family and "bert" in m.config.model_type
    if which == "base":
        dflt = _class(family)(num_hidden_layers=2)            # the defaults ARE bert-base-uncased / roberta-base
        assert {k: tuple(v.shape) for k, v in dflt.state_dict().items()} == want
        c, b = dflt.config, bert_ref.base_config(family)
        assert all(getattr(c, k) == v for k, v in vars(b).items() if k != "num_hidden_layers")
        assert set(SIZES) == {"base", "large"} and SIZES["large"]["hidden_size"] == 1024 and SIZES["large"]["num_hidden_layers"] == 24
        assert SIZES["base"] == {k: getattr(_class(family)().config, k) for k in SIZES["base"]}
    assert list(_native(family, cfg, add_pooling_layer=False).state_dict().keys()) == list(bert_ref.hf_keys(cfg, family, pooler=False))
    pytest.importorskip("transformers")
    hf = _hf(family, cfg)
    assert [(k, tuple(v.shape)) for k, v in hf.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]


@pytest.mark.parametrize("family", FAMILIES)
def test_round_trip_is_bit_exact_and_qkv_are_stored_fused(family):
    cfg = bert_ref.tiny_config(family)
    sd = bert_ref.seeded_weights(cfg, family, seed=7)
    m = _native(family)
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert list(back.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    d = cfg.hidden_size
    assert m.l1_qkv_w.shape == (3 * d, d) and torch.equal(m.l1_qkv_w[d:2 * d], sd["encoder.layer.1.attention.self.key.weight"])
    assert torch.equal(m.pooler_w, sd["pooler.dense.weight"]) and torch.equal(m.pos_emb, sd["embeddings.position_embeddings.weight"])
    assert torch.equal(m.embeddings.word_embeddings(torch.tensor([[3, 1]])), sd["embeddings.word_embeddings.weight"][[3, 1]][None])
    with pytest.raises(RuntimeError, match="token_type_embeddings"):
        m.load_state_dict({k: v for k, v in sd.items() if "token_type_embeddings" not in k})
    with pytest.raises(RuntimeError, match="extra.weight"):
        m.load_state_dict({**sd, "extra.weight": torch.zeros(1)})


@pytest.mark.parametrize("family", FAMILIES)
def test_huggingface_loads_the_native_state_dict_strictly(family):
    pytest.importorskip("transformers")
    cfg = bert_ref.tiny_config(family)
    m = _native(family)
    m.load_state_dict(bert_ref.seeded_weights(cfg, family, seed=17))
    hf = _hf(family, cfg)
    res = hf.load_state_dict(m.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    res = m.load_state_dict(hf.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


# ---- refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kw", [
    dict(position_embedding_type="relative_key"), dict(position_embedding_type="relative_key_query"),
    dict(hidden_act="gelu_new"), dict(hidden_act="relu"), dict(is_decoder=True), dict(add_cross_attention=True),
    dict(num_attention_heads=8),                                                      # head_dim 32
    dict(hidden_size=320, num_attention_heads=5),                                     # no LayerNorm form
    dict(hidden_dropout_prob=0.1), dict(attention_probs_dropout_prob=0.1), dict(type_vocab_size=0), dict(pad_token_id=64),
])
def test_configurations_outside_the_family_are_refused(family, kw):
    with pytest.raises(ValueError, match=_class(family).__name__):
        _native(family, **kw)


@pytest.mark.parametrize("family", FAMILIES)
def test_training_surfaces_are_refused(family):
    m, who = _native(family), _class(family).__name__
    for args, kw in (((1,), {}), ((2,), dict(embeddings=True)), ((0,), dict(embeddings=True)), ((True,), {})):
        with pytest.raises(ValueError, match=who + ".*set_trainable_layers"):
            m.set_trainable_layers(*args, **kw)
    m.set_trainable_layers(0)
    assert m.trainable_layers == 0 and all(not p.requires_grad for p in m.parameters())
    for args in ((0.1, 0.0), (0.0, 0.1), (0.1, 0.1)):
        with pytest.raises(ValueError, match=who + ".*set_dropout"):
            m.set_dropout(*args)
    m.set_dropout(0, 0)
    m.set_dropout(0.0, 0.0)


@pytest.mark.parametrize("family", FAMILIES)
def test_forward_refusals_need_no_gpu(family):
    from mmfusion import ops
    m, who = _native(family), _class(family).__name__
    cfg = m.config
    ids = torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match=who + ".*exactly one"):
        m()
    with pytest.raises(ValueError, match=who + ".*exactly one"):
        m(input_ids=ids, inputs_embeds=torch.zeros(1, 8, cfg.hidden_size))
    with pytest.raises(RuntimeError, match=who + ".*GPU only"):
        m(input_ids=ids)
    with pytest.raises(RuntimeError, match=who + ".*GPU only"):
        m(inputs_embeds=torch.zeros(1, 8, cfg.hidden_size))
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match=who + ".*bf16 storage only"):
            m(input_ids=ids)
    finally:
        ops.set_precision(old)
    assert m._first_position() == (0 if family == "bert" else cfg.pad_token_id + 1)


def test_kernel_wrappers_check_their_operands():
    from mmfusion import lib
    bf16 = torch.bfloat16
    p = lib.AttnProblem(None, None, None, None, None, None, None, None, None, None, 2, 2, 3, 3, 128, 128, 128, 128)
    with pytest.raises(RuntimeError, match="attn_fwd_keymask.*GPU only"):
        lib.attn_fwd_keymask(p, 64, 0.125, torch.zeros(2 * lib.mask_pack_words(3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="mask_pack.*GPU only"):
        lib.mask_pack(None, torch.zeros(8, dtype=torch.int32), 2, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.bert_embed(torch.zeros(4, 8, dtype=bf16), torch.zeros(5, 8), torch.zeros(4, 8), torch.zeros(1, 8), torch.ones(8),
                       torch.zeros(8), 1e-5, 2, "bert", ids=torch.zeros(4, dtype=torch.int64))
    if not torch.cuda.is_available():
        return
    dev = "cuda"
    with pytest.raises(ValueError, match="attn_fwd_keymask"):
        lib.attn_fwd_keymask(p, 64, 0.125, torch.zeros(2 * lib.mask_pack_words(3) - 1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="attn_fwd_keymask"):
        lib.attn_fwd_keymask(p, 64, 0.125, torch.zeros(8, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="mask_pack"):
        lib.mask_pack(torch.ones(2, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev), 2, 3)
    with pytest.raises(ValueError, match="mask_pack"):
        lib.mask_pack(torch.ones(2, 4, device=dev), torch.zeros(8, dtype=torch.int32, device=dev), 2, 3)
    with pytest.raises(ValueError, match="mask_pack"):
        lib.mask_pack(None, torch.zeros(7, dtype=torch.int32, device=dev), 2, 3)
    out, f = torch.zeros(4, 8, dtype=bf16, device=dev), lambda *s: torch.zeros(*s, device=dev)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)
    args = lambda **kw: lib.bert_embed(out, f(5, 8), f(4, 8), f(1, 8), f(8), f(8), 1e-5, kw.pop("T", 2), kw.pop("rule", "bert"), **kw)
    for kw in (dict(), dict(ids=i64(4), embeds=f(4, 8)), dict(ids=i64(3)), dict(ids=i64(4).int()), dict(ids=i64(4), T=3),
               dict(ids=i64(4), rule="xlnet"), dict(embeds=f(4, 7)), dict(ids=i64(4), token_type_ids=i64(5))):
        with pytest.raises(ValueError, match="bert_embed"):
            args(**kw)


# ---- TextEncoder ---------------------------------------------------------------------------------------------------
def _encoder_config(family, **extra):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.text_hidden_size = 256, 256
    cfg.text_backbone = "native-" + family
    bcfg = bert_ref.tiny_config(family)
    cfg.text_backbone_kwargs = {k: v for k, v in bert_ref.config_kwargs(bcfg).items() if k != "hidden_size"}
    for k, v in extra.items():
        setattr(cfg, k, v)
    return cfg, bcfg


@pytest.mark.parametrize("family", FAMILIES)
def test_text_encoder_switch_builds_the_native_class(family):
    from mmfusion.deberta import NativeDeberta
    from models.encoders import TextEncoder
    cfg, bcfg = _encoder_config(family)
    enc = TextEncoder(cfg)
    assert type(enc.model) is _class(family) and enc.hidden_size == 256 and enc._native
    assert list(enc.model.state_dict().keys()) == list(bert_ref.hf_keys(bcfg, family).keys())
    assert "model.embeddings.position_embeddings.weight" in enc.state_dict()
    cfg.text_backbone, cfg.text_backbone_kwargs = "native", dict(vocab_size=50, num_hidden_layers=1, num_attention_heads=4, intermediate_size=64)
    assert type(TextEncoder(cfg).model) is NativeDeberta       # "native" is what it was


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("extra", [dict(text_backbone_trainable_layers=1), dict(text_backbone_trainable_layers="all"),
                                   dict(text_backbone_dropout=True), dict(text_backbone_dropout=(0.1, 0.0))])
def test_text_encoder_refuses_training_this_backbone(family, extra):
    from models.encoders import TextEncoder
    cfg, _ = _encoder_config(family, **extra)
    with pytest.raises(ValueError, match=_class(family).__name__):
        TextEncoder(cfg)
