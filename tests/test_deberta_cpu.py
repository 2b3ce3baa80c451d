"""CPU: the DeBERTa restatement tests/deberta_ref.py against HuggingFace through tests/golden/deberta_tiny.npz (captured by
tools/capture_deberta_golden.py), the relative-position index table against HuggingFace's own tables, and the ``state_dict``
surface, refusals and encoder hook of ``mmfusion.deberta.NativeDeberta`` (which needs no GPU to be built, saved and loaded).

RESTATE_TOL = 2e-5 is the project's bound for a restatement against its reference (float32 HuggingFace against float64), the
one tests/test_w2v_cpu.py holds its restatement to."""
import os

import numpy as np
import pytest
import torch

import deberta_ref
from helpers import l2_rel

RESTATE_TOL = 2e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deberta_tiny.npz")
LARGEST_OTHER_FIXTURE = 746560
TABLES = ((70, 8, 32), (512, 256, 512), (530, 256, 512))


def _native(cfg, **kw):
    from mmfusion.deberta import NativeDeberta
    return NativeDeberta(**{**deberta_ref.config_kwargs(cfg), **kw})


def _golden():
    z = np.load(GOLDEN)
    sd = {}
    for name in z.files:
        tag, _, key = name.partition(":")
        if tag == "q":
            sd[key] = torch.from_numpy(z[name].astype(np.float32)) * float(z["s:" + key])
        elif tag == "f":
            sd[key] = torch.from_numpy(z[name])
    cfg = deberta_ref.tiny_config()
    sd = {k: sd[k] for k in deberta_ref.hf_keys(cfg)}
    return (cfg, sd, torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"]), torch.from_numpy(z["last_hidden_state"]),
            [str(k) for k in z["keys"]])


def _hf_table(T, S, P):
    return torch.from_numpy(np.load(GOLDEN)[f"relpos:{T}:{S}:{P}"].astype(np.int64))


# ---- the index table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,P", TABLES)
def test_bucket_index_is_huggingfaces_table_entry_for_entry(T, S, P):
    """HuggingFace's ``build_relative_position`` (T, T) table, clamped as its attention clamps it, against the (2T - 1) table
    both the restatement and the product build; and the product's copy of the function against the restatement's"""
    from mmfusion import deberta
    hf = _hf_table(T, S, P)
    ar = torch.arange(T)
    delta = ar[:, None] - ar[None, :]
    for fn in (deberta_ref.bucket_index, deberta.bucket_index):
        idx = fn(T, S, P)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (2 * T - 1,)
        assert torch.equal(idx.long()[delta + T - 1], torch.clamp(hf + S, 0, 2 * S - 1))
    if (T, S, P) == (70, 8, 32):
        assert int(hf.min()) == -9 and int(hf.max()) == 9                               # both clamps bind: buckets reach past +-S
        idx = deberta_ref.bucket_index(T, S, P)
        assert int(idx.min()) == 0 and int(idx.max()) == 2 * S - 1 and int((hf + S > 2 * S - 1).sum()) > 0 and int((hf + S < 0).sum()) > 0


@pytest.mark.parametrize("T,S,P", TABLES)
def test_bucket_is_odd_so_one_table_serves_both_gathers(T, S, P):
    """c2p gathers at clamp(bucket(i - j) + S), p2c at clamp(-bucket(j - i) + S) transposed: equal iff -bucket(-delta) == bucket(delta)"""
    hf = _hf_table(T, S, P)
    assert torch.equal(-hf.t(), hf)
    assert torch.equal(torch.clamp(-hf.t() + S, 0, 2 * S - 1), torch.clamp(hf + S, 0, 2 * S - 1))
    delta = torch.arange(-(T - 1), T)
    b = deberta_ref.log_bucket(delta, S, P)
    assert torch.equal(-torch.flip(b, (0,)), b)
    step = b[1:] - b[:-1]
    assert int(step.min()) >= 0 and int(step.max()) <= 1                                # what the attention kernel's row runs rely on


# ---- the restatement -----------------------------------------------------------------------------------------
def test_restatement_matches_the_captured_vector_on_every_row():
    cfg, sd, ids, mask, want, _ = _golden()
    assert tuple(ids.shape) == (2, 70) and int(mask[1, 50:].sum()) == 0 and int(mask.sum()) == 70 + 50
    got = deberta_ref.deberta_forward(sd, ids, mask, cfg)
    err, err_pad, err_real = l2_rel(got, want), l2_rel(got[1, 50:], want[1, 50:]), l2_rel(got[1, :50], want[1, :50])
    no_mask = l2_rel(deberta_ref.deberta_forward(sd, ids, None, cfg), want)
    sd0 = dict(sd, **{"encoder.rel_embeddings.weight": torch.zeros_like(sd["encoder.rel_embeddings.weight"])})
    no_rel = l2_rel(deberta_ref.deberta_forward(sd0, ids, mask, cfg), want)
    print(f"restatement vs captured HuggingFace output: {err:.3e}, padded rows {err_pad:.3e}, real rows of the padded item {err_real:.3e} "
          f"(bound {RESTATE_TOL}); without the mask {no_mask:.3e}; with zero relative embeddings {no_rel:.3e}")
    assert got.shape == want.shape and max(err, err_pad, err_real) <= RESTATE_TOL
    assert no_mask > 100 * RESTATE_TOL and no_rel > 100 * RESTATE_TOL                    # the mask and the bias terms both matter


def test_inputs_embeds_route_equals_the_ids_route():
    cfg, sd, ids, mask, _, _ = _golden()
    emb = sd["embeddings.word_embeddings.weight"][ids]
    a = deberta_ref.deberta_forward(sd, ids, mask, cfg)
    b = deberta_ref.deberta_forward(sd, emb, mask, cfg)
    assert torch.equal(a, b)


def test_bf16_storage_switch_rounds_and_stays_close():
    cfg, sd, ids, mask, _, _ = _golden()
    exact = deberta_ref.deberta_forward(sd, ids, mask, cfg)
    stored = deberta_ref.deberta_forward(sd, ids, mask, cfg, bf16_storage=True)
    err = l2_rel(stored, exact)
    print(f"bf16-storage restatement vs fp64: {err:.3e}")
    assert torch.equal(stored, stored.to(torch.bfloat16).to(stored.dtype))              # the last store is a bf16 store
    assert 1e-4 < err < 2e-2


def test_fixture_is_no_larger_than_the_largest_beside_it():
    assert os.path.getsize(GOLDEN) <= LARGEST_OTHER_FIXTURE


def test_masked_query_rows_are_uniform_and_masked_keys_are_zero():
    """the two mask rules on the attention restatement itself"""
    g = torch.Generator().manual_seed(3)
    n, H, T, S, dh = 1, 2, 9, 4, 8
    q, k, v = (torch.randn(n, H, T, dh, generator=g, dtype=torch.float64) for _ in range(3))
    posq, posk = (torch.randn(H, 2 * S, dh, generator=g, dtype=torch.float64) for _ in range(2))
    idx = deberta_ref.bucket_index(T, S, 16)
    mask = torch.ones(n, T)
    mask[0, 6:] = 0
    out = deberta_ref.disentangled_attention(q, k, v, posq, posk, idx, mask, 3.0)
    assert torch.allclose(out[0, :, 6:], v[0].mean(dim=1, keepdim=True).expand(-1, 3, -1), atol=1e-12)
    v2 = v.clone()
    v2[0, :, 6:] = 1e6
    out2 = deberta_ref.disentangled_attention(q, k, v2, posq, posk, idx, mask, 3.0)
    assert torch.equal(out2[0, :, :6], out[0, :, :6])


# ---- NativeDeberta: the state_dict surface -------------------------------------------------------------------
def test_state_dict_is_huggingfaces_key_for_key():
    cfg, sd, _, _, _, keys = _golden()
    m = _native(cfg)
    mine = m.state_dict()
    assert list(mine.keys()) == keys == list(deberta_ref.hf_keys(cfg).keys())
    assert {k: tuple(v.shape) for k, v in mine.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert all(not p.requires_grad for p in m.parameters())
    assert m.config.model_type == "deberta-v2" and "bert" in m.config.model_type and m.config.hidden_size == cfg.hidden_size


def test_defaults_are_deberta_v3_base():
    import inspect
    from mmfusion.deberta import NativeDeberta
    p = inspect.signature(NativeDeberta.__init__).parameters
    base = deberta_ref.base_config()
    for k, v in deberta_ref.config_kwargs(base).items():
        assert p[k].default == v, k
    want = deberta_ref.hf_keys(base)
    assert len(want) == 3 + 16 * 12 + 3 and want["encoder.rel_embeddings.weight"] == (512, 768)


def test_round_trip_is_bit_exact_and_qkv_is_fused():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=7)
    m = _native(cfg)
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert list(back.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    d = cfg.hidden_size
    a = "encoder.layer.1.attention.self."
    assert torch.equal(m.l1_qkv_w[:d], sd[a + "query_proj.weight"]) and torch.equal(m.l1_qkv_w[d:2 * d], sd[a + "key_proj.weight"])
    assert torch.equal(m.l1_qkv_w[2 * d:], sd[a + "value_proj.weight"]) and torch.equal(m.l1_qkv_b[d:2 * d], sd[a + "key_proj.bias"])


def test_strict_loading_reports_what_is_wrong_and_ignores_what_huggingface_ignores():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=8)
    m = _native(cfg)
    bad = dict(sd)
    bad["encoder.layer.9.output.LayerNorm.weight"] = torch.zeros(3)
    del bad["encoder.LayerNorm.bias"]
    bad["encoder.rel_embeddings.weight"] = torch.zeros(12, cfg.hidden_size)
    with pytest.raises(RuntimeError) as e:
        m.load_state_dict(bad)
    msg = str(e.value)
    assert "encoder.layer.9.output.LayerNorm.weight" in msg and "encoder.LayerNorm.bias" in msg and "size mismatch" in msg
    extra = dict(sd)
    extra["embeddings.position_ids"] = torch.arange(32).unsqueeze(0)
    extra["mask_predictions.dense.weight"] = torch.zeros(4, 4)
    extra["lm_predictions.lm_head.bias"] = torch.zeros(4)
    res = m.load_state_dict(extra)                                                     # strict
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.state_dict()["encoder.rel_embeddings.weight"], sd["encoder.rel_embeddings.weight"])


def test_word_embeddings_is_a_callable_without_autograd():
    cfg = deberta_ref.tiny_config()
    m = _native(cfg)
    ids = torch.tensor([[1, 5, 299]])
    e = m.embeddings.word_embeddings(ids)
    assert e.dtype == torch.float32 and tuple(e.shape) == (1, 3, cfg.hidden_size) and not e.requires_grad
    assert torch.equal(e, m.state_dict()["embeddings.word_embeddings.weight"][ids])
    assert len(list(m.children())) == 0                                                 # the callable adds no module and no state_dict key


# ---- NativeDeberta: refusals --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,names", [
    (dict(relative_attention=False), "relative_attention"), (dict(share_att_key=False), "share_att_key"),
    (dict(pos_att_type="c2p"), "pos_att_type"), (dict(pos_att_type=None), "pos_att_type"), (dict(norm_rel_ebd="none"), "norm_rel_ebd"),
    (dict(position_biased_input=True), "position_biased_input"), (dict(type_vocab_size=2), "type_vocab_size"),
    (dict(conv_kernel_size=3), "conv_kernel_size"), (dict(max_relative_positions=128), "max_relative_positions"),
    (dict(hidden_act="gelu_new"), "hidden_act"), (dict(embedding_size=128), "embedding_size"),
    (dict(hidden_size=768, num_attention_heads=8), "head_dim"),                        # head_dim 96: the base would take it
    (dict(num_attention_heads=8), "head_dim"),                                          # head_dim 32
    (dict(hidden_size=384, num_attention_heads=6), "hidden_size"),                      # not a LayerNorm width
    (dict(position_buckets=300), "position_buckets"), (dict(position_buckets=0), "position_buckets"),
    (dict(intermediate_size=516), "intermediate_size"),
])
def test_configurations_outside_the_v3_family_are_refused_by_name(kw, names):
    with pytest.raises(ValueError, match="NativeDeberta.*" + names):
        _native(deberta_ref.tiny_config(), **kw)


def test_forward_refusals_need_no_gpu():
    cfg = deberta_ref.tiny_config()
    m = _native(cfg)
    ids = torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(input_ids=ids)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(inputs_embeds=torch.zeros(1, 8, cfg.hidden_size))
    with pytest.raises(ValueError, match="exactly one"):
        m()
    with pytest.raises(ValueError, match="exactly one"):
        m(input_ids=ids, inputs_embeds=torch.zeros(1, 8, cfg.hidden_size))
    assert m.workspace_bytes_per_item(70) > 0 and m.workspace_bytes_per_item(140) == 2 * m.workspace_bytes_per_item(70)


def test_kernel_wrappers_refuse_cpu_tensors():
    from mmfusion import lib
    out = torch.zeros(4, 256, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.deberta_embed(out, None, torch.ones(256), torch.zeros(256), 1e-7, embeds=torch.zeros(4, 256))
    with pytest.raises(RuntimeError, match="GPU only"):
        lib.deberta_attn_fwd(torch.zeros(4, 768, dtype=torch.bfloat16), out[:, :256], out[:, :256], torch.zeros(7, dtype=torch.int32), None,
                             out, 1, 4, 4, 2, 13.9)


# ---- the encoder hook ------------------------------------------------------------------------------------------
def _tiny_text_config():
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.text_hidden_size = 256, 256
    cfg.text_backbone = "native"
    cfg.text_backbone_kwargs = {k: v for k, v in deberta_ref.config_kwargs(deberta_ref.tiny_config()).items() if k != "hidden_size"}
    return cfg


def test_text_encoder_builds_the_native_backbone_and_exposes_its_hidden_size():
    from mmfusion.deberta import NativeDeberta
    from models.encoders import TextEncoder
    enc = TextEncoder(_tiny_text_config())
    assert isinstance(enc.model, NativeDeberta) and enc.hidden_size == 256 and enc.projection.in_features == 256
    assert "model.encoder.layer.1.output.LayerNorm.weight" in enc.state_dict()
    assert enc.model.config.vocab_size == 300 and enc.model.config.position_buckets == 8


def test_create_model_with_three_native_backbones():
    import vit_ref
    import w2v_ref
    from mmfusion.deberta import NativeDeberta
    from models.multimodal_model import create_model
    cfg = _tiny_text_config()
    cfg.audio_hidden_size, cfg.audio_backbone = 256, "native"
    cfg.audio_backbone_kwargs = {k: v for k, v in w2v_ref.config_kwargs(w2v_ref.tiny_config()).items() if k != "hidden_size"}
    vcfg = vit_ref.tiny_config()
    cfg.video_hidden_size, cfg.video_frame_size, cfg.video_backbone = vcfg.hidden_size, (vcfg.image_size, vcfg.image_size), "native"
    cfg.video_backbone_kwargs = {k: v for k, v in vit_ref.config_kwargs(vcfg).items() if k not in ("hidden_size", "image_size")}
    model = create_model(cfg)
    assert isinstance(model.text_encoder.model, NativeDeberta) and model.text_encoder.hidden_size == 256
