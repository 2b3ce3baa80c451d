"""GPU: full fine-tuning of the native DeBERTa, ``NativeDeberta.set_trainable_layers(L, embeddings=True)``: every layer and the
six embedding-side tensors (word embeddings, embedding LayerNorm, relative embeddings, encoder LayerNorm), on the ids route, the
prompt route, through ``TextEncoder`` (``text_backbone_trainable_layers = "all"``), across chunk sizes, under the arena's
accumulation protocol and from a captured graph.

Bound: rule (b) per tensor in absolute form, ||got - exact|| <= 2 ||stored - exact||, ``exact`` / ``stored`` the autograd
gradients of ``deberta_ref.deberta_forward`` without / with ``bf16_storage`` with every tensor of the state dict as a leaf;
both sides are computed here and printed per tensor (tests/test_deberta_finetune_gpu.py's ``_rule_b``).

Where two runs of the module are compared bit for bit, the layers' LayerNorm parameters are held to ``F32_TOL`` instead:
``mmf_layernorm_bwd_grouped``'s finalize pass adds the workgroups' column sums with one f32 atomic per slice in the order the
slices arrive, so the last bits of a dgamma / dbeta differ between two runs of the same call
(tests/test_vit_finetune_gpu.py::test_frames_with_an_aug_give_the_pixel_routes_gradients measured it and holds them the same way).
The embedding-side LayerNorms go through ``mmf_deberta_embed_bwd_params``, which has no atomics."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_ref  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402
from test_deberta_finetune_gpu import _douts, _frozen_grads_are_empty, _hf_grads, _layer_keys, _native_wgrads, _ref_wgrads, _rule_b  # noqa: E402
from test_deberta_gpu import _inputs, _model  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402

TABLE = "embeddings.word_embeddings.weight"
EMB_LN = ["embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
POS_SIDE = ["encoder.rel_embeddings.weight", "encoder.LayerNorm.weight", "encoder.LayerNorm.bias"]
EMB_KEYS = [TABLE] + EMB_LN + POS_SIDE


def _all_keys(cfg):
    return list(deberta_ref.hf_keys(cfg))


def _full(cfg, sd, chunk=None):
    m = _model(cfg, sd, chunk=chunk)
    m.set_trainable_layers(cfg.num_hidden_layers, embeddings=True)
    return m


def _unnamed(ids, mask, vocab):
    """the table rows no unmasked token names"""
    rest = torch.ones(vocab, dtype=torch.bool)
    rest[ids[mask != 0] if mask is not None else ids.reshape(-1)] = False
    return rest


def test_every_gradient_against_float64_autograd_tiny():
    """2 layers, d 256, S 8, vocab 300; 2 x 80 ids, the last item padded from token 60 (pad id 0, which only masked tokens carry)"""
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 2, 80, 72, pad_from=60)
    assert int(torch.bincount(ids[mask != 0]).max()) >= 3, "no id occurs three times among the unmasked tokens: pick another seed"
    keys, L = _all_keys(cfg), cfg.num_hidden_layers
    m = _model(cfg, sd)
    with torch.no_grad():
        plain = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state.clone()
    m.set_trainable_layers(L, embeddings=True)
    assert m.trainable_layers == L and m.trainable_embeddings and all(p.requires_grad for p in m.parameters())
    layers_only = _model(cfg, sd)
    layers_only.set_trainable_layers(L)
    rest = _unnamed(ids, mask, cfg.vocab_size)
    assert bool(rest[0]) and int(rest.sum()) > 100
    for tag, dout in zip(("random", "CLS-row"), _douts(cfg, 2, 80, 51)):
        exact = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float64, False, keys)
        stored = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float64, True, keys)
        got, out = _native_wgrads(m, ids.cuda(), mask, dout, keys)
        assert torch.equal(_bits(out), _bits(plain)), "the differentiable forward's bits are not the inference call's"
        _rule_b(f"NativeDeberta tiny 2 x 80, all weights, {tag} dO,", got, exact, stored)
        assert bool((got[TABLE][rest] == 0).all()) and bool((exact[TABLE][rest] == 0).all()), "a table row no unmasked token names has a gradient"
        assert float(got[TABLE].norm()) > 0
        lk = _layer_keys(cfg, L)
        ref, _ = _native_wgrads(layers_only, ids.cuda(), mask, dout, lk)
        for key in lk:
            if "LayerNorm" in key:
                assert l2_rel(got[key], ref[key]) <= F32_TOL, key
            else:
                assert torch.equal(_bits(got[key]), _bits(ref[key])), f"{key} differs from set_trainable_layers({L})'s"
        _frozen_grads_are_empty(layers_only)


def test_embedding_side_gradients_against_autograd_base_sizes():
    """deberta-v3-base sizes with the vocabulary cut to 512 (the kernels' forms do not depend on it): the d = 768 lane form of
    the embedding backward, S = 256, and the 12-layer sum of d rel; one item of 64 ids padded from token 50, float32 references"""
    cfg = deberta_ref.base_config()
    cfg.vocab_size = 512
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 1, 64, 52, pad_from=50)
    dout, _ = _douts(cfg, 1, 64, 53)
    m = _full(cfg, sd)
    exact = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float32, False, EMB_KEYS)
    stored = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float32, True, EMB_KEYS)
    got, _ = _native_wgrads(m, ids.cuda(), mask, dout, EMB_KEYS)
    _rule_b("NativeDeberta base (vocab 512) 1 x 64, all weights,", got, exact, stored)
    assert bool((got[TABLE][_unnamed(ids, mask, cfg.vocab_size)] == 0).all())


def test_prompt_route_keeps_its_input_gradient_bits_and_gains_the_embedding_side():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(54)
    emb = torch.randn(2, 80, cfg.hidden_size, generator=g)
    _, mask = _inputs(cfg, 2, 80, 55, pad_from=60)
    dout, _ = _douts(cfg, 2, 80, 56)
    keys = EMB_LN + POS_SIDE
    m0, m1 = _model(cfg, sd), _full(cfg, sd)
    leaf0, leaf1 = emb.cuda().requires_grad_(True), emb.cuda().requires_grad_(True)
    m0(inputs_embeds=leaf0, attention_mask=mask.cuda()).last_hidden_state.backward(dout.cuda())
    got, _ = _native_wgrads(m1, leaf1, mask, dout, keys)
    assert leaf1.grad is not None and torch.equal(_bits(leaf1.grad), _bits(leaf0.grad)), "d inputs_embeds changed with the embeddings trainable"
    exact = _ref_wgrads(sd, emb, mask, cfg, dout, torch.float64, False, keys)
    stored = _ref_wgrads(sd, emb, mask, cfg, dout, torch.float64, True, keys)
    _rule_b("NativeDeberta tiny prompt route, all weights,", got, exact, stored)
    assert not bool(m1.word_emb.grad.any())                                            # the table is not on this route
    # embeddings that need no gradient: the same parameter gradients (the rows' gradient goes to a buffer of the backward's)
    again, _ = _native_wgrads(m1, emb.cuda(), mask, dout, keys)
    for key in keys:
        assert torch.equal(_bits(again[key]), _bits(got[key])), key


def test_text_encoder_prompt_route_trains_the_table_too():
    import config as cfgmod
    from models.encoders import TextEncoder
    tcfg = deberta_ref.tiny_config()
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.text_hidden_size = 256, 0.0, 256
    cfg.text_backbone = "native"
    cfg.text_backbone_kwargs = {k: v for k, v in deberta_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
    cfg.text_backbone_trainable_layers = "all"
    torch.manual_seed(3)
    enc = TextEncoder(cfg)
    assert enc.model.trainable_embeddings
    sd = deberta_ref.seeded_weights(tcfg, seed=31)
    enc.model.load_state_dict(sd)
    g = torch.Generator().manual_seed(32)
    ids = torch.randint(1, tcfg.vocab_size, (2, 70), generator=g)
    mask = torch.ones(2, 70, dtype=torch.int64)
    ids[1, 50:], mask[1, 50:] = 0, 0
    P = cfg.prompt_length
    full = torch.cat([torch.ones(2, P, dtype=torch.int64), mask], dim=1)
    W_, b_ = enc.projection.weight.detach().double(), enc.projection.bias.detach().double()

    def ref_grads(bf16_storage):
        pe = enc.prompt_embeddings.detach().double().requires_grad_(True)
        table = sd[TABLE].double().requires_grad_(True)
        x = torch.cat([pe.unsqueeze(0).expand(2, -1, -1), table[ids]], dim=1)
        out = deberta_ref.deberta_forward(sd, x, full, tcfg, bf16_storage=bf16_storage)
        (out[:, 0] @ W_.T + b_).sum().backward()
        return {"prompt_embeddings": pe.grad, TABLE: table.grad}
    exact, stored = ref_grads(False), ref_grads(True)
    enc = enc.cuda().eval()
    out = enc(ids.cuda(), mask.cuda(), use_prompt=True)
    assert out["features"].requires_grad
    out["features"].sum().backward()
    torch.cuda.synchronize()
    got = {"prompt_embeddings": enc.prompt_embeddings.grad.detach().cpu(), TABLE: enc.model.word_emb.grad.detach().cpu().clone()}
    _rule_b("TextEncoder prompt route, all weights,", got, exact, stored)
    rest = _unnamed(ids, None, tcfg.vocab_size)
    assert int(rest.sum()) > 100 and bool((got[TABLE][rest] == 0).all()), "a table row no token names has a gradient"
    assert float(got[TABLE].norm()) > 0 and float(enc.model.rel_emb.grad.norm()) > 0


def test_chunking_changes_only_the_summation_order():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 5, 70, 57, pad_from=40)
    dout, _ = _douts(cfg, 5, 70, 58)
    keys = _all_keys(cfg)
    exact = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float64, False, keys)
    stored = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float64, True, keys)
    got = {}
    for chunk in (2, 5):
        got[chunk], _ = _native_wgrads(_full(cfg, sd, chunk=chunk), ids.cuda(), mask, dout, keys)
        _rule_b(f"NativeDeberta tiny 5 x 70, all weights, chunk {chunk},", got[chunk], exact, stored)
    for key in keys:
        e = l2_rel(got[2][key], got[5][key])
        through_pos = "query_proj" in key or "key_proj" in key or key in POS_SIDE       # the one bf16 rounding of dpos can flip between the two
        print(f"chunk 2 vs chunk 5, {key}: rel L2 {e:.3e}" + (" (through the position path: not asserted)" if through_pos else f" (bound {F32_TOL})"))
        assert through_pos or e <= F32_TOL, key


def test_gradients_accumulate_and_the_table_honours_the_lazy_zero_protocol():
    from mmfusion import arena
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(59)
    mask = torch.ones(3, 70, dtype=torch.int64)
    mask[2, 50:] = 0
    ids_a, ids_b = 2 * torch.randint(1, 150, (3, 70), generator=g), 2 * torch.randint(0, 150, (3, 70), generator=g) + 1      # even / odd ids
    ids_a[2, 50:], ids_b[2, 50:] = 0, 0
    dout, _ = _douts(cfg, 3, 70, 60)
    keys = _all_keys(cfg)
    m = _full(cfg, sd, chunk=2)
    once, _ = _native_wgrads(m, ids_a.cuda(), mask, dout, keys)
    twice, _ = _native_wgrads(m, ids_a.cuda(), mask, dout, keys, zero=False)
    for key in keys:
        e = l2_rel(twice[key], 2 * once[key])
        print(f"two backwards vs 2 x one, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    fresh, _ = _native_wgrads(_full(cfg, sd, chunk=2), ids_b.cuda(), mask, dout, keys)
    ar = arena.ensure(m)
    ar.zero_grad(lazy=True)                                                            # the table's gradient holds 2 x A's rows here
    _native_wgrads(m, ids_b.cuda(), mask, dout, keys, zero=False)
    ar.finalize_grads()
    torch.cuda.synchronize()
    again = _hf_grads(m, keys)
    rows_a = torch.zeros(cfg.vocab_size, dtype=torch.bool)
    rows_a[ids_a[mask != 0]] = True
    assert bool(once[TABLE][rows_a].any(dim=1).all()) and bool((again[TABLE][rows_a] == 0).all()), "stale rows of A"
    for key in keys:
        e = l2_rel(again[key], fresh[key])
        print(f"after zero_grad(lazy=True), a step on other ids, {key}: rel L2 vs a fresh step {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key


def test_forward_and_backward_replay_from_a_captured_graph_with_other_ids():
    from mmfusion import arena
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 3, 70, 62, pad_from=50)
    dout, _ = _douts(cfg, 3, 70, 63)
    keys = _all_keys(cfg)
    m = _full(cfg, sd, chunk=2)
    eager, _ = _native_wgrads(m, ids.cuda(), mask, dout, keys)
    ar = arena.ensure(m)
    static, k, dO = ids.cuda().clone(), mask.cuda(), dout.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        m(input_ids=static, attention_mask=k).last_hidden_state.backward(dO)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m(input_ids=static, attention_mask=k).last_hidden_state.backward(dO)
    g = torch.Generator().manual_seed(64)
    other_ids = torch.randint(1, cfg.vocab_size, ids.shape, generator=g)
    with torch.no_grad():
        static.copy_(other_ids.cuda())
    ar.zero_grad()
    graph.replay()
    torch.cuda.synchronize()
    other = _hf_grads(m, keys)
    with torch.no_grad():
        static.copy_(ids.cuda())
    ar.zero_grad()
    graph.replay()
    torch.cuda.synchronize()
    got = _hf_grads(m, keys)
    for key in keys:
        e = l2_rel(got[key], eager[key])
        print(f"captured forward + backward, {key}: rel L2 vs eager {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    named = ~_unnamed(other_ids, mask, cfg.vocab_size)
    assert torch.equal(other[TABLE].abs().sum(dim=1) != 0, named), "the replay with other ids did not put the table's gradient where those ids are"
    assert not torch.equal(named, ~_unnamed(ids, mask, cfg.vocab_size))


def test_text_encoder_all_steps_every_parameter_and_serves_the_new_weights():
    import config as cfgmod
    from mmfusion import arena
    from mmfusion.train import finetune_optimizer
    from models.encoders import TextEncoder
    tcfg = deberta_ref.tiny_config()
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.text_hidden_size = 256, 0.0, 256
    cfg.text_backbone = "native"
    cfg.text_backbone_kwargs = {k: v for k, v in deberta_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
    cfg.text_backbone_trainable_layers = "all"
    torch.manual_seed(3)
    enc = TextEncoder(cfg)
    assert enc.model.trainable_layers == tcfg.num_hidden_layers and enc.model.trainable_embeddings
    enc.model.load_state_dict(deberta_ref.seeded_weights(tcfg, seed=31))
    enc = enc.cuda().train()
    ids, mask = _inputs(tcfg, 2, 70, 61, pad_from=50)
    named = ~_unnamed(ids, mask, tcfg.vocab_size)
    ids, mask = ids.cuda(), mask.cuda()
    ar = arena.ensure(enc)
    opt = finetune_optimizer(enc, ar, lr=1e-2, weight_decay=0.01)
    with torch.no_grad():
        first = enc.model(input_ids=ids, attention_mask=mask).last_hidden_state.clone()
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    for _ in range(2):
        ar.zero_grad()
        feats = enc(ids, mask)["features"]
        assert feats.requires_grad
        feats.sum().backward()
        opt.advance()
        opt.launch()
    torch.cuda.synchronize()
    assert all(p.requires_grad for p in enc.model.parameters())
    for n, p in enc.named_parameters():
        if n.startswith(("model.", "projection.")):                                    # (what the forward does not use has no gradient)
            assert not torch.equal(_bits(p.detach()), _bits(before[n])), f"{n} did not move"
    moved_rows = (enc.model.word_emb.detach() != before["model.word_emb"]).any(dim=1).cpu()
    assert bool(moved_rows[named].all()), "a row of the table the batch names did not move"
    # what the kernels read now (shadows, rel and every layer's position tables) is the stepped weights
    sd = {k: v.detach().cpu().clone() for k, v in enc.model.state_dict().items()}
    assert list(sd) == list(deberta_ref.hf_keys(tcfg))
    with torch.no_grad():
        got = enc.model(input_ids=ids, attention_mask=mask).last_hidden_state
    want = deberta_ref.deberta_forward(sd, ids.cpu(), mask.cpu(), tcfg, bf16_storage=True)
    err, moved = l2_rel(got, want), l2_rel(got, first)
    print(f"TextEncoder, 2 AdamW steps on every parameter: no_grad forward vs the restatement on the new state_dict {err:.3e} (bound {BOUND_A}); "
          f"the output moved by {moved:.3e}")
    assert err <= BOUND_A and moved > 3 * BOUND_A


def test_refusals_and_defaults():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 2, 40, 64)
    dout, _ = _douts(cfg, 2, 40, 65)
    L = cfg.num_hidden_layers
    m = _model(cfg, sd)
    out = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state         # grad mode on, nothing trainable
    assert not out.requires_grad
    with pytest.raises(ValueError):
        m.set_trainable_layers(L - 1, embeddings=True)
    assert m.trainable_layers == 0 and not any(p.requires_grad for p in m.parameters())
    m.set_trainable_layers(L)                                                          # the default: the six tensors stay frozen
    assert not m.trainable_embeddings
    _native_wgrads(m, ids.cuda(), mask, dout, _layer_keys(cfg, L))
    _frozen_grads_are_empty(m)
    assert not any(getattr(m, n).requires_grad for n in m._EMBEDDING_PARAMS)
    m.set_trainable_layers(L, embeddings=True)
    got, _ = _native_wgrads(m, ids.cuda(), mask, dout, EMB_KEYS)
    assert all(float(v.norm()) > 0 for v in got.values())
    m.set_trainable_layers(0)
    again = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    assert not again.requires_grad and torch.equal(_bits(again), _bits(out)) and not any(p.requires_grad for p in m.parameters())
