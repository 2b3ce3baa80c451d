"""GPU: ``NativeDeberta`` with training-mode dropout against float64 autograd through the training-mode restatement
tests/deberta_dropout_ref.py under the masks restated on the host, at ``tiny_config``, N = 3 items of T = 24 tokens, the last one
padded from token 16, (hidden, attention) = (0.1, 0.1), ``ops.seed_dropout(1234)``.

A call of the module on its own starts a training forward itself: the state its launches read is the seeded one + 1 and its sites
are 1 .. 1 + 4 L (``STATE``, ``deberta_dropout_ref.sites``).

Bounds.  The forward: (a) BOUND_A against the bf16-storage restatement, (b) 2 x the storage model's own error against the exact
one (tests/test_deberta_gpu.py).  Every gradient: rule (b) per tensor in absolute form, ||got - exact|| <= 2 ||stored - exact||,
``exact`` / ``stored`` the float64 autograd gradients through the restatement without / with ``bf16_storage``; both sides are
printed (tests/test_deberta_finetune_gpu.py's ``_rule_b``).

Chunk sizes.  What belongs to an item (the result, d inputs_embeds) is bit-equal across ``chunk`` = 1, 2, 3: the masks are keyed
by the element.  A parameter's gradient is a sum over the items that the chunks add up in f32 in their own order, with or
without dropout (tests/test_deberta_full_finetune_gpu.py::test_chunking_changes_only_the_summation_order), so those are held to
F32_TOL, and the ones through the position path, where the one bf16 rounding of dpos can flip an element by an ulp (2^-8 of it,
so at most 2^-8 in relative L2), to BOUND_A; a mask that depended on the chunk would move either by its whole size."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_dropout_ref as D  # noqa: E402
import deberta_ref  # noqa: E402
from helpers import BOUND_A, l2_rel  # noqa: E402
from test_deberta_finetune_gpu import _douts, _frozen_grads_are_empty, _layer_keys, _native_wgrads, _rule_b  # noqa: E402
from test_deberta_full_finetune_gpu import POS_SIDE  # noqa: E402
from test_deberta_gpu import _inputs, _model  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402

N, T, PAD_FROM, P, SEED = 3, 24, 16, (0.1, 0.1), 1234
STATE = (SEED << 20) + 1
_shared = {}


def _case():
    if not _shared:
        cfg = deberta_ref.tiny_config()
        sd = deberta_ref.seeded_weights(cfg, seed=21)
        ids, mask = _inputs(cfg, N, T, 71, pad_from=PAD_FROM)
        dout, _ = _douts(cfg, N, T, 72)
        emb = torch.randn(N, T, cfg.hidden_size, generator=torch.Generator().manual_seed(73))
        masks = D.call_masks(STATE, D.sites(cfg.num_hidden_layers), cfg, N, T, *P)
        _shared.update(cfg=cfg, sd=sd, ids=ids, mask=mask, dout=dout, emb=emb, masks=masks, keys=list(deberta_ref.hf_keys(cfg)))
    return _shared


def _trained(c, chunk=None, p=P, k=None, embeddings=True):
    """the model in train() with dropout ``p``, every parameter trainable (``k`` None) or the top ``k`` layers"""
    m = _model(c["cfg"], c["sd"], chunk=chunk)
    L = c["cfg"].num_hidden_layers
    if k is None:
        m.set_trainable_layers(L, embeddings=embeddings)
    else:
        m.set_trainable_layers(k)
    if p is not None:
        m.set_dropout(*p)
    return m.train()


def _seeded(m, x, c, keys):
    from mmfusion import ops
    ops.seed_dropout(SEED)
    return _native_wgrads(m, x, c["mask"], c["dout"], keys)


def _ref(c, x, keys, bf16_storage, masks=None, want_input=False):
    """float64 autograd through the training-mode restatement -> ({key: gradient} (+ "inputs_embeds"), the output)"""
    leaves = {key: v.double().clone().requires_grad_(key in keys) for key, v in c["sd"].items()}
    wrt = [leaves[key] for key in keys]
    if want_input:
        x = x.double().clone().requires_grad_(True)
        wrt = wrt + [x]
    out = D.deberta_forward(leaves, x, c["mask"], c["cfg"], c["masks"] if masks is None else masks, bf16_storage=bf16_storage)
    grads = torch.autograd.grad(out, wrt, c["dout"].double())
    return dict(zip(list(keys) + (["inputs_embeds"] if want_input else []), grads)), out.detach()


def _ids_refs(c):
    if "exact" not in c:
        c["exact"], c["out_exact"] = _ref(c, c["ids"], c["keys"], False)
        c["stored"], c["out_stored"] = _ref(c, c["ids"], c["keys"], True)
    return c["exact"], c["stored"]


def test_forward_and_every_parameter_gradient_against_the_restatement():
    c = _case()
    exact, stored = _ids_refs(c)
    got, out = _seeded(_trained(c), c["ids"].cuda(), c, c["keys"])
    a, b, model_err = l2_rel(out, c["out_stored"]), l2_rel(out, c["out_exact"]), l2_rel(c["out_stored"], c["out_exact"])
    plain = deberta_ref.deberta_forward(c["sd"], c["ids"], c["mask"], c["cfg"], bf16_storage=True)
    print(f"NativeDeberta tiny {N} x {T}, dropout {P}: forward (a) vs the bf16-storage restatement under the restated masks {a:.3e} "
          f"(bound {BOUND_A}); (b) vs the exact one {b:.3e} (bound {2 * model_err:.3e}); the inference restatement is {l2_rel(out, plain):.3e} away")
    assert a <= BOUND_A and b <= 2 * model_err and l2_rel(out, plain) > 10 * BOUND_A
    _rule_b(f"NativeDeberta tiny {N} x {T}, dropout {P}, all weights,", got, exact, stored)


def test_prompt_route_input_gradient_and_embedding_side_against_the_restatement():
    c = _case()
    keys = ["embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"] + POS_SIDE
    exact, _ = _ref(c, c["emb"], keys, False, want_input=True)
    stored, _ = _ref(c, c["emb"], keys, True, want_input=True)
    leaf = c["emb"].cuda().requires_grad_(True)
    got, _ = _seeded(_trained(c), leaf, c, keys)
    got["inputs_embeds"] = leaf.grad.cpu()
    _rule_b(f"NativeDeberta tiny {N} x {T}, dropout {P}, prompt route,", got, exact, stored)
    assert bool((got["inputs_embeds"][c["mask"] == 0] == 0).all())
    # the frozen backbone under prompt tuning: the same route with nothing but the input to train
    frozen = _trained(c, k=0)
    leaf2 = c["emb"].cuda().requires_grad_(True)
    from mmfusion import ops
    ops.seed_dropout(SEED)
    frozen(inputs_embeds=leaf2, attention_mask=c["mask"].cuda()).last_hidden_state.backward(c["dout"].cuda())
    assert torch.equal(_bits(leaf2.grad), _bits(leaf.grad)), "d inputs_embeds depends on what else trains"


def test_chunk_size_does_not_change_the_result():
    c = _case()
    runs = {}
    for chunk in (1, 2, 3):
        leaf = c["emb"].cuda().requires_grad_(True)
        grads, out = _seeded(_trained(c, chunk=chunk), leaf, c, [k for k in c["keys"] if "word_embeddings" not in k])
        runs[chunk] = (out, leaf.grad.clone(), grads)
    for chunk in (1, 2):
        assert torch.equal(_bits(runs[chunk][0]), _bits(runs[3][0])), f"the output at chunk {chunk} differs from chunk 3's"
        assert torch.equal(_bits(runs[chunk][1]), _bits(runs[3][1])), f"d inputs_embeds at chunk {chunk} differs from chunk 3's"
        for key, g in runs[chunk][2].items():
            e = l2_rel(g, runs[3][2][key])
            through_pos = "query_proj" in key or "key_proj" in key or key in POS_SIDE
            bound = BOUND_A if through_pos else F32_TOL
            print(f"chunk {chunk} vs chunk 3, {key}: rel L2 {e:.3e} (bound {bound})")
            assert e <= bound, key
    # and on the ids route
    outs = [_seeded(_trained(c, chunk=chunk), c["ids"].cuda(), c, [])[1] for chunk in (1, 2, 3)]
    assert torch.equal(_bits(outs[0]), _bits(outs[2])) and torch.equal(_bits(outs[1]), _bits(outs[2]))


def test_eval_no_grad_and_zero_probabilities_give_todays_bits():
    c = _case()
    ids, k, keys = c["ids"].cuda(), c["mask"].cuda(), c["keys"]
    plain = _trained(c, p=None)                          # built without dropout arguments, in train(): today's training call
    want, want_out = _native_wgrads(plain, ids, c["mask"], c["dout"], keys)
    m = _trained(c)
    with torch.no_grad():
        out = m(input_ids=ids, attention_mask=k).last_hidden_state
    assert not out.requires_grad and torch.equal(_bits(out), _bits(want_out)), "no_grad"
    m.eval()
    got, out = _native_wgrads(m, ids, c["mask"], c["dout"], keys)
    assert torch.equal(_bits(out), _bits(want_out)), "eval()"
    m.train()
    m.set_dropout(0.0, 0.0)
    got0, out0 = _native_wgrads(m, ids, c["mask"], c["dout"], keys)
    assert torch.equal(_bits(out0), _bits(want_out)), "p = 0 in train()"
    for key in keys:
        for g in (got, got0):
            if "LayerNorm" in key and "encoder.layer" in key:         # (mmf_layernorm_bwd_grouped's atomics: two runs differ in the last bits)
                assert l2_rel(g[key], want[key]) <= F32_TOL, key
            else:
                assert torch.equal(_bits(g[key]), _bits(want[key])), key
    # a frozen module with dropout set: every call is the inference call
    m.set_dropout(*P)
    m.set_trainable_layers(0)
    again = m(input_ids=ids, attention_mask=k).last_hidden_state
    assert not again.requires_grad and torch.equal(_bits(again), _bits(want_out))
    from mmfusion import ops
    old = ops.set_precision("fp32")
    try:
        with pytest.raises(RuntimeError, match="bf16 storage only"):
            _trained(c)(input_ids=ids, attention_mask=k)
    finally:
        ops.set_precision(old)


def test_successive_calls_draw_new_masks_and_a_state_gives_its_bits_again():
    from mmfusion import ops
    c = _case()
    m = _trained(c, k=0)
    leaf = c["emb"].cuda().requires_grad_(True)
    k, dO = c["mask"].cuda(), c["dout"].cuda()

    def call():
        out = m(inputs_embeds=leaf, attention_mask=k).last_hidden_state
        (g,) = torch.autograd.grad(out, leaf, dO)
        return out.detach().clone(), g.clone()
    ops.seed_dropout(SEED)
    a = call()
    assert int(ops.rng_state().item()) == STATE, "a call on its own advances the state by one"
    b = call()
    assert int(ops.rng_state().item()) == STATE + 1
    ops.seed_dropout(SEED)
    a2 = call()
    assert torch.equal(_bits(a[0]), _bits(a2[0])) and torch.equal(_bits(a[1]), _bits(a2[1]))
    assert not torch.equal(_bits(a[0]), _bits(b[0])) and not torch.equal(_bits(a[1]), _bits(b[1]))
    # under another state tensor (ops.dropout_state) the outer state does not move
    before = int(ops.rng_state().item())
    with ops.dropout_state(torch.tensor([STATE - 1], dtype=torch.int64, device="cuda")) as st:
        inner = call()
        assert int(st.item()) == STATE
    assert int(ops.rng_state().item()) == before
    assert torch.equal(_bits(inner[0]), _bits(a[0])) and torch.equal(_bits(inner[1]), _bits(a[1]))


def test_top_layer_fine_tuning_rebuilds_every_layers_tables():
    """set_trainable_layers(1): layer 0 is frozen, yet its posQ | posK come from this call's rel_0 = dropout_0(rel)"""
    c = _case()
    cfg = c["cfg"]
    keys = _layer_keys(cfg, 1)
    exact, stored = _ids_refs(c)
    m = _trained(c, k=1)
    got, out = _seeded(m, c["ids"].cuda(), c, keys)
    _rule_b(f"NativeDeberta tiny {N} x {T}, dropout {P}, top layer,", got, {k: exact[k] for k in keys}, {k: stored[k] for k in keys})
    _frozen_grads_are_empty(m)
    assert all(getattr(m, n).grad is None or not bool(getattr(m, n).grad.any()) for n in m._layer_params(0))
    cached = D.call_masks(STATE, D.sites(cfg.num_hidden_layers), cfg, N, T, *P)
    cached.rel[0] = None                                 # what a frozen layer's table from the weight-version cache would compute
    wrong = D.deberta_forward(c["sd"], c["ids"], c["mask"], cfg, cached, bf16_storage=True)
    right, far = l2_rel(out, c["out_stored"]), l2_rel(out, wrong)
    print(f"top-layer fine-tuning with dropout: forward vs the restatement {right:.3e} (bound {BOUND_A}); vs the one whose layer 0 reads "
          f"undropped relative embeddings {far:.3e}; those two restatements are {l2_rel(wrong, c['out_stored']):.3e} apart")
    assert right <= BOUND_A and far > 2 * right


def test_forward_and_backward_replay_from_a_captured_graph():
    from mmfusion import ops
    c = _case()
    m = _trained(c, chunk=2, k=0)
    k, dO = c["mask"].cuda(), c["dout"].cuda()

    def eager_at(state):
        ops.rng_state().fill_(state)
        leaf = c["emb"].cuda().requires_grad_(True)
        out = m(inputs_embeds=leaf, attention_mask=k).last_hidden_state
        (g,) = torch.autograd.grad(out, leaf, dO)
        torch.cuda.synchronize()
        return out.detach().clone(), g.clone()
    first, later = eager_at(STATE - 1), eager_at(STATE + 1)
    static = c["emb"].cuda().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        torch.autograd.grad(m(inputs_embeds=static, attention_mask=k).last_hidden_state, static, dO)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ops.rng_state().fill_(STATE - 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(inputs_embeds=static, attention_mask=k).last_hidden_state
        (grad,) = torch.autograd.grad(out, static, dO)
    graph.replay()
    torch.cuda.synchronize()
    assert int(ops.rng_state().item()) == STATE, "the replay advances the device state"
    assert torch.equal(_bits(out), _bits(first[0])) and torch.equal(_bits(grad), _bits(first[1]))
    ops.rng_state().add_(1)
    graph.replay()
    torch.cuda.synchronize()
    assert int(ops.rng_state().item()) == STATE + 2
    assert torch.equal(_bits(out), _bits(later[0])) and torch.equal(_bits(grad), _bits(later[1]))
    assert not torch.equal(_bits(later[1]), _bits(first[1]))


def test_text_encoder_trains_with_backbone_dropout_and_eval_is_the_plain_encoder():
    import config as cfgmod
    from mmfusion import arena, ops
    from mmfusion.train import finetune_optimizer
    from models.encoders import TextEncoder
    tcfg = deberta_ref.tiny_config()

    def build(dropout):
        cfg = cfgmod.ModelConfig()
        cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.text_hidden_size = 256, 0.0, 256
        cfg.text_backbone = "native"
        cfg.text_backbone_kwargs = {k: v for k, v in deberta_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
        cfg.text_backbone_trainable_layers = "all"
        if dropout is not None:
            cfg.text_backbone_dropout = dropout
        torch.manual_seed(3)
        enc = TextEncoder(cfg)
        enc.model.load_state_dict(deberta_ref.seeded_weights(tcfg, seed=31))
        return enc.cuda()
    enc, plain = build(True), build(None)
    assert (enc.model.config.hidden_dropout_prob, enc.model.config.attention_probs_dropout_prob) == (0.1, 0.1)
    ids, mask = _inputs(tcfg, N, T, 74, pad_from=PAD_FROM)
    ids, mask = ids.cuda(), mask.cuda()
    enc.eval(), plain.eval()
    a, b = enc(ids, mask), plain(ids, mask)
    assert a["features"].requires_grad and torch.equal(_bits(a["features"].detach()), _bits(b["features"].detach()))
    assert torch.equal(_bits(a["sequence_output"].detach()), _bits(b["sequence_output"].detach()))
    enc.train(), plain.train()
    ops.seed_dropout(SEED)
    dropped = enc(ids, mask)["sequence_output"].detach()
    assert int(ops.rng_state().item()) == STATE, "under a root module the backbone must not advance the state again"
    assert not torch.equal(_bits(dropped), _bits(plain(ids, mask)["sequence_output"].detach()))
    ar = arena.ensure(enc)
    opt = finetune_optimizer(enc, ar, lr=1e-2, weight_decay=0.01)
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    for _ in range(2):
        ar.zero_grad()
        feats = enc(ids, mask)["features"]
        assert feats.requires_grad
        feats.sum().backward()
        opt.advance()
        opt.launch()
    torch.cuda.synchronize()
    for n, p in enc.named_parameters():
        if n.startswith(("model.", "projection.")):
            assert bool(torch.isfinite(p).all()), n
            assert not torch.equal(_bits(p.detach()), _bits(before[n])), f"{n} did not move"
