"""CPU: the float64 closed forms tests/deberta_embed_grad_ref.py (what the GPU tests hold ``mmf_deberta_embed_bwd_params`` and
``mmf_embedding_scatter_add_f32`` to) against float64 torch autograd through ``LayerNorm(table[ids]) * mask`` and ``index_add_``,
with duplicate ids, ids outside the table and masked rows; and ``NativeDeberta.set_trainable_layers(k, embeddings=...)``'s
bookkeeping, which needs no GPU."""
import pytest
import torch

import deberta_embed_grad_ref as R
import deberta_ref

EPS = 1e-7


def _case(rows, d, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(vocab, d, generator=g, dtype=torch.float64) * 2.0 + 0.3
    ids = torch.randint(0, vocab, (rows,), generator=g)
    ids[1], ids[2], ids[rows - 1] = -3, vocab + 5, ids[0]               # outside the table on both sides, and a duplicate
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
    mask = (torch.rand(rows, generator=g) > 0.3).double()
    mask[0], mask[3] = 1.0, 0.0
    dy = torch.randn(rows, d, generator=g, dtype=torch.float64)
    return table, ids, gamma, beta, mask, dy


@pytest.mark.parametrize("use_mask", [False, True])
def test_closed_form_of_the_embedding_backward_against_autograd(use_mask):
    rows, d, vocab = 23, 16, 9                                          # 23 ids over 9 rows: every row several times
    table, ids, gamma, beta, mask, dy = _case(rows, d, vocab, 5)
    mask = mask if use_mask else None
    m = 1.0 if mask is None else mask.unsqueeze(-1)
    # ids route: the table is the leaf, so autograd's gradient is the scatter of the rows' gradient
    leaf, lg, lb = table.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = deberta_ref.layer_norm(leaf[R.clamp_ids(ids, vocab)], lg, lb, EPS) * m
    dt, dg, db = torch.autograd.grad(y, [leaf, lg, lb], dy)
    (d_rows, dgamma, dbeta), mags = R.embed_bwd_params(dy, gamma, EPS, mask, ids=ids, table=table)
    assert torch.allclose(dgamma, dg, rtol=1e-12, atol=1e-12) and torch.allclose(dbeta, db, rtol=1e-12, atol=1e-12)
    got, count, mag = R.scatter_add(ids, d_rows, vocab, mask)
    assert torch.allclose(got, dt, rtol=1e-12, atol=1e-12)
    assert int(count.sum()) == (rows if mask is None else int(mask.sum())) and int(count.max()) >= 3
    assert bool((mag >= got.abs() - 1e-12).all()) and all(bool((mg >= v.abs() - 1e-12).all()) for mg, v in zip(mags, (d_rows, dgamma, dbeta)))
    if mask is not None:
        assert bool((d_rows[mask == 0] == 0).all())
    # embeds route: the rows themselves are the leaf
    emb = table[R.clamp_ids(ids, vocab)].clone().requires_grad_(True)
    y = deberta_ref.layer_norm(emb, lg, lb, EPS) * m
    de, dg2, db2 = torch.autograd.grad(y, [emb, lg, lb], dy)
    (d_rows2, dgamma2, dbeta2), _ = R.embed_bwd_params(dy, gamma, EPS, mask, embeds=emb.detach())
    assert torch.allclose(d_rows2, de, rtol=1e-12, atol=1e-12) and torch.equal(d_rows2, d_rows)
    assert torch.allclose(dgamma2, dg2, rtol=1e-12, atol=1e-12) and torch.allclose(dbeta2, db2, rtol=1e-12, atol=1e-12)


def test_closed_form_of_the_scatter_against_index_add():
    rows, d, vocab = 40, 8, 11
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(-4, vocab + 4, (rows,), generator=g)
    d_rows = torch.randn(rows, d, generator=g, dtype=torch.float64)
    fill = torch.randn(vocab, d, generator=g, dtype=torch.float64)
    mask = (torch.rand(rows, generator=g) > 0.4).double()
    only = int(R.clamp_ids(ids, vocab)[7])
    mask[R.clamp_ids(ids, vocab) == only] = 0                           # every occurrence of one table row is masked
    for mk in (None, mask):
        keep = torch.ones(rows, dtype=torch.bool) if mk is None else mk != 0
        want = fill.clone().index_add_(0, R.clamp_ids(ids, vocab)[keep], d_rows[keep])
        got, count, mag = R.scatter_add(ids, d_rows, vocab, mk, fill)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
        assert torch.equal(count, torch.bincount(R.clamp_ids(ids, vocab)[keep], minlength=vocab))
        assert torch.equal(got[count == 0], fill[count == 0]) and bool((mag >= got.abs() - 1e-12).all())
    assert int(count[only]) == 0


def test_set_trainable_layers_with_the_embeddings():
    from mmfusion.deberta import NativeDeberta
    cfg = deberta_ref.tiny_config()
    m = NativeDeberta(**deberta_ref.config_kwargs(cfg))
    L = cfg.num_hidden_layers
    emb = sorted(NativeDeberta._EMBEDDING_PARAMS)
    assert emb == ["emb_ln_b", "emb_ln_w", "enc_ln_b", "enc_ln_w", "rel_emb", "word_emb"]
    trainable = lambda: sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert m.trainable_layers == 0 and m.trainable_embeddings is False and trainable() == []
    m.set_trainable_layers(L)
    assert m.trainable_embeddings is False and not set(trainable()) & set(emb)
    m.set_trainable_layers(L, embeddings=True)
    assert m.trainable_layers == L and m.trainable_embeddings is True
    assert trainable() == sorted(n for n, _ in m.named_parameters())          # every parameter, as the reference's optimiser steps
    for bad in ((L - 1, True), (0, True), (L, 1), (L, None)):
        with pytest.raises(ValueError):
            m.set_trainable_layers(bad[0], embeddings=bad[1])
    assert m.trainable_embeddings is True                                    # a refused call changes nothing
    m.set_trainable_layers(0)
    assert m.trainable_layers == 0 and m.trainable_embeddings is False and trainable() == []
    # without a trainable table the gather is the no_grad one, on any device
    ids = torch.tensor([[1, 2, 2]])
    e = m.embeddings.word_embeddings(ids)
    assert not e.requires_grad and torch.equal(e, m.state_dict()["embeddings.word_embeddings.weight"][ids])


def test_text_encoder_maps_all_to_every_layer_and_the_embeddings():
    import config as cfgmod
    from models.encoders import TextEncoder
    tcfg = deberta_ref.tiny_config()
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.text_hidden_size = 256, 0.0, 256
    cfg.text_backbone = "native"
    cfg.text_backbone_kwargs = {k: v for k, v in deberta_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
    cfg.text_backbone_trainable_layers = "all"
    enc = TextEncoder(cfg)
    assert enc.model.trainable_layers == tcfg.num_hidden_layers and enc.model.trainable_embeddings
    assert all(p.requires_grad for p in enc.model.parameters())
    cfg.text_backbone_trainable_layers = 1
    enc = TextEncoder(cfg)
    assert enc.model.trainable_layers == 1 and not enc.model.trainable_embeddings
