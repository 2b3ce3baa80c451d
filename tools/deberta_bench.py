#!/usr/bin/env python3
"""Cost of the native frozen DeBERTa-v3 backbone (mmfusion.deberta.NativeDeberta, deberta-v3-base) on one batch of token ids
(default 16 items of 512 tokens, the last 32 of every second item padded):

  * ms per batch, tokens/s and TFLOP/s (by operation count: 12 layers of linears, the four attention products counted as
    12 T^2 d per layer: QK^T, PV, and the two relative-position products at their bias-free size) of ``forward``, per chunk size;
  * the disentangled attention kernel alone beside ``mmf_attn_fwd_grouped`` on the same fused qkv rows: the bias-free, mask-free
    floor, and the ratio of the two (there is no pass mark: the new kernel forms two more products and gathers);
  * with --table, a per-kernel table of one batch from HIP events around every launch (mmfusion.lib.PROFILE);
  * with --grad, the prompt-tuning cost instead: for (items, tokens) = (16, 10 + 512) and (8, 10 + 128) on input embeddings, ms of
    the inference forward, of the differentiable forward (it also keeps every layer's input) and of forward + backward, their
    ratios to the inference forward, and the per-kernel table of one forward + backward;
  * with --finetune K, the cost of fine-tuning the top K layers instead (``set_trainable_layers(K)``): on token ids, for
    (items, tokens) = (--items, --tokens) and (8, 128), the same three times and ratios (the backward stops below layer L - K and
    adds the K layers' weight gradients into the arena), the per-kernel table, and ``mmf_deberta_attn_bwd_pos`` beside
    ``mmf_deberta_attn_bwd`` on the same operands.  ``--finetune all``: every layer and the embedding side
    (``set_trainable_layers(L, embeddings=True)``); beside the above, on one chunk's operands: ``mmf_deberta_embed_bwd_params``,
    ``mmf_embedding_scatter_add_f32`` on the batch's ids and on skewed ids (one id on a quarter of the tokens), the d rel GEMMs,
    the recomputation of ``rel``, and the whole-table costs the real vocabulary adds to a step: the memset of the table's
    gradient and the AdamW step over the trainable parameters (compare with ``--finetune 12``: the same tree, embeddings frozen);
  * with --dropout P_H,P_A (beside --grad or --finetune), the same training calls in ``train()`` with the backbone's dropout at
    those probabilities (``set_dropout``; compare with the same command without it), and under --finetune the attention forward
    (with lse) and backward (delta + dQ pass + dK/dV pass, and the form with the table gradients) alone with and without the mask.

    python tools/deberta_bench.py [--items 16] [--tokens 512] [--chunks 4,8,16] [--steps 5] [--warmup 2] [--table] [--grad]
                                  [--finetune K|all] [--dropout P_H,P_A]
Prints one JSON line (the tables, when asked for, on the lines before it)."""
import json
import math

from backbone_bench import kernel_table, parser, print_table, sweep, time_eager  # (first: it sets the import path)
import torch


def gflop_per_item(cfg, T: int) -> float:
    d, I = cfg.hidden_size, cfg.intermediate_size
    return cfg.num_hidden_layers * (2.0 * T * (4 * d * d + 2 * d * I) + 12.0 * T * T * d) / 1e9


def grad_mode(model, cfg, args) -> dict:
    res = {"model": "deberta-v3-base, frozen, bf16 storage: gradient with respect to inputs_embeds", "chunk": model.chunk,
           "dropout": args.dropout, "cases": []}
    for N, T in ((16, 10 + 512), (8, 10 + 128)):
        g = torch.Generator().manual_seed(2)
        emb = torch.randn(N, T, cfg.hidden_size, generator=g).cuda()
        leaf = emb.clone().requires_grad_(True)
        dout = torch.randn(N, T, cfg.hidden_size, generator=g).cuda()
        mask = torch.ones(N, T, dtype=torch.int64)
        mask[1::2, T - 32:] = 0
        mask = mask.cuda()

        def infer():
            with torch.no_grad():
                model(inputs_embeds=emb, attention_mask=mask)
        diff = lambda: model(inputs_embeds=leaf, attention_mask=mask)
        both = lambda: torch.autograd.grad(model(inputs_embeds=leaf, attention_mask=mask).last_hidden_state, leaf, dout)
        t_inf, t_diff, t_both = (time_eager(f, args.steps, args.warmup) for f in (infer, diff, both))
        rows = kernel_table(both)
        print(f"forward + backward, {N} items of {T} tokens")
        print_table(rows)
        res["cases"].append({"items": N, "tokens": T, "inference_forward_ms": round(t_inf, 3), "differentiable_forward_ms": round(t_diff, 3),
                             "forward_backward_ms": round(t_both, 3), "differentiable_forward_ratio": round(t_diff / t_inf, 3),
                             "forward_backward_ratio": round(t_both / t_inf, 3),
                             "saved_inputs_mb": round(cfg.num_hidden_layers * N * T * cfg.hidden_size * 2 / 2 ** 20, 1),
                             "grad_workspace_mb_per_item": round(model.grad_workspace_bytes_per_item(T) / 2 ** 20, 2), "kernels": rows})
    return res


def finetune_mode(model, cfg, args) -> dict:
    from mmfusion import lib
    from mmfusion import arena, ops
    from mmfusion.train import finetune_optimizer
    full = args.finetune == "all"
    K, H, S, d = cfg.num_hidden_layers if full else int(args.finetune), cfg.num_attention_heads, cfg.position_buckets, cfg.hidden_size
    model.set_trainable_layers(K, embeddings=full)
    res = {"model": f"deberta-v3-base, bf16 storage: the top {K} layers" + (" and the embeddings" if full else "") + " trainable, token ids",
           "chunk": model.chunk, "dropout": args.dropout, "cases": []}
    for N, T in ((args.items, args.tokens), (8, 128)):
        g = torch.Generator().manual_seed(2)
        ids = torch.randint(1, cfg.vocab_size, (N, T), generator=g).cuda()
        dout = torch.randn(N, T, d, generator=g).cuda()
        mask = torch.ones(N, T, dtype=torch.int64)
        mask[1::2, max(T - 32, 1):] = 0
        mask = mask.cuda()

        def infer():
            with torch.no_grad():
                model(input_ids=ids, attention_mask=mask)
        diff = lambda: model(input_ids=ids, attention_mask=mask)
        both = lambda: model(input_ids=ids, attention_mask=mask).last_hidden_state.backward(dout)     # (the gradients accumulate)
        t_inf, t_diff, t_both = (time_eager(f, args.steps, args.warmup) for f in (infer, diff, both))
        rows = kernel_table(both)
        print(f"forward + backward, top {K} layers" + (" and the embeddings" if full else "") + f" trainable, {N} items of {T} tokens")
        print_table(rows)
        # the attention backward with and without the table gradients, on one chunk's operands
        n = min(N, model.chunk)
        qkv, att, dat = (torch.randn(n * T, w, generator=g).to(torch.bfloat16).cuda() for w in (3 * d, d, d))
        dqkv, lse, delta = torch.empty_like(qkv), torch.zeros(n * H * T, device="cuda"), torch.empty(n * H * T, device="cuda")
        posq, posk = model._pos_tables(ids.device)[0]
        idx, scale, m32 = model._index(T, ids.device), math.sqrt(3.0 * 64), mask[:n].float().contiguous()
        lib.deberta_attn_fwd(qkv, posq, posk, idx, m32, att, n, H, T, S, scale, lse=lse)
        dpos = torch.zeros(2 * S, 2 * d, device="cuda")
        ws = torch.empty(lib.deberta_attn_bwd_pos_workspace_bytes(n, H, T, S) // 4, device="cuda")
        plain = lambda: lib.deberta_attn_bwd(qkv, posq, posk, idx, m32, att, lse, dat, delta, dqkv, n, H, T, S, scale)
        withpos = lambda: lib.deberta_attn_bwd_pos(qkv, posq, posk, idx, m32, att, lse, dat, delta, dqkv, dpos[:, :d], dpos[:, d:], ws,
                                                   n, H, T, S, scale)
        t_plain, t_pos = time_eager(plain, 20, 5), time_eager(withpos, 20, 5)
        extra = {}
        if args.dropout:
            # the attention launches alone with and without the mask, on the same operands
            drop = (args.dropout[1] or 0.1, ops.rng_state(), 3, 0)
            fwd = lambda **kw: lib.deberta_attn_fwd(qkv, posq, posk, idx, m32, att, n, H, T, S, scale, lse=lse, **kw)
            t_fwd, t_fwd_d = time_eager(fwd, 20, 5), time_eager(lambda: fwd(drop=drop), 20, 5)
            t_plain_d = time_eager(lambda: lib.deberta_attn_bwd(qkv, posq, posk, idx, m32, att, lse, dat, delta, dqkv, n, H, T, S, scale, drop=drop), 20, 5)
            t_pos_d = time_eager(lambda: lib.deberta_attn_bwd_pos(qkv, posq, posk, idx, m32, att, lse, dat, delta, dqkv, dpos[:, :d], dpos[:, d:], ws,
                                                                  n, H, T, S, scale, drop=drop), 20, 5)
            extra.update(attn_fwd_lse_ms=round(t_fwd, 4), attn_fwd_lse_drop_ms=round(t_fwd_d, 4), attn_fwd_drop_ratio=round(t_fwd_d / t_fwd, 3),
                         attn_bwd_drop_ms=round(t_plain_d, 4), attn_bwd_drop_ratio=round(t_plain_d / t_plain, 3),
                         attn_bwd_pos_drop_ms=round(t_pos_d, 4), attn_bwd_pos_drop_ratio=round(t_pos_d / t_pos, 3), attn_drop_p=drop[0])
        if full:
            # the embedding side's launches alone, on one chunk's operands
            rows_, part = n * T, ids[:n].reshape(-1).contiguous()
            gx = torch.randn(rows_, d, generator=g).to(torch.bfloat16).cuda()
            d_rows, dgb = torch.empty(rows_, d, device="cuda"), torch.zeros(2, d, device="cuda")
            ews = torch.empty(lib.deberta_embed_bwd_params_workspace_bytes(max(rows_, 2 * S), d) // 4, device="cuda")
            table, dtable = model._f("word_emb"), model.word_emb.grad
            skew = part.clone()
            skew[::4] = 7
            f_a = lambda: lib.deberta_embed_bwd_params(model._f("emb_ln_w"), cfg.layer_norm_eps, m32, gx, d_rows, dgb[0], dgb[1], ews,
                                                       ids=part, table=table)
            f_b = lambda: lib.embedding_scatter_add(part, d_rows, dtable, mask=m32)
            f_skew = lambda: lib.embedding_scatter_add(skew, d_rows, dtable, mask=m32)
            dp16, drel = torch.randn(K, 2 * S, 2 * d, generator=g).to(torch.bfloat16).cuda(), torch.empty(2 * S, d, device="cuda")

            def f_drel():
                for i in range(K):
                    ops.gemm(lib.GEMM_NN, dp16[i], model._w(f"l{i}_qkv_w")[:2 * d], drel, epilogue=lib.EPI_ACCUM if i else 0)
            f_rel = lambda: model._pos_cache(ids.device)
            f_zero = lambda: dtable.zero_()
            extra.update({name + "_ms": round(time_eager(f, 20, 5), 4) for name, f in
                          (("embed_bwd_params", f_a), ("scatter_add", f_b), ("scatter_add_skewed", f_skew), ("drel_gemms", f_drel),
                           ("rel_recompute", f_rel), ("table_grad_memset", f_zero))})
            extra["table_grad_mb"] = round(dtable.numel() * 4 / 2 ** 20, 1)
        opt = finetune_optimizer(model, arena.ensure(model), lr=1e-5, weight_decay=0.01)

        def step():
            opt.advance()
            opt.launch()
        extra["adamw_step_ms"] = round(time_eager(step, 5, 2), 4)
        extra["adamw_parameters_m"] = round(sum(p.numel() for p in model.parameters() if p.requires_grad) / 1e6, 1)
        res["cases"].append({"items": N, "tokens": T, "trainable_layers": K, "embeddings": full, **extra, "inference_forward_ms": round(t_inf, 3),
                             "differentiable_forward_ms": round(t_diff, 3), "forward_backward_ms": round(t_both, 3),
                             "differentiable_forward_ratio": round(t_diff / t_inf, 3), "forward_backward_ratio": round(t_both / t_inf, 3),
                             "saved_inputs_mb": round(K * N * T * d * 2 / 2 ** 20, 1),
                             "attn_bwd_ms": round(t_plain, 4), "attn_bwd_pos_ms": round(t_pos, 4), "attn_bwd_pos_ratio": round(t_pos / t_plain, 3),
                             "pos_workspace_mb": round(ws.numel() * 4 / 2 ** 20, 1), "kernels": rows})
    return res


def main():
    ap = parser(steps=5, warmup=2)
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--finetune", type=lambda v: v if v == "all" else int(v), default=0, metavar="K|all")
    ap.add_argument("--dropout", type=lambda v: tuple(float(p) for p in v.split(",")), default=None, metavar="P_H,P_A")
    args = ap.parse_args()
    if args.dropout and (len(args.dropout) != 2 or not (args.grad or args.finetune)):
        ap.error("--dropout takes P_H,P_A and goes with --grad or --finetune")
    import deberta_ref
    from mmfusion import deberta, lib
    from mmfusion.lib import AttnProblem
    cfg = deberta_ref.base_config()
    model = deberta.NativeDeberta(**deberta_ref.config_kwargs(cfg))
    model.load_state_dict(deberta_ref.seeded_weights(cfg, seed=0))
    model = model.cuda().eval()
    if args.dropout:
        model.set_dropout(*args.dropout)
        model.train()
    if args.grad:
        print(json.dumps(grad_mode(model, cfg, args)))
        return
    if args.finetune:
        print(json.dumps(finetune_mode(model, cfg, args)))
        return
    N, T, d, H = args.items, args.tokens, cfg.hidden_size, cfg.num_attention_heads
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, cfg.vocab_size, (N, T), generator=g).cuda()
    mask = torch.ones(N, T, dtype=torch.int64)
    mask[1::2, max(T - 32, 1):] = 0
    mask = mask.cuda()
    gf = gflop_per_item(cfg, T)

    def rate(ms: float) -> dict:
        return {"ms": round(ms, 3), "tokens_per_s": round(N * T / ms * 1e3, 0), "tflops": round(gf * N / ms, 1)}

    res = {"model": "deberta-v3-base, frozen, bf16 storage", "items": N, "tokens": T, "gflop_per_item": round(gf, 2),
           "default_chunk": deberta.DEFAULT_CHUNK, "workspace_mb_per_item": round(model.workspace_bytes_per_item(T) / 2 ** 20, 2)}
    fwd = lambda: model(input_ids=ids, attention_mask=mask)

    def measure(c):
        res[f"forward_chunk{c}"] = rate(time_eager(fwd, args.steps, args.warmup))
    sweep(model, deberta.DEFAULT_CHUNK, args.chunks, measure)
    if args.table:
        res["kernels"] = kernel_table(fwd)
        print_table(res["kernels"])
    # the attention kernel alone against the bias-free, mask-free fused attention on the same rows
    n = min(N, deberta.DEFAULT_CHUNK)
    qkv = torch.randn(n * T, 3 * d, generator=g).to(torch.bfloat16).cuda()
    att = torch.empty(n * T, d, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(n * H * T, dtype=torch.float32, device="cuda")
    posq, posk = model._pos_tables(ids.device)[0]
    idx = model._index(T, ids.device)
    m32 = mask[:n].float().contiguous()
    scale = math.sqrt(3.0 * 64)
    base = qkv.data_ptr()
    floor = lambda: lib.attn_fwd_grouped([AttnProblem(base, base + 2 * d, base + 4 * d, att.data_ptr(), lse.data_ptr(), None, None, None,
                                                      None, None, n, H, T, T, 3 * d, 3 * d, 3 * d, d)], 64, 1.0 / scale)
    ours = lambda: lib.deberta_attn_fwd(qkv, posq, posk, idx, m32, att, n, H, T, cfg.position_buckets, scale)
    t_ours, t_floor = time_eager(ours, 20, 5), time_eager(floor, 20, 5)
    res["attention"] = {"items": n, "deberta_attn_fwd_ms": round(t_ours, 4), "attn_fwd_grouped_ms": round(t_floor, 4),
                        "ratio": round(t_ours / t_floor, 2), "deberta_tflops_4_products": round(12.0 * n * H * T * T * 64 / t_ours / 1e9, 1),
                        "eager_bias_mb_per_layer": round(n * H * T * T * 4 / 1e6, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
