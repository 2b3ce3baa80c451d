#!/usr/bin/env python3
"""Cost of the native frozen BERT backbone (mmfusion.bert.NativeBert, bert-base sizes, seeded weights) on one MI355X:

  (a) ``forward`` on three batches, 16 x 512 with an all-ones mask, 16 x 512 with lengths drawn uniformly from 32 .. 512 (a padded
      batch: the attention skips the tiles behind each item's last token) and 8 x 128, against HuggingFace's ``BertModel`` in bf16
      through stock torch on the same GPU, same weights and inputs, same timing loop, with the relative L2 between the two;
      skipped with --no-torch or where transformers is missing;
  (b) ``mmf_attn_fwd_keymask`` against ``mmf_attn_fwd_grouped`` on the same problem (B = 16, H = 12, T = 512, head_dim 64, the fused
      qkv rows), with the all-ones mask (the ratio is what reading the mask costs) and with the drawn lengths (what skipping buys);
  (c) ``mmf_bert_embed`` and ``mmf_mask_pack`` on the 16 x 512 batch, with the bytes they have to move;
  and, with --table, the per-kernel table of one 16 x 512 forward from HIP events around every launch (mmfusion.lib.PROFILE).

(b) and (c) are timed in windows of --launches back-to-back launches between two HIP events, the attention kernels alternating
window by window over --rounds rounds (the median window is reported with the spread), so that a drifting clock or a neighbour on
the host hits all alike.

    python tools/bert_bench.py [--steps 5] [--warmup 2] [--launches 200] [--rounds 7] [--table] [--no-torch]
Prints one JSON line (the table, when asked for, on the lines before it)."""
import json

from backbone_bench import kernel_table, parser, print_table, time_eager  # (first: it sets the import path)
import torch

from wavlm_bench import windows


def drawn_mask(N: int, T: int, seed: int = 2) -> torch.Tensor:
    """(N, T) int64: item lengths drawn uniformly from 32 .. T"""
    lengths = torch.randint(32, T + 1, (N,), generator=torch.Generator().manual_seed(seed))
    return (torch.arange(T).view(1, T) < lengths.view(N, 1)).to(torch.int64)


def kernels(model, ids, mask, launches: int, rounds: int) -> dict:
    from mmfusion import lib
    c, dh = model.config, model.head_dim
    H, d = c.num_attention_heads, c.hidden_size
    n, T = ids.shape
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(n * T, 3 * d, generator=g).cuda().to(torch.bfloat16)
    att = [torch.empty(n * T, d, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    ws = {"lse": torch.empty(n * H * T, device="cuda")}
    probs = [model._attn_problem(ws, qkv, a, n, T, T) for a in att]
    words = lib.mask_pack_words(T)
    ones, drawn = (torch.empty(n * words, dtype=torch.int32, device="cuda") for _ in range(2))
    m8 = mask.to(torch.uint8).cuda()
    lib.mask_pack(None, ones, n, T)
    lib.mask_pack(m8, drawn, n, T)
    res = windows({"attn_fwd_keymask_ones": lambda: lib.attn_fwd_keymask(probs[0], dh, dh ** -0.5, ones),
                   "attn_fwd_keymask_drawn": lambda: lib.attn_fwd_keymask(probs[1], dh, dh ** -0.5, drawn),
                   "attn_fwd_grouped": lambda: lib.attn_fwd_grouped([probs[2]], dh, dh ** -0.5)}, launches, rounds)
    flop = 4.0 * n * H * T * T * dh
    for name in ("attn_fwd_keymask_ones", "attn_fwd_grouped"):
        res[name]["tflops"] = round(flop / res[name]["us"] / 1e6, 1)
    res["keymask_ones_over_plain"] = round(res["attn_fwd_keymask_ones"]["us"] / res["attn_fwd_grouped"]["us"], 4)
    res["keymask_drawn_over_plain"] = round(res["attn_fwd_keymask_drawn"]["us"] / res["attn_fwd_grouped"]["us"], 4)
    res["drawn_valid_fraction"] = round(float(mask.float().mean()), 4)
    x = torch.empty(n * T, d, dtype=torch.bfloat16, device="cuda")
    flat = ids.reshape(-1).cuda()
    res.update(windows({"bert_embed": lambda: model._embed(x, T, flat, None, None),
                        "mask_pack": lambda: lib.mask_pack(m8, drawn, n, T)}, launches, rounds))
    nbytes = n * T * (3 * d * 4 + d * 2 + 8)                   # three f32 rows in, one bf16 row out, the id
    res["bert_embed"].update(mbytes=round(nbytes / 2 ** 20, 2), tb_per_s=round(nbytes / res["bert_embed"]["us"] / 1e6, 3))
    nbytes = n * T + n * words * 4
    res["mask_pack"].update(kbytes=round(nbytes / 2 ** 10, 2), gb_per_s=round(nbytes / res["mask_pack"]["us"] / 1e3, 3))
    res["problem"] = {"B": n, "H": H, "T": T, "head_dim": dh, "launches_per_window": launches, "rounds": rounds}
    return res


def main():
    ap = parser(steps=5, warmup=2, torch_yardstick=True)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import bert_ref
    from mmfusion import bert
    model = bert.NativeBert(**bert.FAMILIES["base"])
    cfg = bert_ref.base_config("bert")
    sd = bert_ref.seeded_weights(cfg, "bert", seed=0)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(1)
    shapes = {"16x512_ones": (16, 512, False), "16x512_drawn": (16, 512, True), "8x128_ones": (8, 128, False)}
    batches = {}
    for name, (N, T, draw) in shapes.items():
        ids = torch.randint(1, cfg.vocab_size, (N, T), generator=g)
        mask = drawn_mask(N, T) if draw else torch.ones(N, T, dtype=torch.int64)
        ids = ids * mask                                       # pad id 0 behind each item's length
        batches[name] = (ids.cuda(), mask.cuda())
    res = {"model": "bert-base, frozen, bf16 storage", "chunk": model.chunk,
           "workspace_mb_per_item_512": round(model.workspace_bytes_per_item(512) / 2 ** 20, 2), "forward": {}}
    for name, (ids, mask) in batches.items():
        ms = time_eager(lambda: model(input_ids=ids, attention_mask=mask), args.steps, args.warmup)
        res["forward"][name] = {"ms": round(ms, 3), "items_per_s": round(ids.shape[0] / ms * 1e3, 1)}
    if args.table:
        ids, mask = batches["16x512_ones"]
        res["kernels_of_one_forward"] = kernel_table(lambda: model(input_ids=ids, attention_mask=mask))
        print_table(res["kernels_of_one_forward"])
    ids, mask = batches["16x512_drawn"]
    res["kernels"] = kernels(model, ids.cpu(), mask.cpu(), args.launches, args.rounds)
    if not args.no_torch:
        try:
            import transformers
        except ImportError:
            transformers = None
        if transformers is None:
            res["torch_bf16_forward"] = "not measured: transformers does not import"
        else:
            kw = {k: v for k, v in bert_ref.hf_config_kwargs(cfg).items() if k != "attn_implementation"}       # (its default attention)
            hf = transformers.BertModel(transformers.BertConfig(**kw)).eval()
            hf.load_state_dict(sd)
            hf = hf.cuda().to(torch.bfloat16)
            res["torch_bf16_forward"], res["native_over_torch"], res["native_vs_torch_bf16_rel_l2"] = {}, {}, {}
            for name, (ids, mask) in batches.items():
                def stock():
                    with torch.no_grad():
                        return hf(input_ids=ids, attention_mask=mask).last_hidden_state.float()
                tms = time_eager(stock, args.steps, args.warmup)
                res["torch_bf16_forward"][name] = {"ms": round(tms, 3), "items_per_s": round(ids.shape[0] / tms * 1e3, 1)}
                res["native_over_torch"][name] = round(tms / res["forward"][name]["ms"], 3)
                a, b = model(input_ids=ids, attention_mask=mask).last_hidden_state, stock()
                valid = mask.bool()                            # (the rows of real tokens: what a user reads)
                res["native_vs_torch_bf16_rel_l2"][name] = round(float((a[valid] - b[valid]).norm() / b[valid].norm()), 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
