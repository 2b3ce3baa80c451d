#!/usr/bin/env python3
"""Two checkouts of this project side by side on the three frozen backbones: are their results bit-identical, and is one slower on
the host side.  Each subcommand is one process, so every tree gets a fresh one (``TREE`` = the root of a checkout whose
``libmmfusion.so`` is built; only its ``simple-multimodal_amd`` and ``tests/*_ref.py`` are imported).

    python tools/backbone_compare.py save TREE OUT.pt        outputs of the backbones of TREE: tiny_config (N=3, chunk=2) and base_config
                                                             (N=2), seeded_weights(seed=21), seeded inputs; ViT forward and cls_features,
                                                             Wav2Vec2 on 4000 samples, DeBERTa from ids with a padded tail + mask and
                                                             through inputs_embeds, the gradient of inputs_embeds for a seeded dout,
                                                             and every backward: the top two layers trainable (ViT on both routes), and at
                                                             tiny sizes every layer with the embeddings / the front end (DeBERTa from ids
                                                             and through inputs_embeds with its gradient): every parameter .grad after one
                                                             backward for a seeded dout, and the launches mmfusion.lib.PROFILE recorded.
                                                             Training mode, tiny sizes only, every layer trainable: DeBERTa in train() with
                                                             set_dropout(0.1, 0.1) and the embeddings, from ids with the padded tail;
                                                             Wav2Vec2 in train() with set_regularisation(**REG_960H) and the front end on
                                                             4000 samples, layerdrop_generator seeded; ops.seed_dropout(25) before each
                                                             call: the result, every parameter .grad and the launches.  A launch label
                                                             in RENAMED_LABELS is recorded under its new name, whichever tree is saved
    python tools/backbone_compare.py equal A.pt B.pt REPORT [A2.pt ...]
                                                             torch.equal per case (== for a launch list) -> REPORT; exit 1 unless all are
                                                             equal.  A2.pt ...: further saves of A's tree; a 1-d parameter .grad (a bias or
                                                             LayerNorm gradient: sums through f32 atomics in free order) that differs among
                                                             A's saves is listed as not reproducible, with its distance from B beside A's own
                                                             spread, and not compared; any other case that differs among them fails
    python tools/backbone_compare.py speed RUNS REPORT       RUNS: lines "== TOOL [ARGUMENTS] TAG" (TAG = parent | new) each followed by the
                                                             JSON line that tools/TOOL printed from that tree, the trees alternated.
                                                             -> REPORT: every ``*_chunk*``, ``differentiable_forward_ms`` and
                                                             ``[regularised_[no_layerdrop_]]forward_backward_ms`` figure of every run, both
                                                             medians, the parent's min-max spread; exit 1 unless every new median <= parent
                                                             median + spread
"""
import json
import os
import statistics
import sys


PARAM_GRAD = "grad_param_"      # in a case's name: a parameter's .grad, the only cases `equal` may find unreproducible in one tree
# launch labels (mmfusion.lib._Timed) renamed since the parent commit, old -> new: `save` records the new one for either tree, so
# that the launch lists compare; nothing else is normalised
RENAMED_LABELS = {"deberta_dropout_kernel": "hidden_dropout_kernel"}


def save(tree, out):
    tree = os.path.abspath(tree)
    sys.path.insert(0, os.path.join(tree, "simple-multimodal_amd"))
    sys.path.insert(0, os.path.join(tree, "tests"))
    os.environ.setdefault("MMFUSION_CONFIG_MKDIRS", "0")
    import torch
    import deberta_ref
    import vit_ref
    import w2v_ref
    from mmfusion import arena, backbone, deberta, lib, ops, vit, wav2vec2
    assert os.path.dirname(os.path.abspath(backbone.__file__)) == os.path.join(tree, "simple-multimodal_amd", "mmfusion"), backbone.__file__

    def model(cls, ref, cfg, kw):
        m = cls(**ref.config_kwargs(cfg), **kw)
        m.load_state_dict(ref.seeded_weights(cfg, seed=21))
        return m.cuda().eval()

    res = {}

    def backward(case, m, run, leaf=None, training=False):
        """one differentiable ``run()`` and its backward for a seeded dout, the gradients zeroed before it -> the case's every
        parameter .grad (and ``leaf``'s), and the launches ``lib.PROFILE`` recorded from the call to the end of the backward.
        ``training``: a training-mode call: the dropout state is seeded before it and the result is recorded too"""
        arena.ensure(m).zero_grad()
        if training:
            ops.seed_dropout(25)
        torch.cuda.synchronize()
        lib.PROFILE = []
        try:
            out = run()
            out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(23)).cuda())
            torch.cuda.synchronize()
            res[f"{case}_launches"] = [(RENAMED_LABELS.get(label, label), tuple(tuple(int(v) for v in d) for d in detail))
                                       for label, _, _, _, detail in lib.PROFILE]
        finally:
            lib.PROFILE = None
        if training:
            res[f"{case}_result"] = out.detach().cpu().clone()
        if leaf is not None:
            res[f"{case}_grad_input"] = leaf.grad.cpu().clone()
        res.update({f"{case}_{PARAM_GRAD}{n}": p.grad.cpu().clone() for n, p in m.named_parameters() if p.requires_grad})

    for size in ("tiny", "base"):
        N, kw = (3, dict(chunk=2)) if size == "tiny" else (2, {})
        g = torch.Generator().manual_seed(22)
        cfg = getattr(vit_ref, size + "_config")()
        m = model(vit.NativeViT, vit_ref, cfg, kw)
        x = torch.rand(N, cfg.num_channels, cfg.image_size, cfg.image_size, generator=g).cuda()
        res[f"vit_{size}_forward"] = m(x).last_hidden_state.cpu()
        res[f"vit_{size}_cls_features"] = m.cls_features(x).cpu()
        # the backwards: the top two layers, then (tiny) every layer and the embeddings, on both routes
        for tag, args in (("top2", (2,)), ("all", (cfg.num_hidden_layers, True)))[:2 if size == "tiny" else 1]:
            m.set_trainable_layers(*args)
            backward(f"vit_{size}_{tag}_forward", m, lambda: m(x).last_hidden_state)
            backward(f"vit_{size}_{tag}_cls_features", m, lambda: m.cls_features(x))
        cfg = getattr(w2v_ref, size + "_config")()
        m = model(wav2vec2.NativeWav2Vec2, w2v_ref, cfg, kw)
        wave = (0.5 * torch.randn(N, 4000, generator=g)).cuda()
        res[f"w2v_{size}_forward_4000"] = m(wave).last_hidden_state.cpu()
        for tag, args in (("top2", (2,)), ("all", (cfg.num_hidden_layers, True)))[:2 if size == "tiny" else 1]:
            m.set_trainable_layers(*args)
            backward(f"w2v_{size}_{tag}_4000", m, lambda: m(wave).last_hidden_state)
        if size == "tiny":             # training mode: every regulariser of wav2vec2-base-960h, every layer and the front end
            m.train()
            m.set_regularisation(**wav2vec2.REG_960H)
            m.layerdrop_generator.manual_seed(24)
            backward("w2v_tiny_train_960h_4000", m, lambda: m(wave).last_hidden_state, training=True)
        cfg = getattr(deberta_ref, size + "_config")()
        T, pad = (70, 50) if size == "tiny" else (128, 100)
        m = model(deberta.NativeDeberta, deberta_ref, cfg, kw)
        ids = torch.randint(1, cfg.vocab_size, (N, T), generator=g)
        mask = torch.ones(N, T, dtype=torch.int64)
        ids[N - 1, pad:], mask[N - 1, pad:] = 0, 0
        i, k = ids.cuda(), mask.cuda()
        res[f"deberta_{size}_ids_padded_T{T}"] = m(input_ids=i, attention_mask=k).last_hidden_state.cpu()
        res[f"deberta_{size}_inputs_embeds_T{T}"] = m(inputs_embeds=m.embeddings.word_embeddings(i), attention_mask=k).last_hidden_state.cpu()
        # the backward: d inputs_embeds for a seeded dout, then the .grad of every parameter of the top two layers, ids route
        dout = torch.randn(N, T, cfg.hidden_size, generator=torch.Generator().manual_seed(23)).cuda()
        leaf = m.embeddings.word_embeddings(i).detach().clone().requires_grad_(True)
        res[f"deberta_{size}_grad_inputs_embeds_T{T}"] = torch.autograd.grad(m(inputs_embeds=leaf, attention_mask=k).last_hidden_state, leaf, dout)[0].cpu()
        m.set_trainable_layers(2)
        arena.ensure(m).zero_grad()
        m(input_ids=i, attention_mask=k).last_hidden_state.backward(dout)
        torch.cuda.synchronize()
        res.update({f"deberta_{size}_{PARAM_GRAD}{n}": p.grad.cpu().clone() for n, p in m.named_parameters() if p.requires_grad})
        backward(f"deberta_{size}_top2_ids", m, lambda: m(input_ids=i, attention_mask=k).last_hidden_state)
        if size == "tiny":             # every layer and the embedding side, from ids and through inputs_embeds with its gradient
            m.set_trainable_layers(cfg.num_hidden_layers, embeddings=True)
            backward("deberta_tiny_all_ids", m, lambda: m(input_ids=i, attention_mask=k).last_hidden_state)
            with torch.no_grad():
                leaf = m.embeddings.word_embeddings(i).clone().requires_grad_(True)
            backward("deberta_tiny_all_inputs_embeds", m, lambda: m(inputs_embeds=leaf, attention_mask=k).last_hidden_state, leaf)
            m.train()                  # training mode: HuggingFace's 0.1 / 0.1 at the five sites, every layer and the embeddings
            m.set_dropout(0.1, 0.1)
            backward("deberta_tiny_train_dropout_ids", m, lambda: m(input_ids=i, attention_mask=k).last_hidden_state, training=True)
        del m
        torch.cuda.empty_cache()
    assert all(bool(torch.isfinite(v).all()) for v in res.values() if isinstance(v, torch.Tensor))
    torch.save(res, out)
    print(f"{tree}: saved {len(res)} outputs to {out}")


def equal(path_a, path_b, report, *more_a):
    import torch
    a, b = torch.load(path_a), torch.load(path_b)
    again = [torch.load(p) for p in more_a]
    lines = ["Bit identity of the three backbones between two checkouts (tools/backbone_compare.py save, once per tree in a process of its",
             "own, then equal): torch.equal on the f32 results and gradients, == on the recorded launch lists.  seeded_weights(seed=21),",
             f"seeded inputs; tiny_config: N=3 chunk=2, base_config: N=2 default chunk.  {1 + len(again)} saves of the first tree.",
             "Launch labels recorded under their new names for either tree: " + ", ".join(f"{o} -> {n}" for o, n in RENAMED_LABELS.items()), ""]
    ok, loose = set(a) == set(b) and all(set(a) == set(x) for x in again), 0
    tensor = lambda v: isinstance(v, torch.Tensor)
    equal_ = lambda x, y: (x.shape == y.shape and torch.equal(x, y)) if tensor(x) and tensor(y) else (not tensor(x) and not tensor(y) and x == y)
    far = lambda x, y: float((x - y).abs().max())
    for k in a:
        shape = str(tuple(a[k].shape)) if tensor(a[k]) else f"{len(a[k])} launches"
        if not all(k in x and equal_(a[k], x[k]) for x in again):
            # only a bias or LayerNorm gradient may differ among the first tree's own saves: a 1-d sum through f32 atomics
            vector = PARAM_GRAD in k and tensor(a[k]) and a[k].dim() == 1
            ok = ok and vector
            loose += 1
            where = f": from the second tree max |diff| {far(a[k], b[k]):.3e}, among the first tree's saves {max(far(a[k], x[k]) for x in again):.3e}" \
                if vector and k in b and tensor(b[k]) and b[k].shape == a[k].shape else ""
            lines.append(f"{k:56s} {shape:18s} not reproducible in the first tree (its saves differ)"
                         + (where if vector else ": NOT a 1-d parameter gradient"))
            continue
        same = k in b and equal_(a[k], b[k])
        ok = ok and same
        diff = f"  max |diff| {far(a[k], b[k]):.3e}" if not same and k in b and tensor(a[k]) and tensor(b[k]) and a[k].shape == b[k].shape else ""
        lines.append(f"{k:56s} {shape:18s} {'equal' if same else 'DIFFERENT'}{diff}")
    lines += ["", f"{len(a)} cases, {loose} not reproducible in the first tree and not compared: the others {'all equal' if ok else 'NOT all equal'}"]
    open(report, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return ok


def speed(runs_path, report):
    runs, raw, tool, tag = {}, [], None, None
    timed = ("differentiable_forward_ms", "forward_backward_ms", "regularised_forward_backward_ms", "regularised_no_layerdrop_forward_backward_ms")

    def take(res, prefix=""):
        """the frozen forwards' ``*_chunk*`` entries, a fine-tuning run's two timings, and those of each of its ``cases``"""
        for k, v in res.items():
            if isinstance(v, dict) and "ms" in v and "_chunk" in k:
                runs.setdefault((tool, k), {}).setdefault(tag, []).append(v["ms"])
            elif k in timed:
                runs.setdefault((tool, prefix + k), {}).setdefault(tag, []).append(v)
            elif k == "cases":
                for case in v:
                    take(case, f"{case['items']} x {case['tokens']} ")
    for line in open(runs_path):
        line = line.strip()
        if line.startswith("== "):
            words = line.split()
            tool, tag = " ".join(words[1:-1]), words[-1]
        elif line.startswith("{"):
            res = json.loads(line)
            for case in [res] + res.get("cases", []):
                case.pop("kernels", None)                # (the per-kernel tables of a fine-tuning run: not compared, not kept)
                case.pop("regularised_kernels", None)
            raw.append(f"{tool} {tag}: {json.dumps(res)}")
            take(res)
    lines = ["Host-side speed of the three backbones, parent commit against this one: tools/{vit,w2v,deberta}_bench.py (default chunk,",
             "no --table, --no-torch where offered; the arguments as each heading gives them) from a checkout of each, alternated parent,",
             "new, parent, ... in one visit to one MI355X (tools/backbone_compare.py speed).  ms per batch.  Margin = the parent's own",
             "min-max spread across its repeats; pass: new median <= parent median + spread.", ""]
    ok = True
    for (tool, key), by in runs.items():
        p, n = by.get("parent", []), by.get("new", [])
        pm, nm, spread = statistics.median(p), statistics.median(n), max(p) - min(p)
        good = nm <= pm + spread and len(p) >= 3 and len(n) >= 3
        ok = ok and good
        lines += [f"{tool} {key}", f"  parent runs {p}  median {pm:.3f}  spread {spread:.3f}", f"  new    runs {n}  median {nm:.3f}",
                  f"  new - parent = {nm - pm:+.3f} ms ({(nm / pm - 1) * 100:+.2f} %), margin {spread:.3f}: {'pass' if good else 'SLOWER BEYOND THE MARGIN'}", ""]
    lines += ["all within the margin" if ok else "NOT all within the margin", "", "Every run, in the order made:"] + raw
    open(report, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[:lines.index("Every run, in the order made:")]))
    return ok


if __name__ == "__main__":
    cmd, args = sys.argv[1], sys.argv[2:]
    sys.exit(0 if {"save": save, "equal": equal, "speed": speed}[cmd](*args) is not False else 1)
