#!/usr/bin/env python3
"""Two checkouts of this project side by side on the three frozen backbones: are their results bit-identical, and is one slower on
the host side.  Each subcommand is one process, so every tree gets a fresh one (``TREE`` = the root of a checkout whose
``libmmfusion.so`` is built; only its ``simple-multimodal_amd`` and ``tests/*_ref.py`` are imported).

    python tools/backbone_compare.py save TREE OUT.pt        outputs of the backbones of TREE: tiny_config (N=3, chunk=2) and base_config
                                                             (N=2), seeded_weights(seed=21), seeded inputs; ViT forward and cls_features,
                                                             Wav2Vec2 on 4000 samples, DeBERTa from ids with a padded tail + mask and
                                                             through inputs_embeds, the gradient of inputs_embeds for a seeded dout,
                                                             and, the top two layers trainable, every parameter .grad after one backward
    python tools/backbone_compare.py equal A.pt B.pt REPORT [A2.pt ...]
                                                             torch.equal per case -> REPORT; exit 1 unless all are equal.  A2.pt ...: further
                                                             saves of A's tree; a parameter .grad that differs among A's saves (sums through
                                                             f32 atomics in free order) is listed as not reproducible and not compared; any
                                                             other case that differs among them fails
    python tools/backbone_compare.py speed RUNS REPORT       RUNS: lines "== TOOL TAG" (TAG = parent | new) each followed by the JSON line
                                                             that tools/TOOL printed from that tree, the trees alternated.  -> REPORT: every
                                                             run, both medians, the parent's min-max spread; exit 1 unless every new
                                                             median <= parent median + spread
"""
import json
import os
import statistics
import sys


PARAM_GRAD = "grad_param_"      # in a case's name: a parameter's .grad, the only cases `equal` may find unreproducible in one tree


def save(tree, out):
    tree = os.path.abspath(tree)
    sys.path.insert(0, os.path.join(tree, "simple-multimodal_amd"))
    sys.path.insert(0, os.path.join(tree, "tests"))
    os.environ.setdefault("MMFUSION_CONFIG_MKDIRS", "0")
    import torch
    import deberta_ref
    import vit_ref
    import w2v_ref
    from mmfusion import arena, backbone, deberta, vit, wav2vec2
    assert os.path.dirname(os.path.abspath(backbone.__file__)) == os.path.join(tree, "simple-multimodal_amd", "mmfusion"), backbone.__file__

    def model(cls, ref, cfg, kw):
        m = cls(**ref.config_kwargs(cfg), **kw)
        m.load_state_dict(ref.seeded_weights(cfg, seed=21))
        return m.cuda().eval()

    res = {}
    for size in ("tiny", "base"):
        N, kw = (3, dict(chunk=2)) if size == "tiny" else (2, {})
        g = torch.Generator().manual_seed(22)
        cfg = getattr(vit_ref, size + "_config")()
        m = model(vit.NativeViT, vit_ref, cfg, kw)
        x = torch.rand(N, cfg.num_channels, cfg.image_size, cfg.image_size, generator=g).cuda()
        res[f"vit_{size}_forward"] = m(x).last_hidden_state.cpu()
        res[f"vit_{size}_cls_features"] = m.cls_features(x).cpu()
        cfg = getattr(w2v_ref, size + "_config")()
        m = model(wav2vec2.NativeWav2Vec2, w2v_ref, cfg, kw)
        res[f"w2v_{size}_forward_4000"] = m((0.5 * torch.randn(N, 4000, generator=g)).cuda()).last_hidden_state.cpu()
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
        del m
        torch.cuda.empty_cache()
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
    torch.save(res, out)
    print(f"{tree}: saved {len(res)} outputs to {out}")


def equal(path_a, path_b, report, *more_a):
    import torch
    a, b = torch.load(path_a), torch.load(path_b)
    again = [torch.load(p) for p in more_a]
    lines = ["Bit identity of the three frozen backbones between two checkouts (tools/backbone_compare.py save, once per tree in a process",
             "of its own, then equal): torch.equal on the f32 results.  seeded_weights(seed=21), seeded inputs; tiny_config: N=3 chunk=2,",
             "base_config: N=2 default chunk.", ""]
    ok, loose = set(a) == set(b) and all(set(a) == set(x) for x in again), 0
    for k in a:
        if not all(k in x and torch.equal(a[k], x[k]) for x in again):
            ok = ok and PARAM_GRAD in k
            loose += 1
            lines.append(f"{k:40s} {str(tuple(a[k].shape)):18s} not reproducible in the first tree (its saves differ)"
                         + ("" if PARAM_GRAD in k else ": NOT a parameter gradient"))
            continue
        same = k in b and a[k].shape == b[k].shape and torch.equal(a[k], b[k])
        ok = ok and same
        diff = "" if same or k not in b else f"  max |diff| {float((a[k] - b[k]).abs().max()):.3e}"
        lines.append(f"{k:40s} {str(tuple(a[k].shape)):18s} {'equal' if same else 'DIFFERENT'}{diff}")
    lines += ["", f"{len(a)} cases, {loose} not reproducible in the first tree and not compared: the others {'all equal' if ok else 'NOT all equal'}"]
    open(report, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return ok


def speed(runs_path, report):
    runs, raw, tool, tag = {}, [], None, None
    for line in open(runs_path):
        line = line.strip()
        if line.startswith("== "):
            _, tool, tag = line.split()
        elif line.startswith("{"):
            raw.append(f"{tool} {tag}: {line}")
            for k, v in json.loads(line).items():
                if isinstance(v, dict) and "ms" in v and "_chunk" in k:
                    runs.setdefault((tool, k), {}).setdefault(tag, []).append(v["ms"])
    lines = ["Host-side speed of the three frozen backbones, parent commit against this one: tools/{vit,w2v,deberta}_bench.py at their",
             "defaults (default chunk, no --table, --no-torch where offered) from a checkout of each, alternated parent, new, parent, ...",
             "in one visit to one MI355X (tools/backbone_compare.py speed).  ms per batch.  Margin = the parent's own min-max spread across",
             "its repeats; pass: new median <= parent median + spread.", ""]
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
