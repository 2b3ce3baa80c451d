#!/usr/bin/env python3
"""Cost of an evaluation batch on the MELD-shaped model (hierarchical, d = 512 / 8 heads / G = 512, feature inputs, B = 16,
7 classes, eval mode, no_grad):

  * GPU kernel launches of the metrics tail per batch (torch.profiler): the reference's tail (advanced_trainer.py:231-243:
    CrossEntropyLoss(label_smoothing=0.1) + .item(), argmax, softmax and three .cpu() copies) against
    ``EvalAccumulator.update`` (collecting predictions, targets and probabilities);
  * evaluation ms per batch over --batches batches (wall clock, one sync at the end): the reference-style loop (forward +
    that tail, its host syncs included) against forward + ``update`` and one ``compute()`` at the end;
  * the graph-replayed time of forward + ``update`` for one batch (single-chain capture, bench.single_stream).

    python tools/eval_bench.py [--batches 200] [--warmup 10]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import distill_bench as db                       # noqa: E402  (puts the repository and the package on sys.path)
import torch                                     # noqa: E402
import torch.nn.functional as F                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    from mmfusion.evaluate import EvalAccumulator
    from models.multimodal_model import MultimodalEmotionModel
    torch.manual_seed(0)
    model = MultimodalEmotionModel(db._cfg(512, 8, 512)).cuda().eval()
    ti, au, vi, labels = db._inputs(args.batch)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    res = {"model": "hierarchical 512/8/G512, feature inputs, eval", "B": args.batch, "batches": args.batches}

    def ref_tail(logits, sink):
        sink[0] += crit(logits, labels).item()
        preds = torch.argmax(logits, dim=-1)
        probs = F.softmax(logits, dim=-1)
        sink[1].extend(preds.cpu().numpy())
        sink[2].extend(labels.cpu().numpy())
        sink[3].extend(probs.cpu().numpy())

    with torch.no_grad():
        logits = model(ti, au, vi)["emotion_logits"]
        acc = EvalAccumulator(7, capacity=args.batch * (args.batches + 64))
        sink = [0.0, [], [], []]
        ref_tail(logits, sink), acc.update(logits, labels)             # first-use allocations outside the count
        res["tail_launches_reference"] = db.count_kernels(lambda: ref_tail(logits, sink))
        res["tail_launches_fused"] = db.count_kernels(lambda: acc.update(logits, labels))

        def ref_pass(n):
            s = [0.0, [], [], []]
            for _ in range(n):
                ref_tail(model(ti, au, vi)["emotion_logits"], s)
            return s

        def new_pass(n):
            a = EvalAccumulator(7, capacity=args.batch * n)
            for _ in range(n):
                a.update(model(ti, au, vi)["emotion_logits"], labels)
            return a.compute()

        for name, fn in (("reference", ref_pass), ("fused", new_pass)):
            fn(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.batches)
            torch.cuda.synchronize()
            res[f"eval_ms_per_batch_{name}"] = round((time.perf_counter() - t0) * 1e3 / args.batches, 4)

    gacc = EvalAccumulator(7)

    def fwd_update():
        with torch.no_grad():
            gacc.update(model(ti, au, vi)["emotion_logits"], labels)

    try:
        res["graph_ms_forward_update"] = round(db.time_graph(fwd_update, args.batches, args.warmup), 4)
    except RuntimeError as e:                                           # reported, not hidden
        res["graph_ms_forward_update"] = f"not measured: {str(e).splitlines()[0][:160]}"
    res["eager_ms_forward_update"] = round(db.time_eager(fwd_update, args.batches, args.warmup), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
