#!/usr/bin/env python3
"""Cost of the few-shot episode step on the MELD-shaped model (hierarchical d = 512 / 8 heads / G = 512, feature inputs,
n_way = 7, Nq = 16, n_shot in {1, 5, 10}):

  * ms/step, eager and graph-replayed (single-chain capture, bench.single_stream), of ``FewShotTrainStep``;
  * weight-gradient problems queued per step (mmfusion.ops deferred wgrad queue): the few-shot step with its frozen
    encoders against ``FusionTrainStep``'s forward + backward on the same base model;
  * GPU kernel launches of the episode head, forward + backward of the loss (torch.profiler): the fused head against
    the torch formulation of the reference (mean, prototype MLP, cdist, softmax, CrossEntropy on the probabilities).

    python tools/fewshot_bench.py [--steps 50] [--warmup 10]
Prints one JSON line."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "simple-multimodal_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
os.environ.setdefault("MMFUSION_CONFIG_MKDIRS", "0")
import torch

from distill_bench import _cfg, count_kernels, time_eager, time_graph


def _data(B, seed):
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B, 9, 768, generator=g).cuda()
    audio = torch.randn(B, 21, 768, generator=g).cuda()
    video = torch.randn(B, 6, 768, generator=g).cuda()
    return {"input_ids": text, "attention_mask": torch.ones(B, 9, dtype=torch.long).cuda()}, audio, video


def queued_wgrad(fn) -> int:
    """weight-gradient problems one forward + backward queues"""
    from mmfusion import ops
    ops.set_manual_wgrad_flush(True)
    try:
        fn()
        pend = ops.take_pending_wgrad()
        ops.issue_wgrad(pend)
    finally:
        ops.set_manual_wgrad_flush(False)
    torch.cuda.synchronize()
    return len(pend)


def torch_head(model, support, query, n_way, n_shot, targets):
    sf = support[0] + support[1] + support[2]
    prototypes = model.prototype_network(sf.view(n_way, n_shot, -1).mean(1))
    qf = query[0] + query[1] + query[2]
    pred = torch.softmax(-torch.cdist(qf, prototypes, p=2), dim=-1)
    return torch.nn.functional.cross_entropy(pred, targets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nq", type=int, default=16)
    args = ap.parse_args()
    from mmfusion import arena as arena_mod, small_ops
    from mmfusion.train import FewShotTrainStep, FusionTrainStep, backward_from, fusion_loss
    from models.multimodal_model import FewShotModel, MultimodalEmotionModel
    n_way, Nq, d = 7, args.nq, 512
    res = {"model": "few-shot wrapper over hierarchical 512/8/G512, feature inputs", "n_way": n_way, "Nq": Nq}

    # the standard step on the same base model shape: its queued weight-gradient problems
    torch.manual_seed(0)
    base = MultimodalEmotionModel(_cfg(512, 8, 512)).cuda().train()
    fs = FusionTrainStep(base, None, arena_mod.ensure(base), lr=1e-4, total_steps=1000)
    ti, au, vi = _data(16, 1)
    labels16 = torch.randint(0, 7, (16,), generator=torch.Generator().manual_seed(7)).cuda()

    def fusion_fwd_bwd():
        fs.arena.zero_grad(overlap=True, lazy=True)
        loss = fusion_loss(base(ti, au, vi, compute_contrastive_loss=True), labels16)
        backward_from(loss)
        fs.arena.finalize_grads()
        return loss

    fusion_fwd_bwd()
    res["fusion_wgrad_problems"] = queued_wgrad(fusion_fwd_bwd)

    torch.manual_seed(0)
    cfg = _cfg(512, 8, 512)
    model = FewShotModel(MultimodalEmotionModel(cfg), cfg).cuda().train()
    query = _data(Nq, 2)
    targets = torch.randint(0, n_way, (Nq,), generator=torch.Generator().manual_seed(3)).cuda()
    for n_shot in (1, 5, 10):
        support = _data(n_way * n_shot, 10 + n_shot)
        ts = FewShotTrainStep(model, n_way, n_shot, lr=1e-4)
        step = lambda: ts(support, query, targets)
        res[f"shot{n_shot}_eager_ms"] = round(time_eager(step, args.steps, args.warmup), 4)
        res[f"shot{n_shot}_graph_ms"] = round(time_graph(step, args.steps, args.warmup), 4)
        res[f"shot{n_shot}_launches_eager"] = count_kernels(step)
        res[f"shot{n_shot}_wgrad_problems"] = queued_wgrad(lambda: ts.fwd_bwd(support, query, targets))
    res["fewshot_optimizer_ranges"] = len(ts.opt.ranges)

    # the head alone at n_shot = 5, forward + backward from the loss
    n_shot = 5
    sup = [torch.randn(n_way * n_shot, d, device="cuda", requires_grad=True) for _ in range(3)]
    qry = [torch.randn(Nq, d, device="cuda", requires_grad=True) for _ in range(3)]
    arena_mod.ensure(model)
    pn = [p for p in model.prototype_network.parameters()]

    def fused():
        out = model.head(sup, qry, n_way, n_shot)
        loss = small_ops.fusion_loss(out[4], targets, 0.0, [], [])
        backward_from(loss)

    def plain():
        torch.autograd.grad(torch_head(model, sup, qry, n_way, n_shot, targets), [*sup, *qry, *pn])

    for fn in (fused, plain):
        fn()                                     # first-use allocations outside the count
    torch.cuda.synchronize()
    res["head_launches_fused"] = count_kernels(fused)
    res["head_launches_torch"] = count_kernels(plain)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
