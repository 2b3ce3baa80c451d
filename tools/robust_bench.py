#!/usr/bin/env python3
"""Cost of the robust (missing-modality) training step on the MELD-shaped model (hierarchical d = 512 / 8 heads / G = 512,
feature inputs, B = 16, dropout as configured by default):

  * ms/step, eager and graph-replayed (single-chain capture, bench.single_stream), of ``RobustTrainStep`` with the
    scenarios [] and ["audio"] missing, next to ``FusionTrainStep`` on the same base model (CE + 0.1 x contrastive on
    the fused loss, clipped OneCycle AdamW over the whole arena);
  * GPU kernel launches of the robust head, forward + backward (torch.profiler): the fused ``small_ops.robust_head``
    against the plain torch formulation of the reference over the same parameters (both after the hidden layer, which
    is the same row linear in either case).

    python tools/robust_bench.py [--steps 50] [--warmup 10]
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

from distill_bench import _cfg, _inputs, count_kernels, time_eager, time_graph


def torch_head(f_t, f_a, f_v, h, module, available=None):
    """the reference's head after the hidden layer (models/multimodal_model.py:404-440), torch ops"""
    a = module.modality_predictor[3](module.modality_predictor[2](h))
    p = [module.text_only_classifier(f_t), module.audio_only_classifier(f_a), module.video_only_classifier(f_v)]
    w = a / (torch.sum(a, dim=1, keepdim=True) + 1e-8)
    y = w[:, 0:1] * p[0] + w[:, 1:2] * p[1] + w[:, 2:3] * p[2]
    return a, p[0], p[1], p[2], w, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    from mmfusion import arena as arena_mod, small_ops
    from mmfusion.train import FusionTrainStep, RobustTrainStep
    from models.multimodal_model import RobustMultimodalModel
    torch.manual_seed(0)
    model = RobustMultimodalModel(_cfg(512, 8, 512)).cuda().train()
    ti, au, vi, labels = _inputs(args.batch)
    res = {"model": "robust wrapper over hierarchical 512/8/G512, feature inputs", "B": args.batch}

    # the base model alone, its own arena and the standard step
    torch.manual_seed(0)
    from models.multimodal_model import MultimodalEmotionModel
    base = MultimodalEmotionModel(_cfg(512, 8, 512)).cuda().train()
    fs = FusionTrainStep(base, None, arena_mod.ensure(base), lr=1e-4, total_steps=1000)

    def fusion_step():
        fs.arena.zero_grad(overlap=True, lazy=True)
        from mmfusion.train import backward_from, fusion_loss
        out = base(ti, au, vi, compute_contrastive_loss=True)
        loss = fusion_loss(out, labels)
        backward_from(loss)
        fs.arena.finalize_grads()
        fs.opt.advance()
        fs.opt.launch()
        return loss

    rs = RobustTrainStep(model, lr=1e-4)
    steps = {"fusion": fusion_step,
             "robust_all": lambda: rs(ti, au, vi, labels),
             "robust_audio_missing": lambda: rs(ti, au, vi, labels, missing_modalities=["audio"])}
    for name, fn in steps.items():
        res[f"{name}_eager_ms"] = round(time_eager(fn, args.steps, args.warmup), 4)
        res[f"{name}_launches_eager"] = count_kernels(fn)
        res[f"{name}_graph_ms"] = round(time_graph(fn, args.steps, args.warmup), 4)
    res["robust_optimizer_ranges"] = len(rs.opt.ranges)

    # the head alone, forward + backward from a loss on robust_prediction and the availability
    B, d = args.batch, 512
    f = [torch.randn(B, d, device="cuda", requires_grad=True) for _ in range(3)]
    h = torch.relu(torch.randn(B, d, device="cuda")).requires_grad_(True)
    gy, ga = torch.randn(B, 7, device="cuda"), torch.randn(B, 3, device="cuda")
    arena_mod.ensure(model)

    params = [q for l in (model.modality_predictor[2], model.text_only_classifier, model.audio_only_classifier,
                          model.video_only_classifier) for q in (l.weight, l.bias)]

    def run(head):
        # every gradient of the head: the features, h and (torch) the parameters; the fused kernel writes the
        # parameter gradients into the arena itself and hands autograd None for them
        def fn():
            a, pt, pa, pv, w, y = head(*f, h, model)
            torch.autograd.grad([y, a], [*f, h, *params], [gy, ga], allow_unused=True)
        return fn

    fused, plain = run(small_ops.robust_head), run(torch_head)
    for fn in (fused, plain):
        fn()                                     # first-use allocations outside the count
    res["head_launches_fused"] = count_kernels(fused)
    res["head_launches_torch"] = count_kernels(plain)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
