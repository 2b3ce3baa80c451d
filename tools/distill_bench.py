#!/usr/bin/env python3
"""Cost of knowledge distillation on the MELD-shaped pair (teacher: hierarchical d = 512 / 8 heads / G = 512; student:
d = 256 / 4 heads / G = 256; feature inputs, B = 16, dropout as configured by default):

  * ms/step, eager and graph-replayed (single-chain capture, bench.single_stream), of the student-alone training step
    (CE(ls=0.1) + 0.1 x contrastive on the fused loss kernel, backward, fused AdamW) and of ``DistillTrainStep``;
  * GPU kernel launches per step of each (torch.profiler, one eager step);
  * launches of the loss tail: the fused ``mmf_fusion_loss_kd`` against torch's CE(ls=0.1) + 0.1 x contrastive + 0.5 x
    kl_div(log_softmax(s / T), softmax(t / T)) * T^2, forward and backward, with the KD part counted on its own.

    python tools/distill_bench.py [--steps 50] [--warmup 10]
Prints one JSON line."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "simple-multimodal_amd"))
os.environ.setdefault("MMFUSION_CONFIG_MKDIRS", "0")
import torch
import torch.nn.functional as F

import bench


def _cfg(d, heads, G):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.feature_inputs = True
    cfg.fusion_type = "hierarchical"
    cfg.fusion_hidden_size, cfg.fusion_num_heads, cfg.graph_hidden_size = d, heads, G
    return cfg


def _inputs(B):
    g = torch.Generator().manual_seed(1234)
    text = torch.randn(B, 9, 768, generator=g).cuda()
    audio = torch.randn(B, 21, 768, generator=g).cuda()
    video = torch.randn(B, 6, 768, generator=g).cuda()
    mask = torch.ones(B, 9, dtype=torch.long).cuda()
    labels = torch.randint(0, 7, (B,), generator=torch.Generator().manual_seed(7)).cuda()
    return {"input_ids": text, "attention_mask": mask}, audio, video, labels


def count_kernels(fn) -> int:
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def time_eager(fn, steps, warmup) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def time_graph(fn, steps, warmup) -> float:
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with bench.single_stream():
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    from mmfusion import arena as arena_mod
    from mmfusion.train import DistillTrainStep, FusedAdamW, backward_from, fusion_loss
    from models.multimodal_model import KnowledgeDistillationModel, MultimodalEmotionModel
    torch.manual_seed(0)
    kd = KnowledgeDistillationModel(MultimodalEmotionModel(_cfg(512, 8, 512)), _cfg(256, 4, 256)).cuda().train()
    ti, au, vi, labels = _inputs(args.batch)
    res = {"pair": "teacher 512/8/G512, student 256/4/G256, hierarchical, feature inputs", "B": args.batch}

    # student alone: a second student of the same shape, its own arena and optimiser
    torch.manual_seed(1)
    solo = MultimodalEmotionModel(_cfg(256, 4, 256)).cuda().train()
    ar = arena_mod.ensure(solo)
    opt = FusedAdamW(ar, lr=1e-4, weight_decay=1e-5, max_grad_norm=1.0)
    opt.set_schedule(1e-4, 1000)

    def solo_step():
        ar.zero_grad(overlap=True, lazy=True)
        out = solo(ti, au, vi, compute_contrastive_loss=True)
        loss = fusion_loss(out, labels)
        backward_from(loss)
        ar.finalize_grads()
        opt.advance()
        opt.launch()
        return loss

    ts = DistillTrainStep(kd, lr=1e-4, weight_decay=1e-5, max_grad_norm=1.0, total_steps=1000)

    def kd_step():
        return ts(ti, au, vi, labels)

    for name, fn in (("student_alone", solo_step), ("distill", kd_step)):
        res[f"{name}_eager_ms"] = round(time_eager(fn, args.steps, args.warmup), 4)
        res[f"{name}_launches_eager"] = count_kernels(fn)
        res[f"{name}_graph_ms"] = round(time_graph(fn, args.steps, args.warmup), 4)

    # the loss tail on (B, 7) logits: fused vs torch
    from mmfusion import small_ops
    T = kd.temperature
    s = torch.randn(args.batch, 7, device="cuda", requires_grad=True)
    t = torch.randn(args.batch, 7, device="cuda")
    cl = [torch.rand((), device="cuda", requires_grad=True) for _ in range(3)]

    def fused_tail():
        loss = small_ops.fusion_loss_kd(s, labels, 0.1, cl, [0.1] * 3, t, T, 0.5)
        torch.autograd.grad([loss], [s, *cl], [small_ops.loss_seed(s.device)])     # (no accumulation into leaf .grad)

    def torch_ce():
        loss = F.cross_entropy(s, labels, label_smoothing=0.1) + 0.1 * sum(cl)
        torch.autograd.grad([loss], [s, *cl])

    def torch_ce_kd():
        loss = F.cross_entropy(s, labels, label_smoothing=0.1) + 0.1 * sum(cl)
        loss = loss + 0.5 * (F.kl_div(F.log_softmax(s / T, dim=-1), F.softmax(t / T, dim=-1), reduction="batchmean") * T ** 2)
        torch.autograd.grad([loss], [s, *cl])

    for fn in (fused_tail, torch_ce, torch_ce_kd):
        fn()                                     # first-use allocations outside the count
    res["loss_tail_launches_fused"] = count_kernels(fused_tail)
    res["loss_tail_launches_torch_ce"] = count_kernels(torch_ce)
    res["loss_tail_launches_torch_ce_kd"] = count_kernels(torch_ce_kd)
    res["loss_tail_launches_torch_kd_part"] = res["loss_tail_launches_torch_ce_kd"] - res["loss_tail_launches_torch_ce"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
