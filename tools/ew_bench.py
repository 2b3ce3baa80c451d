#!/usr/bin/env python3
"""Streaming-kernel microbench: f32->bf16 cast of the MulT weight arena, LayerNorm fwd/bwd, add3, meanpool at the
MulT shapes, their grouped forms, the fan-out gradient sums and the bias-gradient column sums; prints achieved HBM GB/s of
algorithmic bytes."""
import ctypes as C, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simple-multimodal_amd"))
import torch
from mmfusion import lib, ops

def timeit(fn, reps=20, inner=5):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s): fn()
    torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner): fn()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * inner)

L = lib.load()
n = 51_400_000 // 64 * 64
src = torch.randn(n, device="cuda"); dst = torch.empty(n, device="cuda", dtype=torch.bfloat16)
us = timeit(lambda: lib.check(L.mmf_cast_f32_to_bf16(src.data_ptr(), dst.data_ptr(), n, lib.stream_ptr())))
print(f"cast f32->bf16 {n/1e6:.1f} M elements: {us:7.1f} us  {6.0*n/us/1e3:7.0f} GB/s")
us = timeit(lambda: lib.check(L.mmf_cast_bf16_to_f32(dst.data_ptr(), src.data_ptr(), n, lib.stream_ptr())))
print(f"cast bf16->f32 {n/1e6:.1f} M elements: {us:7.1f} us  {6.0*n/us/1e3:7.0f} GB/s")
d = 768
rows = [8192, 8192, 6400, 6400, 480, 480]
xs = [torch.randn(r, d, device="cuda").bfloat16().requires_grad_(True) for r in rows]
gs = [torch.nn.Parameter(torch.ones(d, device="cuda")) for _ in rows]; bs = [torch.nn.Parameter(torch.zeros(d, device="cuda")) for _ in rows]
for p in gs + bs: p.grad = torch.zeros_like(p)
nb = sum(rows) * d * 2
us = timeit(lambda: ops.layernorm_group([(x.detach(), g, b) for x, g, b in zip(xs, gs, bs)]))
print(f"layernorm fwd x6 ({sum(rows)} rows): {us:7.1f} us  {2.0*nb/us/1e3:7.0f} GB/s")
ys = ops.layernorm_group([(x, g, b) for x, g, b in zip(xs, gs, bs)])
dys = [torch.randn_like(y) for y in ys]
torch.autograd.backward(ys, dys, retain_graph=True, inputs=xs)       # eager (the backward allocates its workspace)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20): torch.autograd.backward(ys, dys, retain_graph=True, inputs=xs)
e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 1e3 / 20
print(f"layernorm bwd x6 (eager, incl. launch gaps): {us:7.1f} us  {3.0*nb/us/1e3:7.0f} GB/s")
a3 = [torch.randn(8192, d, device="cuda").bfloat16() for _ in range(3)]
us = timeit(lambda: ops.add3(*a3))
print(f"add3 8192x768: {us:7.1f} us  {4.0*8192*d*2/us/1e3:7.0f} GB/s")
mp = [torch.randn(16, t, d, device="cuda").bfloat16() for t in (512, 400, 30)]
us = timeit(lambda: ops.meanpool_cat(mp))
print(f"meanpool_cat 16x(512,400,30)x768: {us:7.1f} us  {sum(m.numel() for m in mp)*2/us/1e3:7.0f} GB/s")
trip = [tuple(torch.randn(r, d, device="cuda").bfloat16() for _ in range(3)) for r in (8192, 6400, 480)]
us = timeit(lambda: ops.add3_group(trip))
print(f"add3_group 8192/6400/480 x768: {us:7.1f} us  {4.0*15072*d*2/us/1e3:7.0f} GB/s")
NG = 7                                                     # gradients per MulT input tensor (ops.fanout_group's backward)
gr = [[torch.randn(r, d, device="cuda").bfloat16() for _ in range(NG)] for r in (8192, 6400, 480)]
go = [torch.empty_like(g[0]) for g in gr]
pr = (lib.AddNProblem * 3)()
for q, g, o in zip(pr, gr, go):
    for k, t in enumerate(g): q.x[k] = t.data_ptr()
    q.y, q.numel, q.n = o.data_ptr(), o.numel(), NG
us = timeit(lambda: lib.check(L.mmf_addn_grouped(pr, 3, lib.stream_ptr())))
print(f"fanout_group bwd (addn_grouped) {NG} x 8192/6400/480 x768: {us:7.1f} us  {(NG+1.0)*15072*d*2/us/1e3:7.0f} GB/s")
p1 = (C.c_void_p * NG)(*[t.data_ptr() for t in gr[0]])
us = timeit(lambda: lib.check(L.mmf_addn_bf16(p1, NG, go[0].data_ptr(), go[0].numel(), 0, lib.stream_ptr())))
print(f"fanout bwd (addn) {NG} x 8192x768: {us:7.1f} us  {(NG+1.0)*8192*d*2/us/1e3:7.0f} GB/s")
cx = [torch.randn(m, n, device="cuda").bfloat16() for m, n in ((8192, 2304), (6400, 768), (480, 768))]
co = [torch.zeros(x.shape[1], device="cuda") for x in cx]
cp = [lib.ColsumProblem(x.data_ptr(), o.data_ptr(), x.shape[0], x.shape[1], x.shape[1]) for x, o in zip(cx, co)]
us = timeit(lambda: lib.colsum_grouped(cp))
print(f"colsum 8192x2304 + 6400x768 + 480x768: {us:7.1f} us  {sum(x.numel() for x in cx)*2/us/1e3:7.0f} GB/s")
dyp = torch.randn(16, 3 * d, device="cuda").bfloat16()
dxp = [torch.empty_like(m) for m in mp]
pp, tp = (C.c_void_p * 3)(*[t.data_ptr() for t in dxp]), (C.c_int * 3)(512, 400, 30)
us = timeit(lambda: lib.check(L.mmf_meanpool_cat_bwd(dyp.data_ptr(), pp, tp, 3, 16, d, 3 * d, lib.stream_ptr())))
print(f"meanpool_cat bwd 16x(512,400,30)x768: {us:7.1f} us  {sum(m.numel() for m in mp)*2/us/1e3:7.0f} GB/s")
y1 = torch.empty(16, d, device="cuda", dtype=torch.bfloat16)
us = timeit(lambda: lib.check(L.mmf_meanpool_fwd(mp[0].data_ptr(), y1.data_ptr(), 16, 512, d, d, lib.stream_ptr())))
print(f"meanpool fwd 16x512x768: {us:7.1f} us  {mp[0].numel()*2/us/1e3:7.0f} GB/s")
us = timeit(lambda: lib.check(L.mmf_meanpool_bwd(y1.data_ptr(), dxp[0].data_ptr(), 16, 512, d, d, lib.stream_ptr())))
print(f"meanpool bwd 16x512x768: {us:7.1f} us  {mp[0].numel()*2/us/1e3:7.0f} GB/s")
