"""What tools/vit_bench.py and tools/w2v_bench.py share: the event-timed loop and the per-kernel table read from
mmfusion.lib.PROFILE.  Imported by those two (which set up ``sys.path``); not a command of its own."""
import torch


def time_eager(fn, steps, warmup) -> float:
    """ms per call of ``fn`` over ``steps`` calls after ``warmup`` untimed ones, from HIP events"""
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


def kernel_table(fn, bytes_of=None) -> list:
    """One call of ``fn`` (after a warm-up call) as rows per kernel, slowest first: calls, ms, share, TFLOP/s where the
    wrapper counts operations.  ``bytes_of(label, detail)``: the HBM bytes a launch has to move; when given, the rows also
    carry ``tb_per_s``."""
    from mmfusion import lib
    fn()
    torch.cuda.synchronize()
    lib.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        recs = lib.PROFILE
    finally:
        lib.PROFILE = None
    agg = {}
    for label, flops, e0, e1, detail in recs:
        key = label
        if label.startswith("gemm") and detail:
            key = f"{label} N={detail[0][1]} K={detail[0][2]}" + (" (+1)" if len(detail) > 1 else "")
        row = agg.setdefault(key, {"kernel": key, "calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
        row["calls"] += 1
        row["ms"] += e0.elapsed_time(e1)
        row["flops"] += flops
        row["bytes"] += bytes_of(label, detail) if bytes_of and detail else 0.0
    total = sum(r["ms"] for r in agg.values())
    rows = sorted(agg.values(), key=lambda r: -r["ms"])
    for r in rows:
        flops, nbytes = r.pop("flops"), r.pop("bytes")
        r["share"] = round(r["ms"] / total, 4)
        r["tflops"] = round(flops / r["ms"] / 1e9, 1) if flops else None
        if bytes_of:
            r["tb_per_s"] = round(nbytes / r["ms"] / 1e9, 2) if nbytes else None
        r["ms"] = round(r["ms"], 4)
    return rows
