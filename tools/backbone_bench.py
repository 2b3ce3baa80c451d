"""What tools/vit_bench.py, tools/w2v_bench.py and tools/deberta_bench.py share: the import path, the common arguments, the
event-timed loop, the chunk sweep and the per-kernel table read from mmfusion.lib.PROFILE.  Imported by those three ahead of
anything of the project's; not a command of its own."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "simple-multimodal_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
os.environ.setdefault("MMFUSION_CONFIG_MKDIRS", "0")
import torch  # noqa: E402


def parser(steps: int, warmup: int, torch_yardstick: bool = False) -> argparse.ArgumentParser:
    """--chunks --steps --warmup --table (and --no-torch where the script has a stock-torch yardstick); the script adds its inputs' sizes"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="")
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--table", action="store_true")
    if torch_yardstick:
        ap.add_argument("--no-torch", action="store_true")
    return ap


def sweep(model, default_chunk: int, chunks: str, measure) -> None:
    """``measure(c)`` with ``model.chunk = c`` and a fresh workspace for every ``c`` of the comma-separated ``chunks`` (none: the
    default alone); leaves the model at its default chunk without a workspace"""
    for c in [int(v) for v in chunks.split(",") if v] or [default_chunk]:
        model.chunk, model._ws = c, None
        measure(c)
    model.chunk, model._ws = default_chunk, None


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


def print_table(rows: list) -> None:
    """``kernel_table``'s rows as text (the TB/s column where the rows carry it)"""
    tb = bool(rows) and "tb_per_s" in rows[0]
    show = lambda v, w: f"{v if v is not None else '':>{w}}"
    print(f"{'kernel':58s} {'calls':>5s} {'ms':>9s} {'share':>7s} {'TFLOP/s':>8s}" + (f" {'TB/s':>6s}" if tb else ""))
    for r in rows:
        print(f"{r['kernel']:58s} {r['calls']:5d} {r['ms']:9.4f} {r['share']:7.2%} {show(r['tflops'], 8)}" + (f" {show(r['tb_per_s'], 6)}" if tb else ""))
