"""Autograd wrappers around the HIP kernels of ``libmmfusion.so``.

Data layout: activations are bf16, row-major 2-D ``(rows, features)`` with
``rows = B*T``; parameters are fp32 masters living in a flat arena (``mmfusion.arena``) with a
bf16 shadow copy used by the MFMA kernels; weight/bias/LayerNorm gradients are accumulated by
the kernels **directly into ``param.grad``** (an fp32 view of the flat gradient arena, the buffer
RCCL all-reduces), so the Functions return ``None`` for parameters.

Every op is *grouped*: it takes a list of independent problems and issues one launch for all of
them (the six cross-modal blocks of MulT, reference models/fusion_layers.py:146-153, are mutually
independent), which is what fills 256 CUs with these small per-block shapes.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from itertools import accumulate
from typing import List, Optional, Sequence, Tuple

import torch

from . import lib
from .lib import (AttnProblem, GemmProblem, LnProblem, EPI_ACCUM, EPI_ADD_AUX, EPI_BIAS, EPI_COLSUM_A,
                  EPI_DROPOUT, EPI_MASK_AUX, EPI_MASK_BITS, EPI_RELU, EPI_RELU_BITS, GEMM_NN, GEMM_NT, GEMM_TN)

BF16 = torch.bfloat16

# --------------------------------------------------------------------------------------------
# precision mode of the running root forward: "bf16" (default: bf16 storage, bf16 MFMA, f32 accumulate) or "fp32"
# (parity mode: f32 storage, exact f32 MFMA — mmfusion.ops_f32).  Set by models.fusion_layers._FusionBase for the
# duration of a root module's forward; the autograd Functions are separate per mode, so backward needs no flag.
# --------------------------------------------------------------------------------------------
_PRECISION = "bf16"


def set_precision(mode: str) -> str:
    global _PRECISION
    if mode not in ("bf16", "fp32"):
        raise ValueError(f"precision must be 'bf16' or 'fp32', got {mode!r}")
    old, _PRECISION = _PRECISION, mode
    return old


def fp32_mode() -> bool:
    return _PRECISION == "fp32"


def _f32():
    from . import ops_f32
    return ops_f32


# --------------------------------------------------------------------------------------------
# parameter references
# --------------------------------------------------------------------------------------------
@dataclass
class W:
    """Rows [r0, r1) of a (out, in) weight parameter: fp32 master + bf16 shadow."""
    p: torch.nn.Parameter
    r0: int = 0
    r1: Optional[int] = None

    def rows(self) -> Tuple[int, int]:
        return self.r0, (self.p.shape[0] if self.r1 is None else self.r1)

    @property
    def w16(self) -> torch.Tensor:
        return shadow(self.p)[self.rows()[0]:self.rows()[1]]

    @property
    def grad(self) -> torch.Tensor:
        g = self.p.grad
        if g is None or g.dtype != torch.float32 or not g.is_contiguous():
            raise RuntimeError("parameter has no fp32 arena gradient: call mmfusion.arena.ensure(module)")
        a, b = self.rows()
        return g[a:b]

    @property
    def master(self) -> torch.Tensor:
        a, b = self.rows()
        return self.p.detach()[a:b]


def shadow(p: torch.nn.Parameter) -> torch.Tensor:
    """bf16 shadow of an arena-managed parameter.  Parameters outside the arena's early block are cast
    on a side stream: reading one first joins that stream (mmfusion.arena.ParamArena.join)."""
    s = getattr(p, "_mmf_bf16", None)
    if s is None:
        raise RuntimeError("parameter is not arena-managed: call mmfusion.arena.ensure(module) first")
    if _PRECISION == "fp32":
        return p.detach()
    if p._mmf_late:
        p._mmf_arena.join()
    return s


def _ld(t: torch.Tensor) -> int:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"expected a 2-D row-major (possibly row-strided) tensor, got {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0)


def _req(t: torch.Tensor, dtype) -> None:
    if not t.is_cuda:
        raise RuntimeError("mmfusion ops run on the GPU only (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _column_views(t: Optional[torch.Tensor], widths: Sequence[int]) -> list:
    """t's adjacent column blocks of the given widths, from column 0 (a None per block for t = None)"""
    offs = [0, *accumulate(widths)]
    return [None if t is None else t[:, a:b] for a, b in zip(offs, offs[1:])]


def _column_blocks(ts: Sequence[torch.Tensor]) -> Optional[torch.Tensor]:
    """The contiguous 2-D tensor that ``ts`` are views of and whose columns they tile — in order, from its first
    element, without gap, overlap or rest (what ``_column_views`` returns); None for anything else.  Metadata only."""
    base = ts[0]._base if len(ts) else None
    if base is None or base.dim() != 2 or not base.is_contiguous():
        return None
    rows, width = base.shape
    off = 0
    for t in ts:
        if (t._base is not base or t.dtype != base.dtype or t.dim() != 2 or t.shape[0] != rows
                or t.stride() != (width, 1) or t.data_ptr() != base.data_ptr() + base.element_size() * off):
            return None
        off += t.shape[1]
    return base if off == width else None


# --------------------------------------------------------------------------------------------
# raw (non-autograd) helpers
# --------------------------------------------------------------------------------------------
def cast_to_bf16(x: torch.Tensor) -> torch.Tensor:
    _req(x, torch.float32)
    if (x.dim() == 2 and not x.is_contiguous() and x.stride(1) == 1 and x.shape[1] % 4 == 0 and x.stride(0) % 4 == 0
            and x.data_ptr() % 16 == 0):
        # a column block of a wider tensor (what autograd returns for a torch.cat input): cast it where it lies
        y = torch.empty(x.shape, dtype=BF16, device=x.device)
        lib.check(lib.load().mmf_cast_f32_to_bf16_2d(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], x.stride(0),
                                                     lib.stream_ptr()))
        return y
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=BF16, device=x.device)
    lib.check(lib.load().mmf_cast_f32_to_bf16(x.data_ptr(), y.data_ptr(), x.numel(), lib.stream_ptr()))
    return y


def cast_to_f32(x: torch.Tensor) -> torch.Tensor:
    _req(x, BF16)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    lib.check(lib.load().mmf_cast_bf16_to_f32(x.data_ptr(), y.data_ptr(), x.numel(), lib.stream_ptr()))
    return y


def _grad_bf16(g: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A bf16 or f32 gradient as contiguous bf16 (None stays None).  The cast comes first: it takes a row-strided f32
    column block where it lies, in one launch, where ``.contiguous()`` ahead of it would add a copy."""
    if g is None:
        return None
    return g.contiguous() if g.dtype == BF16 else cast_to_bf16(g)


def _gemm_problems(layout: int, probs: Sequence[tuple], epilogue: int, dtype, c_dtype) -> List[GemmProblem]:
    """One GemmProblem per (A, B, C, bias|None, aux|None): M, N from C, K from A.  A and B must be ``dtype``, every C
    ``c_dtype``; the bias is f32, contiguous, [N] ([M] for the fused bias gradient); aux has C's shape — or, with
    EPI_RELU_BITS / EPI_MASK_BITS, is the problem's bit buffer (``relu_bits_buffer``)."""
    ps: List[GemmProblem] = []
    bits = bool(epilogue & (EPI_RELU_BITS | EPI_MASK_BITS))
    for (A, Bm, Cm, bias, aux) in probs:
        _req(A, dtype), _req(Bm, dtype)
        M, N = Cm.shape
        K = A.shape[0] if layout == GEMM_TN else A.shape[1]
        a_shape, b_shape = (K, M) if layout == GEMM_TN else (M, K), (N, K) if layout == GEMM_NT else (K, N)
        if A.shape != a_shape or Bm.shape != b_shape or Cm.dtype != c_dtype:
            raise ValueError(f"gemm layout {layout}: A{tuple(A.shape)} B{tuple(Bm.shape)} C{tuple(Cm.shape)} {Cm.dtype}")
        if bits:
            if aux is None or aux.dtype != torch.uint8 or not aux.is_contiguous() or aux.numel() < lib.load().mmf_gemm_relu_bits_bytes(M, N):
                raise ValueError("the bit forms take a contiguous uint8 buffer of mmf_gemm_relu_bits_bytes(M, N) bytes as aux")
        elif aux is not None and tuple(aux.shape) != (M, N):
            raise ValueError("aux must match C")
        if bias is not None:
            _req(bias, torch.float32)
            if bias.numel() != (M if epilogue & EPI_COLSUM_A else N) or not bias.is_contiguous():
                raise ValueError("bias must be contiguous [N] ([M] for the fused bias gradient)")
        ps.append(GemmProblem(A.data_ptr(), Bm.data_ptr(), Cm.data_ptr(), _ptr(bias), _ptr(aux), M, N, K,
                              _ld(A), _ld(Bm), _ld(Cm), _ld(aux) if aux is not None and not bits else 0))
    return ps


def relu_bits_buffer(h: torch.Tensor) -> torch.Tensor:
    """The buffer of the keep-mask bits of an activation tensor of h's shape (layout: include/mmfusion.h, MMF_EPI_RELU_BITS)."""
    return torch.empty(lib.load().mmf_gemm_relu_bits_bytes(*h.shape), dtype=torch.uint8, device=h.device)


def relu_bits_available(layout: int, probs: Sequence[tuple], epilogue: int, alpha: float = 1.0,
                        dropout: Optional[tuple] = None) -> bool:
    """Whether ``gemm_group`` with these arguments, the epilogue holding EPI_RELU_BITS or EPI_MASK_BITS, is a launch the
    library has the bit form for (one launch on the persistent kernel); the caller decides per launch and keeps
    EPI_MASK_AUX on the activation tensor where it is not."""
    if len(probs) > lib.GEMM_MAX_PROBLEMS or probs[0][2].dtype != BF16:
        return False
    ps = _gemm_problems(layout, probs, epilogue, BF16, BF16)
    if dropout is not None:
        return lib.gemm_relu_bits_available(ps, layout, epilogue | EPI_DROPOUT, alpha, dropout[0], rng_state().data_ptr(), dropout[1])
    return lib.gemm_relu_bits_available(ps, layout, epilogue, alpha)


def gemm(layout: int, A: torch.Tensor, Bm: torch.Tensor, C: torch.Tensor, *, bias=None, aux=None,
         epilogue: int = 0) -> None:
    """Single-problem convenience over gemm_group (shapes are taken from C and the layout)."""
    gemm_group(layout, [(A, Bm, C, bias, aux)], epilogue)


def gemm_group(layout: int, probs: Sequence[tuple], epilogue: int, alpha: float = 1.0,
               dropout: Optional[tuple] = None) -> None:
    """probs: (A, B, C, bias|None, aux|None) tensors; M,N from C; K from A.
    alpha scales the result after the mask step; dropout = (p, site) adds MMF_EPI_DROPOUT."""
    out_f32 = probs[0][2].dtype == torch.float32
    ps = _gemm_problems(layout, probs, epilogue, BF16, torch.float32 if out_f32 else BF16)
    if dropout is not None:
        if len(ps) > lib.GEMM_MAX_PROBLEMS:
            raise ValueError("a dropout GEMM group must fit one launch (the problem index keys the mask)")
        lib.gemm_grouped(ps, layout, epilogue | EPI_DROPOUT, out_f32, alpha, dropout[0],
                         rng_state().data_ptr(), dropout[1])
        return
    for i in range(0, len(ps), lib.GEMM_MAX_PROBLEMS):
        lib.gemm_grouped(ps[i:i + lib.GEMM_MAX_PROBLEMS], layout, epilogue, out_f32, alpha)


def _gemm_chains(chains: Sequence[tuple]) -> List[lib.GemmChain]:
    """One lib.GemmChain per (C, bias|None, aux|None, [(A_0, B_0), (A_1, B_1), ...]) of bf16 row matrices (NN: A_s is
    (M, K_s), B_s is (K_s, N)): C = sum_s A_s B_s in one accumulator chain."""
    cs: List[lib.GemmChain] = []
    for (Cm, bias, aux, segs) in chains:
        _req(Cm, BF16)
        M, N = Cm.shape
        if not 0 < len(segs) <= lib.GEMM_CHAIN_MAX_SEGMENTS:
            raise ValueError(f"a chain has 1..{lib.GEMM_CHAIN_MAX_SEGMENTS} segments, got {len(segs)}")
        if aux is not None and (aux.dtype != BF16 or tuple(aux.shape) != (M, N)):
            raise ValueError("aux must match C")
        if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous()):
            raise ValueError("bias must be contiguous f32 [N]")
        c = lib.GemmChain()
        c.C, c.bias, c.aux, c.M, c.N, c.ldc, c.num_segments = Cm.data_ptr(), _ptr(bias), _ptr(aux), M, N, _ld(Cm), len(segs)
        c.ldaux = _ld(aux) if aux is not None else 0
        for k, (A, Bm) in enumerate(segs):
            _req(A, BF16), _req(Bm, BF16)
            if A.dim() != 2 or Bm.dim() != 2 or A.shape[0] != M or Bm.shape != (A.shape[1], N):
                raise ValueError(f"chain segment {k}: A{tuple(A.shape)} B{tuple(Bm.shape)} C{tuple(Cm.shape)}")
            c.seg[k].A, c.seg[k].B, c.seg[k].K, c.seg[k].lda, c.seg[k].ldb = A.data_ptr(), Bm.data_ptr(), A.shape[1], _ld(A), _ld(Bm)
        cs.append(c)
    return cs


def gemm_chain_available(chains: Sequence[tuple], epilogue: int) -> bool:
    """whether ``gemm_chain_group`` has its launch for these chains (``lib.gemm_chain_available``); host only"""
    return lib.gemm_chain_available(_gemm_chains(chains), GEMM_NN, epilogue)


def gemm_chain_group(chains: Sequence[tuple], epilogue: int) -> None:
    """chains: (C, bias|None, aux|None, [(A_s, B_s), ...]); C = sum_s A_s B_s (+ bias | + aux) for every chain in ONE launch,
    each output tile accumulated over its chain's segments and stored once (``mmf_gemm_grouped_chain``: NN, bf16)."""
    lib.gemm_grouped_chain(_gemm_chains(chains), GEMM_NN, epilogue)


# --------------------------------------------------------------------------------------------
# dropout: device-resident RNG state + per-call-site ids
# --------------------------------------------------------------------------------------------
# Masks are a stateless hash of (state, site, element).  `state` is ONE int64 on the device: the root
# forward of a training step adds 1 to it with a (graph-capturable) kernel, so every step — also every
# replay of a captured step — draws new masks, and the backward pass regenerates the forward's masks
# from the same (state, site).  `site` numbers the dropout call sites of one forward in call order.
_rng_state: Optional[torch.Tensor] = None
_site = 0


def rng_state() -> torch.Tensor:
    global _rng_state
    if _rng_state is None:
        _rng_state = torch.full((1,), (torch.initial_seed() & 0x7FFFFFFF) << 20, dtype=torch.int64, device="cuda")
    return _rng_state


def seed_dropout(seed: int) -> None:
    rng_state().fill_((seed & 0x7FFFFFFF) << 20)


def begin_training_forward() -> None:
    """Called once per root forward in training mode: new masks, site numbering restarts."""
    global _site
    _site = 0
    rng_state().add_(1)


def next_site() -> int:
    global _site
    _site += 1
    return _site


_roots = 0


def root_entered() -> None:
    """A root module's forward (``models.fusion_layers._FusionBase``) is running: it has called ``begin_training_forward`` where
    it trains, and what runs inside takes its sites from that numbering"""
    global _roots
    _roots += 1


def root_left() -> None:
    global _roots
    _roots -= 1


def inside_root() -> bool:
    """False for a module called on its own: with dropout on, it must call ``begin_training_forward`` itself"""
    return _roots > 0


class dropout_state:
    """Within: dropout masks come from ``state`` (a device int64 [1]) with a site numbering of their own, and the outer
    state tensor and site counter are untouched — ``begin_training_forward`` advances ``state``, not the outer one.  For a
    second root module run between another root's forward and its backward (the distillation teacher): the outer root's
    backward regenerates its masks from the live outer state, which must not have moved.  The swap is host-side and names
    another device tensor, so it holds under graph capture too."""

    def __init__(self, state: torch.Tensor):
        self.state = state

    def __enter__(self):
        global _rng_state, _site
        self.saved = (rng_state(), _site)
        _rng_state, _site = self.state, 0
        return self.state

    def __exit__(self, *exc):
        global _rng_state, _site
        _rng_state, _site = self.saved


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, site):
        x = x.contiguous()
        y = torch.empty_like(x)
        lib.check(lib.load().mmf_dropout(x.data_ptr(), y.data_ptr(), x.numel(), int(x.dtype == torch.float32), p,
                                         rng_state().data_ptr(), site, lib.stream_ptr()))
        ctx.p, ctx.site = p, site
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        dx = torch.empty_like(g)
        lib.check(lib.load().mmf_dropout(g.data_ptr(), dx.data_ptr(), g.numel(), int(g.dtype == torch.float32), ctx.p,
                                         rng_state().data_ptr(), ctx.site, lib.stream_ptr()))
        return dx, None, None


def dropout(x: torch.Tensor, p: float, training: bool) -> torch.Tensor:
    """nn.Dropout(p) on a bf16 or fp32 tensor (identity when not training or p == 0)."""
    if not training or p <= 0.0:
        return x
    if _PRECISION == "fp32":
        raise RuntimeError("the fp32 parity mode runs without dropout (use p = 0 or eval())")
    if x.dtype not in (BF16, torch.float32):
        raise TypeError("dropout expects bf16 or fp32")
    return _Dropout.apply(x, float(p), next_site())


# --------------------------------------------------------------------------------------------
# deferred weight gradients
# --------------------------------------------------------------------------------------------
# dW = dy^T x has a tiny output (768 x 768 ... 3072 x 768) and a long reduction (B*T rows): one
# block's wgrads are ~100 tiles, far fewer than 256 CUs.  Nothing downstream in the backward pass
# reads dW, so every Function only *queues* its wgrad problems and one autograd end-of-backward
# callback issues them all as grouped launches (>= 1000 tiles for MulT), bias gradients included.
#
# What the end-of-backward callback (_flush_wgrad) does with the queue is one of three modes:
#   automatic   issue everything on the current stream (what is left after the optional early launch, below);
#   manual      park it for the caller (set_manual_wgrad_flush: bench.py's overlapped data-parallel step);
#   round hook  hand it to a hook in rounds, the first ones during backward (set_wgrad_rounds: mmfusion.dp.BackwardExchange).
# Early flush (MMF_WGRAD_EARLY=1; measured +0.4 % and left OFF by default — with it the dominant kernel shares the chip with
# the input-gradient sums, so its duration in a profile of the timed steps no longer equals its stand-alone duration, which
# is what bench.py's roofline is built on): the number of weight-gradient problems a backward queues is the same every
# step, so when the count of the previous backward is reached the whole deferred launch is issued at once on its own
# stream instead of from the end-of-backward callback.  What the backward still has to do after its last Linear (the
# N-way input-gradient sums of the fan-outs: three HBM-bound kernels, 40 us + launch gaps at the MulT bench shapes)
# then runs beside the wgrad launch instead of in front of it.  A backward that queues more, or fewer, than the last one
# is still complete: whatever is pending when the callback runs is issued there, and the callback joins the stream.
# A weight with requires_grad = False (few-shot training freezes everything but the adapters, the prompt and the prototype
# network) queues nothing, its bias gradient included; the input gradient still flows through it.  Its arena gradient then
# stays as zero_grad left it (lazy zeroing: ParamArena.finalize_grads clears it).
_WGRAD_EARLY = os.environ.get("MMF_WGRAD_EARLY", "0") == "1"
_pending_wgrad: List[tuple] = []
_wgrad_stream: Optional[torch.cuda.Stream] = None


class _Backward:
    """Bookkeeping of the backward pass in progress.  The end-of-backward callback replaces it with a fresh one that carries
    over what this backward taught: how many problems it queued and which gradient regions it wrote more than once."""

    def __init__(self, expected: int = 0):
        self.expected = expected                  # problems the previous backward queued (0: unknown)
        self.multi_writer: set = set()            # gradient pointers the previous backward wrote twice (round hook only)
        self.callback_queued = False
        self.early = 0                            # problems issued by the early launch
        self.round_issued = 0                     # problems handed to the round hook before the end of backward
        self.rounds_cut = 0                       # rounds handed over so far
        self.round_ptrs: List[int] = []           # gradient pointers handed over in those rounds


_bw = _Backward()


_branch_streams: List[torch.cuda.Stream] = []


def branch_stream(i: int = 0) -> torch.cuda.Stream:
    """Extra stream i for work that runs beside the main chain (HierarchicalFusion's small branches, the concurrent
    half of MulT's cross blocks).  The deferred wgrad flush and anything else that consumes its results on the
    main stream joins every branch stream first (``join_branch_streams``)."""
    while len(_branch_streams) <= i:
        _branch_streams.append(torch.cuda.Stream())
    return _branch_streams[i]


def join_branch_streams() -> None:
    cur = torch.cuda.current_stream()
    for s in _branch_streams:
        cur.wait_stream(s)


def _wgrad_rounds(pend: List[tuple]) -> List[List[tuple]]:
    """Split queued problems into launch rounds such that no two problems of one round write overlapping gradient
    memory (a weight used twice in one forward, e.g. a shared ``nn.Linear``): the GEMM epilogue's accumulate is a
    plain read-add-write, so two writers of one region inside ONE grouped launch would race and drop updates.  The
    k-th writer of a region goes to round k; queue order is kept inside a region, so its first-touch overwrite
    (lazy zeroing) still runs before its accumulates."""
    rounds: List[List[tuple]] = []
    spans: List[Tuple[int, int, int]] = []               # (start, end, round) of every destination placed so far
    def span(t: torch.Tensor) -> Tuple[int, int]:
        # bytes the kernel may touch: for a row-strided view (a column block of a packed weight) the last row ends at
        # (rows - 1) * ld + cols, not at numel
        if t.dim() == 2:
            return t.data_ptr(), t.data_ptr() + 4 * ((t.shape[0] - 1) * t.stride(0) + t.shape[1])
        return t.data_ptr(), t.data_ptr() + 4 * t.numel()

    for q in pend:
        mine = [span(q[2])]
        if q[3] is not None:
            mine.append(span(q[3]))
        r = 0
        for a, b in mine:
            for s0, e0, r0 in spans:
                if a < e0 and s0 < b:
                    r = max(r, r0 + 1)
        for a, b in mine:
            spans.append((a, b, r))
        while len(rounds) <= r:
            rounds.append([])
        rounds[r].append(q)
    return rounds


def _issue_wgrad(pend: List[tuple]) -> None:
    for rnd in _wgrad_rounds(pend):
        # (has bias, overwrite) -> problems; overwrite = first wgrad of a lazily-zeroed step (arena.zero_grad(lazy=True))
        groups: dict = {}
        for q in rnd:
            groups.setdefault((q[3] is not None, q[5]), []).append(q[:5])
        # longest tiles first (a tile's duration goes with K = the rows of dy), big outputs first among equals: the
        # kernel hands tiles to the CUs in this order, so the tail of the launch is made of the short tiles.
        # Overwrite groups before accumulate groups.
        for (has_bias, overwrite), group in sorted(groups.items(), key=lambda kv: (not kv[0][1], not kv[0][0])):
            group.sort(key=lambda t: (-t[0].shape[0], -(t[2].shape[0] * t[2].shape[1])))
            gemm_group(GEMM_TN, group, (0 if overwrite else EPI_ACCUM) | (EPI_COLSUM_A if has_bias else 0))


def issue_wgrad(pend: List[tuple], side: bool = False) -> None:
    """Issue queued wgrad problems now, as grouped launches (as the automatic flush does): on the current stream, or with
    ``side`` on the wgrad stream (``wgrad_stream()``) behind the current stream and every branch stream."""
    global _wgrad_stream
    if not pend:
        return
    if not side:
        _issue_wgrad(pend)
        return
    if _wgrad_stream is None:
        _wgrad_stream = torch.cuda.Stream()
    cur = torch.cuda.current_stream()
    _wgrad_stream.wait_stream(cur)                       # the queued dy / x are complete on the main stream
    for st in _branch_streams:                           # ... and on the branch streams other backward nodes ran on
        if st != cur:
            _wgrad_stream.wait_stream(st)
    with torch.cuda.stream(_wgrad_stream):
        _issue_wgrad(pend)
    for q in pend:                                       # keep the operands' memory until the side kernels ran
        q[0].record_stream(_wgrad_stream)
        q[1].record_stream(_wgrad_stream)


def wgrad_stream() -> Optional[torch.cuda.Stream]:
    """The stream ``issue_wgrad(..., side=True)`` launches on; None until the first such launch."""
    return _wgrad_stream


# Manual flush (data-parallel overlap, bench.py / mmfusion.dp): the end-of-backward callback only parks the queued
# problems; the caller takes them (take_pending_wgrad), splits them by gradient-arena offset (split_wgrad_by_offset)
# and issues the parts itself (issue_wgrad) with the all-reduce of a finished arena range started in between.
_MANUAL_FLUSH = False
_parked_wgrad: List[tuple] = []


def set_manual_wgrad_flush(on: bool) -> None:
    global _MANUAL_FLUSH
    _MANUAL_FLUSH = bool(on)


def take_pending_wgrad() -> List[tuple]:
    """The problems the last backward parked (manual flush mode), in queue order; the list is handed over."""
    global _parked_wgrad
    pend, _parked_wgrad = _parked_wgrad, []
    return pend


def wgrad_offset(q: tuple) -> int:
    """Element offset of a queued problem's weight gradient inside its gradient arena."""
    from .arena import arena_of
    ar = arena_of(q[2])
    if ar is None:
        raise ValueError("queued weight gradient does not live in a gradient arena")
    return (q[2].data_ptr() - ar.grads.data_ptr()) // 4


def split_wgrad_by_offset(pend: List[tuple], nparts: int = 2) -> Tuple[List[List[tuple]], List[int]]:
    """Partition queued problems into `nparts` consecutive gradient-arena ranges of about equal GEMM work
    (sum of M N K).  Returns (parts, bounds): part i holds every problem whose gradient starts in
    [bounds[i], bounds[i+1]); bounds[0] = 0 and the last bound is open (the caller's arena size).  Problems that write
    the same region fall in the same part, so the overwrite-then-accumulate order inside a part is kept."""
    items = sorted(((wgrad_offset(q), i, q) for i, q in enumerate(pend)), key=lambda t: (t[0], t[1]))
    work = [q[2].shape[0] * q[2].shape[1] * q[0].shape[0] for _, _, q in items]
    total, acc, cuts = float(sum(work)) or 1.0, 0.0, []
    for k in range(len(items)):
        if len(cuts) < nparts - 1 and k > 0 and items[k][0] != items[k - 1][0] and acc >= total * (len(cuts) + 1) / nparts:
            cuts.append(k)
        acc += work[k]
    edges = [0] + cuts + [len(items)]
    parts = [[q for _, _, q in items[edges[i]:edges[i + 1]]] for i in range(len(edges) - 1)]
    bounds = [0] + [items[c][0] for c in cuts]
    while len(parts) < nparts:                            # fewer distinct regions than parts: empty trailing parts
        parts.append([])
        bounds.append(bounds[-1] if not items else items[-1][0] + items[-1][2][2].numel())
    return parts, bounds


# Round flush (data-parallel exchange INSIDE backward, SURVEY 8e / VERDICT r2 item 5a): with a hook installed, the backward
# hands its queued weight-gradient problems over in `n` rounds in reverse-autograd order — round i as soon as i/n of the
# problems the PREVIOUS backward queued have been queued again — and whatever is left from the end-of-backward callback
# (final=True).  The hook issues a round's GEMMs and starts the all-reduce of the gradient regions they complete
# (mmfusion.dp.BackwardExchange), so the exchange of the early rounds runs beside the rest of backward.  A region with
# several writers in one backward (a weight used twice) only completes with its last writer: such problems are held back
# for the final round (the set is learned from the previous backward, like the count).  The first backward after
# installing the hook has nothing to learn from and delivers everything in the final round.
_ROUND_HOOK = None
_ROUND_N = 0


def set_wgrad_rounds(n: int, hook) -> None:
    """hook(problems, final) or None to remove.  Excludes the manual flush."""
    global _ROUND_HOOK, _ROUND_N
    if hook is not None and (_MANUAL_FLUSH or n < 1):
        raise RuntimeError("wgrad rounds need no manual flush and n >= 1")
    _ROUND_HOOK, _ROUND_N = hook, int(n)
    _bw.expected = 0


def _maybe_cut_round() -> None:
    """queue_wgrad: hand over a round when its share of the expected problems has been queued."""
    global _pending_wgrad
    if _ROUND_HOOK is None or not _bw.expected or _ROUND_N < 2:
        return
    done = _bw.round_issued + len(_pending_wgrad)
    k = _bw.rounds_cut + 1                                             # the round being filled, 1-based
    if k >= _ROUND_N or done * _ROUND_N < k * _bw.expected:
        return                                                         # (the last round is the end-of-backward callback's)
    _bw.rounds_cut = k
    ready = [q for q in _pending_wgrad if q[2].data_ptr() not in _bw.multi_writer]
    if not ready:
        return
    _pending_wgrad = [q for q in _pending_wgrad if q[2].data_ptr() in _bw.multi_writer]
    _bw.round_issued += len(ready)
    _bw.round_ptrs.extend(q[2].data_ptr() for q in ready)
    _ROUND_HOOK(ready, False)


def _flush_wgrad() -> None:
    """The end-of-backward callback: what is still queued goes to the flush mode in force."""
    global _bw, _pending_wgrad
    bw, pend, _pending_wgrad = _bw, _pending_wgrad, []
    _bw = _Backward(expected=bw.early + bw.round_issued + len(pend))    # what the next backward is expected to queue
    if _ROUND_HOOK is not None:
        seen: dict = {}
        for ptr in bw.round_ptrs + [q[2].data_ptr() for q in pend]:
            seen[ptr] = seen.get(ptr, 0) + 1
        _bw.multi_writer = {ptr for ptr, c in seen.items() if c > 1}
        _ROUND_HOOK(pend, True)
        return
    if _branch_streams:                                  # operands queued by backward nodes that ran on a branch stream
        cur = torch.cuda.current_stream()
        join_branch_streams()
        for q in pend:
            q[0].record_stream(cur)
            q[1].record_stream(cur)
    if _MANUAL_FLUSH:
        _parked_wgrad.extend(pend)
        return
    if bw.early:
        # gradients complete when backward returns — and BEFORE any left-over problem is issued here: a left-over may
        # accumulate into a region the early launch is still writing (a weight used twice)
        torch.cuda.current_stream().wait_stream(_wgrad_stream)
    issue_wgrad(pend)


def queue_wgrad(dy: torch.Tensor, x: torch.Tensor, wgrad: torch.Tensor, bgrad: Optional[torch.Tensor]) -> None:
    """wgrad (f32, [N_out, K_in]) += dy^T x ;  bgrad (f32 [N_out]) += column sums of dy.
    If the gradient lives in an arena that was zeroed lazily this step and nothing has written it yet, the
    GEMM overwrites instead (``ParamArena.take_first_touch``)."""
    global _pending_wgrad
    overwrite = False
    from .arena import arena_of
    ar = arena_of(wgrad)
    if ar is not None:
        overwrite = ar.take_first_touch(wgrad)
    if not _bw.callback_queued:
        torch.autograd.Variable._execution_engine.queue_callback(_flush_wgrad)
        _bw.callback_queued = True
    _pending_wgrad.append((dy, x, wgrad, bgrad, None, overwrite))
    _maybe_cut_round()
    if (_WGRAD_EARLY and not _MANUAL_FLUSH and _ROUND_HOOK is None and _bw.expected and not _bw.early
            and len(_pending_wgrad) == _bw.expected):
        pend, _pending_wgrad = _pending_wgrad, []
        _bw.early = len(pend)
        issue_wgrad(pend, side=True)


# --------------------------------------------------------------------------------------------
# dtype boundary
# --------------------------------------------------------------------------------------------
class _ToBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return cast_to_bf16(x)

    @staticmethod
    def backward(ctx, g):
        return cast_to_f32(g)


class _ToF32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return cast_to_f32(x)

    @staticmethod
    def backward(ctx, g):
        return cast_to_bf16(g)


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """To the activation dtype of the running mode: bf16 (f32 in the fp32 parity mode)."""
    if _PRECISION == "fp32":
        return x if x.dtype == torch.float32 else _ToF32.apply(x)
    return x if x.dtype == BF16 else _ToBF16.apply(x)


def to_f32(x: torch.Tensor) -> torch.Tensor:
    return x if x.dtype == torch.float32 else _ToF32.apply(x)


# --------------------------------------------------------------------------------------------
# grouped Linear:  y_i = act(x_i W_i^T + b_i) (+ residual_i)
# --------------------------------------------------------------------------------------------
@dataclass
class LinearSpec:
    w: W
    b: Optional[W] = None          # bias parameter rows [r0, r1) (1-D parameter)
    relu: bool = False


def _relu_mask(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dz (bf16) = g * (y > 0) for a ReLU output y; g and y may be f32 (an f32-output linear) — narrowed and masked
    by ONE kernel instead of cast, cast, mask (these are (B, d)-row tensors: a launch costs more than the work)."""
    g, y = g.contiguous(), y.contiguous()
    if g.shape != y.shape:
        raise ValueError("relu mask: gradient and saved output differ in shape")
    dz = torch.empty(g.shape, dtype=BF16, device=g.device)
    L, st = lib.load(), lib.stream_ptr()
    if g.dtype == BF16 and y.dtype == BF16:
        lib.check(L.mmf_relu_bwd_bf16(g.data_ptr(), y.data_ptr(), dz.data_ptr(), g.numel(), st))
    else:
        for t in (g, y):
            if t.dtype not in (BF16, torch.float32):
                raise TypeError("relu mask: bf16 or f32 tensors only")
        lib.check(L.mmf_relu_bwd_mixed(g.data_ptr(), int(g.dtype == torch.float32), y.data_ptr(),
                                       int(y.dtype == torch.float32), dz.data_ptr(), g.numel(), st))
    return dz


def _skinny(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, bias=None, aux=None) -> lib.SkinnyProblem:
    """y (M, K or N) from x (M rows) and w (N, K): forward y = x w^T with x (M, K), input gradient y = x w with x (M, N)."""
    return lib.SkinnyProblem(x.data_ptr(), w.data_ptr(), y.data_ptr(), _ptr(bias), _ptr(aux), x.shape[0], *w.shape,
                             _ld(x), _ld(w), _ld(y), _ld(aux) if aux is not None else 0)


def _flatten_items(items: Sequence[tuple], residual: bool = True) -> Tuple[list, list]:
    """linear_group's (x, spec, residual|None) items -> (specs, [x_0, res_0|None, w_0.p, b_0.p|None, x_1, ...]) as the
    Functions take them (without the residuals: three tensors per item)."""
    specs, tensors = [], []
    for x, spec, res in items:
        specs.append(spec)
        tensors += [x, *([res] if residual else []), spec.w.p, spec.b.p if spec.b is not None else None]
    return specs, tensors


def _one_epilogue(specs: Sequence[LinearSpec], ress: Sequence = ()) -> Tuple[bool, bool, bool]:
    """(relu, has bias, has residual) of a linear group, which are one launch's epilogue and so the same for every problem"""
    relu, has_bias, has_res = specs[0].relu, specs[0].b is not None, bool(ress) and ress[0] is not None
    if (any(s.relu != relu or (s.b is not None) != has_bias for s in specs)
            or any((r is not None) != has_res for r in ress)):
        raise ValueError("a linear group must share one epilogue")
    return relu, has_bias, has_res


def _linear_outputs(xs: Sequence[torch.Tensor], ws: Sequence[torch.Tensor], dtype, cat: bool) -> Tuple[Optional[torch.Tensor], list]:
    """(None, the (M_i, N_i) outputs of a linear group), or with ``cat`` (ONE (M, sum N_i) tensor, its column blocks as
    the outputs): torch.cat / torch.stack of the outputs without a copy, and one gradient coming back instead of n slices."""
    if not cat:
        return None, [torch.empty((x.shape[0], w.shape[0]), dtype=dtype, device=x.device) for x, w in zip(xs, ws)]
    if any(x.shape[0] != xs[0].shape[0] for x in xs):
        raise ValueError("a concatenated linear group needs equal row counts")
    widths = [w.shape[0] for w in ws]
    base = torch.empty((xs[0].shape[0], sum(widths)), dtype=dtype, device=xs[0].device)
    return base, _column_views(base, widths)


class _GroupedLinear(torch.autograd.Function):
    """tensors = [x_0, res_0|None, w_0.p, b_0.p|None, x_1, ...]; returns one output per spec, or with ``cat`` the one
    tensor that holds them side by side (``_linear_outputs``)."""

    @staticmethod
    def forward(ctx, specs: List[LinearSpec], out_f32: bool, cat: bool, *tensors):
        relu, has_bias, has_res = _one_epilogue(specs, tensors[1::4])
        xs, ress = tensors[0::4], tensors[1::4]
        # an f32 input (a module's f32 output fed on, e.g. MulT's pooled projections) is narrowed here and its
        # gradient written as f32 by the dgrad kernel: no bf16 -> f32 cast node in the backward chain
        f32_in = xs[0].dtype == torch.float32
        if any((x.dtype == torch.float32) != f32_in for x in xs):
            raise ValueError("a linear group's inputs must share one dtype")
        ws = [s.w.w16 for s in specs]
        if f32_in:
            xs = [cast_to_bf16(x.contiguous()) for x in xs]
        for x in xs:
            _req(x, BF16)
        base, outs = _linear_outputs(xs, ws, torch.float32 if out_f32 else BF16, cat)
        probs = [(x, w, y, s.b.master if has_bias else None, res) for x, w, y, s, res in zip(xs, ws, outs, specs, ress)]
        epi = (EPI_BIAS if has_bias else 0) | (EPI_RELU if relu else 0) | (EPI_ADD_AUX if has_res else 0)
        if not has_res and all(x.shape[0] <= lib.SKINNY_MAX_M and x.shape[1] % 8 == 0 for x in xs):
            # (B, d)-row problems: weight-streaming kernels instead of the 256-row tile
            lib.skinny_fwd([_skinny(x, w, y, b) for (x, w, y, b, _) in probs], epi, out_f32)
        else:
            gemm_group(GEMM_NT, probs, epi)
        ctx.specs, ctx.cat, ctx.f32_in, ctx.has_res = specs, cat, f32_in, has_res
        ctx.save_for_backward(*xs, *(([base] if cat else outs) if relu else []))
        ctx.x_needs = [x.requires_grad for x in tensors[0::4]]
        return base if cat else tuple(outs)

    @staticmethod
    def backward(ctx, *gys):
        specs = ctx.specs
        n = len(specs)
        relu, has_bias = specs[0].relu, specs[0].b is not None
        xs = ctx.saved_tensors[:n]
        ys = ctx.saved_tensors[n:] if relu else [None] * n
        ws = [s.w.w16 for s in specs]

        def narrow(g, y):                          # to bf16; behind a ReLU dz = dy * (y > 0) in the same kernel
            return _relu_mask(g, y) if relu and g is not None else _grad_bf16(g)
        if ctx.cat:                                # one gradient for the concatenated output: slice it, no copies
            dys = _column_views(narrow(gys[0], ys[0]), [w.shape[0] for w in ws])
        else:
            dys = [narrow(g, y) for g, y in zip(gys, ys)]
        grads: List[Optional[torch.Tensor]] = [None] * (4 * n)
        # inputs that are the adjacent column blocks of one contiguous tensor (small_ops.split3 of a pooled (B, 3d)
        # buffer) get their gradients as the same blocks of one buffer, so the split's backward has nothing to copy
        dxs = []
        if n > 1 and not ctx.f32_in and all(ctx.x_needs) and all(g is not None for g in dys):
            xbase = _column_blocks(xs)
            if xbase is not None:
                dxs = _column_views(torch.empty_like(xbase), [x.shape[1] for x in xs])
        dgrad = []
        for i, s in enumerate(specs):
            g = dys[i]
            if g is None:
                continue
            if ctx.x_needs[i]:
                dx = dxs[i] if dxs else torch.empty(xs[i].shape, dtype=torch.float32 if ctx.f32_in else BF16, device=g.device)
                dgrad.append((g, ws[i], dx, None, None))
                grads[4 * i] = dx
            # wgrad; the bias gradient (column sums of dy) rides along in the same kernel (none for a frozen weight)
            if s.w.p.requires_grad:
                queue_wgrad(g, xs[i], s.w.grad, s.b.grad if has_bias else None)
            if ctx.has_res:
                grads[4 * i + 1] = g
        if dgrad:
            if all(g.shape[0] <= lib.SKINNY_MAX_M for (g, _, _, _, _) in dgrad):
                lib.skinny_dgrad([_skinny(g, w, dx) for (g, w, dx, _, _) in dgrad], 0, 1.0, ctx.f32_in)
            else:
                gemm_group(GEMM_NN, dgrad, 0)
        return (None, None, None, *grads)


def _rows2d(t: torch.Tensor) -> torch.Tensor:
    """2-D, last dimension contiguous (row-strided views — column blocks of a wider tensor — pass as they are)"""
    if t.dim() != 2:
        raise ValueError(f"expected a 2-D tensor, got {tuple(t.shape)}")
    return t if t.stride(1) == 1 else t.contiguous()


class _RowLinear(torch.autograd.Function):
    """(B, d)-row linears — M <= 64 rows: the Early / Contrastive / Adaptive / Graph / meta / classifier MLPs and the encoder
    projection tails — with the launches AROUND them folded in (round 4; mmf_skinny_linear_*_ex).  At these sizes a launch costs
    ~5 us and the arithmetic nothing: a Linear + ReLU + Dropout fed by an f32 tensor was cast, linear, dropout (3 launches)
    forward and dropout, ReLU mask, (cast), dgrad (3-4) backward; here it is one launch each way:
      forward   y = dropout(act(x W^T + b)): x may be f32 (narrowed while loaded; the bf16 copy the weight gradient needs is
                written by the kernel's first workgroup), the dropout mask is drawn in the epilogue, and with ``dual`` a second
                copy of y in the other dtype comes out of the same launch (the bf16 operand of the next linear beside the f32
                value the module returns);
      backward  dz = g * (y > 0) / (1 - p) — a ReLU + dropout output is exactly 0 where either gate is closed — or, for dropout
                without ReLU, the regenerated mask, is formed while the dgrad kernel loads g (bf16 or f32, row-strided views
                welcome); dz (bf16) is written once for the deferred weight-gradient launch.
    tensors = [x_0, w_0.p, b_0.p | None, x_1, ...]; returns the n outputs (+ n second copies with ``dual``)."""

    @staticmethod
    def forward(ctx, specs: List[LinearSpec], opts, *tensors):
        out_f32, p, dual = opts
        n = len(specs)
        relu, has_bias, _ = _one_epilogue(specs)
        xs = [_rows2d(tensors[3 * i]) for i in range(n)]
        f32_in = xs[0].dtype == torch.float32
        for x in xs:
            if not x.is_cuda:
                raise RuntimeError("mmfusion ops run on the GPU only (no CPU fallback)")
            if x.dtype not in (BF16, torch.float32) or (x.dtype == torch.float32) != f32_in:
                raise TypeError("a row-linear group's inputs must share one dtype (bf16 or f32)")
        site = next_site() if p > 0.0 else 0
        probs, outs, outs2, x16s = [], [], [], []
        for i, s in enumerate(specs):
            x, w16 = xs[i], s.w.w16
            M, K, N = x.shape[0], x.shape[1], w16.shape[0]
            y = torch.empty((M, N), dtype=torch.float32 if out_f32 else BF16, device=x.device)
            y2 = torch.empty((M, N), dtype=BF16 if out_f32 else torch.float32, device=x.device) if dual else None
            x16 = torch.empty((M, K), dtype=BF16, device=x.device) if f32_in else x
            bias = s.b.master if has_bias else None
            probs.append(lib.SkinnyProblemEx(
                _skinny(x, w16, y, bias), _ptr(y2), None, x16.data_ptr() if f32_in else None,
                _ld(y2) if y2 is not None else 0, 0, _ld(x16) if f32_in else 0, 0))
            outs.append(y), outs2.append(y2), x16s.append(x16)
        flags = (EPI_BIAS if has_bias else 0) | (EPI_RELU if relu else 0) | (EPI_DROPOUT if p > 0.0 else 0)
        extra = lib.SkinnyExtra(int(f32_in), 0, 1.0, float(p), rng_state().data_ptr() if p > 0.0 else None, site, 0)
        lib.skinny_fwd_ex(probs, flags, out_f32, extra)
        ctx.specs, ctx.opts, ctx.site, ctx.f32_in = specs, opts, site, f32_in
        ctx.save_for_backward(*x16s, *(outs if relu else []))
        ctx.x_needs = [tensors[3 * i].requires_grad for i in range(n)]
        return tuple(outs) + (tuple(outs2) if dual else ())

    @staticmethod
    def backward(ctx, *gs):
        specs = ctx.specs
        out_f32, p, dual = ctx.opts
        n = len(specs)
        relu, has_bias = specs[0].relu, specs[0].b is not None
        saved = ctx.saved_tensors
        x16s, ys = saved[:n], (saved[n:] if relu else [None] * n)
        grads: List[Optional[torch.Tensor]] = [None] * (3 * n)
        todo = []
        for i in range(n):
            g, g2 = gs[i], (gs[n + i] if dual else None)
            if g is not None and g2 is not None:             # both copies of the output were used downstream
                g = g.float() + g2.float()
            elif g is None:
                g = g2
            if g is not None:
                g = _rows2d(g)
                if g.data_ptr() % 16 or g.stride(0) % (4 if g.dtype == torch.float32 else 8):
                    g = g.contiguous()                       # (a view whose rows lose the 16-byte alignment of the vector loads)
                todo.append((i, g))
        # one launch per gradient dtype (the kernel narrows f32 gradients itself)
        for want_f32 in (False, True):
            grp = [(i, g) for i, g in todo if (g.dtype == torch.float32) == want_f32]
            if not grp:
                continue
            gated = relu or p > 0.0
            probs, dxs = [], []
            for i, g in grp:
                w16 = specs[i].w.w16
                M, N, K = g.shape[0], w16.shape[0], w16.shape[1]
                if g.dtype not in (BF16, torch.float32):
                    raise TypeError("row-linear backward: bf16 or f32 gradients only")
                dz = torch.empty((M, N), dtype=BF16, device=g.device) if (gated or want_f32) else g
                dx = torch.empty((M, K), dtype=torch.float32 if ctx.f32_in else BF16, device=g.device)
                y = ys[i]
                probs.append(lib.SkinnyProblemEx(
                    _skinny(g, w16, dx), None, _ptr(y), dz.data_ptr() if dz is not g else None,
                    0, _ld(y) if y is not None else 0, _ld(dz) if dz is not g else 0, 0))
                dxs.append(dx)
                if specs[i].w.p.requires_grad:               # a frozen weight: input gradient only
                    queue_wgrad(dz, x16s[i], specs[i].w.grad, specs[i].b.grad if has_bias else None)
                if ctx.x_needs[i]:
                    grads[3 * i] = dx
            regen = p > 0.0 and not relu                      # dropout without ReLU: the mask is drawn again from (state, site)
            extra = lib.SkinnyExtra(int(want_f32), int(relu and ys[grp[0][0]].dtype == torch.float32),
                                    1.0 / (1.0 - p) if (relu and p > 0.0) else 1.0, float(p) if regen else 0.0,
                                    rng_state().data_ptr() if regen else None, ctx.site, 0)
            lib.skinny_dgrad_ex(probs, EPI_DROPOUT if regen else 0, 1.0, ctx.f32_in, extra)
        return (None, None, *grads)


def row_linear_ok(items: Sequence[tuple]) -> bool:
    """whether a linear group can take the fused (B, d)-row form: bf16 mode, <= 64 rows, no residual, one launch"""
    if _PRECISION == "fp32" or len(items) > lib.SKINNY_MAX_PROBLEMS:
        return False
    for x, spec, res in items:
        if res is not None or x.dim() != 2 or x.shape[0] > lib.SKINNY_MAX_M or x.shape[1] % 8 or spec.w.w16.shape[0] % 4:
            return False
        if x.dtype == torch.float32 and (x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16):
            return False
        if x.dtype == BF16 and (x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16):
            return False
    return True


def linear_group(items: Sequence[tuple], out_f32: bool = False, cat: bool = False, dropout_p: float = 0.0, dual: bool = False):
    """items: (x_bf16 [M,K], LinearSpec, residual_bf16|None).  One NT launch for the group.  Returns the list of
    outputs, or with ``cat`` ONE (M, sum N_i) tensor whose column blocks are the outputs (equal M required).
    ``dropout_p``: nn.Dropout(p) on every output (training-mode probability: pass 0 in eval).  ``dual``: every output also as
    a second tensor in the OTHER dtype — the return value is then a list of (y, y_other) pairs.  Groups of (B, d)-row problems
    (``row_linear_ok``) run both inside the linear's own launch (``_RowLinear``); otherwise they are separate kernels."""
    if _PRECISION == "fp32":
        ys = _f32().linear_group(items, cat)
        if dropout_p > 0.0:
            raise RuntimeError("the fp32 parity mode runs without dropout (use p = 0 or eval())")
        return [(y, y) for y in ys] if dual else ys
    if not cat and row_linear_ok(items):
        specs, tensors = _flatten_items(items, residual=False)
        outs = _RowLinear.apply(specs, (bool(out_f32), float(dropout_p), bool(dual)), *tensors)
        n = len(specs)
        return [(outs[i], outs[n + i]) for i in range(n)] if dual else list(outs)
    specs, tensors = _flatten_items(items)
    if cat:
        if dropout_p > 0.0 or dual:
            raise ValueError("a concatenated linear group has no dropout / dual form")
        return _GroupedLinear.apply(specs, bool(out_f32), True, *tensors)
    ys = [dropout(y, dropout_p, True) for y in _GroupedLinear.apply(specs, bool(out_f32), False, *tensors)]
    if dual:
        return [(y, (to_bf16(y) if out_f32 else to_f32(y))) for y in ys]
    return ys


def linear(x: torch.Tensor, w: W, b: Optional[W] = None, relu: bool = False,
           residual: Optional[torch.Tensor] = None, out_f32: bool = False, dropout_p: float = 0.0, dual: bool = False):
    return linear_group([(x, LinearSpec(w, b, relu), residual)], out_f32, dropout_p=dropout_p, dual=dual)[0]


# --------------------------------------------------------------------------------------------
# grouped position-wise FFN with residual:  y_i = x_i + W2_i relu(W1_i x_i + b1_i) + b2_i
# (reference models/fusion_layers.py:195-200,208-209 before norm2).  Fused so that the backward can
# apply the ReLU mask and the residual-gradient add in the dgrad GEMM epilogues:
#   dH = (dY W2) * (h > 0)        NN GEMM, MASK_AUX epilogue (aux = h)
#   dX = dH W1 + dY               NN GEMM, ADD_AUX epilogue  (aux = dY)
# h is M x 4d and the mask is all that dH wants of it: where both launches have the bit form (relu_bits_available), the
# forward GEMM also writes (h > 0) as one bit per element (RELU_BITS) and dH reads those (MASK_BITS) instead of h.
# --------------------------------------------------------------------------------------------
class _GroupedFFN(torch.autograd.Function):
    """tensors = [x_0, W1_0, b1_0, W2_0, b2_0, x_1, ...] (parameters passed so autograd runs backward)."""

    @staticmethod
    def forward(ctx, layers, drop, want_bits, *tensors):
        n = len(layers)
        xs = [tensors[5 * i] for i in range(n)]
        for x in xs:
            _req(x, BF16)
        hs = [torch.empty((x.shape[0], l1.weight.shape[0]), dtype=BF16, device=x.device) for x, (l1, _) in zip(xs, layers)]
        # h = dropout(relu(x W1^T + b1)) in one epilogue; dropped units are exactly 0 in h
        bits = [relu_bits_buffer(h) for h in hs] if want_bits else [None] * n
        ffn1 = [(x, shadow(l1.weight), h, l1.bias.detach(), b) for x, h, b, (l1, _) in zip(xs, hs, bits, layers)]
        if want_bits and relu_bits_available(GEMM_NT, ffn1, EPI_BIAS | EPI_RELU | EPI_RELU_BITS, dropout=drop):
            gemm_group(GEMM_NT, ffn1, EPI_BIAS | EPI_RELU | EPI_RELU_BITS, dropout=drop)
        else:
            bits = []
            gemm_group(GEMM_NT, [q[:4] + (None,) for q in ffn1], EPI_BIAS | EPI_RELU, dropout=drop)
        ctx.keep_scale = 1.0 / (1.0 - drop[0]) if drop is not None else 1.0
        ys = [torch.empty_like(x) for x in xs]
        gemm_group(GEMM_NT, [(h, shadow(l2.weight), y, l2.bias.detach(), x)
                             for x, h, y, (_, l2) in zip(xs, hs, ys, layers)], EPI_BIAS | EPI_ADD_AUX)
        ctx.layers = layers
        ctx.save_for_backward(*xs, *hs, *bits)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        layers = ctx.layers
        n = len(layers)
        xs, hs, bits = ctx.saved_tensors[:n], ctx.saved_tensors[n:2 * n], ctx.saved_tensors[2 * n:]
        idx = [i for i, g in enumerate(gys) if g is not None]
        dys = {i: gys[i].contiguous() for i in idx}
        dhs = {i: torch.empty_like(hs[i]) for i in idx}
        dxs = {i: torch.empty_like(xs[i]) for i in idx}
        # (h > 0) is ReLU mask AND dropout mask at once; only the 1/(1-p) factor is left to apply
        dh = [(dys[i], shadow(layers[i][1].weight), dhs[i], None, bits[i] if bits else hs[i]) for i in idx]
        if bits and relu_bits_available(GEMM_NN, dh, EPI_MASK_BITS, alpha=ctx.keep_scale):
            gemm_group(GEMM_NN, dh, EPI_MASK_BITS, alpha=ctx.keep_scale)
        else:
            gemm_group(GEMM_NN, [q[:4] + (hs[i],) for q, i in zip(dh, idx)], EPI_MASK_AUX, alpha=ctx.keep_scale)
        gemm_group(GEMM_NN, [(dhs[i], shadow(layers[i][0].weight), dxs[i], None, dys[i]) for i in idx], EPI_ADD_AUX)
        for i in idx:
            for l, dy_, x_ in ((layers[i][1], dys[i], hs[i]), (layers[i][0], dhs[i], xs[i])):
                if l.weight.requires_grad:
                    queue_wgrad(dy_, x_, l.weight.grad, l.bias.grad)
        grads: List[Optional[torch.Tensor]] = [None] * (5 * n)
        for i in idx:
            grads[5 * i] = dxs[i]
        return (None, None, None, *grads)


def ffn_residual_group(items: Sequence[tuple], dropout_p: float = 0.0) -> List[torch.Tensor]:
    """items: (x_bf16 [M, d], linear1 (d -> 4d), linear2 (4d -> d)); returns x + ffn(x) per item.
    dropout_p > 0: nn.Dropout on the hidden activations (reference :198), fused into the first GEMM."""
    if _PRECISION == "fp32":
        if dropout_p > 0.0:
            raise RuntimeError("the fp32 parity mode runs without dropout (use p = 0 or eval())")
        return _f32().ffn_residual_group(items)
    layers, tensors = [], []
    for x, l1, l2 in items:
        for p in (l1.weight, l1.bias, l2.weight, l2.bias):
            if getattr(p, "_mmf_bf16", None) is None or p.grad is None:
                raise RuntimeError("FFN parameters are not arena-managed: call mmfusion.arena.ensure(module)")
        layers.append((l1, l2))
        tensors += [x, l1.weight, l1.bias, l2.weight, l2.bias]
    drop = (float(dropout_p), next_site()) if dropout_p > 0.0 else None
    want_bits = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)       # only a forward that will be differentiated
    return list(_GroupedFFN.apply(layers, drop, want_bits, *tensors))


# --------------------------------------------------------------------------------------------
# grouped LayerNorm
# --------------------------------------------------------------------------------------------
class _GroupedLayerNorm(torch.autograd.Function):
    """tensors = [x_0, gamma_0, beta_0, x_1, ...]"""

    @staticmethod
    def forward(ctx, eps: float, *tensors):
        n = len(tensors) // 3
        d = tensors[0].shape[-1]
        outs, stats, probs, keep = [], [], [], []
        for i in range(n):
            x, g, b = tensors[3 * i:3 * i + 3]
            _req(x, BF16)
            x = x.contiguous()
            keep.append(x)
            rows = x.numel() // d
            y = torch.empty_like(x)
            st = torch.empty((2, rows), dtype=torch.float32, device=x.device)
            probs.append(LnProblem(x.data_ptr(), y.data_ptr(), g.data_ptr(), b.data_ptr(), st[0].data_ptr(),
                                   st[1].data_ptr(), None, None, None, None, rows))
            outs.append(y), stats.append(st)
        for i in range(0, n, lib.LN_MAX_PROBLEMS):
            lib.layernorm_fwd_grouped(probs[i:i + lib.LN_MAX_PROBLEMS], d, eps)
        ctx.n, ctx.d = n, d
        ctx.params = [(tensors[3 * i + 1], tensors[3 * i + 2]) for i in range(n)]
        ctx.save_for_backward(*[tensors[3 * i] for i in range(n)], *stats)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gys):
        n, d = ctx.n, ctx.d
        xs, stats = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        grads: List[Optional[torch.Tensor]] = [None] * (3 * n)
        probs, keep = [], []
        for i, g in enumerate(gys):
            if g is None:
                continue
            g = g.contiguous()
            x = xs[i].contiguous()
            keep += [g, x]
            gamma, beta = ctx.params[i]
            if gamma.grad is None or beta.grad is None:
                raise RuntimeError("LayerNorm parameters have no arena gradient")
            dx = torch.empty_like(x)
            rows = x.numel() // d
            probs.append(LnProblem(x.data_ptr(), None, gamma.data_ptr(), None, stats[i][0].data_ptr(),
                                   stats[i][1].data_ptr(), g.data_ptr(), dx.data_ptr(),
                                   gamma.grad.data_ptr(), beta.grad.data_ptr(), rows))
            grads[3 * i] = dx
        ws_bytes = lib.load().mmf_layernorm_bwd_workspace_bytes(d)
        for i in range(0, len(probs), lib.LN_MAX_PROBLEMS):
            ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=xs[0].device)
            keep.append(ws)
            lib.layernorm_bwd_grouped(probs[i:i + lib.LN_MAX_PROBLEMS], d, ws)
        return (None, *grads)


def layernorm_group(items: Sequence[tuple], eps: float = 1e-5) -> List[torch.Tensor]:
    """items: (x_bf16 [..., d], gamma_param, beta_param)."""
    if _PRECISION == "fp32":
        return _f32().layernorm_group(items, eps)
    flat = []
    for x, g, b in items:
        flat += [x, g, b]
    return list(_GroupedLayerNorm.apply(eps, *flat))


class _GroupedLn2Add3(torch.autograd.Function):
    """tensors = [x_0, pre_a_0, gamma_a_0, beta_a_0, pre_b_0, gamma_b_0, beta_b_0, x_1, ...]:
    e_i = x_i + LN(pre_a_i) + LN(pre_b_i) in ONE launch, bit-equal to _GroupedLayerNorm over (pre_a_0, pre_b_0, pre_a_1, ...)
    followed by _Add3Group.  Saves what _GroupedLayerNorm saves; the backward is its backward with the two problems of a sum
    sharing the sum's gradient, which is also the gradient of x."""

    @staticmethod
    def forward(ctx, eps: float, *tensors):
        n = len(tensors) // 7
        d = tensors[0].shape[-1]
        outs, stats, probs, keep = [], [], [], []
        for i in range(n):
            x, pa, ga, ba, pb, gb, bb = tensors[7 * i:7 * i + 7]
            _req(x, BF16), _req(pa, BF16), _req(pb, BF16)
            if x.shape != pa.shape or x.shape != pb.shape:
                raise ValueError("ln2_add3 group: operands of one sum must have one shape")
            x, pa, pb = x.contiguous(), pa.contiguous(), pb.contiguous()
            keep += [x, pa, pb]
            rows = x.numel() // d
            e = torch.empty_like(x)
            st = torch.empty((4, rows), dtype=torch.float32, device=x.device)      # mean_a, rstd_a, mean_b, rstd_b
            probs.append(lib.Ln2Add3Problem(x.data_ptr(), pa.data_ptr(), ga.data_ptr(), ba.data_ptr(), pb.data_ptr(), gb.data_ptr(),
                                            bb.data_ptr(), e.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
                                            st[3].data_ptr(), rows))
            outs.append(e), stats.append(st)
        lib.layernorm2_add3_fwd_grouped(probs, d, eps)
        ctx.n, ctx.d = n, d
        ctx.params = [tuple(tensors[7 * i + j] for j in (2, 3, 5, 6)) for i in range(n)]
        ctx.save_for_backward(*[keep[3 * i + j] for i in range(n) for j in (1, 2)], *stats)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        n, d = ctx.n, ctx.d
        pres, stats = ctx.saved_tensors[:2 * n], ctx.saved_tensors[2 * n:]
        grads: List[Optional[torch.Tensor]] = [None] * (7 * n)
        probs, keep = [], []
        for i, g in enumerate(gs):
            if g is None:
                continue
            g = g.contiguous()
            keep.append(g)
            grads[7 * i] = g
            for j in (0, 1):                                  # the two norms of the sum: one dy
                pre, gamma, beta = pres[2 * i + j], ctx.params[i][2 * j], ctx.params[i][2 * j + 1]
                if gamma.grad is None or beta.grad is None:
                    raise RuntimeError("LayerNorm parameters have no arena gradient")
                dx = torch.empty_like(pre)
                probs.append(LnProblem(pre.data_ptr(), None, gamma.data_ptr(), None, stats[i][2 * j].data_ptr(),
                                       stats[i][2 * j + 1].data_ptr(), g.data_ptr(), dx.data_ptr(),
                                       gamma.grad.data_ptr(), beta.grad.data_ptr(), pre.numel() // d))
                grads[7 * i + 1 + 3 * j] = dx
        if probs:
            ws = torch.empty(lib.load().mmf_layernorm_bwd_workspace_bytes(d) // 4, dtype=torch.float32, device=pres[0].device)
            keep.append(ws)
            lib.layernorm_bwd_grouped(probs, d, ws)
        return (None, *grads)


def ln2_add3_group(items: Sequence[tuple], eps: float = 1e-5) -> List[torch.Tensor]:
    """items: (x, pre_a, norm_a, pre_b, norm_b) with bf16 [rows, d] tensors and nn.LayerNorm modules: x + norm_a(pre_a) +
    norm_b(pre_b) per item — MulT's three-way sum over the second LayerNorms of two cross-modal blocks.  One fused launch
    where the library has it (lib.layernorm2_add3_available); else, and in fp32 mode, the two launches it stands for."""
    rows = [x.numel() // x.shape[-1] for x, *_ in items]
    if (_PRECISION == "fp32" or len(items) > lib.LN2_ADD3_MAX_PROBLEMS
            or not lib.layernorm2_add3_available(rows, items[0][0].shape[-1])):
        ys = layernorm_group([(pre, nm.weight, nm.bias) for _, pa, na, pb, nb in items for pre, nm in ((pa, na), (pb, nb))], eps)
        return add3_group([(x, ys[2 * i], ys[2 * i + 1]) for i, (x, *_) in enumerate(items)])
    flat = []
    for x, pa, na, pb, nb in items:
        flat += [x, pa, na.weight, na.bias, pb, nb.weight, nb.bias]
    return list(_GroupedLn2Add3.apply(eps, *flat))


# --------------------------------------------------------------------------------------------
# grouped fused attention
# --------------------------------------------------------------------------------------------
@dataclass
class AttnSpec:
    """One attention problem.  q/k/v are (source index, first column) into the `srcs` list of 2-D
    bf16 buffers (rows = B*T, row-major); heads are laid out as consecutive head_dim column groups."""
    B: int
    Tq: int
    Tk: int
    q: Tuple[int, int]
    k: Tuple[int, int]
    v: Tuple[int, int]


def _attn_forward(specs: List[AttnSpec], H: int, dh: int, drop, srcs) -> Tuple[list, list]:
    """the grouped forward launch(es): per problem the (B*Tq, d) bf16 output and the f32 LSE"""
    scale = 1.0 / math.sqrt(dh)
    d = H * dh
    outs, lses, probs = [], [], []
    for s in specs:
        for (si, col), T in ((s.q, s.Tq), (s.k, s.Tk), (s.v, s.Tk)):
            t = srcs[si]
            _req(t, BF16)
            if t.dim() != 2 or not t.is_contiguous() or t.shape[0] != s.B * T or col + d > t.shape[1]:
                raise ValueError(f"attention source {si}: shape {tuple(t.shape)} does not hold B*T={s.B * T} rows x {d} columns at {col}")
        dev = srcs[0].device
        o = torch.empty((s.B * s.Tq, d), dtype=BF16, device=dev)
        lse = torch.empty((s.B * H * s.Tq,), dtype=torch.float32, device=dev)
        qs, ks, vs = srcs[s.q[0]], srcs[s.k[0]], srcs[s.v[0]]
        probs.append(AttnProblem(qs.data_ptr() + 2 * s.q[1], ks.data_ptr() + 2 * s.k[1], vs.data_ptr() + 2 * s.v[1],
                                 o.data_ptr(), lse.data_ptr(), None, None, None, None, None,
                                 s.B, H, s.Tq, s.Tk, qs.shape[1], ks.shape[1], vs.shape[1], d))
        outs.append(o), lses.append(lse)
    if drop is not None and len(probs) > lib.ATTN_MAX_PROBLEMS:
        raise ValueError("an attention group with dropout must fit one launch (the problem index keys the mask)")
    dp_, st_, site_ = (drop[0], rng_state().data_ptr(), drop[1]) if drop is not None else (0.0, None, 0)
    for i in range(0, len(probs), lib.ATTN_MAX_PROBLEMS):
        lib.attn_fwd_grouped(probs[i:i + lib.ATTN_MAX_PROBLEMS], dh, scale, dp_, st_, site_)
    return outs, lses


def _attn_backward_problems(specs: List[AttnSpec], H: int, dh: int, srcs, outs, lses, gos) -> Tuple[list, list, list]:
    """The backward's problem table for output gradients ``gos`` (contiguous bf16; a None skips its problem): the problems, one
    gradient buffer per source (None where nothing flows) and the temporaries the table points into."""
    d = H * dh
    # one gradient buffer per source; zero-filled only when some column range is not covered
    covered = [set() for _ in srcs]
    for s, g in zip(specs, gos):
        if g is None:
            continue
        for si, col in (s.q, s.k, s.v):
            covered[si].add(col)
    gsrc: List[Optional[torch.Tensor]] = []
    for si, t in enumerate(srcs):
        if not covered[si]:
            gsrc.append(None)
            continue
        full = len(covered[si]) * d == t.shape[1]
        gsrc.append(torch.empty_like(t) if full else torch.zeros_like(t))
    probs, keep = [], []          # `keep`: every temporary whose pointer sits in a problem table must
    for i, (s, g) in enumerate(zip(specs, gos)):      # outlive the launch, or the caching allocator
        if g is None:                                 # hands its block to the next problem
            continue
        delta = torch.empty_like(lses[i])
        keep += [g, delta]
        qs, ks, vs = srcs[s.q[0]], srcs[s.k[0]], srcs[s.v[0]]
        probs.append(AttnProblem(qs.data_ptr() + 2 * s.q[1], ks.data_ptr() + 2 * s.k[1], vs.data_ptr() + 2 * s.v[1],
                                 outs[i].data_ptr(), lses[i].data_ptr(), g.data_ptr(), delta.data_ptr(),
                                 gsrc[s.q[0]].data_ptr() + 2 * s.q[1], gsrc[s.k[0]].data_ptr() + 2 * s.k[1],
                                 gsrc[s.v[0]].data_ptr() + 2 * s.v[1],
                                 s.B, H, s.Tq, s.Tk, qs.shape[1], ks.shape[1], vs.shape[1], d))
    return probs, gsrc, keep


class _GroupedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, specs: List[AttnSpec], H: int, dh: int, drop, *srcs):
        outs, lses = _attn_forward(specs, H, dh, drop, srcs)
        ctx.specs, ctx.H, ctx.dh, ctx.nsrc, ctx.drop = specs, H, dh, len(srcs), drop
        ctx.save_for_backward(*srcs, *outs, *lses)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gos):
        specs, H, dh, ns = ctx.specs, ctx.H, ctx.dh, ctx.nsrc
        n = len(specs)
        srcs = ctx.saved_tensors[:ns]
        outs = ctx.saved_tensors[ns:ns + n]
        lses = ctx.saved_tensors[ns + n:]
        probs, gsrc, keep = _attn_backward_problems(specs, H, dh, srcs, outs, lses,
                                                    [None if g is None else g.contiguous() for g in gos])
        drop = ctx.drop
        if drop is not None and len(probs) != len(specs):
            raise RuntimeError("attention dropout backward needs the gradient of every problem of the group")
        dp_, st_, site_ = (drop[0], rng_state().data_ptr(), drop[1]) if drop is not None else (0.0, None, 0)
        for i in range(0, len(probs), lib.ATTN_MAX_PROBLEMS):
            lib.attn_bwd_grouped(probs[i:i + lib.ATTN_MAX_PROBLEMS], dh, 1.0 / math.sqrt(dh), dp_, st_, site_)
        return (None, None, None, None, *gsrc)


def attention_group(specs: List[AttnSpec], H: int, dh: int, srcs: Sequence[torch.Tensor],
                    dropout_p: float = 0.0) -> List[torch.Tensor]:
    """Each (source, column) pair may be the k or v of several problems only if those problems'
    gradients are wanted separately — within one call every (source, column) range must be
    written by at most one problem's dK/dV (true for MulT: each block has its own K/V projection)."""
    if _PRECISION == "fp32":
        if dropout_p > 0.0:
            raise RuntimeError("the fp32 parity mode runs without dropout (use p = 0 or eval())")
        return _f32().attention_group(specs, H, dh, srcs)
    drop = (float(dropout_p), next_site()) if dropout_p > 0.0 else None
    return list(_GroupedAttention.apply(specs, H, dh, drop, *srcs))


class _AttentionMeanPool(torch.autograd.Function):
    """``meanpool_cat`` of ``attention_group``'s outputs as one node: the forward is those two steps' launches; the backward never
    writes the (B*T, d) output gradients — every row of a batch row's is the same u[b] = bf16(g[b] / T) — and hands the (B, d)
    rows to the uniform attention backward (include/mmfusion.h: mmf_attn_bwd_grouped_uniform)."""

    @staticmethod
    def forward(ctx, specs: List[AttnSpec], H: int, dh: int, *srcs):
        outs, lses = _attn_forward(specs, H, dh, None, srcs)
        n, B, d = len(specs), specs[0].B, H * dh
        y = torch.empty((B, n * d), dtype=BF16, device=srcs[0].device)
        ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        Ts = (C.c_int * n)(*[s.Tq for s in specs])
        lib.check(lib.load().mmf_meanpool_cat_fwd(ptrs, Ts, n, y.data_ptr(), B, d, n * d, lib.stream_ptr()))
        ctx.specs, ctx.H, ctx.dh, ctx.nsrc = specs, H, dh, len(srcs)
        ctx.save_for_backward(*srcs, *outs, *lses)
        return y

    @staticmethod
    def backward(ctx, g):
        specs, H, dh, ns = ctx.specs, ctx.H, ctx.dh, ctx.nsrc
        n, B, d = len(specs), specs[0].B, H * dh
        srcs = ctx.saved_tensors[:ns]
        outs = ctx.saved_tensors[ns:ns + n]
        lses = ctx.saved_tensors[ns + n:]
        if g.dtype != BF16 or g.stride(1) != 1 or g.stride(0) % 8 or g.data_ptr() % 16:
            g = g.contiguous()
        u = torch.empty((n, B, d), dtype=BF16, device=g.device)                 # one gradient row per batch row, written by the launch
        probs, gsrc, keep = _attn_backward_problems(specs, H, dh, srcs, outs, lses, [u[i] for i in range(n)])
        ws = torch.empty((lib.attn_bwd_uniform_workspace_bytes(probs) // 4,), dtype=torch.float32, device=g.device)
        lib.attn_bwd_grouped_uniform(probs, dh, 1.0 / math.sqrt(dh), ws,
                                     pooled=([g.data_ptr() + 2 * i * d for i in range(n)], g.stride(0)))
        return (None, None, None, *gsrc)


def attention_meanpool_group(specs: List[AttnSpec], H: int, dh: int, srcs: Sequence[torch.Tensor],
                             dropout_p: float = 0.0) -> torch.Tensor:
    """``meanpool_cat`` of ``attention_group``'s outputs, (B, n*d) bf16, for attentions that are consumed through their mean over
    the queries only (MulT's self-attentions).  Forward: those two steps' launches.  Backward: the uniform attention backward
    where the library has it for this head_dim and dropout (``lib.attn_bwd_uniform_available``); else, and in fp32 mode, the
    two steps as they are."""
    if (_PRECISION == "fp32" or not 0 < len(specs) <= min(lib.POOL_MAX, lib.ATTN_MAX_PROBLEMS) or any(s.B != specs[0].B for s in specs)
            or not lib.attn_bwd_uniform_available(dh, float(dropout_p))):
        att = attention_group(specs, H, dh, srcs, dropout_p=dropout_p)
        return meanpool_cat([o.view(s.B, s.Tq, H * dh) for o, s in zip(att, specs)])
    return _AttentionMeanPool.apply(specs, H, dh, *srcs)


# --------------------------------------------------------------------------------------------
# elementwise / pooling
# --------------------------------------------------------------------------------------------
class _Add3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, c):
        _req(a, BF16)
        a, b = a.contiguous(), b.contiguous()
        c = c.contiguous() if c is not None else None
        y = torch.empty_like(a)
        lib.check(lib.load().mmf_add3_bf16(a.data_ptr(), b.data_ptr(), c.data_ptr() if c is not None else None,
                                           y.data_ptr(), a.numel(), lib.stream_ptr()))
        ctx.has_c = c is not None
        return y

    @staticmethod
    def backward(ctx, g):
        return g, g, (g if ctx.has_c else None)


def add3(a, b, c=None):
    if _PRECISION == "fp32":
        return a + b if c is None else a + b + c
    return _Add3.apply(a, b, c)


class _Add3Group(torch.autograd.Function):
    """tensors = [a_0, b_0, c_0, a_1, ...] (bf16): y_i = a_i + b_i + c_i for all i in ONE launch."""

    @staticmethod
    def forward(ctx, *tensors):
        n = len(tensors) // 3
        probs, outs, keep = [], [], []
        for i in range(n):
            a, b, c = (t.contiguous() for t in tensors[3 * i:3 * i + 3])
            _req(a, BF16), _req(b, BF16), _req(c, BF16)
            if a.shape != b.shape or a.shape != c.shape:
                raise ValueError("add3 group: operands of one sum must have one shape")
            y = torch.empty_like(a)
            keep += [a, b, c]
            outs.append(y)
            probs.append(lib.Add3Problem(a.data_ptr(), b.data_ptr(), c.data_ptr(), y.data_ptr(), a.numel()))
        arr = (lib.Add3Problem * n)(*probs)
        lib.check(lib.load().mmf_add3_grouped(arr, n, lib.stream_ptr()))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        out = []
        for g in gs:
            out += [g, g, g]
        return tuple(out)


def add3_group(triples: Sequence[tuple]) -> List[torch.Tensor]:
    """[(a, b, c), ...] -> [a + b + c, ...], one launch (up to lib.ADD3_MAX sums)."""
    if _PRECISION == "fp32":
        return [a + b + c for a, b, c in triples]
    if not 0 < len(triples) <= lib.ADD3_MAX:
        raise ValueError(f"add3 group of {len(triples)} sums (1..{lib.ADD3_MAX})")
    return list(_Add3Group.apply(*[t for tr in triples for t in tr]))


class _Fanout(torch.autograd.Function):
    """n aliases of one bf16 tensor for n consumers; the backward receives all n gradients at once and sums them in
    ONE pass (mmf_addn_bf16, f32 accumulate) instead of the n - 1 pairwise adds autograd would issue."""

    @staticmethod
    def forward(ctx, x, n: int):
        ctx.n = n
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        live = [g for g in gs if g is not None]
        if not live:
            return None, None
        if len(live) == 1:
            return live[0], None
        live = [_grad_bf16(g) for g in live]
        out = torch.empty_like(live[0])
        for i in range(0, len(live), lib.ADDN_MAX - 1):            # chunks of <= 8 operands (running sum carried)
            chunk = live[i:i + lib.ADDN_MAX - 1] + ([out] if i > 0 else [])
            if len(chunk) == 1:
                chunk.append(torch.zeros_like(out))
            ptrs = (C.c_void_p * len(chunk))(*[g.data_ptr() for g in chunk])
            lib.check(lib.load().mmf_addn_bf16(ptrs, len(chunk), out.data_ptr(), out.numel(), 0, lib.stream_ptr()))
        return out, None


def fanout(x: torch.Tensor, n: int) -> List[torch.Tensor]:
    """n handles on x (bf16) whose gradients are summed by one kernel.  Identity when x needs no gradient."""
    if n < 2 or not x.requires_grad or x.dtype != BF16 or _PRECISION == "fp32":
        return [x] * n
    return list(_Fanout.apply(x, n))


class _FanoutGroup(torch.autograd.Function):
    """_Fanout for several tensors at once: n aliases of each of m bf16 tensors; the backward receives all m * n gradients
    together and sums them per tensor in ONE grouped launch (mmf_addn_grouped).  MulT's three modalities' input-gradient
    sums all complete at the end of the backward; as three nodes they were three launches with graph-node gaps between
    them, alone on the chip in front of the deferred wgrad launch (57 us per step in round 3's timeline)."""

    @staticmethod
    def forward(ctx, n: int, *xs):
        ctx.n, ctx.m = n, len(xs)
        return tuple(x.view_as(x) for x in xs for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        n, m = ctx.n, ctx.m
        return (None, *_sum_gradient_groups([gs[i * n:(i + 1) * n] for i in range(m)]))


def _sum_gradient_groups(groups: Sequence[Sequence[Optional[torch.Tensor]]]) -> List[Optional[torch.Tensor]]:
    """One bf16 sum per group of gradients (None entries skipped; an empty group gives None), all groups in ONE grouped launch
    (mmf_addn_grouped, f32 accumulate)."""
    outs: List[Optional[torch.Tensor]] = []
    probs, keep = [], []
    for grads in groups:
        live = [g for g in grads if g is not None]
        if not live:
            outs.append(None)
            continue
        if len(live) == 1:
            outs.append(live[0])
            continue
        live = [_grad_bf16(g) for g in live]
        if len(live) > lib.ADDN_MAX or live[0].numel() % 8 or any(g.data_ptr() % 16 for g in live):
            # a gradient the grouped kernel cannot take (a view at an odd offset, an over-wide fan-out): sum this tensor's
            # gradients with stock adds in f32 rather than raising from inside backward
            acc = live[0].float()
            for g in live[1:]:
                acc = acc + g.float()
            outs.append(acc.to(BF16))
            continue
        out = torch.empty_like(live[0])
        q = lib.AddNProblem()
        for k, g in enumerate(live):
            q.x[k] = g.data_ptr()
        q.y, q.numel, q.n = out.data_ptr(), out.numel(), len(live)
        probs.append(q)
        keep += live
        outs.append(out)
    for i in range(0, len(probs), lib.ADDN_GROUP_MAX):
        chunk = probs[i:i + lib.ADDN_GROUP_MAX]
        arr = (lib.AddNProblem * len(chunk))(*chunk)
        lib.check(lib.load().mmf_addn_grouped(arr, len(chunk), lib.stream_ptr()))
    return outs


def fanout_group(xs: Sequence[torch.Tensor], n: int) -> List[List[torch.Tensor]]:
    """[fanout(x, n) for x in xs] whose backward sums every tensor's n gradients in one grouped launch.  Falls back to
    per-tensor fanout when some tensor needs no gradient (or in the fp32 parity mode)."""
    if n < 2 or n > lib.ADDN_MAX or _PRECISION == "fp32" or not all(x.requires_grad and x.dtype == BF16 for x in xs):
        return [fanout(x, n) for x in xs]
    flat = _FanoutGroup.apply(n, *xs)
    return [list(flat[i * n:(i + 1) * n]) for i in range(len(xs))]


# --------------------------------------------------------------------------------------------
# the linears that read one input, with that input's pass-through uses, as ONE node: its backward forms each input's
# gradient in one accumulator chain per output tile (lib.gemm_grouped_chain) instead of one dgrad per linear plus a sum
# --------------------------------------------------------------------------------------------
class _FanoutLinear(torch.autograd.Function):
    """tensors = [x_0 .. x_{m-1}, w_0.p, b_0.p, w_1.p, ...]; ``src[i]``: the input linear i reads; ``npass`` further handles
    on every input.  Returns the linears' outputs, then the m * npass handles.  The forward is the launch ``linear_group``
    makes of the same items.  The backward receives every gradient of an input at once:
        dx_j = sum over the linears i that read x_j of dy_i W_i  +  the sum of the npass handle gradients
    as one chain per input (the handle gradients summed first, left to right, by ``mmf_add3_grouped`` and added in the
    chain's drain) where the library takes it, else as the dgrad launch and the grouped sum ``_GroupedLinear`` and
    ``_FanoutGroup`` make.  Weight gradients are queued as ``_GroupedLinear`` queues them."""

    @staticmethod
    def forward(ctx, specs: List[LinearSpec], src: List[int], npass: int, m: int, *tensors):
        xs = tensors[:m]
        for x in xs:
            _req(x, BF16)
        _one_epilogue(specs)
        has_bias = specs[0].b is not None
        ws = [s.w.w16 for s in specs]
        ins = [xs[j] for j in src]
        _, outs = _linear_outputs(ins, ws, BF16, False)
        gemm_group(GEMM_NT, [(x, w, y, s.b.master if has_bias else None, None) for x, w, y, s in zip(ins, ws, outs, specs)],
                   EPI_BIAS if has_bias else 0)
        ctx.specs, ctx.src, ctx.npass, ctx.m = specs, src, npass, m
        ctx.save_for_backward(*xs)
        return (*outs, *(x.view_as(x) for x in xs for _ in range(npass)))

    @staticmethod
    def backward(ctx, *gs):
        specs, src, npass, m = ctx.specs, ctx.src, ctx.npass, ctx.m
        xs = ctx.saved_tensors
        n = len(specs)
        has_bias = specs[0].b is not None
        ws = [s.w.w16 for s in specs]
        dys = [_grad_bf16(g) for g in gs[:n]]
        passes = [[_grad_bf16(g) for g in gs[n + j * npass:n + (j + 1) * npass]] for j in range(m)]
        for i, s in enumerate(specs):               # the weight gradients: the operands _GroupedLinear queues, in its order
            if dys[i] is not None and s.w.p.requires_grad:
                queue_wgrad(dys[i], xs[src[i]], s.w.grad, s.b.grad if has_bias else None)
        dxs = _chained_input_grads(xs, src, ws, dys, passes)
        if dxs is None:                             # the launches of the separate nodes
            parts = [torch.empty_like(xs[src[i]]) if dys[i] is not None else None for i in range(n)]
            dgrad = [(dys[i], ws[i], parts[i], None, None) for i in range(n) if dys[i] is not None]
            if dgrad:
                gemm_group(GEMM_NN, dgrad, 0)
            # (operand order of fanout_group's sum in MulT: the linears, then the handles with the first one last)
            dxs = _sum_gradient_groups([[parts[i] for i in range(n) if src[i] == j] + passes[j][1:] + passes[j][:1] for j in range(m)])
        return (None, None, None, None, *dxs, *([None] * (2 * n)))


def _chained_input_grads(xs, src, ws, dys, passes) -> Optional[List[torch.Tensor]]:
    """``_FanoutLinear``'s input gradients by one chained launch, or None where that launch does not exist: a gradient is
    missing, an input has more linears than a chain has segments or other than three handles, or the library refuses the
    shapes (``lib.gemm_chain_available``)."""
    m = len(xs)
    if any(g is None for g in dys) or any(len(p) != 3 or any(g is None for g in p) for p in passes):
        return None
    chains, sums, dxs = [], [], []
    for j in range(m):
        mine = [i for i in range(len(src)) if src[i] == j]
        if not 0 < len(mine) <= lib.GEMM_CHAIN_MAX_SEGMENTS or any(g.shape != xs[j].shape for g in passes[j]):
            return None
        if any(dys[i].shape != (xs[j].shape[0], ws[i].shape[0]) or dys[i].stride(1) != 1 or ws[i].stride(1) != 1 for i in mine):
            return None
        s, dx = torch.empty_like(passes[j][0]), torch.empty_like(passes[j][0])
        chains.append((dx, None, s, [(dys[i], ws[i]) for i in mine]))
        sums.append(lib.Add3Problem(*(g.data_ptr() for g in passes[j]), s.data_ptr(), s.numel()))
        dxs.append(dx)
    if m > lib.ADD3_MAX or m > lib.GEMM_MAX_CHAINS or not gemm_chain_available(chains, EPI_ADD_AUX):
        return None
    lib.check(lib.load().mmf_add3_grouped((lib.Add3Problem * m)(*sums), m, lib.stream_ptr()))
    gemm_chain_group(chains, EPI_ADD_AUX)
    return dxs


def fanout_linear_ok(xs: Sequence[torch.Tensor], items: Sequence[tuple]) -> bool:
    """whether ``fanout_linear_group`` has its node for these inputs and (input index, LinearSpec) items: bf16 mode, every
    input a bf16 row matrix that needs a gradient, one launch, no ReLU"""
    return (_PRECISION != "fp32" and 0 < len(items) <= lib.GEMM_MAX_PROBLEMS
            and all(x.is_cuda and x.dtype == BF16 and x.requires_grad and x.dim() == 2 for x in xs)
            and not any(spec.relu for _, spec in items))


def fanout_linear_group(xs: Sequence[torch.Tensor], items: Sequence[tuple], npass: int) -> Tuple[List[torch.Tensor], List[List[torch.Tensor]]]:
    """(``linear_group([(xs[j], spec, None) for j, spec in items])``, ``npass`` further handles on every x) as one node
    (``_FanoutLinear``); call where ``fanout_linear_ok``."""
    specs, src = [spec for _, spec in items], [j for j, _ in items]
    params = [t for s in specs for t in (s.w.p, s.b.p if s.b is not None else None)]
    flat = _FanoutLinear.apply(specs, src, int(npass), len(xs), *xs, *params)
    n = len(specs)
    return list(flat[:n]), [list(flat[n + j * npass:n + (j + 1) * npass]) for j in range(len(xs))]


class _MeanPoolCat(torch.autograd.Function):
    """xs: (B, T_i, d) bf16 -> (B, n*d) bf16 = cat_i mean_t x_i  (fusion_layers.py:166-171)."""

    @staticmethod
    def forward(ctx, *xs):
        B, _, d = xs[0].shape
        n = len(xs)
        y = torch.empty((B, n * d), dtype=BF16, device=xs[0].device)
        L, st = lib.load(), lib.stream_ptr()
        xs = [x.contiguous() for x in xs]
        for x in xs:
            _req(x, BF16)
        if n <= lib.POOL_MAX:                            # all modalities in one launch
            ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
            Ts = (C.c_int * n)(*[x.shape[1] for x in xs])
            lib.check(L.mmf_meanpool_cat_fwd(ptrs, Ts, n, y.data_ptr(), B, d, n * d, st))
        else:
            for i, x in enumerate(xs):
                lib.check(L.mmf_meanpool_fwd(x.data_ptr(), y.data_ptr() + 2 * i * d, B, x.shape[1], d, n * d, st))
        ctx.shapes = [tuple(x.shape) for x in xs]
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        L, st = lib.load(), lib.stream_ptr()
        n = len(ctx.shapes)
        out = [torch.empty((B, T, d), dtype=BF16, device=g.device) for (B, T, d) in ctx.shapes]
        B, _, d = ctx.shapes[0]
        if n <= lib.POOL_MAX:
            ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in out])
            Ts = (C.c_int * n)(*[sh[1] for sh in ctx.shapes])
            lib.check(L.mmf_meanpool_cat_bwd(g.data_ptr(), ptrs, Ts, n, B, d, n * d, st))
        else:
            for i, (B, T, d) in enumerate(ctx.shapes):
                lib.check(L.mmf_meanpool_bwd(g.data_ptr() + 2 * i * d, out[i].data_ptr(), B, T, d, n * d, st))
        return tuple(out)


def meanpool_cat(xs: Sequence[torch.Tensor]) -> torch.Tensor:
    if _PRECISION == "fp32":
        return torch.cat([x.float().mean(dim=1) for x in xs], dim=-1)
    return _MeanPoolCat.apply(*xs)
