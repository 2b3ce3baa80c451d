"""autograd wrappers of the small fused branch kernels (``csrc/small.hip``): dense 3-node GAT layer, L2-normalise
+ symmetric InfoNCE, adaptive softmax-weighted combination, narrow linear heads, node stacking with type
embedding, per-sample modality masks.  Conventions as in ``mmfusion.ops``: GPU only (no fallback), parameter
gradients are accumulated by the kernels straight into ``param.grad`` (the fp32 gradient arena) and the Function
returns ``None`` for them."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import lib, ops
from .ops import BF16, _column_blocks, _grad_bf16, _ptr, _req

F32 = torch.float32
NCE_MAX_B = 64
NARROW_MAX_N = 16


def _grad_of(p: torch.nn.Parameter) -> torch.Tensor:
    g = p.grad
    if g is None or g.dtype != F32 or not g.is_contiguous():
        raise RuntimeError("parameter has no fp32 arena gradient: call mmfusion.arena.ensure(module)")
    return g


# --------------------------------------------------------------------------------------------
# (B, 3d) "cat3" views: the three modality feature matrices side by side
# --------------------------------------------------------------------------------------------
def cat3(t: torch.Tensor, a: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """fp32 (B, 3d) = cat([t, a, v], -1).  When the three are the column thirds of one contiguous fp32 buffer
    (hier-seq: the pooled sequence means) that buffer itself is returned — no copy, gradients flow to it."""
    base = _column_blocks((t, a, v))
    if base is not None and base.dtype == F32 and t.shape[1] == a.shape[1] == v.shape[1]:
        return base
    return torch.cat([t.float(), a.float(), v.float()], dim=-1)


split3_nocopy_hits = 0          # times _Split3.backward returned the producer's buffer (tests)


class _Split3(torch.autograd.Function):
    """The three column thirds of a (B, 3d) tensor as row-strided views.  Plain slicing would do, but its backward
    is three zero-fills plus three copies; this one is a single ``torch.cat``."""

    @staticmethod
    def forward(ctx, c):
        d = c.shape[1] // 3
        ctx.meta = (c.shape[0], d, c.dtype, c.device)
        return c[:, :d], c[:, d:2 * d], c[:, 2 * d:]

    @staticmethod
    def backward(ctx, g0, g1, g2):
        B, d, dtype, dev = ctx.meta
        # the producer (ops._GroupedLinear.backward) writes the three input gradients as the column thirds of one
        # buffer when its inputs were such thirds: that buffer is the gradient, no concatenation kernel
        if g0 is not None and g1 is not None and g2 is not None:
            base = _column_blocks((g0, g1, g2))
            if base is not None and base.dtype == dtype and tuple(base.shape) == (B, 3 * d):
                global split3_nocopy_hits
                split3_nocopy_hits += 1
                return base
        gs = [g if g is not None else torch.zeros((B, d), dtype=dtype, device=dev) for g in (g0, g1, g2)]
        return torch.cat([g.to(dtype) for g in gs], dim=1)


def split3(c: torch.Tensor):
    return _Split3.apply(c)


class _Stack3Embed(torch.autograd.Function):
    """x[b][m][:] = cat3[b][m*d:(m+1)*d] + emb[m][:]  ->  bf16 (B*3, d) rows (GraphFusion :255-264; emb None =
    plain stacking)."""

    @staticmethod
    def forward(ctx, c3: torch.Tensor, emb: Optional[torch.nn.Parameter]):
        _req(c3, F32)
        c3 = c3.contiguous()
        B, d = c3.shape[0], c3.shape[1] // 3
        x = torch.empty((B * 3, d), dtype=BF16, device=c3.device)
        p = c3.data_ptr()
        lib.check(lib.load().mmf_stack3_embed_fwd(p, p + 4 * d, p + 8 * d, _ptr(emb), x.data_ptr(), B, d, 3 * d,
                                                  lib.stream_ptr()))
        ctx.emb, ctx.B, ctx.d, ctx.need = emb, B, d, c3.requires_grad
        return x

    @staticmethod
    def backward(ctx, dx):
        B, d = ctx.B, ctx.d
        dx = dx.contiguous()
        dc3 = torch.empty((B, 3 * d), dtype=F32, device=dx.device) if ctx.need else None
        p = _ptr(dc3)
        demb = _grad_of(ctx.emb).data_ptr() if ctx.emb is not None else None
        lib.check(lib.load().mmf_stack3_embed_bwd(dx.data_ptr(), p, p + 4 * d if p else None, p + 8 * d if p else None,
                                                  demb, B, d, 3 * d, lib.stream_ptr()))
        return dc3, None


def stack3_embed(c3: torch.Tensor, emb: Optional[torch.nn.Parameter]) -> torch.Tensor:
    return _Stack3Embed.apply(c3, emb)


# --------------------------------------------------------------------------------------------
# dense 3-node GAT layer
# --------------------------------------------------------------------------------------------
class _Gat3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, att_src, att_dst, bias, B: int, heads: int, relu: bool, pool: bool, drop):
        _req(h, F32)
        h = h.contiguous()
        C_ = h.shape[1] // heads
        dev = h.device
        y = torch.empty((B * 3, C_), dtype=BF16, device=dev)
        pooled = torch.empty((B, C_), dtype=BF16, device=dev) if pool else None
        alpha = torch.empty((B, 3, 3, heads), dtype=F32, device=dev)
        sdots = torch.empty((B, 2, 3, heads), dtype=F32, device=dev)
        prm = lib.Gat3Params(B, heads, C_, int(relu), 0.2, drop[0] if drop else 0.0,
                             ops.rng_state().data_ptr() if drop else None, drop[1] if drop else 0)
        lib.check(lib.load().mmf_gat3_dense_fwd(h.data_ptr(), att_src.data_ptr(), att_dst.data_ptr(), bias.data_ptr(),
                                                y.data_ptr(), _ptr(pooled), alpha.data_ptr(), sdots.data_ptr(),
                                                C.byref(prm), lib.stream_ptr()))
        ctx.params, ctx.cfg = (att_src, att_dst, bias), (B, heads, C_, relu, drop)
        ctx.save_for_backward(h, y, alpha, sdots)
        ctx.pool = pool
        if pool:
            return y, pooled
        return y

    @staticmethod
    def backward(ctx, *gs):
        h, y, alpha, sdots = ctx.saved_tensors
        B, heads, C_, relu, drop = ctx.cfg
        att_src, att_dst, bias = ctx.params
        dy, dpool = _grad_bf16(gs[0]), (_grad_bf16(gs[1]) if ctx.pool else None)
        if dy is None and dpool is None:
            return (None,) * 9
        dh = torch.empty_like(h)
        prm = lib.Gat3Params(B, heads, C_, int(relu), 0.2, drop[0] if drop else 0.0,
                             ops.rng_state().data_ptr() if drop else None, drop[1] if drop else 0)
        lib.check(lib.load().mmf_gat3_dense_bwd(h.data_ptr(), att_src.data_ptr(), att_dst.data_ptr(), y.data_ptr(),
                                                alpha.data_ptr(), sdots.data_ptr(), _ptr(dy), _ptr(dpool), dh.data_ptr(),
                                                _grad_of(att_src).data_ptr(), _grad_of(att_dst).data_ptr(),
                                                _grad_of(bias).data_ptr(), C.byref(prm), lib.stream_ptr()))
        return (dh,) + (None,) * 8


def gat3(h: torch.Tensor, att_src, att_dst, bias, B: int, heads: int, relu: bool = True, pool: bool = False,
         dropout_p: float = 0.0):
    """h: f32 (B*3, heads*C) = node features after the layer's linear map.  Returns y bf16 (B*3, C) = relu(GAT(h))
    and, with ``pool``, also the mean over the three nodes, bf16 (B, C)."""
    drop = (float(dropout_p), ops.next_site()) if dropout_p > 0.0 else None
    return _Gat3.apply(h, att_src, att_dst, bias, B, heads, relu, pool, drop)


def gat3_f32(h: torch.Tensor, att_src, att_dst, bias, B: int, heads: int, pool: bool = False):
    """fp32 parity mode: relu(GATConv) on the 3-clique + self loops as f32 torch ops on the (B, 3) nodes (the same
    dense arithmetic as csrc/small.hip gat3_*, reference :267-282 via PyG; parity unpinned).  h: f32 (B*3, heads*C)."""
    Cc = h.shape[1] // heads
    hh = h.view(B, 3, heads, Cc)
    s_src = (hh * att_src.view(1, 1, heads, Cc)).sum(-1)
    s_dst = (hh * att_dst.view(1, 1, heads, Cc)).sum(-1)
    e = torch.nn.functional.leaky_relu(s_dst.unsqueeze(2) + s_src.unsqueeze(1), 0.2)       # (B, i, j, H)
    ex = torch.exp(e - e.max(dim=2, keepdim=True).values)
    alpha = ex / (ex.sum(dim=2, keepdim=True) + 1e-16)
    y = torch.relu(torch.einsum("bijh,bjhc->bihc", alpha, hh).mean(dim=2) + bias)
    rows = y.reshape(B * 3, Cc)
    return (rows, y.mean(dim=1)) if pool else rows


# --------------------------------------------------------------------------------------------
# L2-normalise + symmetric InfoNCE of the three pairs
# --------------------------------------------------------------------------------------------
class _ContrastiveNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, temperature: float, with_loss: bool, z0, z1, z2):
        zs = [z.contiguous() for z in (z0, z1, z2)]
        for z in zs:
            _req(z, F32)
        B, D = zs[0].shape
        dev = zs[0].device
        ns = [torch.empty_like(z) for z in zs]
        inv = torch.empty((3, B), dtype=F32, device=dev)
        losses = torch.empty(3, dtype=F32, device=dev) if with_loss else None
        lse = torch.empty((3, 2, B), dtype=F32, device=dev) if with_loss else None
        P3 = C.c_void_p * 3
        lib.check(lib.load().mmf_infonce_fwd(P3(*[z.data_ptr() for z in zs]), P3(*[n.data_ptr() for n in ns]),
                                             inv.data_ptr(), _ptr(losses), _ptr(lse), B, D, temperature, lib.stream_ptr()))
        ctx.save_for_backward(*ns, inv, *([lse] if with_loss else []))
        ctx.cfg = (B, D, temperature, with_loss)
        if with_loss:
            return (*ns, *losses.unbind(0))
        return tuple(ns)

    @staticmethod
    def backward(ctx, *gs):
        B, D, temperature, with_loss = ctx.cfg
        saved = ctx.saved_tensors
        ns, inv = saved[:3], saved[3]
        lse = saved[4] if with_loss else None
        dn = [g.contiguous() if g is not None else None for g in gs[:3]]
        dl = [g.contiguous().float() if g is not None else None for g in gs[3:6]] if with_loss else [None] * 3
        dz = [torch.empty_like(n) for n in ns]
        P3 = C.c_void_p * 3
        lib.check(lib.load().mmf_infonce_bwd(P3(*[n.data_ptr() for n in ns]), inv.data_ptr(), _ptr(lse),
                                             P3(*[_ptr(g) for g in dn]), P3(*[_ptr(g) for g in dl]),
                                             P3(*[z.data_ptr() for z in dz]), B, D, temperature, lib.stream_ptr()))
        return (None, None, *dz)


def normalize_infonce(zs: Sequence[torch.Tensor], temperature: float, with_loss: bool
                      ) -> Tuple[List[torch.Tensor], Optional[List[torch.Tensor]]]:
    """zs: three f32 (B, D) projections.  Returns the L2-normalised projections and, if ``with_loss``, the
    symmetric InfoNCE losses of the pairs (0,1), (0,2), (1,2) as 0-dim tensors.  B <= 64."""
    out = _ContrastiveNCE.apply(float(temperature), bool(with_loss), *zs)
    return list(out[:3]), (list(out[3:6]) if with_loss else None)


# --------------------------------------------------------------------------------------------
# AdaptiveFusion's weighting
# --------------------------------------------------------------------------------------------
class _AdaptiveCombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp, attended, w2, b2):
        _req(hp, F32), _req(attended, F32)
        hp, attended = hp.contiguous(), attended.contiguous()
        B, d = hp.shape
        aw = torch.empty((B, 3), dtype=F32, device=hp.device)
        weighted = torch.empty((B, d), dtype=BF16, device=hp.device)
        lib.check(lib.load().mmf_adaptive_combine_fwd(hp.data_ptr(), w2.data_ptr(), b2.data_ptr(), attended.data_ptr(),
                                                      aw.data_ptr(), weighted.data_ptr(), B, d, lib.stream_ptr()))
        ctx.save_for_backward(hp, attended, aw)
        ctx.params = (w2, b2)
        return weighted, aw

    @staticmethod
    def backward(ctx, dweighted, daw):
        hp, attended, aw = ctx.saved_tensors
        w2, b2 = ctx.params
        B, d = hp.shape
        dweighted = _grad_bf16(dweighted)
        if daw is not None:
            daw = daw.contiguous().float()
        datt = torch.empty_like(attended)
        dhp = torch.empty_like(hp)
        lib.check(lib.load().mmf_adaptive_combine_bwd(hp.data_ptr(), w2.data_ptr(), attended.data_ptr(), aw.data_ptr(),
                                                      _ptr(dweighted), _ptr(daw), datt.data_ptr(), dhp.data_ptr(),
                                                      _grad_of(w2).data_ptr(), _grad_of(b2).data_ptr(), B, d,
                                                      lib.stream_ptr()))
        return dhp, datt, None, None


def adaptive_combine(hp: torch.Tensor, attended: torch.Tensor, w2: torch.nn.Parameter, b2: torch.nn.Parameter):
    """hp f32 (B, d), attended f32 (B, 3, d) -> (weighted bf16 (B, d), adaptive weights f32 (B, 3))."""
    return _AdaptiveCombine.apply(hp, attended, w2, b2)


# --------------------------------------------------------------------------------------------
# narrow linear heads (N <= 16), f32 masters
# --------------------------------------------------------------------------------------------
class _NarrowLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        _req(x, F32)
        x = x.contiguous()
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty((M, N), dtype=F32, device=x.device)
        lib.check(lib.load().mmf_linear_narrow_fwd(x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), M, N, K, lib.stream_ptr()))
        ctx.save_for_backward(x)
        ctx.params, ctx.need = (w, b), x.requires_grad
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        w, b = ctx.params
        M, K = x.shape
        N = w.shape[0]
        dy = dy.contiguous().float()
        dx = torch.empty_like(x) if ctx.need else None
        lib.check(lib.load().mmf_linear_narrow_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(), _ptr(dx), _grad_of(w).data_ptr(),
                                                   _grad_of(b).data_ptr() if b is not None else None, M, N, K, lib.stream_ptr()))
        return dx, None, None


def narrow_linear(x: torch.Tensor, layer: torch.nn.Linear) -> torch.Tensor:
    """y = x W^T + b for an nn.Linear with <= 16 outputs (fp32 in, fp32 master weights, fp32 out)."""
    if layer.weight.shape[0] > NARROW_MAX_N:
        raise ValueError("narrow_linear handles at most 16 output features")
    return _NarrowLinear.apply(x.float(), layer.weight, layer.bias)


# --------------------------------------------------------------------------------------------
# per-sample modality masks
# --------------------------------------------------------------------------------------------
class _RowMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        _req(x, F32), _req(mask, F32)
        x, mask = x.contiguous(), mask.contiguous()
        y = torch.empty_like(x)
        B, d = x.shape
        lib.check(lib.load().mmf_rowmask_apply(x.data_ptr(), mask.data_ptr(), y.data_ptr(), B, d, lib.stream_ptr()))
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = dy.contiguous().float()
        dx = torch.empty_like(dy)
        B, d = dy.shape
        lib.check(lib.load().mmf_rowmask_apply(dy.data_ptr(), mask.data_ptr(), dx.data_ptr(), B, d, lib.stream_ptr()))
        return dx, None


def rowmask(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """y[b, :] = x[b, :] * mask[b]  (fp32 (B, d), fp32 (B,))."""
    return _RowMask.apply(x.float(), mask)


# --------------------------------------------------------------------------------------------
# ModalityDropout and the training-step loss as one launch each (round 4; csrc/loss.hip)
# --------------------------------------------------------------------------------------------
def _ptr3(ts):
    return (C.c_void_p * 3)(*[t.data_ptr() for t in ts])


class _ModalityDropout(torch.autograd.Function):
    """reference models/encoders.py:289-321 on the three (B, d) f32 feature tensors: masks drawn and applied by ONE kernel
    (mmf_modality_dropout); the backward applies the saved (B, 3) masks with the same kernel."""

    @staticmethod
    def forward(ctx, t, a, v, p, site):
        xs = [x.float().contiguous() for x in (t, a, v)]
        B, d = xs[0].shape
        ys = [torch.empty_like(x) for x in xs]
        keep = torch.empty((B, 3), dtype=F32, device=xs[0].device)
        lib.check(lib.load().mmf_modality_dropout(_ptr3(xs), _ptr3(ys), keep.data_ptr(), B, d, float(p), ops.rng_state().data_ptr(),
                                                  int(site), 1, lib.stream_ptr()))
        ctx.save_for_backward(keep)
        ctx.mark_non_differentiable(keep)
        return ys[0], ys[1], ys[2], keep

    @staticmethod
    def backward(ctx, gt, ga, gv, _gk):
        keep, = ctx.saved_tensors
        B = keep.shape[0]
        ref = next(g for g in (gt, ga, gv) if g is not None)
        gs = [(g if g is not None else torch.zeros_like(ref)).float().contiguous() for g in (gt, ga, gv)]
        d = gs[0].shape[1]
        dx = [torch.empty_like(g) for g in gs]
        lib.check(lib.load().mmf_modality_dropout(_ptr3(gs), _ptr3(dx), keep.data_ptr(), B, d, 0.0, None, 0, 0, lib.stream_ptr()))
        return dx[0], dx[1], dx[2], None, None


def modality_dropout(t: torch.Tensor, a: torch.Tensor, v: torch.Tensor, p: float):
    """-> (t', a', v', keep (B, 3)); masks from the build's counter-based RNG (mmfusion.ops: dropout section)"""
    return _ModalityDropout.apply(t, a, v, float(p), ops.next_site())


_ONE: dict = {}


def loss_seed(device) -> torch.Tensor:
    """the resident d(loss)/d(loss) = 1 tensor of ``backward_from``: a backward started with it costs the fused loss no launch"""
    key = str(device)
    if key not in _ONE:
        _ONE[key] = torch.ones((), dtype=F32, device=device)
    return _ONE[key]


def backward_from(loss: torch.Tensor) -> None:
    """loss.backward() without the fill kernel that builds the unit gradient (and, for ``fusion_loss``, without the
    multiplications by it)"""
    torch.autograd.backward([loss], [loss_seed(loss.device)])


_SCALARS: dict = {}


def _resident_scalar(v: float, device) -> torch.Tensor:
    """a 0-d f32 tensor holding v, created once per (value, device): gradients of constant weight cost no fill launch"""
    key = (v, str(device))
    if key not in _SCALARS:
        _SCALARS[key] = torch.full((), v, dtype=F32, device=device)
    return _SCALARS[key]


def _rows_f32(x: torch.Tensor) -> torch.Tensor:
    """(B, C) f32 rows with unit column stride (a row-strided view passes as is: the kernels take its leading dimension)"""
    x = x.float()
    return x if x.stride(1) == 1 else x.contiguous()


class _LossTail(torch.autograd.Function):
    """The fused loss tail of ``csrc/loss.hip``, value and d/d(logits) in one launch: with ``targets``, mean CE(label
    smoothing) over (B, C) logits + sum_j w_j * extra_j (device scalars); with ``teacher``, + kd_weight * T^2 *
    KL(softmax(teacher / T) || softmax(logits / T)), batchmean (reference models/multimodal_model.py:250-256).  The
    teacher's logits get no gradient."""

    @staticmethod
    def forward(ctx, logits, targets, teacher, smoothing, temperature, kd_weight, weights, *extras):
        s = _rows_f32(logits)
        B, Cn = s.shape
        if teacher is not None:
            t = _rows_f32(teacher.detach())
            if tuple(t.shape) != (B, Cn):
                raise ValueError(f"{'distill_kl' if targets is None else 'fusion_loss_kd'}: logits {tuple(s.shape)} vs "
                                 f"teacher {tuple(t.shape)}")
        loss = torch.empty((), dtype=F32, device=s.device)
        dlog = torch.empty((B, Cn), dtype=F32, device=s.device) if ctx.needs_input_grad[0] else None
        L, rows, out = lib.load(), (s.data_ptr(), s.stride(0)), (loss.data_ptr(), _ptr(dlog), lib.stream_ptr())
        if targets is None:
            rc = L.mmf_distill_kl(*rows, t.data_ptr(), t.stride(0), B, Cn, temperature, *out)
        else:
            ex = [e.float().reshape(1) for e in extras]
            ce = (*rows, targets.data_ptr(), B, Cn, smoothing, (C.c_void_p * max(len(ex), 1))(*[e.data_ptr() for e in ex]),
                  (C.c_float * max(len(ex), 1))(*weights), len(ex))
            rc = (L.mmf_fusion_loss(*ce, *out) if teacher is None
                  else L.mmf_fusion_loss_kd(*ce, t.data_ptr(), t.stride(0), temperature, kd_weight, *out))
        lib.check(rc)
        ctx.save_for_backward(dlog)
        ctx.weights = weights
        ctx.wt = [_resident_scalar(w, s.device) for w in weights]
        return loss

    @staticmethod
    def backward(ctx, g):
        dlog, = ctx.saved_tensors
        if g.data_ptr() == loss_seed(g.device).data_ptr():       # started by backward_from: the gradient IS one
            return (dlog, None, None, None, None, None, None, *ctx.wt)
        return (None if dlog is None else dlog * g, None, None, None, None, None, None, *[g * w for w in ctx.weights])


def _targets(targets: torch.Tensor) -> torch.Tensor:
    return (targets if targets.dtype == torch.int64 else targets.long()).contiguous()


def fusion_loss(logits: torch.Tensor, targets: torch.Tensor, smoothing: float, extras, weights) -> torch.Tensor:
    """-> 0-d f32 CE(logits, targets, label_smoothing) + sum_j weights[j] * extras[j] (C <= 64)"""
    return _LossTail.apply(logits, _targets(targets), None, float(smoothing), 1.0, 1.0, [float(w) for w in weights], *extras)


def distill_kl(student_logits: torch.Tensor, teacher_logits: torch.Tensor, temperature: float) -> torch.Tensor:
    """-> 0-d f32 ``F.kl_div(log_softmax(s / T), softmax(t / T), reduction="batchmean") * T**2`` (C <= 64)"""
    return _LossTail.apply(student_logits, None, teacher_logits, 0.0, float(temperature), 1.0, [])


def fusion_loss_kd(logits: torch.Tensor, targets: torch.Tensor, smoothing: float, extras, weights,
                   teacher_logits: torch.Tensor, temperature: float, kd_weight: float) -> torch.Tensor:
    """``fusion_loss`` + kd_weight * ``distill_kl(logits, teacher_logits, temperature)``, one launch forward, none backward"""
    return _LossTail.apply(logits, _targets(targets), teacher_logits, float(smoothing), float(temperature), float(kd_weight),
                           [float(w) for w in weights], *extras)


# --------------------------------------------------------------------------------------------
# robust head of RobustMultimodalModel (csrc/small.hip mmf_robust_head_*)
# --------------------------------------------------------------------------------------------
ROBUST_MAX_B = 256
_MODALITIES = ("text", "audio", "video")


def availability_mask(available) -> int:
    """``available_modalities`` -> the kernels' argument: None -> -1 (predicted weights), a list of names -> the 3-bit mask
    (bit 0 text, 1 audio, 2 video; unknown names are ignored, [] gives 0), an int passes through."""
    if available is None:
        return -1
    if isinstance(available, int):
        return available
    return sum(1 << i for i, m in enumerate(_MODALITIES) if m in available)


class _RobustHead(torch.autograd.Function):
    """(f_t, f_a, f_v, h) -> (a, p_t, p_a, p_v, wn, y) in one launch, all six gradients back in one (see include/mmfusion.h).
    Outputs the loss ignores arrive as None (``set_materialize_grads(False)``) and cost nothing."""

    @staticmethod
    def forward(ctx, ft, fa, fv, h, avail, w2, b2, wt, bt, wa, ba, wv, bv):
        fs = [x.float().contiguous() for x in (ft, fa, fv)]
        h = h.float().contiguous()
        for x in (*fs, h):
            _req(x, F32)
        B, d = fs[0].shape
        Cn = wt.shape[0]
        if any(tuple(x.shape) != (B, d) for x in (*fs, h)):
            raise ValueError(f"robust_head: features {[tuple(x.shape) for x in fs]} / hidden {tuple(h.shape)} differ")
        dev = h.device
        a = torch.empty((B, 3), dtype=F32, device=dev)
        ps = [torch.empty((B, Cn), dtype=F32, device=dev) for _ in range(3)]
        wn = torch.empty((B, 3), dtype=F32, device=dev)
        y = torch.empty((B, Cn), dtype=F32, device=dev)
        wm, bm = (wt, wa, wv), (bt, ba, bv)
        lib.check(lib.load().mmf_robust_head_fwd(_ptr3(fs), h.data_ptr(), w2.data_ptr(), b2.data_ptr(), _ptr3(wm), _ptr3(bm),
                                                 int(avail), a.data_ptr(), _ptr3(ps), wn.data_ptr(), y.data_ptr(), B, d, Cn,
                                                 lib.stream_ptr()))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*fs, h, a, *ps, wn)
        ctx.params, ctx.avail = (w2, b2, wm, bm), int(avail)
        if avail >= 0:
            ctx.mark_non_differentiable(wn)              # constant weights: nothing flows back through them
        return a, ps[0], ps[1], ps[2], wn, y

    @staticmethod
    def backward(ctx, ga, gpt, gpa, gpv, gwn, gy):
        ft, fa, fv, h, a, pt, pa, pv, wn = ctx.saved_tensors
        w2, b2, wm, bm = ctx.params
        B, d = h.shape
        Cn = pt.shape[1]
        if ga is None and gpt is None and gpa is None and gpv is None and gwn is None and gy is None:
            return (None,) * 13

        def rows(g):
            return None if g is None else g.float().contiguous()
        g = rows(gy) if gy is not None else torch.zeros((B, Cn), dtype=F32, device=h.device)
        dps = [rows(x) for x in (gpt, gpa, gpv)]
        ga, gwn = rows(ga), (rows(gwn) if ctx.avail < 0 else None)
        need = ctx.needs_input_grad
        dfs = [torch.empty((B, d), dtype=F32, device=h.device) if need[i] else None for i in range(3)]
        # with a given mask only a direct gradient of the availability reaches the predictor
        dh = torch.empty((B, d), dtype=F32, device=h.device) if need[3] and (ctx.avail < 0 or ga is not None) else None
        dP = (C.c_void_p * 3)(*[_ptr(x) for x in dps])
        dF = (C.c_void_p * 3)(*[_ptr(x) for x in dfs])
        lib.check(lib.load().mmf_robust_head_bwd(_ptr3((ft, fa, fv)), h.data_ptr(), w2.data_ptr(), _ptr3(wm), a.data_ptr(),
                                                 _ptr3((pt, pa, pv)), wn.data_ptr(), ctx.avail, g.data_ptr(), dP, _ptr(ga),
                                                 _ptr(gwn), dF, _ptr(dh), _grad_of(w2).data_ptr(), _grad_of(b2).data_ptr(),
                                                 _ptr3([_grad_of(w) for w in wm]), _ptr3([_grad_of(b) for b in bm]),
                                                 B, d, Cn, lib.stream_ptr()))
        return (dfs[0], dfs[1], dfs[2], dh) + (None,) * 9


def robust_head(f_t: torch.Tensor, f_a: torch.Tensor, f_v: torch.Tensor, h: torch.Tensor, module, available=None):
    """The robust head of ``RobustMultimodalModel`` after its predictor's hidden layer ``h`` (f32 (B, d)): -> (availability
    (B, 3), text / audio / video predictions (B, C) each, normalised weights (B, 3), robust prediction (B, C)), f32.
    ``module`` holds ``modality_predictor`` and the three ``*_only_classifier`` layers (f32 masters in an arena);
    ``available``: None (predicted weights), a list of modality names or a 3-bit mask.  B <= 256, C <= 16, d % 4 == 0."""
    avail = availability_mask(available)
    if not 0 <= avail + 1 <= 8:
        raise ValueError(f"robust_head: availability mask {avail} (-1 or 0..7)")
    lin2 = module.modality_predictor[2]
    heads = (module.text_only_classifier, module.audio_only_classifier, module.video_only_classifier)
    if heads[0].weight.shape[0] > NARROW_MAX_N or f_t.shape[0] > ROBUST_MAX_B:
        raise ValueError(f"robust_head: C = {heads[0].weight.shape[0]} (<= {NARROW_MAX_N}), B = {f_t.shape[0]} (<= {ROBUST_MAX_B})")
    return _RobustHead.apply(f_t, f_a, f_v, h, avail, lin2.weight, lin2.bias,
                             *[t for l in heads for t in (l.weight, l.bias)])


# --------------------------------------------------------------------------------------------
# episode head of FewShotModel (csrc/fewshot.hip mmf_fewshot_*)
# --------------------------------------------------------------------------------------------
FEWSHOT_MAX_D, FEWSHOT_MAX_WAY, FEWSHOT_MAX_SHOT, FEWSHOT_MAX_Q = 1024, 64, 64, 1024


def _feat3(xs, who: str):
    fs = [x.float().contiguous() for x in xs]
    for x in fs:
        _req(x, F32)
    if any(x.dim() != 2 or x.shape != fs[0].shape for x in fs):
        raise ValueError(f"{who}: the three feature tensors must share one (rows, d) shape, got {[tuple(x.shape) for x in fs]}")
    return fs


class _FewShotPrototypes(torch.autograd.Function):
    """(t, a, v) support rows (class-major, n_way * n_shot) -> (support_features = (t + a) + v, class means) in one launch;
    the backward is one launch too, and its result is the gradient of all three inputs."""

    @staticmethod
    def forward(ctx, t, a, v, n_way, n_shot):
        fs = _feat3((t, a, v), "fewshot_prototypes")
        S, d = fs[0].shape
        sf = torch.empty((S, d), dtype=F32, device=fs[0].device)
        mean = torch.empty((n_way, d), dtype=F32, device=fs[0].device)
        lib.check(lib.load().mmf_fewshot_proto_fwd(_ptr3(fs), sf.data_ptr(), mean.data_ptr(), n_way, n_shot, d, lib.stream_ptr()))
        ctx.set_materialize_grads(False)
        ctx.dims = (n_way, n_shot, d)
        return sf, mean

    @staticmethod
    def backward(ctx, gsf, gmean):
        n_way, n_shot, d = ctx.dims
        need = ctx.needs_input_grad[:3]
        if not any(need) or (gsf is None and gmean is None):
            return (None,) * 5
        dev = (gsf if gsf is not None else gmean).device
        gm = gmean.float().contiguous() if gmean is not None else torch.zeros((n_way, d), dtype=F32, device=dev)
        gs = gsf.float().contiguous() if gsf is not None else None
        ds = torch.empty((n_way * n_shot, d), dtype=F32, device=dev)
        lib.check(lib.load().mmf_fewshot_proto_bwd(gm.data_ptr(), _ptr(gs), ds.data_ptr(), n_way, n_shot, d, lib.stream_ptr()))
        return tuple(ds if n else None for n in need) + (None, None)


class _FewShotScores(torch.autograd.Function):
    """(t, a, v) query rows, prototypes P -> (query_features = (t + a) + v, distances, softmax(-distances)) in one launch;
    dQ and dP in one launch back (the gradient of query_features, if any, is added to dQ)."""

    @staticmethod
    def forward(ctx, t, a, v, P):
        fs = _feat3((t, a, v), "fewshot_scores")
        P = P.float().contiguous()
        _req(P, F32)
        Nq, d = fs[0].shape
        n_way = P.shape[0]
        if P.dim() != 2 or P.shape[1] != d:
            raise ValueError(f"fewshot_scores: prototypes {tuple(P.shape)} against query features (.., {d})")
        dev = P.device
        qf = torch.empty((Nq, d), dtype=F32, device=dev)
        dist = torch.empty((Nq, n_way), dtype=F32, device=dev)
        pred = torch.empty((Nq, n_way), dtype=F32, device=dev)
        lib.check(lib.load().mmf_fewshot_dist_fwd(_ptr3(fs), P.data_ptr(), qf.data_ptr(), dist.data_ptr(), pred.data_ptr(),
                                                  Nq, n_way, d, lib.stream_ptr()))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(qf, P, dist, pred)
        return qf, dist, pred

    @staticmethod
    def backward(ctx, gqf, gdist, gpred):
        qf, P, dist, pred = ctx.saved_tensors
        need_q, need_p = any(ctx.needs_input_grad[:3]), ctx.needs_input_grad[3]
        Nq, d = qf.shape
        n_way = P.shape[0]
        dq = dp = None
        if gdist is not None or gpred is not None:
            dq = torch.empty((Nq, d), dtype=F32, device=qf.device) if need_q else None
            dp = torch.empty((n_way, d), dtype=F32, device=qf.device) if need_p else None
            gd = gdist.float().contiguous() if gdist is not None else None
            gp = gpred.float().contiguous() if gpred is not None else None
            lib.check(lib.load().mmf_fewshot_dist_bwd(qf.data_ptr(), P.data_ptr(), dist.data_ptr(), pred.data_ptr(), _ptr(gd),
                                                      _ptr(gp), _ptr(dq), _ptr(dp), Nq, n_way, d, lib.stream_ptr()))
        if need_q and gqf is not None:
            dq = gqf.float() if dq is None else dq + gqf.float()
        return tuple(dq if n else None for n in ctx.needs_input_grad[:3]) + (dp,)


def _fewshot_check(rows: int, d: int, who: str, n_way: int, n_shot: int = 1) -> None:
    if d % 4 or d > FEWSHOT_MAX_D or not 1 <= n_way <= FEWSHOT_MAX_WAY or not 1 <= n_shot <= FEWSHOT_MAX_SHOT:
        raise ValueError(f"{who}: d = {d} (multiple of 4, <= {FEWSHOT_MAX_D}), n_way = {n_way} (1..{FEWSHOT_MAX_WAY}), "
                         f"n_shot = {n_shot} (1..{FEWSHOT_MAX_SHOT})")
    if not 1 <= rows <= FEWSHOT_MAX_Q * FEWSHOT_MAX_SHOT:
        raise ValueError(f"{who}: {rows} rows")


def fewshot_prototypes(t: torch.Tensor, a: torch.Tensor, v: torch.Tensor, n_way: int, n_shot: int):
    """Support features (f32 (n_way * n_shot, d) each, class-major: row c * n_shot + s) -> (support_features (t + a) + v,
    class means (n_way, d)), f32.  d % 4 == 0, d <= 1024, n_way and n_shot in 1..64."""
    n_way, n_shot = int(n_way), int(n_shot)
    _fewshot_check(t.shape[0], t.shape[-1], "fewshot_prototypes", n_way, n_shot)
    if t.shape[0] != n_way * n_shot:
        raise ValueError(f"fewshot_prototypes: {t.shape[0]} support rows, n_way * n_shot = {n_way * n_shot}")
    return _FewShotPrototypes.apply(t, a, v, n_way, n_shot)


def fewshot_scores(t: torch.Tensor, a: torch.Tensor, v: torch.Tensor, prototypes: torch.Tensor):
    """Query features (f32 (Nq, d) each) and prototypes (n_way, d) -> (query_features (t + a) + v, distances (Nq, n_way)
    = cdist(query_features, prototypes), predictions = softmax(-distances)), f32.  Nq <= 1024, n_way <= 64."""
    _fewshot_check(t.shape[0], t.shape[-1], "fewshot_scores", prototypes.shape[0])
    if t.shape[0] > FEWSHOT_MAX_Q:
        raise ValueError(f"fewshot_scores: {t.shape[0]} query rows (<= {FEWSHOT_MAX_Q})")
    return _FewShotScores.apply(t, a, v, prototypes)
