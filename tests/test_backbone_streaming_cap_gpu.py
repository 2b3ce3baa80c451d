"""GPU: every streaming kernel of the native backbones past the cap of its grid, where the grid-stride loop takes a later turn.

``mmf_stream_grid`` (csrc/mmf_internal.h) gives one workgroup of THREADS = 256 lanes per 256 per-lane vectors, CAP = 2048 workgroups at
the most: TURN = 524 288 vectors (4 194 304 bf16 elements) per grid row and turn, whatever lies beyond is the ``v += stride`` turn's.
``hidden_dropout_kernel`` and ``w2v_mask_drop_kernel`` also cap gridDim.y at Y_CAP = 65 535 items and walk the rest in ``g += gridDim.y``.

Audit.  Every kernel of csrc/ whose trip count depends on a capped grid (each ``mmf_stream_grid`` call, each ``gridDim.x *`` stride, each
``g += gridDim.y``), the largest number of vectors per grid row (or units, where the kernel counts something else) that a kernel test with
NaN-pre-filled outputs reached before this file, and the trips that makes:

  kernel (file)                                  largest before this file                                          cap      trips
  bias_gelu / _bwd (vit)                         37 x 1024 / 8 = 4 736 (test_vit_gpu); 65 280 / 8 = 8 160          524 288  1
                                                 (test_gelu_domain_gpu, 255 x 256)
  bias_gelu_drop<fwd, bwd> (vit)                 447 x 512 / 8 = 28 608 (test_w2v_regularise_kernels_gpu)          524 288  1
  vit_patchify (vit)                             3 x 224 x 224 / 8 = 18 816 per image (test_vit_gpu)               524 288  1
  vit_embed_tokens (vit)                         197 x 768 / 8 = 18 912 (test_vit_gpu)                             524 288  1
  vit_embed_tokens_bwd (vit)                     145 x 768 / 8 = 13 920 (test_vit_finetune_kernels_gpu)            524 288  1
  whisper_gelu_window (whisper)                  255 x 3 x 256 / 8 = 24 480 per clip (test_gelu_domain_gpu)        524 288  1
  whisper_stem_out (whisper)                     2 x 40 x 384 / 8 = 3 840 (test_whisper_kernels_gpu); 8 160        524 288  1
  w2v_gelu_window (wav2vec2)                     127 x 3 x 256 / 8 = 12 192 per clip (test_gelu_domain_gpu)        524 288  1
  w2v_window_fold_gelu_bwd (wav2vec2)            255 x 256 / 8 = 8 160 per clip (test_gelu_domain_gpu)             524 288  1
  w2v_ln_gelu_window (wav2vec2)                  39 rows of 1024 channels, 2 a workgroup pass: 20 row blocks per   2 048    1
                                                 clip (test_w2v_ln_gpu)
                                                 (the grid is row blocks / passes, passes = N x row blocks / 2048)
  w2v_conv0_ln_gelu (wav2vec2)                   L = 4003, C0 = 512: 799 frames, 4 per workgroup: 200 workgroups   1 024    1
                                                 (test_w2v_ln_gpu)
  hidden_dropout (elementwise)                   x: 16 x 768 / 8 = 1 536; y: 5 items (test_deberta_dropout_-       524 288  1
                                                 kernels_gpu)                                                      65 535   1
  w2v_mask_drop (wav2vec2)                       x: 149 x 256 / 8 = 4 768; y: 3 items (test_w2v_regularise_-       524 288  1
                                                 kernels_gpu)                                                      65 535   1
  swap01 (lstm; its own cap of 4096)             12 x 9 x 64 / 8 = 864 chunks (test_lstm_gpu, whose outputs it     1048 576 1
                                                 allocates itself: not pre-filled); test_lstm_kernel_gpu reaches
                                                 it through lstm_ops.swap01 at T x B x In / 8 of a few thousand
  -- past their cap already, not repeated here --
  w2v_conv0_norm_gelu (wav2vec2, cap 1024)       4 119 frames, 4 per workgroup: 1 030 (test_w2v_conv0_kernels_gpu) 1 024    2
  w2v_conv0_stats / _bwd_stats / _bwd_wgrad      600 frames on 128 frame slots (test_w2v_feature_encoder_-        128      5
  (wav2vec2: frame slots, MMF_W2V_STATS_SLOTS)   kernels_gpu), 4 119 on 128 (test_w2v_conv0_kernels_gpu)                    33
  elementwise.hip casts, add3 / addn, dropout,   test_streaming_small_gpu (N_CAP + ..., the unrolled loop, the     524 288  3
  relu_bwd, meanpool_bwd, zero_ranges; small.hip remainder loop and the tail), test_keyed_masks_gpu
  and optim.hip                                  ("n = 2048 x 256 + 1")
  prep.hip                                       test_prep_gpu ("the grid-stride loop takes a second turn")        524 288  2
  deberta_embed_grad (deberta, line 423)         test_deberta_embed_grad_kernels_gpu                               -        2
  -- seen, out of scope --
  gemm7_body (gemm7, line 260)                   a persistent tile walk, ``round * nwg + ...``: the trips of a workgroup depend on gridDim.x,
                                                 but it is no streaming kernel and matches none of the three patterns; its rounds, the partial
                                                 last one included, are pinned by test_gemm7_tile_forms_gpu and test_kernel_forms_gpu

Every case here states its size from the constants and asserts that it is past the cap; the ``SIZE`` line it prints says how many vectors
(items, row blocks) fall in the later turns.  Rules of every case: outputs NaN-filled between NaN guard regions, NaN padding columns where
ld > cols, guards and padding bit-identical afterwards, inputs untouched; the float64 (or exact) reference is evaluated over the WHOLE
output under the bound of the kernel's existing test, imported from it (tests/gelu_domain.py's allowance for the GELU family,
test_w2v_ln_gpu's ``_check`` for the layer-norm kernels, ``fold_bound`` of test_w2v_feature_encoder_kernels_gpu, ``stem_out_allowance``
of test_whisper_kernels_gpu, test_vit_finetune_kernels_gpu's ``F32_TOL``, bit equality for patchify, embed_tokens, swap01 and every
dropout mask and value); the same data launched in pieces that each fit in one turn (the launches pinned
before this file) gives the long launch's bits; two long launches give the same bits.  ``PARITY`` lines carry err / bound (0 for a bit
equality that held); profiles/backbone_streaming_past_cap.txt is those lines from an MI355X.

Two sizes per kernel: the cap plus a ragged handful (two turns), and two full turns plus a ragged third (``_past(...) == 3``) wherever a
tensor stays near 17 MB, since a loop that takes exactly one extra turn passes every two-turn case.  Exempt from the larger size:
``vit_patchify`` (its f32 pixels would be 67 MB), ``vit_embed_tokens`` and its backward (the f32 position table and its gradient would be
34 MB, the backward's five images of bf16 84 MB) and ``swap01`` (a cap of 4096 workgroups: 34 MB of bf16, 67 MB of f32).  The y loops
take their third trip at 131 071 items.

Two kernels have no piecewise form in x: an element of ``hidden_dropout`` / ``w2v_mask_drop`` is keyed by its index INSIDE the item, and an
entry cannot start an item in the middle.  Their x loops are held to the restated mask and the exact value instead (stronger than a
piecewise equality), their y loops also piecewise, ``item0`` advanced.

Out of reach, not tested: the 2^31-vector row split of ``bias_gelu_run`` (csrc/vit.hip) needs 32 GiB of bf16; the 2^32-element wrap of a
dropout index needs an 8 GiB tensor (tests/test_keyed_masks_gpu.py notes the same)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as A  # noqa: E402
import deberta_dropout_ref as DD  # noqa: E402
import gelu_domain as D  # noqa: E402
import keyed_dropout_ref as KD  # noqa: E402
import vit_ref  # noqa: E402
import w2v_ref  # noqa: E402
import w2v_regularise_ref as WR  # noqa: E402
import whisper_ref  # noqa: E402
from helpers import _lib  # noqa: E402
from test_attention_paths_gpu import rec  # noqa: E402,F401
from test_deberta_dropout_kernels_gpu import _fma_bf16  # noqa: E402
from test_gelu_domain_gpu import GUARD, Guarded, Unchanged, _bias, _dev, _v  # noqa: E402
from test_vit_finetune_kernels_gpu import F32_TOL  # noqa: E402
from test_w2v_feature_encoder_kernels_gpu import _fold_case, fold_bound  # noqa: E402
from test_w2v_ln_gpu import EPS, _affine, _check, _ln_gelu  # noqa: E402
from test_w2v_regularise_kernels_gpu import _scale_bf16  # noqa: E402
from test_whisper_kernels_gpu import stem_out_allowance  # noqa: E402
from w2v_kernel_checks import bits  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
THREADS, CAP = 256, 2048                 # VIT_THREADS / W2V_THREADS / EW_THREADS; mmf_stream_grid's cap
TURN = THREADS * CAP                     # vectors of one grid row that one turn of the loop covers
Y_CAP = 65535                            # gridDim.y of hidden_dropout_kernel and w2v_mask_drop_kernel
CONV0_CAP, SWAP_CAP = 1024, 4096         # mmf_w2v_conv0_ln_gelu's and mmf_swap01's own workgroup caps
STATE, SITE, ITEM0, P = (0x1234567 << 32) | 0x89ABCDEF, 4, 5, 0.1
THRESH = A.mmf_drop_thresh(P)
INV = A.inv_keep_of(THRESH)


# ---- what every case uses ------------------------------------------------------------------------------------------------------
def _past(what, nvec, cap=TURN, unit="vectors per grid row"):
    """asserts that ``nvec`` is past the cap and says what falls in the later turns -> the number of turns"""
    assert nvec > cap, f"{what}: {nvec} {unit} do not cross the cap of {cap}"
    turns = -(-nvec // cap)
    print(f"SIZE {what}: {nvec} {unit} = {nvec // cap} full turn(s) of {cap} + {nvec % cap}; {nvec - cap} in the later turn(s)")
    return turns


def _fits(nvec, cap=TURN):
    assert 0 < nvec <= cap, f"a piece of {nvec} does not fit in one turn of {cap}"


def _split(n, parts):
    """[0, n) in ``parts`` nearly equal ranges"""
    edges = [n * i // parts for i in range(parts + 1)]
    return list(zip(edges[:-1], edges[1:]))


def _same(rec, name, got, want):
    got, want = bits(got.cpu()), bits(want.cpu())
    ok = got.shape == want.shape and bool(torch.equal(got, want))
    rec(name, 0.0 if ok else float("inf"))
    assert ok, f"{name}: {int((got != want).sum()) if got.shape == want.shape else 'all'} elements differ"


def _hold(rec, name, ratio, v):
    w, at, fails = D.report(name, ratio, v)
    rec(name, w)
    assert fails == 0, f"{name}: {fails} of {ratio.numel()} outputs over the allowance, worst {w:.3f} at v = {at!r}"


def _bound(rec, name, err, bound):
    r = float((err / bound.clamp_min(1e-300)).max()) if bool(torch.isfinite(err).all()) else float("inf")
    rec(name, r)
    assert r <= 1.0, f"{name}: worst error / bound {r:.3f}"


def _state():
    return KD.state_tensor(STATE, "cuda")


def _drop(p=P, item0=ITEM0):
    return (p, _state() if p else None, SITE, item0)


def _nan(shape, dtype=BF16):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _signed(shape, seed):
    """bf16 values of magnitude 1 .. 2 and either sign: never zero, so a zero in a product with them is a dropped element"""
    g = torch.Generator().manual_seed(seed)
    return ((1.0 + torch.rand(shape, generator=g)) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)).to(BF16)


# =================================================================================== csrc/vit.hip: the GELU family
COLS, LD = 1032, 1040                    # cv = 129 vectors a row (odd: v / cv is no shift), 8 NaN padding columns
CV = COLS // 8
ROWS = 4070                              # 525 030 vectors: 742 past the first turn, which begins inside row 4064
ROWS3 = 8130                             # 1 048 770 vectors: two full turns and 194 vectors of a third; 16.9 MB a tensor
IPR = 5                                  # rows per item of the dropout entries: 814 (1626) items, row 4065 = item 813's first lies in turn two
SIZES = pytest.mark.parametrize("rows", [ROWS, ROWS3], ids=["cap-plus", "two-turns-plus"])


@functools.lru_cache(maxsize=None)
def _x(rows):
    """the pre-activation rows, both tails of the GELU included; shared and never written"""
    return (3.0 * torch.randn(rows, COLS, generator=torch.Generator().manual_seed(rows))).clamp(-9.5, 9.5).to(BF16)


@functools.lru_cache(maxsize=None)
def _keep(rows):
    items = rows // IPR
    keep = np.concatenate([KD.gemm_keep(STATE, SITE, ITEM0 + g, IPR, COLS, THRESH) for g in range(items)], axis=0)
    keep = torch.from_numpy(np.ascontiguousarray(keep))
    assert keep.shape == (rows, COLS) and bool(keep.any()) and not bool(keep.all())
    return keep


def _row_pieces(rows):
    pieces = _split(rows, -(-rows * CV // TURN) + 1)
    for a, b in pieces:
        _fits((b - a) * CV)
    return pieces


@pytest.mark.parametrize("bias", ["none", "rand"])
@SIZES
def test_bias_gelu_in_place_and_out_of_place(rec, rows, bias):  # noqa: F811
    lib, x, b = _lib(), _x(rows), _bias(bias, COLS)
    assert _past(f"bias_gelu rows={rows}", rows * CV) == (2 if rows == ROWS else 3)
    bd, v = _dev(b), _v(x, b)
    h, inplace, g = Guarded(rows, COLS, LD, init=x), Guarded(rows, COLS, LD, init=x), Guarded(rows, COLS, LD)
    ins = Unchanged(h.flat, bd)
    lib.bias_gelu_to(h.v, bd, g.v)
    lib.bias_gelu(inplace.v, bd)
    ins.check()
    assert h.intact() and inplace.intact() and g.intact()
    got = g.host()
    _hold(rec, f"bias_gelu_to bias={bias}", D.ratio_fwd(got, v), v)
    _same(rec, "in-place", inplace.host(), got)
    pieces, again = Guarded(rows, COLS, LD), Guarded(rows, COLS, LD)
    for r0, r1 in _row_pieces(rows):
        lib.bias_gelu_to(h.v[r0:r1], bd, pieces.v[r0:r1])
    lib.bias_gelu_to(h.v, bd, again.v)
    ins.check()
    assert pieces.intact() and again.intact()
    _same(rec, "pieces", pieces.host(), got)
    _same(rec, "again", again.host(), got)


@pytest.mark.parametrize("bias", ["none", "rand"])
@SIZES
def test_bias_gelu_bwd_separate_and_aliased(rec, rows, bias):  # noqa: F811
    lib, x, b, d = _lib(), _x(rows), _bias(bias, COLS), _signed((rows, COLS), 7)
    assert _past(f"bias_gelu_bwd rows={rows}", rows * CV) == (2 if rows == ROWS else 3)
    bd, v = _dev(b), _v(x, b)
    h, g, dh, alias = Guarded(rows, COLS, LD, init=x), Guarded(rows, COLS, LD, init=d), Guarded(rows, COLS, LD), Guarded(rows, COLS, LD, init=d)
    ins = Unchanged(h.flat, g.flat, bd)
    lib.bias_gelu_bwd(g.v, h.v, bd, dh.v)
    lib.bias_gelu_bwd(alias.v, h.v, bd, alias.v)
    ins.check()
    assert h.intact() and g.intact() and dh.intact() and alias.intact()
    got = dh.host()
    _hold(rec, f"bias_gelu_bwd bias={bias}", D.ratio_bwd(got, v, d), v)
    _same(rec, "aliased", alias.host(), got)
    pieces, again = Guarded(rows, COLS, LD), Guarded(rows, COLS, LD)
    for r0, r1 in _row_pieces(rows):
        lib.bias_gelu_bwd(g.v[r0:r1], h.v[r0:r1], bd, pieces.v[r0:r1])
    lib.bias_gelu_bwd(g.v, h.v, bd, again.v)
    ins.check()
    assert pieces.intact() and again.intact()
    _same(rec, "pieces", pieces.host(), got)
    _same(rec, "again", again.host(), got)


def _item_boundary_in_turn_two():
    """a row that begins an item and lies past the first turn: the key changes there, inside the later turn"""
    r = -(-TURN // CV // IPR) * IPR
    while r * CV < TURN:
        r += IPR
    assert r % IPR == 0 and TURN <= r * CV < ROWS * CV and ROWS % IPR == 0 and ROWS3 % IPR == 0
    return r


@pytest.mark.parametrize("bwd", [False, True], ids=["drop_to", "drop_bwd"])
@SIZES
def test_bias_gelu_drop_both_directions(rec, rows, bwd):  # noqa: F811
    lib, x, b, keep = _lib(), _x(rows), _bias("rand", COLS), _keep(rows)
    turns = _past(f"bias_gelu_drop rows={rows}", rows * CV)
    assert turns == (2 if rows == ROWS else 3)
    items, edge = rows // IPR, _item_boundary_in_turn_two()
    print(f"SIZE bias_gelu_drop: {items} items of {IPR} rows; row {edge} begins item {edge // IPR} inside turn two")
    bd, v = _dev(b), _v(x, b)
    d = _signed((rows, COLS), 8)
    h, g, out = Guarded(rows, COLS, LD, init=x), Guarded(rows, COLS, LD, init=d), Guarded(rows, COLS, LD)
    ins = Unchanged(h.flat, g.flat, bd)

    def run(to, r0=0, r1=rows, p=P):
        dr = _drop(p, ITEM0 + r0 // IPR)
        if bwd:
            lib.bias_gelu_drop_bwd(g.v[r0:r1], h.v[r0:r1], bd, to.v[r0:r1], (r1 - r0) // IPR, dr)
        else:
            lib.bias_gelu_drop_to(h.v[r0:r1], bd, to.v[r0:r1], (r1 - r0) // IPR, dr)
    run(out)
    ins.check()
    assert h.intact() and g.intact() and out.intact()
    got = out.host()
    assert bool((v != 0).all())
    rec("mask", 0.0 if torch.equal(got.float() != 0, keep) else float("inf"))
    assert torch.equal(got.float() != 0, keep), "the kept set is not the restated one"
    ratio = D.ratio_bwd(got, v, d, scale=INV) if bwd else D.ratio_fwd(got, v, scale=INV)
    _hold(rec, "kept elements", ratio[keep], v[keep])
    pieces, again, zero, plain = (Guarded(rows, COLS, LD) for _ in range(4))
    for i0, i1 in _split(items, turns + 1):
        _fits((i1 - i0) * IPR * CV)
        run(pieces, i0 * IPR, i1 * IPR)
    run(again)
    run(zero, p=0.0)
    if bwd:
        lib.bias_gelu_bwd(g.v, h.v, bd, plain.v)
    else:
        lib.bias_gelu_to(h.v, bd, plain.v)
    ins.check()
    assert pieces.intact() and again.intact() and zero.intact() and plain.intact()
    _same(rec, "pieces", pieces.host(), got)
    _same(rec, "again", again.host(), got)
    _same(rec, "p=0 is the plain kernel", zero.host(), plain.host())


# =================================================================================== csrc/vit.hip: patches and tokens
def test_patchify_is_unfold_with_one_rounding(rec):  # noqa: F811
    lib = _lib()
    N, C, H, W, Pp = 2, 3, 1184, 1184, 16
    per_image = C * H * W // 8
    _past("vit_patchify", per_image)
    gh, gw, K = H // Pp, W // Pp, C * Pp * Pp
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(3))
    xd = x.cuda()
    out, again, pieces = (Guarded(N * gh * gw, K) for _ in range(3))
    ins = Unchanged(xd)
    lib.vit_patchify(xd, out.v, N, C, H, W, Pp)
    lib.vit_patchify(xd, again.v, N, C, H, W, Pp)
    for n in range(N):                                     # image n's later turn starts from blockIdx.y x the per-image stride
        for y0, y1 in _split(gh, 2):
            _fits(C * (y1 - y0) * Pp * W // 8)
            part = xd[n:n + 1, :, y0 * Pp:y1 * Pp].contiguous()
            lib.vit_patchify(part, pieces.v[(n * gh + y0) * gw:(n * gh + y1) * gw], 1, C, (y1 - y0) * Pp, W, Pp)
    ins.check()
    assert out.intact() and again.intact() and pieces.intact()
    want = vit_ref.patchify(x, Pp).to(BF16)
    unfold = torch.nn.functional.unfold(x, kernel_size=Pp, stride=Pp).transpose(1, 2).reshape(-1, K).to(BF16)
    assert torch.equal(bits(want), bits(unfold))
    _same(rec, "patches", out.host(), want)
    _same(rec, "pieces", pieces.host(), out.host())
    _same(rec, "again", again.host(), out.host())


def test_embed_tokens_is_f32_add_with_one_rounding(rec):  # noqa: F811
    lib = _lib()
    N, T, d = 2, 4097, 1024
    _past("vit_embed_tokens", T * d // 8)
    g = torch.Generator().manual_seed(T)
    pe = torch.randn(N * (T - 1), d, generator=g).to(BF16)
    cls, pos = torch.randn(d, generator=g), torch.randn(T, d, generator=g)
    ped, cd, pd = pe.cuda(), cls.cuda(), pos.cuda()
    tok, again, pieces = (Guarded(N * T, d) for _ in range(3))
    ins = Unchanged(ped, cd, pd)
    lib.vit_embed_tokens(ped, cd, pd, tok.v, N, T, d)
    lib.vit_embed_tokens(ped, cd, pd, again.v, N, T, d)
    # rows a .. b - 1 of image n as a launch of their own: the row before a patch row stands where the CLS row stands, as f32 (exact)
    for n in range(N):
        for a, b in _split(T, 2):
            _fits((b - a) * d // 8)
            first = cd if a == 0 else ped[n * (T - 1) + a - 1].float()
            lib.vit_embed_tokens(ped[n * (T - 1) + a:n * (T - 1) + b - 1], first, pd[a:b], pieces.v[n * T + a:n * T + b], 1, b - a, d)
    ins.check()
    assert tok.intact() and again.intact() and pieces.intact()
    want = (torch.cat([cls.expand(N, 1, d), pe.float().view(N, T - 1, d)], dim=1) + pos).to(BF16).view(N * T, d)
    _same(rec, "tokens", tok.host(), want)                 # the CLS row is vector 0 .. 127, the last rows are the later turn's
    _same(rec, "pieces", pieces.host(), tok.host())
    _same(rec, "again", again.host(), tok.host())


def test_embed_tokens_bwd_ordered_f32_sum(rec):  # noqa: F811
    lib = _lib()
    N, T, d = 5, 4097, 1024                                # four images unrolled and one in the remainder loop
    _past("vit_embed_tokens_bwd", T * d // 8)
    gen = torch.Generator().manual_seed(41)
    g = torch.randn(N, T, d, generator=gen).to(BF16)
    c0, p0 = 3.0 * torch.randn(d, generator=gen), 3.0 * torch.randn(T, d, generator=gen)       # the kernel accumulates onto these
    gd = g.cuda()
    ins = Unchanged(gd)

    def run(gpart, c_init, p_init, Tp):
        dcls, dpos = Guarded(1, d, dtype=F32, init=c_init), Guarded(Tp, d, dtype=F32, init=p_init)
        dpe = Guarded(N * (Tp - 1), d)
        lib.vit_embed_tokens_bwd(gpart, dcls.flat[GUARD:GUARD + d], dpos.flat[GUARD:GUARD + Tp * d], dpe.v, N, Tp, d)
        torch.cuda.synchronize()
        assert dcls.intact() and dpos.intact() and dpe.intact()
        return dcls.host().view(d), dpos.host(), dpe.host().view(N, Tp - 1, d)
    dcls, dpos, dpe = run(gd, c0, p0, T)
    s = torch.zeros(T, d)
    for n in range(N):                                     # the kernel's chain: images in order, f32
        s = s + g[n].float()
    _same(rec, "dpos", dpos, p0 + s)
    _same(rec, "dcls", dcls, c0 + s[0])
    _same(rec, "dpatch_emb", dpe, g[:, 1:])
    g64 = g.double()
    _bound(rec, "dpos against float64", (dpos.double() - (g64.sum(0) + p0)).abs(), F32_TOL * (g64.abs().sum(0) + p0.abs()))
    _bound(rec, "dcls against float64", (dcls.double() - (g64[:, 0].sum(0) + c0)).abs(), F32_TOL * (g64[:, 0].abs().sum(0) + c0.abs()))
    # positions a .. b - 1 as a launch of their own, one row earlier so that row a is not taken for the CLS row
    for a, b in _split(T, 2):
        lo = max(a - 1, 0)
        _fits((b - lo) * d // 8)
        pc, pp, ppe = run(gd[:, lo:b].contiguous(), c0, p0[lo:b], b - lo)
        _same(rec, "pieces dpos", pp[a - lo:], dpos[a:b])
        _same(rec, "pieces dpatch_emb", ppe, dpe[:, lo:b - 1])          # token rows lo + 1 .. b - 1
        if a == 0:
            _same(rec, "pieces dcls", pc, dcls)
    again = run(gd, c0, p0, T)
    for name, t, w in zip(("dcls", "dpos", "dpatch_emb"), again, (dcls, dpos, dpe)):
        _same(rec, f"again {name}", t, w)
    ins.check()


# =================================================================================== csrc/whisper.hip: the stem
def _stem_inputs(shape, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = (3.0 * torch.randn(shape, generator=g)).clamp(-9.0, 9.0).to(BF16)
    return x, (0.2 * torch.randn(C, generator=g)).clamp(-0.5, 0.5)


@pytest.mark.parametrize("N,T_in,turns", [(2, 2199, 2), (1, 4369, 3)], ids=["cap-plus", "two-turns-plus"])
def test_whisper_gelu_window(rec, N, T_in, turns):  # noqa: F811
    """T_in odd: row 0's first tap and the last row's last tap are padding, and the last row is the last turn's.  One clip of 4369
    frames is 2185 rows: 1 048 800 vectors, 16.8 MB"""
    lib = _lib()
    C, k, s, pad = 1280, 3, 2, 1
    T_out = (T_in + 2 * pad - k) // s + 1
    rowv = k * C // 8
    assert _past(f"whisper_gelu_window N={N} T_in={T_in}", T_out * rowv) == turns
    x, bias = _stem_inputs((N, T_in, C), C, 11)
    xd, bd = x.cuda(), bias.cuda()
    out, again = Guarded(N * T_out, k * C), Guarded(N * T_out, k * C)
    ins = Unchanged(xd, bd)
    lib.whisper_gelu_window(xd, bd, out.v, N, T_in, C, k, s, pad)
    lib.whisper_gelu_window(xd, bd, again.v, N, T_in, C, k, s, pad)
    ins.check()
    assert out.intact() and again.intact()
    v = x.float() + bias                                   # the f32 sum the kernel forms, exactly
    act = D.gelu64(v)
    want, allow = whisper_ref.window_form(act, k, s, pad), whisper_ref.window_form(D.allow_fwd(v, act), k, s, pad)
    inside = whisper_ref.window_form(torch.ones(N, T_in, C, dtype=F64), k, s, pad) > 0
    assert not bool(inside[:, 0, :C].any()) and not bool(inside[:, -1, -C:].any()) and int((~inside).sum()) == 2 * N * C
    assert (T_out - 1) * rowv + (k - 1) * C // 8 >= (turns - 1) * TURN, "the padding tap of the last row must lie in the last turn"
    got = out.host().view(N, T_out, k * C)
    rec("padding is zero bits", 0.0 if not bool(bits(got)[~inside].any()) else float("inf"))
    assert not bool(bits(got)[~inside].any()), "a padding tap is not all zero bits"
    _bound(rec, "inside the clip", (got.double() - want).abs()[inside], allow[inside])
    _same(rec, "again", again.host(), out.host())
    # output rows t0 .. t1 - 1 of every clip from a launch of their own.  A piece that does not begin the clip starts one row early:
    # its row 0 is padded on the left, which is wrong in the middle of a clip, and is dropped.  A piece that does not end the clip
    # stops at frame s t1 - 1, the last its rows read (k = 3, s = 2, pad = 1), so nothing of it is padded on the right
    for t0, t1 in _split(T_out, turns):
        lo, hi, drop = (s * (t0 - 1) if t0 else 0), (T_in if t1 == T_out else s * t1), (1 if t0 else 0)
        rows = t1 - t0 + drop
        _fits(rows * rowv)
        assert (hi - lo + 2 * pad - k) // s + 1 == rows
        piece = Guarded(N * rows, k * C)
        lib.whisper_gelu_window(xd[:, lo:hi].contiguous(), bd, piece.v, N, hi - lo, C, k, s, pad)
        assert piece.intact()
        _same(rec, "pieces", piece.host().view(N, rows, k * C)[:, drop:], got[:, t0:t1])


def test_whisper_stem_out(rec):  # noqa: F811
    """T = 20: row 3280 begins a clip (row % T wraps to 0) past the first turn, which ends inside row 3276"""
    lib = _lib()
    rows, T, d = 3300, 20, 1280
    dv = d // 8
    _past("whisper_stem_out", rows * dv)
    wrap = -(-TURN // dv // T) * T
    assert TURN <= wrap * dv < rows * dv and rows % T == 0
    x, bias = _stem_inputs((rows, d), d, 12)
    pos = torch.randn(T, d, generator=torch.Generator().manual_seed(13))
    xd, bd, pd = x.cuda(), bias.cuda(), pos.cuda()
    out, inplace, again, pieces = Guarded(rows, d), Guarded(rows, d, init=x), Guarded(rows, d), Guarded(rows, d)
    ins = Unchanged(xd, bd, pd)
    lib.whisper_stem_out(xd, bd, pd, out.v, T)
    lib.whisper_stem_out(inplace.v, bd, pd, inplace.v, T)
    lib.whisper_stem_out(xd, bd, pd, again.v, T)
    for c0, c1 in _split(rows // T, 3):
        _fits((c1 - c0) * T * dv)
        lib.whisper_stem_out(xd[c0 * T:c1 * T], bd, pd, pieces.v[c0 * T:c1 * T], T)
    ins.check()
    assert out.intact() and inplace.intact() and again.intact() and pieces.intact()
    v = x.float() + bias
    act = D.gelu64(v)
    want = act + pos.double().repeat(rows // T, 1)
    tol = stem_out_allowance(v, act, want)
    got = out.host()
    _bound(rec, "stem_out", (got.double() - want).abs(), tol)
    _same(rec, "in place", inplace.host(), got)
    _same(rec, "pieces", pieces.host(), got)
    _same(rec, "again", again.host(), got)


def test_whisper_stem_out_two_turns_and_a_third(rec):  # noqa: F811
    lib = _lib()
    rows, T, d = 6560, 1640, 1280                          # 1 049 600 vectors; 16.8 MB a tensor
    assert _past("whisper_stem_out", rows * d // 8) == 3
    x, bias = _stem_inputs((rows, d), d, 14)
    pos = torch.randn(T, d, generator=torch.Generator().manual_seed(15))
    xd, bd, pd = x.cuda(), bias.cuda(), pos.cuda()
    out, again = Guarded(rows, d), Guarded(rows, d)
    ins = Unchanged(xd, bd, pd)
    lib.whisper_stem_out(xd, bd, pd, out.v, T)
    lib.whisper_stem_out(xd, bd, pd, again.v, T)
    ins.check()
    assert out.intact() and again.intact()
    v = x.float() + bias
    act = D.gelu64(v)
    want = act + pos.double().repeat(rows // T, 1)
    tol = stem_out_allowance(v, act, want)
    _bound(rec, "stem_out", (out.host().double() - want).abs(), tol)
    _same(rec, "again", again.host(), out.host())


# =================================================================================== csrc/wav2vec2.hip: the window forms
@pytest.mark.parametrize("N,T_in,turns", [(2, 5463, 2), (1, 10925, 3)], ids=["cap-plus", "two-turns-plus"])
def test_w2v_gelu_window(rec, N, T_in, turns):  # noqa: F811
    """one clip of 10 925 frames is 5462 rows: 1 048 704 vectors, 16.8 MB"""
    lib = _lib()
    C, k, s = 512, 3, 2
    T_out = (T_in - k) // s + 1
    rowv = k * C // 8
    assert _past(f"w2v_gelu_window N={N} T_in={T_in}", T_out * rowv) == turns
    x = (3.0 * torch.randn(N, T_in, C, generator=torch.Generator().manual_seed(21))).clamp(-9.5, 9.5).to(BF16)
    xd = x.cuda()
    out, again = Guarded(N * T_out, k * C), Guarded(N * T_out, k * C)
    ins = Unchanged(xd)
    lib.w2v_gelu_window(xd, out.v, N, T_in, C, k, s)
    lib.w2v_gelu_window(xd, again.v, N, T_in, C, k, s)
    ins.check()
    assert out.intact() and again.intact()
    v = w2v_ref.window(x.float(), k, s)
    got = out.host().view(N, T_out, k * C)
    _hold(rec, "w2v_gelu_window", D.ratio_fwd(got, v), v)
    _same(rec, "again", again.host(), out.host())
    for t0, t1 in _split(T_out, turns):                        # output rows t0 .. t1 - 1 read the frames s t0 .. s (t1 - 1) + k - 1
        _fits((t1 - t0) * rowv)
        piece = Guarded(N * (t1 - t0), k * C)
        part = xd[:, s * t0:s * (t1 - 1) + k].contiguous()
        lib.w2v_gelu_window(part, piece.v, N, part.shape[1], C, k, s)
        assert piece.intact()
        _same(rec, "pieces", piece.host().view(N, t1 - t0, k * C), got[:, t0:t1])


FOLD_CASES = [(3, 2, 8194, 2, 2), (2, 2, 8195, 2, 2), (2, 2, 16387, 1, 3)]


@pytest.mark.parametrize("k,s,T_in,N,turns", FOLD_CASES, ids=["k3s2", "k2s2", "k2s2-two-turns-plus"])
def test_w2v_window_fold_gelu_bwd(rec, k, s, T_in, N, turns):  # noqa: F811
    """every shape leaves its last frame unread (an exact zero, written in the last turn) behind a frame that is read there.  One clip
    of 16 387 frames is 1 048 768 vectors, 16.8 MB"""
    lib = _lib()
    C = 512
    c = _fold_case(k, s, T_in, C, N)                       # tests/test_w2v_feature_encoder_kernels_gpu.py's case and float64 autograd
    T_out, last = c["T_out"], c["last"]
    cv = C // 8
    assert c["x"].shape[0] == N and _past(f"w2v_window_fold_gelu_bwd k={k} T_in={T_in}", T_in * cv) == turns
    assert last == T_in - 2 and last * cv >= (turns - 1) * TURN, "a frame that is read and one that is not, both in the last turn"
    xd, dwd = c["x"].cuda(), c["dwin"].cuda()
    dx, again, alias = Guarded(N * T_in, C), Guarded(N * T_in, C), Guarded(N * T_in, C, init=c["x"])
    ins = Unchanged(xd, dwd)
    lib.w2v_window_fold_gelu_bwd(dwd, xd, dx.v, N, T_in, C, k, s)
    lib.w2v_window_fold_gelu_bwd(dwd, xd, again.v, N, T_in, C, k, s)
    lib.w2v_window_fold_gelu_bwd(dwd, alias.v, alias.v, N, T_in, C, k, s)
    ins.check()
    assert dx.intact() and again.intact() and alias.intact()
    got = dx.host().view(N, T_in, C)
    _bound(rec, "dx", (got.double() - c["dx"]).abs(), fold_bound(c))
    rec("unread frames are zero bits", 0.0 if not bool(bits(got)[:, last + 1:].any()) else float("inf"))
    assert not bool(bits(got)[:, last + 1:].any()) and not bool(c["dx"][:, last + 1:].any())
    _same(rec, "again", again.host(), dx.host())
    _same(rec, "dx in the place of x", alias.host(), dx.host())
    # frames f0 .. f1 - 1 from a launch on the windows that read them, t_lo .. t_hi, and the frames those windows cover; of the
    # frames a piece holds only some windows of (before f0, from f1 on) nothing is kept
    edges = [T_in * i // (turns + 1) // s * s for i in range(turns + 1)] + [T_in]
    for f0, f1 in zip(edges[:-1], edges[1:]):
        t_lo, t_hi = max(-(-(f0 - k + 1) // s), 0), min((f1 - 1) // s, T_out - 1)
        a, b = s * t_lo, (T_in if f1 == T_in else s * t_hi + k)
        _fits((b - a) * cv)
        assert (b - a - k) // s + 1 == t_hi - t_lo + 1
        piece = Guarded(N * (b - a), C)
        lib.w2v_window_fold_gelu_bwd(dwd[:, t_lo:t_hi + 1].contiguous(), xd[:, a:b].contiguous(), piece.v, N, b - a, C, k, s)
        assert piece.intact()
        _same(rec, "pieces", piece.host().view(N, b - a, C)[:, f0 - a:f1 - a], got[:, f0:f1])


# =================================================================================== csrc/wav2vec2.hip: the layer-norm family
def _ln_grid(N, T_in, C, k, s):
    """mmf_w2v_ln_gelu_window's launch -> (T_out, row blocks, passes, gridDim.x, the trips of workgroup 0)"""
    T_out = (T_in - k) // s + 1 if k else T_in
    T_read = s * (T_out - 1) + k if k else T_in
    rpb = THREADS // (C // 8)
    row_blocks = -(-T_read // rpb)
    passes = min(max(N * row_blocks // CAP, 1), 8)
    grid = min(max(-(-row_blocks // passes), 1), CAP)
    return T_out, row_blocks, passes, grid, -(-row_blocks // grid)


LN_CASES = [("cap", 1, 8202, 3, 2), ("passes", 2, 8200, 2, 2), ("rows-in-place", 1, 8201, 0, 0), ("three-trips", 1, 16394, 2, 2)]


@pytest.mark.parametrize("name,N,T_in,k,s", LN_CASES, ids=[c[0] for c in LN_CASES])
def test_w2v_ln_gelu_window(rec, name, N, T_in, k, s):  # noqa: F811
    """cap: 2051 row blocks of 4 rows on 2048 workgroups, three of which take a second trip (and row 8201 is read by no window);
    passes: N x row blocks = 4100 >= 4096, so the grid is 1025 workgroups a clip of two trips each; rows-in-place: the k = 0 form
    on x itself, 8201 rows, so the last row block is ragged and a second trip's; three-trips: one clip of 4099 row blocks, which asks
    for two passes and so for 2050 workgroups, capped at 2048: two full trips and three workgroups in a third (16.8 MB out)"""
    lib = _lib()
    C = 512
    T_out, row_blocks, passes, grid, trips = _ln_grid(N, T_in, C, k, s)
    if name == "passes":
        assert N * row_blocks >= 2 * CAP and passes >= 2 and grid < CAP and trips == passes
    elif name == "three-trips":
        assert passes == 2 and grid == CAP and _past(f"w2v_ln_gelu_window {name}", row_blocks, CAP, "row blocks per clip") == 3 == trips
    else:
        assert passes == 1 and grid == CAP
        _past(f"w2v_ln_gelu_window {name}", row_blocks, CAP, "row blocks per clip")
    print(f"SIZE w2v_ln_gelu_window {name}: {row_blocks} row blocks a clip, {passes} pass(es), {grid} workgroups, {trips} trips; "
          f"{row_blocks - grid} row blocks in the later trips")
    assert trips >= 2
    g = torch.Generator().manual_seed(T_in + C)
    x = (3.0 * torch.randn(N, T_in, C, generator=g) + 0.5).to(BF16)
    gamma, beta = _affine(C, g, False)
    want, y, terms = ((w2v_ref.window(t, k, s) if k else t) for t in _ln_gelu(x.double(), gamma, beta))
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()

    def run(src, Tp, in_place):
        """one launch on (N, Tp, C) rows -> the Guarded output; in place: the output starts as the input"""
        To = _ln_grid(N, Tp, C, k, s)[0]
        out = Guarded(N * (To * k if k else Tp), C, init=src if in_place else None)
        lib.w2v_ln_gelu_window(out.v if in_place else src, gd, bd, out.v, N, Tp, C, k, s if k else 1, EPS)
        torch.cuda.synchronize()
        assert out.intact()
        return out
    ins = Unchanged(xd, gd, bd)
    out = run(xd, T_in, k == 0)
    _check(f"PARITY ln_gelu_window {name} N={N} T_in={T_in} C={C} k={k} s={s}", out.flat[GUARD:], want, y, terms)
    _same(rec, "again", run(xd, T_in, k == 0).host(), out.host())
    got = out.host().view(N, T_out if k else T_in, (k if k else 1) * C)
    for t0, t1 in _split(T_out, trips):                      # output rows t0 .. t1 - 1, from a launch in which no workgroup loops
        part = xd[:, s * t0:s * (t1 - 1) + k].contiguous() if k else xd[:, t0:t1].contiguous()
        assert _ln_grid(N, part.shape[1], C, k, s)[2:] == (1, _ln_grid(N, part.shape[1], C, k, s)[1], 1)
        piece = run(part, part.shape[1], k == 0)
        _same(rec, "pieces", piece.host().view(N, t1 - t0, -1), got[:, t0:t1])
    ins.check()


@pytest.mark.parametrize("N,L,turns", [(2, 20600, 2), (1, 40990, 3)], ids=["cap-plus", "two-turns-plus"])
def test_w2v_conv0_ln_gelu_past_its_own_cap(rec, N, L, turns):  # noqa: F811
    """the audit's find: layer 0 of the layer-norm family caps its grid at 1024 workgroups of 4 frames (C0 = 512) and the kernel
    tests stayed at 200; L = 20600 is 4119 frames, 1030 workgroups' worth (tests/test_w2v_conv0_kernels_gpu.py's size for the base
    family's layer 0); L = 40990 is 8197 frames, 2050 workgroups' worth (12.6 MB out)"""
    lib = _lib()
    C0, k0, s0, k1, s1 = 512, 10, 5, 3, 2
    T0 = (L - k0) // s0 + 1
    T1 = (T0 - k1) // s1 + 1
    nfl = THREADS // (C0 // 8)
    assert _past(f"w2v_conv0_ln_gelu L={L}", -(-(s1 * (T1 - 1) + k1) // nfl), CONV0_CAP, "workgroups' worth of frames per clip") == turns
    g = torch.Generator().manual_seed(L + C0 + k0)
    wave = 0.5 * torch.randn(N, L, generator=g) + 0.5
    w = 0.4 * torch.randn(C0, 1, k0, generator=g)
    bias = 0.3 * torch.randn(C0, generator=g)
    gamma, beta = _affine(C0, g, False)
    raw = w2v_ref.conv0_raw(wave.double(), w.double(), s0) + bias.double()
    mag = w2v_ref.conv0_raw(wave.double().abs(), w.double().abs(), s0) + bias.double().abs()
    want, y, terms = (w2v_ref.window(t, k1, s1) for t in _ln_gelu(raw, gamma, beta, mag))
    dev = [t.cuda() for t in (wave, w, bias, gamma, beta)]
    ins = Unchanged(*dev)

    def run(wv, rows):
        out = Guarded(N * rows, k1 * C0)
        lib.w2v_conv0_ln_gelu(wv, *dev[1:], out.v, k0, s0, k1, s1, EPS)
        torch.cuda.synchronize()
        assert out.intact()
        return out
    out = run(dev[0], T1)
    _check(f"PARITY conv0_ln_gelu N={N} L={L} C0={C0}", out.flat[GUARD:], want, y, terms)
    _same(rec, "again", run(dev[0], T1).host(), out.host())
    got = out.host().view(N, T1, k1 * C0)
    for t0, t1 in _split(T1, turns):                       # window rows t0 .. t1 - 1 read frames s1 t0 .. s1 (t1 - 1) + k1 - 1
        part = dev[0][:, s0 * s1 * t0:s0 * (s1 * (t1 - 1) + k1 - 1) + k0].contiguous()
        _fits(-(-(s1 * (t1 - t0 - 1) + k1) // nfl), CONV0_CAP)
        piece = run(part, t1 - t0)
        _same(rec, "pieces", piece.host().view(N, t1 - t0, -1), got[:, t0:t1])
    ins.check()


# =================================================================================== the keyed streaming dropouts
def _hidden_want(y, resid, keep, f32):
    if f32:
        return torch.where(keep, (y.double() * INV).float(), torch.zeros_like(y))
    r = torch.zeros_like(y) if resid is None else resid
    return torch.where(keep, _fma_bf16(y, INV, r), r)


def _hidden_run(items, per, y, resid, item0=ITEM0, in_place=False):
    lib = _lib()
    f32 = y.dtype == F32
    out = Guarded(items, per, dtype=y.dtype, init=y if in_place else None)
    yd, rd = (out.flat[GUARD:GUARD + items * per] if in_place else y.cuda()), _dev(resid)
    ins = Unchanged(None if in_place else yd, rd)
    lib.hidden_dropout(yd.view(items, per), out.flat[GUARD:GUARD + items * per].view(items, per), items, _drop(P, item0), resid=rd)
    ins.check()
    assert out.intact()
    return out.host()


@pytest.mark.parametrize("form", ["bf16", "resid", "in-place", "f32"])
def test_hidden_dropout_x_loop(rec, form):  # noqa: F811
    """two items of TURN + 3 vectors each: item 1's later turn starts from g x per8 + v with g = 1"""
    items, per = 2, 8 * (TURN + 3)
    _past("hidden_dropout x", per // 8)
    keep = DD.hidden_keep(STATE, SITE, ITEM0, items, per, THRESH)
    y = _signed((items, per), 31)
    y = y.float() * 1.2345 if form == "f32" else y
    resid = torch.randn(items, per, generator=torch.Generator().manual_seed(32)).to(BF16) if form in ("resid", "in-place") else None
    got = _hidden_run(items, per, y, resid, in_place=form == "in-place")
    if resid is None:
        rec("mask", 0.0 if torch.equal(got.float() != 0, keep) else float("inf"))
        assert torch.equal(got.float() != 0, keep), "the kept set is not the restated one"
    _same(rec, "values", got, _hidden_want(y, resid, keep, form == "f32"))
    _same(rec, "again", _hidden_run(items, per, y, resid, in_place=form == "in-place"), got)


def test_hidden_dropout_x_loop_two_turns_and_a_third(rec):  # noqa: F811
    items, per = 1, 8 * (2 * TURN + 3)                     # 16.8 MB a tensor
    assert _past("hidden_dropout x", per // 8) == 3
    keep = DD.hidden_keep(STATE, SITE, ITEM0, items, per, THRESH)
    y = _signed((items, per), 33)
    got = _hidden_run(items, per, y, None)
    rec("mask", 0.0 if torch.equal(got.float() != 0, keep) else float("inf"))
    assert torch.equal(got.float() != 0, keep), "the kept set is not the restated one"
    _same(rec, "values", got, _hidden_want(y, None, keep, False))
    _same(rec, "again", _hidden_run(items, per, y, None), got)


Y_ITEMS = pytest.mark.parametrize("items,trips", [(Y_CAP + 2, 2), (2 * Y_CAP + 1, 3)], ids=["cap-plus", "two-trips-plus"])


@Y_ITEMS
@pytest.mark.parametrize("item0", [0, ITEM0])
@pytest.mark.parametrize("form", ["bf16", "resid", "f32"])
def test_hidden_dropout_y_loop(rec, form, item0, items, trips):  # noqa: F811
    """65 537 items of one vector: items 65 535 and 65 536 are the second trip of g += gridDim.y, keyed by item0 + g; 131 071 items:
    two full trips and item 131 070 in a third"""
    per = 8
    assert _past("hidden_dropout y", items, Y_CAP, "items") == trips
    keep = DD.hidden_keep(STATE, SITE, item0, items, per, THRESH)
    y = _signed((items, per), 34)
    y = y.float() * 1.2345 if form == "f32" else y
    resid = torch.randn(items, per, generator=torch.Generator().manual_seed(35)).to(BF16) if form == "resid" else None
    got = _hidden_run(items, per, y, resid, item0)
    if resid is None:
        assert torch.equal(got.float() != 0, keep), "the kept set is not the restated one"
    _same(rec, "values", got, _hidden_want(y, resid, keep, form == "f32"))
    _same(rec, "again", _hidden_run(items, per, y, resid, item0), got)
    for g0, g1 in _split(items, trips):
        _fits(g1 - g0, Y_CAP)
        part = _hidden_run(g1 - g0, per, y[g0:g1].contiguous(), None if resid is None else resid[g0:g1].contiguous(), item0 + g0)
        _same(rec, "pieces", part, got[g0:g1])


def _mask_drop_run(x, items, T, length, p, starts, embed, item0=ITEM0, in_place=False):
    lib = _lib()
    d = x.shape[1]
    out = Guarded(items * T, d, init=x if in_place else None)
    xd, sd, ed = (out.v if in_place else x.cuda()), _dev(starts), _dev(embed)
    ins = Unchanged(None if in_place else xd, sd, ed)
    lib.w2v_mask_drop(xd, out.v, items, T, length, _drop(p, item0), sd, ed)
    ins.check()
    assert out.intact()
    return out.host()


def _mask_drop_want(x, span, keep, embed, p):
    c = INV if p else 1.0
    kept = torch.where(keep, _scale_bf16(x, c), torch.zeros_like(x))
    inside = embed.to(BF16)[None, :].expand_as(x) if embed is not None else torch.zeros_like(x)
    return torch.where(span[:, None], inside, kept)


MASK_FORMS = [("embed-spans", True, True, P), ("spans", False, True, P), ("dropout", False, False, P), ("embed-spans-p0", True, True, 0.0)]


def _mask_drop_x(rec, items, T, with_embed, with_spans, p, turns):
    d, length = 1024, 10
    assert _past(f"w2v_mask_drop x items={items} T={T}", T * d // 8) == turns
    x = (1.0 + torch.rand(items * T, d, generator=torch.Generator().manual_seed(36))).to(BF16)      # never 0
    embed = 1.2345 * torch.randn(d, generator=torch.Generator().manual_seed(37)) if with_embed else None
    keep = DD.hidden_keep(STATE, SITE, ITEM0, items, T * d, THRESH).reshape(items * T, d) if p else torch.ones(items * T, d, dtype=torch.bool)
    table = WR.span_table(STATE, SITE + 1, ITEM0, items, T, 0.2, length, 2, T // 45) if with_spans else None
    span = WR.rows_of(table, T, length).reshape(-1) if with_spans else torch.zeros(items * T, dtype=torch.bool)
    if with_spans:
        table[-1, int((table[-1] >= 0).sum())] = T - length    # a span that ends with the last clip: its rows are the last turn's
        span = WR.rows_of(table, T, length).reshape(-1)
        assert bool(span[-1]) and bool((table[:, -1] == -1).all())
    got = _mask_drop_run(x, items, T, length, p, table, embed)
    _same(rec, "values", got, _mask_drop_want(x, span, keep, embed, p))
    _same(rec, "in place", _mask_drop_run(x, items, T, length, p, table, embed, in_place=True), got)
    _same(rec, "again", _mask_drop_run(x, items, T, length, p, table, embed), got)


@pytest.mark.parametrize("form,with_embed,with_spans,p", MASK_FORMS, ids=[f[0] for f in MASK_FORMS])
def test_w2v_mask_drop_x_loop(rec, form, with_embed, with_spans, p):  # noqa: F811
    """two clips of 4097 x 1024 / 8 = TURN + 128 vectors: the last frame of each clip is the later turn's"""
    _mask_drop_x(rec, 2, 4097, with_embed, with_spans, p, 2)


@pytest.mark.parametrize("form,with_embed,with_spans,p", MASK_FORMS[:2], ids=[f[0] for f in MASK_FORMS[:2]])
def test_w2v_mask_drop_x_loop_two_turns_and_a_third(rec, form, with_embed, with_spans, p):  # noqa: F811
    """one clip of 8193 x 1024 / 8 = 2 TURN + 128 vectors (16.8 MB), both template instances"""
    _mask_drop_x(rec, 1, 8193, with_embed, with_spans, p, 3)


@Y_ITEMS
@pytest.mark.parametrize("form,with_embed,with_spans,p", MASK_FORMS[:3], ids=[f[0] for f in MASK_FORMS[:3]])
def test_w2v_mask_drop_y_loop(rec, form, with_embed, with_spans, p, items, trips):  # noqa: F811
    """65 537 clips of one frame of 8: clips 65 535 and 65 536 are the second trip of g += gridDim.y; 131 071 clips: two full trips and
    one clip in a third; every third clip is masked"""
    T, d, length = 1, 8, 1
    assert _past("w2v_mask_drop y", items, Y_CAP, "items") == trips
    x = (1.0 + torch.rand(items * T, d, generator=torch.Generator().manual_seed(38))).to(BF16)
    embed = 1.2345 * torch.randn(d, generator=torch.Generator().manual_seed(39)) if with_embed else None
    keep = DD.hidden_keep(STATE, SITE, ITEM0, items, T * d, THRESH).reshape(items * T, d)
    table = None
    span = torch.zeros(items, dtype=torch.bool)
    if with_spans:
        span = torch.arange(items) % 3 == 0
        table = torch.stack([torch.where(span, 0, -1), torch.full((items,), -1)], dim=1).to(torch.int32)
        assert bool(span[(trips - 1) * Y_CAP]) and torch.equal(WR.rows_of(table, T, length).reshape(-1), span)
    got = _mask_drop_run(x, items, T, length, p, table, embed)
    _same(rec, "values", got, _mask_drop_want(x, span, keep, embed, p))
    _same(rec, "again", _mask_drop_run(x, items, T, length, p, table, embed), got)
    for g0, g1 in _split(items, trips):
        _fits(g1 - g0, Y_CAP)
        part = _mask_drop_run(x[g0:g1].contiguous(), g1 - g0, T, length, p, None if table is None else table[g0:g1].contiguous(), embed, ITEM0 + g0)
        _same(rec, "pieces", part, got[g0:g1])


# =================================================================================== csrc/lstm.hip: swap01 (the audit's other find)
@pytest.mark.parametrize("in_f32,out_f32", [(False, False), (True, False), (False, True), (True, True)], ids=["bf16-bf16", "f32-bf16", "bf16-f32", "f32-f32"])
def test_swap01_past_its_own_cap(rec, in_f32, out_f32):  # noqa: F811
    """(n0, n1, d) -> (n1, n0, d): 129 x 128 x 64 = 1 056 768 chunks of 8 on at most 4096 workgroups of 256, 8 192 in the second turn"""
    lib = _lib()
    n0, n1, d = 129, 128, 512
    _past("swap01", n0 * n1 * d // 8, SWAP_CAP * THREADS, "chunks")
    x = torch.randn(n0, n1, d, generator=torch.Generator().manual_seed(51))
    x = x if in_f32 else x.to(BF16)
    xd = x.cuda()
    ins = Unchanged(xd)

    def run(src, rows0):
        out = Guarded(n1 * rows0, d, dtype=F32 if out_f32 else BF16)
        lib.check(lib.load().mmf_swap01(src.data_ptr(), out.flat[GUARD:].data_ptr(), rows0, n1, d, int(in_f32), int(out_f32), lib.stream_ptr()))
        torch.cuda.synchronize()
        assert out.intact()
        return out.host().view(n1, rows0, d)
    got = run(xd, n0)
    _same(rec, "swap01", got, x.transpose(0, 1).to(F32 if out_f32 else BF16))
    _same(rec, "again", run(xd, n0), got)
    for a, b in _split(n0, 2):
        _fits((b - a) * n1 * d // 8, SWAP_CAP * THREADS)
        _same(rec, "pieces", run(xd[a:b].contiguous(), b - a), got[:, a:b])
    ins.check()
