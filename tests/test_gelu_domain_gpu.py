"""GPU: every exact-GELU site of the native backbones against float64 under the domain rule of tests/gelu_domain.py.

Sites that take the pre-activation as a bf16 tensor run all 65 280 finite bf16 inputs in one launch (``domain()``: 255 rows of 256):
``bias_gelu`` / ``bias_gelu_to`` / ``bias_gelu_drop_to`` and their backwards (csrc/vit.hip), ``w2v_gelu_window`` and
``w2v_window_fold_gelu_bwd`` (csrc/wav2vec2.hip), ``whisper_gelu_window`` and ``whisper_stem_out`` (csrc/whisper.hip).  Sites that reach
it only through a per-channel f32 vector run ``edge_points(256)`` with everything else arranged so that the pre-activation IS that
vector: the positional convolution on x = 0 (z = bias), and layer 0's kernels and the layer-norm family's with gamma = 0 (the affine
step is fma(., 0, beta) = beta).  Where a kernel adds an f32 bias, v is restated as the f32 sum it forms, which is exact.

Every output sits between NaN-filled guard regions (and NaN padding columns where the row stride exceeds the row) that must come back
untouched, every input must come back with its bits unless the kernel was asked to write in place, and every case prints its worst
error / allowance and the input where it occurred."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as A  # noqa: E402
import gelu_domain as D  # noqa: E402
import keyed_dropout_ref as KD  # noqa: E402
import w2v_ref  # noqa: E402
from helpers import _lib  # noqa: E402
from w2v_kernel_checks import bits  # noqa: E402

BF16 = torch.bfloat16
GUARD = 1024                                         # elements on either side of an output
ROWS, COLS, LD = 255, 256, 264
STATE, SITE, ITEM0, ITEMS = (91 << 20) + 7, 4, 3, 5  # 5 items of 51 rows
EPS = 1e-5
X = D.domain()                                       # (255, 256) bf16, shared and never written
EDGE = D.edge_points(COLS)
BIASES = ["none", "zero", "rand", "minus6"]
DGS = ["one", "normal"]


class Guarded:
    """a (rows, cols) device block of row stride ``ld`` between two guard regions; guards, padding columns and, until it is written,
    the block itself are NaN"""

    def __init__(self, rows, cols, ld=None, dtype=BF16, init=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.flat = torch.full((2 * GUARD + rows * self.ld,), float("nan"), dtype=dtype, device="cuda")
        self.full = self.flat[GUARD:GUARD + rows * self.ld].view(rows, self.ld)
        self.v = self.full[:, :cols]
        if init is not None:
            self.v.copy_(init.reshape(rows, cols))

    def host(self):
        return self.v.cpu()

    def intact(self):
        f = self.flat.cpu()
        pad = f[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, self.cols:]
        return bool(torch.isnan(f[:GUARD]).all()) and bool(torch.isnan(f[-GUARD:]).all()) and bool(torch.isnan(pad).all())


class Unchanged:
    """the bits of the inputs of a launch, to compare after it"""

    def __init__(self, *ts):
        self.ts = [t for t in ts if t is not None]
        self.before = [bits(t).clone() for t in self.ts]

    def check(self):
        torch.cuda.synchronize()
        assert all(torch.equal(bits(t), b) for t, b in zip(self.ts, self.before)), "an input was changed"


def _bias(kind, cols=COLS):
    """-> the f32 bias of a case (None: the kernel's form without one)"""
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(cols)
    if kind == "rand":
        return torch.rand(cols, generator=torch.Generator().manual_seed(cols)) - 0.5
    return torch.full((cols,), -6.0)                 # drags half the grid into the left tail


def _v(x, b):
    """the pre-activation the kernel forms: the f32 (IEEE) sum of the bf16 value and the f32 bias, exactly"""
    return x.float() if b is None else x.float() + b


def _dev(t):
    return None if t is None else t.cuda()


def _dg(kind, shape, seed=5):
    if kind == "one":
        return torch.ones(shape, dtype=BF16)
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF16)


def _hold(what, ratio, v):
    w, at, fails = D.report(what, ratio, v)
    assert fails == 0, f"{what}: {fails} of {ratio.numel()} inputs over the allowance, worst {w:.3f} at v = {at!r}"


def _keep():
    th = A.mmf_drop_thresh(0.1)
    keep = np.concatenate([KD.gemm_keep(STATE, SITE, ITEM0 + g, ROWS // ITEMS, COLS, th) for g in range(ITEMS)], axis=0)
    keep = torch.from_numpy(np.ascontiguousarray(keep))
    assert keep.shape == (ROWS, COLS) and bool(keep.any()) and not bool(keep.all())
    return keep, A.inv_keep_of(th)


def _drop(p):
    return (p, KD.state_tensor(STATE, "cuda"), SITE, ITEM0)


# ---- csrc/vit.hip: the FFN activation of ViT, DeBERTa, BERT / RoBERTa, Wav2Vec2, WavLM and Whisper ---------------------------------
@pytest.mark.parametrize("bias", BIASES)
def test_bias_gelu_in_place_and_out_of_place(bias):
    lib, b = _lib(), _bias(bias)
    bd, v = _dev(b), _v(X, b)
    inplace, h, g = Guarded(ROWS, COLS, LD, init=X), Guarded(ROWS, COLS, LD, init=X), Guarded(ROWS, COLS, LD)
    ins = Unchanged(h.flat, bd)
    lib.bias_gelu(inplace.v, bd)
    lib.bias_gelu_to(h.v, bd, g.v)
    ins.check()
    assert inplace.intact() and h.intact() and g.intact()
    _hold(f"bias_gelu_to bias={bias}", D.ratio_fwd(g.host(), v), v)
    assert torch.equal(bits(inplace.host()), bits(g.host())), "the in-place entry must give the out-of-place entry's bits"
    if bias == "zero":                               # x + 0 is x in IEEE except -0 + 0 = +0, whose GELU is +0
        plain = Guarded(ROWS, COLS, LD)
        lib.bias_gelu_to(h.v, None, plain.v)
        torch.cuda.synchronize()
        same = bits(v) == bits(X.float())
        assert int((~same).sum()) == 1 and float(X.float()[~same]) == 0.0
        assert torch.equal(bits(g.host())[same], bits(plain.host())[same]) and int(bits(g.host())[~same]) == 0


@pytest.mark.parametrize("bias", BIASES[1:])
def test_bias_gelu_drop_to(bias):
    lib, b = _lib(), _bias(bias)
    bd, v = _dev(b), _v(X, b)
    keep, c = _keep()
    h, g = Guarded(ROWS, COLS, LD, init=X), Guarded(ROWS, COLS, LD)
    ins = Unchanged(h.flat, bd)
    lib.bias_gelu_drop_to(h.v, bd, g.v, ITEMS, _drop(0.1))
    ins.check()
    assert h.intact() and g.intact()
    got = g.host()
    assert bool((got[~keep].float() == 0).all()), "a dropped element is not an exact zero"
    _hold(f"bias_gelu_drop_to p=0.1 bias={bias} (kept elements)", D.ratio_fwd(got, v, scale=c)[keep], v[keep])
    zero, plain = Guarded(ROWS, COLS, LD), Guarded(ROWS, COLS, LD)
    lib.bias_gelu_drop_to(h.v, bd, zero.v, ITEMS, _drop(0.0))
    lib.bias_gelu_to(h.v, bd, plain.v)
    torch.cuda.synchronize()
    assert zero.intact() and torch.equal(bits(zero.host()), bits(plain.host())), "p = 0 must be bias_gelu_to bit for bit"


@pytest.mark.parametrize("dg", DGS)
@pytest.mark.parametrize("bias", BIASES)
def test_bias_gelu_bwd_separate_and_aliased(bias, dg):
    lib, b, d = _lib(), _bias(bias), _dg(dg, (ROWS, COLS))
    bd, v = _dev(b), _v(X, b)
    h, g, dh, alias = Guarded(ROWS, COLS, LD, init=X), Guarded(ROWS, COLS, LD, init=d), Guarded(ROWS, COLS, LD), Guarded(ROWS, COLS, LD, init=d)
    ins = Unchanged(h.flat, g.flat, bd)
    lib.bias_gelu_bwd(g.v, h.v, bd, dh.v)
    lib.bias_gelu_bwd(alias.v, h.v, bd, alias.v)
    ins.check()
    assert h.intact() and g.intact() and dh.intact() and alias.intact()
    _hold(f"bias_gelu_bwd bias={bias} dg={dg}", D.ratio_bwd(dh.host(), v, d), v)
    assert torch.equal(bits(alias.host()), bits(dh.host())), "dh aliased onto dg must give the separate output's bits"


@pytest.mark.parametrize("dg", DGS)
@pytest.mark.parametrize("bias", BIASES[1:])
def test_bias_gelu_drop_bwd(bias, dg):
    lib, b, d = _lib(), _bias(bias), _dg(dg, (ROWS, COLS))
    bd, v = _dev(b), _v(X, b)
    keep, c = _keep()
    h, g, dh = Guarded(ROWS, COLS, LD, init=X), Guarded(ROWS, COLS, LD, init=d), Guarded(ROWS, COLS, LD)
    ins = Unchanged(h.flat, g.flat, bd)
    lib.bias_gelu_drop_bwd(g.v, h.v, bd, dh.v, ITEMS, _drop(0.1))
    ins.check()
    assert h.intact() and g.intact() and dh.intact()
    got = dh.host()
    assert bool((got[~keep].float() == 0).all()), "a dropped element is not an exact zero"
    _hold(f"bias_gelu_drop_bwd p=0.1 bias={bias} dg={dg} (kept elements)", D.ratio_bwd(got, v, d, scale=c)[keep], v[keep])


# ---- csrc/wav2vec2.hip: the feature encoder's GELU + window form and its mirror -------------------------------------------------
def _frames(T_in, k, s, pad=0):
    """-> (T_out, the input frame of every (row, tap) slot of the window form, which slots lie inside the clip)"""
    T_out = (T_in + 2 * pad - k) // s + 1
    f = torch.arange(T_out)[:, None] * s + torch.arange(k)[None, :] - pad
    return T_out, f, (f >= 0) & (f < T_in)


@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
def test_w2v_gelu_window(k, s):
    lib = _lib()
    T_out, f, inside = _frames(ROWS, k, s)
    assert bool(inside.all())
    x, out = Guarded(ROWS, COLS, init=X), Guarded(T_out, k * COLS)
    ins = Unchanged(x.flat)
    lib.w2v_gelu_window(x.v, out.v, 1, ROWS, COLS, k, s)
    ins.check()
    assert x.intact() and out.intact()
    got = out.host().view(T_out, k, COLS)
    v = X.float()[f]                                                                  # (T_out, k, C)
    assert torch.equal(v.reshape(1, T_out, k * COLS), w2v_ref.window(X.float()[None], k, s))
    _hold(f"w2v_gelu_window k={k} s={s}", D.ratio_fwd(got, v), v)
    first = torch.zeros(ROWS, COLS, dtype=torch.int16)
    first[f.reshape(-1)] = bits(got).view(T_out * k, COLS)                            # one copy per frame ...
    assert torch.equal(first[f], bits(got)), "the tap copies of one frame differ"  # ... is every copy


@pytest.mark.parametrize("dg", DGS)
@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
def test_w2v_window_fold_gelu_bwd(k, s, dg):
    """dwin is non-zero in one tap at a time, so the fold of a frame has one term and is exact; the taps together reach every frame
    some window reads, and a frame none reads is an exact zero"""
    lib = _lib()
    T_out, f, _ = _frames(ROWS, k, s)
    d = _dg(dg, (ROWS, COLS))                                                         # the gradient of frame f, wherever it is put
    x, seen = Guarded(ROWS, COLS, init=X), torch.zeros(ROWS, dtype=torch.bool)
    for j in range(k):
        win = torch.zeros(T_out, k, COLS, dtype=BF16)
        win[:, j] = d[f[:, j]]
        dwin, dx = Guarded(T_out, k * COLS, init=win), Guarded(ROWS, COLS)
        ins = Unchanged(x.flat, dwin.flat)
        lib.w2v_window_fold_gelu_bwd(dwin.v, x.v, dx.v, 1, ROWS, COLS, k, s)
        ins.check()
        assert dx.intact()
        fed = torch.zeros(ROWS, dtype=torch.bool)
        fed[f[:, j]] = True
        seen |= fed
        got = dx.host()
        assert bool((got[~fed].float() == 0).all()), "a frame whose fold is zero is not an exact zero"
        dfed = torch.where(fed[:, None], d, torch.zeros_like(d))
        _hold(f"w2v_window_fold_gelu_bwd k={k} s={s} tap {j} dg={dg}", D.ratio_bwd(got, X.float(), dfed), X.float())
    read = torch.zeros(ROWS, dtype=torch.bool)
    read[f.reshape(-1)] = True
    assert torch.equal(seen, read) and int(read.sum()) >= ROWS - 1


# ---- csrc/whisper.hip: the convolution stem ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", ["zero", "minus6"])
@pytest.mark.parametrize("k,s,pad", [(3, 2, 1), (3, 1, 1)])
def test_whisper_gelu_window(k, s, pad, bias):
    lib, b = _lib(), _bias(bias)
    bd = _dev(b)
    T_out, f, inside = _frames(ROWS, k, s, pad)
    assert not bool(inside.all())
    x, out = Guarded(ROWS, COLS, init=X), Guarded(T_out, k * COLS)
    ins = Unchanged(x.flat, bd)
    lib.whisper_gelu_window(x.v.view(1, ROWS, COLS), bd, out.v.view(1, T_out, k * COLS), 1, ROWS, COLS, k, s, pad)
    ins.check()
    assert x.intact() and out.intact()
    got = out.host().view(T_out, k, COLS)
    assert bool((bits(got)[~inside] == 0).all()), "a padding row is not all zero bits"
    v = _v(X, b)[f.clamp(0, ROWS - 1)]
    _hold(f"whisper_gelu_window k={k} s={s} pad={pad} bias={bias}", D.ratio_fwd(got, v)[inside], v[inside])


@pytest.mark.parametrize("bias", BIASES[1:])
def test_whisper_stem_out_with_a_zero_position_table(bias):
    lib, b = _lib(), _bias(bias)
    bd, v = _dev(b), _v(X, b)
    pos = torch.zeros(ROWS, COLS, device="cuda")
    x, out, inplace = Guarded(ROWS, COLS, init=X), Guarded(ROWS, COLS), Guarded(ROWS, COLS, init=X)
    ins = Unchanged(x.flat, bd, pos)
    lib.whisper_stem_out(x.v, bd, pos, out.v, ROWS)
    lib.whisper_stem_out(inplace.v, bd, pos, inplace.v, ROWS)
    ins.check()
    assert x.intact() and out.intact() and inplace.intact()
    _hold(f"whisper_stem_out bias={bias}", D.ratio_fwd(out.host(), v), v)
    assert torch.equal(bits(inplace.host()), bits(out.host())), "in place must give the out-of-place bits"


# ---- sites behind a per-channel vector: the pre-activation is made to BE edge_points(C) --------------------------------------------
PC = dict(N=2, T=5, C=COLS, groups=16, k=3)          # group width 16, the narrowest the kernel takes


def _posconv_operands():
    N, T, C, groups, k = (PC[n] for n in ("N", "T", "C", "groups", "k"))
    cg = C // groups
    Kp = (k * cg + 31) // 32 * 32
    w = torch.randn(groups, cg, Kp, generator=torch.Generator().manual_seed(3)).to(BF16)
    return torch.zeros(N * T, C, dtype=BF16).cuda(), w.cuda(), EDGE.cuda()


def test_w2v_posconv_forward_on_a_zero_input():
    """x = 0: the convolution is exactly zero whatever the weights, z = bias and y = 0 + gelu(bias)"""
    lib = _lib()
    x, w, bd = _posconv_operands()
    y = Guarded(PC["N"] * PC["T"], COLS)
    ins = Unchanged(x, w, bd)
    lib.w2v_posconv(x, w, bd, y.v, **PC)
    ins.check()
    assert y.intact()
    v = EDGE.expand(PC["N"] * PC["T"], COLS)
    _hold("w2v_posconv forward, z = bias", D.ratio_fwd(y.host(), v), v)


@pytest.mark.parametrize("dg", DGS)
def test_w2v_posconv_backward_activation_on_a_zero_input(dg):
    lib = _lib()
    x, w, bd = _posconv_operands()
    d = _dg(dg, (PC["N"] * PC["T"], COLS))
    dy, dz = Guarded(PC["N"] * PC["T"], COLS, init=d), Guarded(PC["N"] * PC["T"], COLS)
    ins = Unchanged(x, w, bd, dy.flat)
    lib.w2v_posconv_bwd_act(x, w, bd, dy.v, dz.v, **PC)
    ins.check()
    assert dz.intact()
    v = EDGE.expand(PC["N"] * PC["T"], COLS)
    _hold(f"w2v_posconv_bwd_act dg={dg}, z = bias", D.ratio_bwd(dz.host(), v, d), v)


def _conv0_operands(k0, N=2, T0=8, s0=5):
    g = torch.Generator().manual_seed(k0)
    wave = 0.5 * torch.randn(N, k0 + s0 * (T0 - 1), generator=g)
    w = 0.4 * torch.randn(COLS, 1, k0, generator=g)
    stats = torch.cat([torch.full((N, 1, COLS), 0.25), torch.ones(N, 1, COLS)], dim=1)     # mean | variance, as the kernel is given them
    return wave.cuda(), w.cuda(), stats.cuda(), torch.zeros(COLS).cuda(), EDGE.cuda()


@pytest.mark.parametrize("k0", [10, 12], ids=["taps10", "taps16"])
def test_w2v_conv0_norm_gelu_with_a_zero_gamma(k0):
    """gamma = 0: scale = 0 and shift = beta - mean x 0 = beta, so y = fma(conv, 0, beta) = beta in both register tap forms"""
    lib = _lib()
    wave, w, stats, gamma, beta = _conv0_operands(k0)
    N, k1, s1, T1 = 2, 3, 2, 3                                                        # T0 = 8: frame 7 is not read
    out = Guarded(N * T1, k1 * COLS)
    ins = Unchanged(wave, w, stats, gamma, beta)
    lib.w2v_conv0_norm_gelu(wave, w, stats, gamma, beta, out.v, k0, 5, k1, s1, EPS)
    ins.check()
    assert out.intact()
    got = out.host().view(N * T1 * k1, COLS)
    v = EDGE.expand_as(got)
    _hold(f"w2v_conv0_norm_gelu k0={k0}, y = beta", D.ratio_fwd(got, v), v)


def test_w2v_conv0_ln_gelu_with_a_zero_gamma():
    lib = _lib()
    wave, w, _, gamma, beta = _conv0_operands(10)
    cbias = (0.1 * torch.randn(COLS, generator=torch.Generator().manual_seed(1))).cuda()
    N, k1, s1, T1 = 2, 3, 2, 3
    out = Guarded(N * T1, k1 * COLS)
    ins = Unchanged(wave, w, cbias, gamma, beta)
    lib.w2v_conv0_ln_gelu(wave, w, cbias, gamma, beta, out.v, 10, 5, k1, s1, EPS)
    ins.check()
    assert out.intact()
    got = out.host().view(N * T1 * k1, COLS)
    v = EDGE.expand_as(got)
    _hold("w2v_conv0_ln_gelu, y = beta", D.ratio_fwd(got, v), v)


@pytest.mark.parametrize("k,s", [(3, 2), (0, 1)], ids=["window", "rows"])
def test_w2v_ln_gelu_window_with_a_zero_gamma(k, s):
    lib = _lib()
    N, T_in = 2, 9
    rows = ((T_in - k) // s + 1) * k if k else T_in
    x = Guarded(N * T_in, COLS, init=torch.randn(N * T_in, COLS, generator=torch.Generator().manual_seed(9)).to(BF16))
    gamma, beta = torch.zeros(COLS).cuda(), EDGE.cuda()
    out = Guarded(N * rows, COLS)
    ins = Unchanged(x.flat, gamma, beta)
    lib.w2v_ln_gelu_window(x.v, gamma, beta, out.v, N, T_in, COLS, k, s, EPS)
    ins.check()
    assert x.intact() and out.intact()
    v = EDGE.expand(N * rows, COLS)
    _hold(f"w2v_ln_gelu_window k={k} s={s}, y = beta", D.ratio_fwd(out.host(), v), v)


@pytest.mark.parametrize("dg", DGS)
@pytest.mark.parametrize("k0", [10, 12], ids=["taps10", "taps16"])
def test_w2v_conv0_backward_with_a_zero_gamma_and_one_live_frame(k0, dg):
    """gamma = 0 and an upstream gradient that is non-zero in one (clip, row, tap) slot of the window form, whose frame no other slot
    reads: dbeta[c] = da[c] gelu'(beta[c]) is a sum of one term and zeros.  dbeta is f32: the allowance has no store term"""
    lib = _lib()
    wave, w, stats, gamma, beta = _conv0_operands(k0)
    N, k1, s1, T1 = 2, 3, 2, 3
    da = _dg(dg, (COLS,), seed=k0)
    win = torch.zeros(N, T1, k1, COLS, dtype=BF16)
    win[1, 1, 1] = da                                                                  # frame 2 x 1 + 1 = 3: odd frames are read by tap 1 alone
    dwin = win.view(N, T1, k1 * COLS).cuda()
    sums, partial = Guarded(N * 2, COLS, dtype=torch.float32), torch.full((N * lib.W2V_STATS_SLOTS * 2 * COLS,), float("nan"), device="cuda")
    dgamma, dbeta = Guarded(1, COLS, dtype=torch.float32), Guarded(1, COLS, dtype=torch.float32)
    ins = Unchanged(wave, w, stats, gamma, beta, dwin)
    lib.w2v_conv0_bwd_stats(wave, w, stats, gamma, beta, dwin, sums.flat[GUARD:GUARD + N * 2 * COLS], partial, dgamma.flat[GUARD:GUARD + COLS],
                            dbeta.flat[GUARD:GUARD + COLS], k0, 5, k1, s1, EPS, accumulate=False)
    ins.check()
    assert sums.intact() and dgamma.intact() and dbeta.intact()
    assert bool(torch.isfinite(dgamma.host()).all())
    got = dbeta.host().view(COLS)
    _hold(f"w2v_conv0_bwd_stats k0={k0} dg={dg}: dbeta = da gelu'(beta)", D.ratio_bwd(got, EDGE, da, stored=False), EDGE)
