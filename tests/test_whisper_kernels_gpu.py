"""GPU: the kernels of csrc/whisper.hip against the float64 restatement tests/whisper_ref.py.

``mmf_whisper_logmel``, element by element.  The kernel's DFT is an f32 product: a frame's spectrum X_f carries an absolute error of
at most e = 2^-21 sum_t |x_t w_t| (400 f32 multiply-adds of terms bounded by |x_t w_t|, 2^-24 each, with the table's and the
product x w's own roundings: 8 x 2^-24 x the l1 norm is generous for a chain whose errors do not all line up), so the power
|X_f|^2 is off by at most 2 |X_f| e + e^2, the mel value by E = sum_f M[f][m] (2 |X_f| e + e^2) + 2^-22 mel (the filter's own f32
sum), its log10 by (E / mel) / ln 10 and the feature, (x + 4) / 4, by a quarter of that plus 2^-16 for the f32 log and the final
scaling at values up to 2.  The clamp max(x, clip maximum - 8) is 1-Lipschitz in both arguments, so an element's bound is raised
to the bound of the clip's arg-max element.  The window output is held to that plus one bf16 rounding (half a unit of 8 significant bits: 2^-8 relative), and must
be the bf16 of the feature output bit for bit.  The bound is only worth something where it is tight: on every case at least 99 %
of the elements must have a bound under 4e-3 (a pure tone would not: no case is one).  Cases: ``max_source_positions`` 50 and 100
(windows of 1 s and 2 s: 100 and 200 frames, so the second pass-1 workgroup of 64 frames is ragged in both), 80 and 128 mel bins,
and the clips of ``CLIPS``.

The two stem kernels against float64 under the allowance of tests/gelu_domain.py: the pre-activation is restated as the f32 sum x +
bias the kernels form, which is exact, so nothing is granted for it; the position is one more f32 add (2^-24 of the result) before the
one rounding of the store.  The inputs reach -9.5 .. 9.5, both tails of the GELU; tests/test_gelu_domain_gpu.py runs the two kernels
over every finite bf16 input.

Outputs are pre-filled with a sentinel and sit between guard regions; guards must come back bit-identical, as must the inputs, and
a second run must give the same bits.  Every documented refusal returns its code with nothing written."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gelu_domain  # noqa: E402
import whisper_ref as R  # noqa: E402
from helpers import _bf16_ulp  # noqa: E402
from mmfusion import lib  # noqa: E402
from mmfusion import whisper as W  # noqa: E402

E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
GUARD = 64                                   # guard elements on both sides of every output (a multiple of 16 bytes for each dtype)
TIGHT = 4e-3


class Guarded:
    """an output of ``numel`` elements between two guard regions, everything pre-filled with a sentinel bit pattern"""

    def __init__(self, shape, dtype):
        numel = int(np.prod(shape))
        self.whole = torch.empty(numel + 2 * GUARD, dtype=dtype, device=DEV)
        self._bits().fill_(0x5A5B if dtype == BF16 else 0x7FC05A5A)        # (the f32 pattern is a NaN)
        self.t = self.whole[GUARD:GUARD + numel].view(shape)
        self.before = self._bits().clone()

    def _bits(self):
        return self.whole.view(torch.int16 if self.whole.dtype == BF16 else torch.int32)

    def guards_intact(self) -> bool:
        now = self._bits()
        return torch.equal(now[:GUARD], self.before[:GUARD]) and torch.equal(now[-GUARD:], self.before[-GUARD:])

    def untouched(self) -> bool:
        return torch.equal(self._bits(), self.before)


def _noise(L, seed, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)


def _clips(name: str, n_samples: int) -> np.ndarray:
    """the case ``name`` as (B, L) f32"""
    if name == "full":
        return _noise(n_samples, 1)[None]
    if name == "L9001":
        return _noise(9001, 2)[None]
    if name == "L1":
        return np.full((1, 1), 0.7, dtype=np.float32)
    if name == "half_silent":
        x = _noise(n_samples, 3)
        x[n_samples // 2:] = 0.0
        return x[None]
    if name == "zero":
        return np.zeros((1, n_samples), dtype=np.float32)
    if name == "speech":
        return R.speech_like(n_samples, seed=4)[None]
    if name == "three":                      # one loud, one 40 dB down, one half silent: a batch-wide maximum would clamp the second
        x = np.stack([R.speech_like(n_samples, seed=5), _noise(n_samples, 6, amp=3e-4), _noise(n_samples, 7, amp=0.05)])
        x[2, n_samples // 2:] = 0.0
        return x
    raise KeyError(name)


CLIPS = ("full", "L9001", "L1", "half_silent", "zero", "speech", "three")
CASES = [(T, M, c) for T in (50, 100) for M in (80, 128) for c in CLIPS]


@pytest.fixture(scope="module")
def tables():
    """the package's f32 tables on the device, per mel count"""
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(F32).to(DEV)
    win, dft = f32(W.hann_window()), f32(W.dft_table())
    return {M: (win, dft, f32(W.mel_filter_bank(M))) for M in (80, 128)}


def _ld(wave) -> int:
    """the row stride (a single row's is whatever the tensor says: its length then)"""
    return wave.stride(0) if wave.shape[0] > 1 else wave.shape[1]


def _logmel_raw(wave, tabs, feats, win, scratch, n_samples, n_mels, Kw, *, N=None, L=None, ld=None, scratch_bytes=None):
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    return lib.load().mmf_whisper_logmel(p(wave), _ld(wave) if ld is None else ld, p(tabs[0]), p(tabs[1]), p(tabs[2]), p(feats), p(win),
                                         p(scratch), scratch.numel() * 4 if scratch_bytes is None else scratch_bytes,
                                         wave.shape[0] if N is None else N, wave.shape[1] if L is None else L, n_samples, n_mels, Kw,
                                         lib.stream_ptr())


def _run_logmel(x: np.ndarray, tabs, T: int, M: int, Kw: int):
    """-> (features Guarded, window Guarded, scratch) after one launch of both outputs"""
    B, n_samples, Tm = x.shape[0], 320 * T, 2 * T
    wave = torch.from_numpy(x).to(DEV)
    feats, win = Guarded((B, M, Tm), F32), Guarded((B, Tm, Kw), BF16)
    scratch = torch.empty(lib.whisper_logmel_scratch_bytes(B, n_samples, M) // 4, dtype=F32, device=DEV)
    keep = [t.clone() for t in (wave, *tabs)]
    assert _logmel_raw(wave, tabs, feats.t, win.t, scratch, n_samples, M, Kw) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (wave, *tabs))), "an input was written"
    return feats, win, wave


@pytest.mark.parametrize("T,M,clip", CASES, ids=[f"T{T}-M{M}-{c}" for T, M, c in CASES])
def test_logmel_element_by_element_against_float64(tables, T, M, clip):
    x = _clips(clip, 320 * T)
    B, Tm, Kw = x.shape[0], 2 * T, 3 * M + 16                       # 16 zero columns behind the three taps
    want = torch.from_numpy(R.log_mel(x.astype(np.float64), M, T))
    bound = torch.from_numpy(R.log_mel_bound(x.astype(np.float64), M, T))
    tight = float((bound < TIGHT).double().mean())
    feats, win, wave = _run_logmel(x, tables[M], T, M, Kw)
    assert feats.guards_intact() and win.guards_intact()
    got = feats.t.cpu().double()
    ratio = ((got - want).abs() / bound)
    print(f"logmel T={T} M={M} {clip}: max |err| {float((got - want).abs().max()):.3e}, worst err / bound {float(ratio.max()):.3f}, "
          f"{100 * tight:.2f} % of the bounds under {TIGHT}")
    assert tight >= 0.99, "the bound is loose on this case: it shows nothing"
    assert torch.isfinite(got).all() and float(ratio.max()) <= 1.0
    if clip == "zero":
        assert torch.equal(feats.t, torch.full_like(feats.t, -1.5))
    # the window form: the bf16 of the feature output, bit for bit, with zero rows outside the clip and zero columns behind
    w = win.t.cpu()
    fb = feats.t.cpu().to(BF16).transpose(1, 2)                                              # (B, Tm, M)
    z = torch.zeros(B, 1, M, dtype=BF16)
    padded = torch.cat([z, fb, z], dim=1)
    for j in range(3):
        assert torch.equal(w[:, :, j * M:(j + 1) * M].view(torch.int16), padded[:, j:j + Tm].contiguous().view(torch.int16)), f"tap {j}"
    assert not w[:, :, 3 * M:].view(torch.int16).any()
    centre = w[:, :, M:2 * M].double().transpose(1, 2)
    assert bool(((centre - want).abs() <= bound + 2.0 ** -8 * (want.abs() + bound)).all())
    # the same bits again, and from the features alone
    feats2, win2, _ = _run_logmel(x, tables[M], T, M, Kw)
    assert torch.equal(feats2.t.view(torch.int32), feats.t.view(torch.int32)) and torch.equal(win2.t.view(torch.int16), win.t.view(torch.int16))
    win3 = Guarded((B, Tm, Kw), BF16)
    lib.whisper_feature_window(feats.t.contiguous(), win3.t)
    torch.cuda.synchronize()
    assert win3.guards_intact() and torch.equal(win3.t.view(torch.int16), win.t.view(torch.int16))


def test_logmel_one_output_at_a_time_and_strided_rows(tables):
    """either output may be NULL; a row stride above L reads the same clips"""
    T, M = 50, 80
    x = _clips("three", 320 * T)[:, :9001]
    both_f, both_w, _ = _run_logmel(x, tables[M], T, M, 3 * M)
    wide = torch.full((3, 9001 + 37), 9.0, dtype=F32, device=DEV)
    wide[:, :9001] = torch.from_numpy(x).to(DEV)
    wave = wide[:, :9001]
    scratch = torch.empty(lib.whisper_logmel_scratch_bytes(3, 320 * T, M) // 4, dtype=F32, device=DEV)
    f, w = Guarded((3, M, 2 * T), F32), Guarded((3, 2 * T, 3 * M), BF16)
    assert _logmel_raw(wave, tables[M], f.t, None, scratch, 320 * T, M, 0) == 0
    assert _logmel_raw(wave, tables[M], None, w.t, scratch, 320 * T, M, 3 * M) == 0
    torch.cuda.synchronize()
    assert f.guards_intact() and w.guards_intact()
    assert torch.equal(f.t.view(torch.int32), both_f.t.view(torch.int32)) and torch.equal(w.t.view(torch.int16), both_w.t.view(torch.int16))


def test_logmel_maximum_is_per_clip(tables):
    """the ``batch_max`` mutant of the restatement leaves the bound on the quiet clip of ``three``: the kernel must not follow it"""
    T, M = 50, 80
    x = _clips("three", 320 * T)
    got = _run_logmel(x, tables[M], T, M, 3 * M)[0].t.cpu().double()
    want = torch.from_numpy(R.log_mel(x.astype(np.float64), M, T))
    wrong = torch.from_numpy(R.log_mel(x.astype(np.float64), M, T, mutant="batch_max"))
    bound = torch.from_numpy(R.log_mel_bound(x.astype(np.float64), M, T))
    assert bool(((got - want).abs() <= bound).all()) and float(((wrong - want).abs() / bound)[1].max()) > 10.0


# ---- the stem kernels ---------------------------------------------------------------------------------------------------
def _stem_inputs(shape, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = (3.0 * torch.randn(shape, generator=g)).clamp(-9.0, 9.0).to(BF16)
    bias = (0.2 * torch.randn(C, generator=g)).clamp(-0.5, 0.5)
    return x, bias


WINDOW_CASES = [(C, T_in, k, s, pad) for C in (128, 384) for T_in in (1, 37, 40) for (k, s, pad) in ((3, 2, 1), (3, 1, 1))]


@pytest.mark.parametrize("C,T_in,k,s,pad", WINDOW_CASES, ids=[f"C{C}-T{T}-k{k}s{s}p{p}" for C, T, k, s, p in WINDOW_CASES])
def test_gelu_window_within_one_bf16_ulp_of_float64(C, T_in, k, s, pad):
    N = 2
    x, bias = _stem_inputs((N, T_in, C), C, seed=C + T_in)
    T_out = (T_in + 2 * pad - k) // s + 1
    out = Guarded((N, T_out, k * C), BF16)
    xd, bd = x.to(DEV), bias.to(DEV)
    keep = xd.clone()
    lib.whisper_gelu_window(xd, bd, out.t, N, T_in, C, k, s, pad)
    torch.cuda.synchronize()
    assert out.guards_intact() and torch.equal(xd.view(torch.int16), keep.view(torch.int16))
    v = x.float() + bias                                              # the f32 sum the kernel forms, exactly
    act = gelu_domain.gelu64(v)
    want, allow = R.window_form(act, k, s, pad), R.window_form(gelu_domain.allow_fwd(v, act), k, s, pad)
    inside = R.window_form(torch.ones(N, T_in, C, dtype=F64), k, s, pad) > 0
    got = out.t.cpu().double()
    assert bool((got[~inside] == 0).all()) and (pad == 0 or bool((~inside).any()))
    assert bool(((got - want).abs() <= allow)[inside].all())
    again = Guarded((N, T_out, k * C), BF16)
    lib.whisper_gelu_window(xd, bd, again.t, N, T_in, C, k, s, pad)
    torch.cuda.synchronize()
    assert torch.equal(again.t.view(torch.int16), out.t.view(torch.int16))


def stem_out_allowance(v, act, want):
    """the module docstring's allowance of ``mmf_whisper_stem_out``: the GELU's (tests/gelu_domain.py) with its store term moved to
    the sum ``want`` = act + position, and 2^-24 of the sum for the f32 add of the position"""
    return 0.5 * _bf16_ulp(want) + 2.0 ** -24 * want.abs() + (gelu_domain.allow_fwd(v, act) - 0.5 * _bf16_ulp(act))


@pytest.mark.parametrize("d,T", [(d, T) for d in (128, 384) for T in (1, 37, 40)])
def test_stem_out_within_one_bf16_ulp_of_float64(d, T):
    n = 2
    x, bias = _stem_inputs((n * T, d), d, seed=d + T + 1)
    pos = torch.randn(T, d, generator=torch.Generator().manual_seed(d + T + 2))
    v = x.float() + bias                                              # the f32 sum the kernel forms, exactly
    act = gelu_domain.gelu64(v)
    want = act + pos.double().repeat(n, 1)
    tol = stem_out_allowance(v, act, want)
    xd, bd, pd = x.to(DEV), bias.to(DEV), pos.to(DEV)
    keep = xd.clone()
    out = Guarded((n * T, d), BF16)
    lib.whisper_stem_out(xd, bd, pd, out.t, T)
    torch.cuda.synchronize()
    assert out.guards_intact() and torch.equal(xd.view(torch.int16), keep.view(torch.int16))
    assert bool(((out.t.cpu().double() - want).abs() <= tol).all())
    place = Guarded((n * T, d), BF16)                                 # in place: out may be x
    place.t.copy_(xd)
    lib.whisper_stem_out(place.t, bd, pd, place.t, T)
    torch.cuda.synchronize()
    assert place.guards_intact() and torch.equal(place.t.view(torch.int16), out.t.view(torch.int16))


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_logmel_refusals_write_nothing(tables):
    T, M, n_samples = 50, 80, 16000
    wave = torch.from_numpy(_clips("L9001", n_samples)).to(DEV)
    tabs = tables[M]
    f, w = Guarded((1, M, 2 * T), F32), Guarded((1, 2 * T, 3 * M), BF16)
    scratch = torch.full((lib.whisper_logmel_scratch_bytes(1, n_samples, M) // 4 + 4,), 7.0, dtype=F32, device=DEV)
    run = lambda **kw: _logmel_raw(kw.pop("wave", wave), kw.pop("tabs", tabs), kw.pop("f", f.t), kw.pop("w", w.t), kw.pop("scratch", scratch),
                                   kw.pop("n_samples", n_samples), kw.pop("M", M), kw.pop("Kw", 3 * M), **kw)
    odd = lambda t: t.data_ptr() + 2
    cases = [
        (dict(f=None, w=None), E_SHAPE), (dict(tabs=(None, tabs[1], tabs[2])), E_SHAPE), (dict(tabs=(tabs[0], None, tabs[2])), E_SHAPE),
        (dict(tabs=(tabs[0], tabs[1], None)), E_SHAPE), (dict(N=0), E_SHAPE), (dict(L=0), E_SHAPE), (dict(L=n_samples + 1, ld=n_samples + 1), E_SHAPE),
        (dict(n_samples=16160), E_SHAPE), (dict(ld=9000), E_SHAPE), (dict(Kw=3 * M - 8), E_SHAPE), (dict(Kw=3 * M + 4), E_SHAPE),
        (dict(scratch_bytes=scratch.numel() * 4 - 64), E_SHAPE),
        (dict(M=64, Kw=3 * M), E_UNSUPPORTED), (dict(M=96, Kw=3 * 96), E_UNSUPPORTED), (dict(N=65536), E_UNSUPPORTED),
        (dict(f=odd(f.t)), E_ALIGN), (dict(w=w.t.data_ptr() + 8), E_ALIGN), (dict(scratch=scratch[1:]), E_ALIGN),
    ]
    for kw, code in cases:
        assert run(**dict(kw)) == code, kw
    torch.cuda.synchronize()
    assert f.untouched() and w.untouched() and bool((scratch == 7.0).all())
    assert lib.load().mmf_whisper_feature_window(None, w.t.data_ptr(), 1, M, 2 * T, 3 * M, lib.stream_ptr()) == E_SHAPE
    assert lib.load().mmf_whisper_feature_window(scratch.data_ptr(), w.t.data_ptr(), 1, 64, 2 * T, 3 * M, lib.stream_ptr()) == E_UNSUPPORTED
    assert lib.load().mmf_whisper_feature_window(scratch.data_ptr(), w.t.data_ptr() + 8, 1, M, 2 * T, 3 * M, lib.stream_ptr()) == E_ALIGN
    assert lib.load().mmf_whisper_feature_window(scratch.data_ptr(), w.t.data_ptr(), 1, M, 2 * T, 3 * M - 8, lib.stream_ptr()) == E_SHAPE
    torch.cuda.synchronize()
    assert w.untouched()


def test_stem_refusals_write_nothing():
    N, T_in, C = 2, 10, 128
    x, bias = _stem_inputs((N, T_in, C), C, seed=9)
    xd, bd = x.to(DEV), bias.to(DEV)
    out = Guarded((N, 5, 3 * C), BF16)
    L, s = lib.load(), lib.stream_ptr()
    gw = lambda x_=xd.data_ptr(), b=bd.data_ptr(), o=out.t.data_ptr(), N_=N, T=T_in, C_=C, k=3, st=2, pad=1: \
        L.mmf_whisper_gelu_window(x_, b, o, N_, T, C_, k, st, pad, s)
    for kw, code in [(dict(x_=None), E_SHAPE), (dict(b=None), E_SHAPE), (dict(o=None), E_SHAPE), (dict(N_=0), E_SHAPE), (dict(st=0), E_SHAPE),
                     (dict(pad=-1), E_SHAPE), (dict(pad=3), E_SHAPE), (dict(T=1, k=4, pad=1), E_SHAPE),
                     (dict(C_=132), E_UNSUPPORTED), (dict(N_=65536), E_UNSUPPORTED), (dict(o=xd.data_ptr()), E_UNSUPPORTED),
                     (dict(x_=xd.data_ptr() + 2), E_ALIGN), (dict(o=out.t.data_ptr() + 2), E_ALIGN), (dict(b=bd.data_ptr() + 4), E_ALIGN)]:
        assert gw(**kw) == code, kw
    pos = torch.randn(T_in, C, device=DEV)
    res = Guarded((N * T_in, C), BF16)
    so = lambda x_=xd.data_ptr(), b=bd.data_ptr(), p=pos.data_ptr(), o=res.t.data_ptr(), rows=N * T_in, T=T_in, d=C: \
        L.mmf_whisper_stem_out(x_, b, p, o, rows, T, d, s)
    for kw, code in [(dict(x_=None), E_SHAPE), (dict(b=None), E_SHAPE), (dict(p=None), E_SHAPE), (dict(o=None), E_SHAPE), (dict(rows=0), E_SHAPE),
                     (dict(T=0), E_SHAPE), (dict(rows=N * T_in - 1), E_SHAPE), (dict(d=132), E_UNSUPPORTED),
                     (dict(x_=xd.data_ptr() + 2), E_ALIGN), (dict(p=pos.data_ptr() + 4), E_ALIGN), (dict(o=res.t.data_ptr() + 2), E_ALIGN)]:
        assert so(**kw) == code, kw
    torch.cuda.synchronize()
    assert out.untouched() and res.untouched()
