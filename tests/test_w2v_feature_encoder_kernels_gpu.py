"""GPU: the kernels of the feature extractor's backward (csrc/wav2vec2.hip) through the C ABI against float64 autograd of the
restatement's pieces (``w2v_ref.window`` / ``gelu_erf`` / ``conv0_raw`` / ``conv0_stats``) on the same bf16 inputs:
``mmf_w2v_window_fold_gelu_bwd`` (the mirror of ``mmf_w2v_gelu_window``) and layer 0's two passes ``mmf_w2v_conv0_bwd_stats`` /
``mmf_w2v_conv0_bwd_wgrad``.

Bounds.  The fold: per element |got - exact| <= 2^-8 |exact| + 1e-6 sum |terms|: the result is one bf16 rounding (2^-9 relative) of
an f32 product of an exactly representable sum (at most k bf16 values) with gelu'(x) in f32.  Layer 0: dW0, dgamma and dbeta to a
relative L2 of ``F32_TOL`` (1e-5): everything is f32, and the same arithmetic in stock float32 on a CPU is at 1.4e-7 to 4.3e-7, so the
bound is not the reference's own noise.  Every measured figure is printed (profiles/w2v_feature_encoder.txt holds those lines from
an MI355X)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_ref  # noqa: E402
from helpers import _lib, l2_rel  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402

BF16 = torch.bfloat16
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
N = 2
# (k, s, T_in): (3, 2, 37) has no unread tail, (3, 2, 38), (2, 2, 9) and (4, 3, 23) leave their last frame unread
FOLD_SHAPES = [(3, 2, 37), (3, 2, 38), (2, 2, 9), (3, 1, 20), (4, 3, 23)]
FOLD_CASES = [(k, s, T, C) for k, s, T in FOLD_SHAPES for C in (8, 256, 512)]
FOLD_IDS = [f"k{k}-s{s}-T{T}-C{C}" for k, s, T, C in FOLD_CASES]
_fold, _l0 = {}, {}


def _fold_case(k, s, T_in, C, n=N):
    """bf16 x and dwin of ``n`` clips, and on them in float64: dx = d/dx <dwin, window(gelu(x))> and sum |terms| (the same with |dwin|, in
    absolute value)"""
    key = (k, s, T_in, C) if n == N else (k, s, T_in, C, n)
    if key not in _fold:
        g = torch.Generator().manual_seed(1000 * k + 100 * s + T_in + C)
        T_out = (T_in - k) // s + 1
        x = (1.5 * torch.randn(n, T_in, C, generator=g)).to(BF16)
        dwin = torch.randn(n, T_out, k * C, generator=g).to(BF16)
        xd = x.double().requires_grad_(True)
        out = w2v_ref.window(w2v_ref.gelu_erf(xd), k, s)
        (dx,) = torch.autograd.grad(out, xd, dwin.double(), retain_graph=True)
        (terms,) = torch.autograd.grad(out, xd, dwin.double().abs())
        _fold[key] = dict(x=x, dwin=dwin, dx=dx, terms=terms.abs(), T_out=T_out, last=s * (T_out - 1) + k - 1)
    return _fold[key]


def fold_bound(c):
    """the module docstring's bound of the fold, per element of dx"""
    return 2.0 ** -8 * c["dx"].abs() + 1e-6 * c["terms"]


def _run_fold(c, k, s, T_in, C, in_place=False):
    lib = _lib()
    x = c["x"].cuda()
    dx = x if in_place else torch.full((N, T_in, C), float("nan"), dtype=BF16, device="cuda")
    lib.w2v_window_fold_gelu_bwd(c["dwin"].cuda(), x, dx, N, T_in, C, k, s)
    torch.cuda.synchronize()
    return dx.cpu()


@pytest.mark.parametrize("k,s,T_in,C", FOLD_CASES, ids=FOLD_IDS)
def test_window_fold_against_float64(k, s, T_in, C):
    c = _fold_case(k, s, T_in, C)
    got = _run_fold(c, k, s, T_in, C)
    assert bool(torch.isfinite(got).all()), "a row of dx was skipped (the output was prefilled with NaN)"
    err = (got.double() - c["dx"]).abs()
    bound = fold_bound(c)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"window_fold_gelu_bwd k={k} s={s} T_in={T_in} C={C}: worst |got - exact| / bound {worst:.3f}, rel L2 {l2_rel(got, c['dx']):.3e}, "
          f"{T_in - 1 - c['last']} unread frame(s)")
    assert bool((err <= bound).all())
    if c["last"] < T_in - 1:                                       # frames no window reads: zeros, written
        assert not bool(got[:, c["last"] + 1:].any()) and not bool(c["dx"][:, c["last"] + 1:].any())
    again = _run_fold(c, k, s, T_in, C)
    assert torch.equal(_bits(again), _bits(got)), "two launches differ"
    assert torch.equal(_bits(_run_fold(c, k, s, T_in, C, in_place=True)), _bits(got)), "dx in the place of x differs"


# ---- layer 0 ----------------------------------------------------------------------------------------------------------
K0, S0, K1, S1 = 10, 5, 3, 2
L0_CASES = [(C0, L) for L in (3007, 310) for C0 in (8, 256, 512)]
L0_IDS = [f"C{C0}-L{L}" for C0, L in L0_CASES]


def _l0_case(C0, L):
    """wave, f32 parameters, a bf16 dwin_1, and the float64 autograd gradients of <dwin_1, window(gelu(groupnorm(conv0(wave))))>"""
    key = (C0, L)
    if key not in _l0:
        g = torch.Generator().manual_seed(C0 + L)
        T0 = (L - K0) // S0 + 1
        T1 = (T0 - K1) // S1 + 1
        wave = 0.5 * torch.randn(N, L, generator=g) + 0.1
        w = torch.randn(C0, 1, K0, generator=g) * math.sqrt(2.0 / K0)
        gamma, beta = 1.0 + 0.2 * torch.randn(C0, generator=g), 0.1 * torch.randn(C0, generator=g)
        dwin = torch.randn(N, T1, K1 * C0, generator=g).to(BF16)
        wd, gd, bd = (t.double().requires_grad_(True) for t in (w, gamma, beta))
        raw = w2v_ref.conv0_raw(wave.double(), wd, S0)
        mean, var = w2v_ref.conv0_stats(raw)
        y = (raw - mean) / torch.sqrt(var + w2v_ref.GN_EPS) * gd + bd
        dw, dgamma, dbeta = torch.autograd.grad(w2v_ref.window(w2v_ref.gelu_erf(y), K1, S1), [wd, gd, bd], dwin.double())
        _l0[key] = dict(wave=wave, w=w, gamma=gamma, beta=beta, dwin=dwin, dw=dw, dgamma=dgamma, dbeta=dbeta, T0=T0, T1=T1)
    return _l0[key]


def _run_l0(c, C0, into=None, accumulate=False):
    """-> (dW0, dgamma, dbeta) on the CPU; ``into``: what the three outputs hold before the launches (None: NaN)"""
    lib = _lib()
    dev = "cuda"
    wave, w, gamma, beta, dwin = (c[n].cuda() for n in ("wave", "w", "gamma", "beta", "dwin"))
    stats = torch.empty(N * 2 * C0, device=dev)
    part = torch.empty(N * lib.W2V_STATS_SLOTS * 2 * C0, device=dev)
    lib.w2v_conv0_stats(wave, w, stats, part, K0, S0)
    outs = [torch.full_like(t, float("nan")) for t in (w, gamma, beta)] if into is None else [t.cuda().clone() for t in into]
    dw, dgamma, dbeta = outs
    sums = torch.full((N * 2 * C0,), float("nan"), device=dev)
    lib.w2v_conv0_bwd_stats(wave, w, stats, gamma, beta, dwin, sums, part, dgamma, dbeta, K0, S0, K1, S1, w2v_ref.GN_EPS, accumulate)
    wpart = torch.full((N * lib.W2V_STATS_SLOTS * C0 * K0,), float("nan"), device=dev)
    lib.w2v_conv0_bwd_wgrad(wave, w, stats, gamma, beta, dwin, sums, wpart, dw, K0, S0, K1, S1, w2v_ref.GN_EPS, accumulate)
    torch.cuda.synchronize()
    return [t.cpu() for t in outs]


@pytest.mark.parametrize("C0,L", L0_CASES, ids=L0_IDS)
def test_layer0_backward_against_float64(C0, L):
    """L = 3007: T0 = 600, frame 599 is read by no window of layer 1 and two samples by no frame; L = 310: T0 = 61, fewer frames
    than frame lanes.  Overwriting (NaN underneath), accumulating onto a fill, and the bits of two launches"""
    c = _l0_case(C0, L)
    assert (c["T0"], S1 * (c["T1"] - 1) + K1 - 1) == ((600, 598) if L == 3007 else (61, 60))
    got = _run_l0(c, C0)
    exact = (c["dw"], c["dgamma"], c["dbeta"])
    for name, a, b in zip(("dW0", "dgamma", "dbeta"), got, exact):
        e = l2_rel(a.double(), b)
        print(f"conv0 backward C0={C0} L={L}: {name} rel L2 {e:.3e} (bound {F32_TOL})")
        assert bool(torch.isfinite(a).all()) and e <= F32_TOL, name
    again = _run_l0(c, C0)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again)), "two launches differ"
    g = torch.Generator().manual_seed(9)
    fill = [torch.randn(t.shape, generator=g) * float(t.abs().max()) for t in exact]
    added = _run_l0(c, C0, into=fill, accumulate=True)
    for name, a, f, b in zip(("dW0", "dgamma", "dbeta"), added, fill, exact):
        e = l2_rel(a.double(), f.double() + b)
        print(f"conv0 backward C0={C0} L={L}: {name} added to what the buffer held, rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, name
    over = _run_l0(c, C0, into=fill, accumulate=False)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(over, got)), "overwriting depends on what the buffer held"


def test_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    Lb = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    nan32 = torch.full((1 << 17,), float("nan"), device="cuda")
    f = torch.zeros(1 << 16, device="cuda")
    b = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    fold = lambda dwin=p(b), x=p(b, 1 << 15), dx=p(nan16), N_=1, T=20, C=16, k=3, s_=2: \
        Lb.mmf_w2v_window_fold_gelu_bwd(dwin, x, dx, N_, T, C, k, s_, s)
    st = lambda wave=p(f), w=p(f), stats=p(f), ga=p(f), be=p(f), dwin=p(b), sums=p(nan32), part=p(nan32, 1 << 12), dg=p(nan32, 1 << 16), \
        db=p(nan32, (1 << 16) + 256), N_=1, L=100, C0=16, k0=10, s0=5, k1=3, s1=2: \
        Lb.mmf_w2v_conv0_bwd_stats(wave, w, stats, ga, be, dwin, sums, part, dg, db, N_, L, C0, k0, s0, k1, s1, 1e-5, 0, s)
    wg = lambda wave=p(f), w=p(f), stats=p(f), ga=p(f), be=p(f), dwin=p(b), sums=p(f), part=p(nan32), dw=p(nan32, 1 << 18), N_=1, L=100, \
        C0=16, k0=10, s0=5, k1=3, s1=2: \
        Lb.mmf_w2v_conv0_bwd_wgrad(wave, w, stats, ga, be, dwin, sums, part, dw, N_, L, C0, k0, s0, k1, s1, 1e-5, 0, s)
    F, S, W = "mmf_w2v_window_fold_gelu_bwd", "mmf_w2v_conv0_bwd_stats", "mmf_w2v_conv0_bwd_wgrad"
    cases = [
        (F, lambda: fold(dwin=None), E_SHAPE), (F, lambda: fold(x=None), E_SHAPE), (F, lambda: fold(dx=None), E_SHAPE),
        (F, lambda: fold(T=0), E_SHAPE), (F, lambda: fold(T=2), E_SHAPE), (F, lambda: fold(k=0), E_SHAPE), (F, lambda: fold(s_=0), E_SHAPE),
        (F, lambda: fold(C=12), E_UNSUPPORTED), (F, lambda: fold(k=2, s_=3), E_UNSUPPORTED), (F, lambda: fold(N_=65536), E_UNSUPPORTED),
        (F, lambda: fold(dwin=p(nan16)), E_UNSUPPORTED), (F, lambda: fold(dwin=p(b, 1 << 15)), E_UNSUPPORTED),
        (F, lambda: fold(dx=p(nan16, 8)), E_ALIGN), (F, lambda: fold(dwin=p(b, 2)), E_ALIGN),
        (S, lambda: st(wave=None), E_SHAPE), (S, lambda: st(dwin=None), E_SHAPE), (S, lambda: st(sums=None), E_SHAPE),
        (S, lambda: st(db=None), E_SHAPE), (S, lambda: st(L=9), E_SHAPE), (S, lambda: st(N_=0), E_SHAPE), (S, lambda: st(k1=0), E_SHAPE),
        (S, lambda: st(L=15, k1=3), E_SHAPE),                                          # T0 = 2 frames under a kernel of 3
        (S, lambda: st(C0=12), E_UNSUPPORTED), (S, lambda: st(k0=17), E_UNSUPPORTED), (S, lambda: st(C0=2056), E_UNSUPPORTED),
        (S, lambda: st(dwin=p(b, 2)), E_ALIGN), (S, lambda: st(sums=p(nan32, 4)), E_ALIGN), (S, lambda: st(wave=p(f, 2)), E_ALIGN),
        (W, lambda: wg(w=None), E_SHAPE), (W, lambda: wg(dwin=None), E_SHAPE), (W, lambda: wg(dw=None), E_SHAPE),
        (W, lambda: wg(L=9), E_SHAPE), (W, lambda: wg(s1=0), E_SHAPE), (W, lambda: wg(L=15, k1=3), E_SHAPE),
        (W, lambda: wg(C0=12), E_UNSUPPORTED), (W, lambda: wg(k0=17), E_UNSUPPORTED), (W, lambda: wg(N_=65536), E_UNSUPPORTED),
        (W, lambda: wg(dwin=p(b, 8)), E_ALIGN), (W, lambda: wg(dw=p(nan32, 2)), E_ALIGN),
    ]
    for i, (name, fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, (i, name, rc, want, Lb.mmf_last_error())
        assert name.encode() in Lb.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all())           # nothing was launched
