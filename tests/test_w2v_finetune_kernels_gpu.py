"""GPU: the kernels of the positional convolution's backward (csrc/wav2vec2.hip) against float64 autograd on the same bf16 inputs:
``mmf_w2v_posconv_bwd_act`` (dz = dy gelu'(z), z computed again), ``mmf_w2v_posconv_wgrad`` (the weight gradient, an MFMA GEMM
over time), ``mmf_w2v_posconv_dgrad`` (the forward's kernel on the reversed / swapped weight) and ``mmf_w2v_weightnorm_bwd``.

Bound: relative L2 <= BOUND_A, the project's bound for a kernel against an oracle with the same storage format, on the whole
tensor and separately on the first and last k/2 frames (dz, dx0) and on the first, middle and last tap (dW).  Every measured error
is printed (profiles/w2v_finetune.txt holds those lines from an MI355X)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_grad_ref as G  # noqa: E402
import w2v_ref  # noqa: E402
from helpers import BOUND_A, _lib, l2_rel  # noqa: E402
from test_deberta_grad_gpu import F32_TOL, _bits  # noqa: E402

BF16 = torch.bfloat16
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
CASES = [
    (2, 499, 16, 48, 128),            # the real shape
    (3, 199, 4, 64, 16),              # even k, 64 wide
    (2, 77, 4, 48, 15),               # odd k, T below one time block
    (1, 130, 2, 16, 5),               # T just past a 128-row block
    (1, 9, 2, 32, 16),                # T shorter than k
]
IDS = [f"T{c[1]}-cg{c[3]}-k{c[4]}" for c in CASES]
_cases = {}


def _packed(p, Kp):
    out = torch.zeros(p.shape[0], Kp, dtype=p.dtype)
    out[:, :p.shape[1]] = p
    return out


def _case(N, T, groups, cg, k):
    """bf16 operands and the float64 autograd results on them, once per case: dz of (x, w, bias, dy); dW of (x, bf16(dz)); dx0 of
    (bf16(dz), w, dy)"""
    key = (N, T, groups, cg, k)
    if key in _cases:
        return _cases[key]
    C = groups * cg
    g = torch.Generator().manual_seed(T + k)
    x = torch.randn(N, T, C, generator=g).to(BF16)
    w = (torch.randn(C, cg, k, generator=g) * math.sqrt(2.0 / (cg * k))).to(BF16)
    bias = 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(N, T, C, generator=g).to(BF16)
    Kp = (k * cg + 31) // 32 * 32
    c = dict(C=C, Kp=Kp, x=x, w=w, bias=bias, dy=dy, packed=_packed(G.pack(w), Kp), packed_t=_packed(G.pack_transposed(w), Kp))
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    z = w2v_ref.pos_conv(xd, wd, bias.double(), groups).detach().requires_grad_(True)
    (c["dz"],) = torch.autograd.grad(w2v_ref.gelu_erf(z), z, dy.double())
    c["dz16"] = c["dz"].to(BF16)
    dx, dw = torch.autograd.grad(w2v_ref.pos_conv(xd, wd, bias.double(), groups), [xd, wd], c["dz16"].double())
    c["dx0"], c["dw"] = dy.double() + dx, dw                                            # (C, cg, k)
    _cases[key] = c
    return c


def _edges(T, k):
    h = max(k // 2, 1)
    return torch.unique(torch.cat([torch.arange(0, min(h, T)), torch.arange(max(T - h, 0), T)]))


def _unpacked(dw, C, cg, k):
    return G.unpack(dw.view(C, -1)[:, :k * cg], cg)


def _run_wgrad(c, N, T, groups, k, slabs=1, accumulate=False, into=None, x=None, dz=None):
    lib = _lib()
    C, Kp = c["C"], c["Kp"]
    x, dz = (c["x"] if x is None else x), (c["dz16"] if dz is None else dz)
    n = x.shape[0]
    dw = torch.full((slabs, C, Kp), float("nan"), device="cuda") if into is None else into
    lib.w2v_posconv_wgrad(dz.cuda().contiguous(), x.cuda().contiguous(), dw, n, T, C, groups, k, slabs=slabs, accumulate=accumulate)
    if slabs > 1:
        out = torch.full((C, Kp), float("nan"), device="cuda")
        lib.sum_slabs(dw.view(slabs, -1), out, False)
        dw = out
    torch.cuda.synchronize()
    return dw.view(C, Kp).cpu()


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_bwd_act_against_float64(N, T, groups, cg, k):
    lib, c = _lib(), _case(N, T, groups, cg, k)
    C = c["C"]
    x, dy = c["x"].cuda(), c["dy"].cuda()
    before = _bits(x), _bits(dy)
    dz = torch.full((N, T, C), float("nan"), dtype=BF16, device="cuda")
    lib.w2v_posconv_bwd_act(x, c["packed"].cuda(), c["bias"].cuda(), dy, dz, N, T, C, groups, k)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), before[0]) and torch.equal(_bits(dy), before[1])
    got, e = dz.cpu().double(), _edges(T, k)
    err, err_edge = l2_rel(got, c["dz"]), l2_rel(got[:, e], c["dz"][:, e])
    print(f"posconv_bwd_act cg={cg} k={k} T={T}: dz rel L2 {err:.3e}, boundary frames {err_edge:.3e} (bound {BOUND_A})")
    assert not torch.isnan(got).any() and err <= BOUND_A and err_edge <= BOUND_A


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_dgrad_against_float64(N, T, groups, cg, k):
    lib, c = _lib(), _case(N, T, groups, cg, k)
    C = c["C"]
    dx = torch.full((N, T, C), float("nan"), dtype=BF16, device="cuda")
    lib.w2v_posconv_dgrad(c["dz16"].cuda(), c["packed_t"].cuda(), c["dy"].cuda(), dx, N, T, C, groups, k)
    torch.cuda.synchronize()
    got, e = dx.cpu().double(), _edges(T, k)
    conv = c["dx0"] - c["dy"].double()                                                  # without the residual, which would hide it
    err, err_edge = l2_rel(got, c["dx0"]), l2_rel(got[:, e], c["dx0"][:, e])
    err_conv = l2_rel(got - c["dy"].double(), conv)
    print(f"posconv_dgrad cg={cg} k={k} T={T}: dx0 rel L2 {err:.3e}, boundary frames {err_edge:.3e}, the convolution's part alone "
          f"{err_conv:.3e} (bound {BOUND_A})")
    assert not torch.isnan(got).any() and err <= BOUND_A and err_edge <= BOUND_A and err_conv <= BOUND_A


@pytest.mark.parametrize("slabs", [1, 2], ids=["plain", "two-slabs"])
@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_wgrad_against_float64(N, T, groups, cg, k, slabs):
    c = _case(N, T, groups, cg, k)
    C, Kp = c["C"], c["Kp"]
    if slabs > N * ((T + 127) // 128):
        slabs = 1                                                                       # (one unit: the plain form again)
    raw = _run_wgrad(c, N, T, groups, k, slabs)
    again = _run_wgrad(c, N, T, groups, k, slabs)
    assert torch.equal(_bits(raw), _bits(again)), "two runs differ"
    assert bool(torch.isfinite(raw).all()) and bool((raw[:, k * cg:] == 0).all())      # the padding columns are written as zeros
    got, want = _unpacked(raw, C, cg, k).double(), c["dw"]
    err = l2_rel(got, want)
    taps = {"first": 0, "middle": k // 2, "last": k - 1}
    per = {n: l2_rel(got[:, :, j], want[:, :, j]) for n, j in taps.items()}
    print(f"posconv_wgrad cg={cg} k={k} T={T} slabs={slabs}: dW rel L2 {err:.3e}; " + ", ".join(f"{n} tap {v:.3e}" for n, v in per.items())
          + f" (bound {BOUND_A})")
    assert err <= BOUND_A and all(v <= BOUND_A for v in per.values())


@pytest.mark.parametrize("N,T,groups,cg,k", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_wgrad_accumulates_over_two_calls(N, T, groups, cg, k):
    """call 1 (written) + call 2 (added) on the two parts of the clips = the oracle of all clips"""
    c = _case(N, T, groups, cg, k)
    C, Kp = c["C"], c["Kp"]
    dw = torch.full((1, C, Kp), float("nan"), device="cuda")
    _run_wgrad(c, N, T, groups, k, into=dw, x=c["x"][:1], dz=c["dz16"][:1])
    raw = _run_wgrad(c, N, T, groups, k, accumulate=True, into=dw, x=c["x"][1:], dz=c["dz16"][1:])
    err = l2_rel(_unpacked(raw, C, cg, k).double(), c["dw"])
    print(f"posconv_wgrad cg={cg} k={k} T={T}: call 1 + call 2 against the oracle of all clips, rel L2 {err:.3e} (bound {BOUND_A})")
    assert bool((raw[:, k * cg:] == 0).all()) and err <= BOUND_A


@pytest.mark.parametrize("C,cg,k", [(768, 48, 128), (256, 64, 16), (192, 48, 15), (32, 16, 5)])
def test_weightnorm_bwd_against_float64(C, cg, k):
    lib = _lib()
    g = torch.Generator().manual_seed(C + k)
    gain = 1.0 + torch.rand(1, 1, k, generator=g)
    v = torch.randn(C, cg, k, generator=g)
    dw = torch.randn(C, cg, k, generator=g)
    Kp = (k * cg + 31) // 32 * 32
    want_g, want_v = G.weightnorm_bwd(dw.double(), gain.double(), v.double())
    leaves = gain.double().requires_grad_(True), v.double().requires_grad_(True)
    ag, av = torch.autograd.grad(w2v_ref.pos_weight({w2v_ref.WN_NEW[0]: leaves[0], w2v_ref.WN_NEW[1]: leaves[1]}), leaves, dw.double())
    assert l2_rel(want_g, ag) < 1e-10 and l2_rel(want_v, av) < 1e-10
    packed = _packed(G.pack(dw), Kp).cuda()
    fill_g, fill_v = torch.randn(1, 1, k, generator=g), torch.randn(C, cg, k, generator=g)
    outs = []
    for over in (True, False, True):
        dg, dv = fill_g.cuda().clone(), fill_v.cuda().clone()
        lib.w2v_weightnorm_bwd(packed, gain.cuda(), v.cuda(), dg, dv, over)
        torch.cuda.synchronize()
        outs.append((dg.cpu(), dv.cpu()))
    (dg, dv), (dg_add, dv_add), (dg2, dv2) = outs
    assert torch.equal(_bits(dv), _bits(dv2)) and torch.equal(_bits(dg), _bits(dg2)), "two runs differ"
    e_g, e_v = l2_rel((dg - fill_g).double(), ag), l2_rel(dv.double(), av)
    e_add = l2_rel((dv_add - fill_v).double(), av)
    print(f"weightnorm_bwd C={C} cg={cg} k={k}: dg rel L2 {e_g:.3e}, dv {e_v:.3e}, dv added to what the buffer held {e_add:.3e} (bound {BOUND_A})")
    assert e_g <= BOUND_A and e_v <= BOUND_A and e_add <= BOUND_A
    assert e_g <= 1e-4 and e_v <= 1e-4                    # f32 throughout: well inside the storage bound


def test_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    nan32 = torch.full((1 << 16,), float("nan"), device="cuda")
    f = torch.zeros(1 << 16, device="cuda")
    b = torch.zeros(1 << 18, dtype=BF16, device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    act = lambda x=p(b), w=p(b), bias=p(f), dy=p(b), dz=p(nan16), N=1, T=40, C=64, G_=2, k=5: \
        L.mmf_w2v_posconv_bwd_act(x, w, bias, dy, dz, N, T, C, G_, k, s)
    dgr = lambda dz=p(b), w=p(b), dy=p(b), dx=p(nan16), N=1, T=40, C=64, G_=2, k=5: L.mmf_w2v_posconv_dgrad(dz, w, dy, dx, N, T, C, G_, k, s)
    wgr = lambda dz=p(b), x=p(b), dw=p(nan32), N=1, T=40, C=64, G_=2, k=5, S=1, acc=0: L.mmf_w2v_posconv_wgrad(dz, x, dw, N, T, C, G_, k, S, acc, s)
    wn = lambda dw=p(f), g=p(f), v=p(f), dg=p(nan32), dv=p(nan32, 4096), C=32, cg=16, k=5, over=1: L.mmf_w2v_weightnorm_bwd(dw, g, v, dg, dv, C, cg, k, over, s)
    cases = [
        ("mmf_w2v_posconv_bwd_act", lambda: act(x=None), E_SHAPE), ("mmf_w2v_posconv_bwd_act", lambda: act(bias=None), E_SHAPE),
        ("mmf_w2v_posconv_bwd_act", lambda: act(dy=None), E_SHAPE), ("mmf_w2v_posconv_bwd_act", lambda: act(T=0), E_SHAPE),
        ("mmf_w2v_posconv_bwd_act", lambda: act(C=64, G_=3), E_SHAPE), ("mmf_w2v_posconv_bwd_act", lambda: act(C=48, G_=2), E_UNSUPPORTED),
        ("mmf_w2v_posconv_bwd_act", lambda: act(C=160, G_=2), E_UNSUPPORTED), ("mmf_w2v_posconv_bwd_act", lambda: act(C=128, G_=2, k=400), E_UNSUPPORTED),
        ("mmf_w2v_posconv_bwd_act", lambda: act(x=p(nan16)), E_UNSUPPORTED), ("mmf_w2v_posconv_bwd_act", lambda: act(dy=p(b, 2)), E_ALIGN),
        ("mmf_w2v_posconv_bwd_act", lambda: act(dz=p(nan16, 8)), E_ALIGN),
        ("mmf_w2v_posconv_dgrad", lambda: dgr(w=None), E_SHAPE), ("mmf_w2v_posconv_dgrad", lambda: dgr(k=0), E_SHAPE),
        ("mmf_w2v_posconv_dgrad", lambda: dgr(C=48, G_=2), E_UNSUPPORTED), ("mmf_w2v_posconv_dgrad", lambda: dgr(C=128, G_=2, k=400), E_UNSUPPORTED),
        ("mmf_w2v_posconv_dgrad", lambda: dgr(dz=p(nan16)), E_UNSUPPORTED), ("mmf_w2v_posconv_dgrad", lambda: dgr(dx=p(nan16, 4)), E_ALIGN),
        ("mmf_w2v_posconv_wgrad", lambda: wgr(dw=None), E_SHAPE), ("mmf_w2v_posconv_wgrad", lambda: wgr(S=0), E_SHAPE),
        ("mmf_w2v_posconv_wgrad", lambda: wgr(S=2), E_SHAPE),                       # more slabs than (clip, block) units
        ("mmf_w2v_posconv_wgrad", lambda: wgr(N=2, S=2, acc=1), E_SHAPE),           # slab partials are written, not added to
        ("mmf_w2v_posconv_wgrad", lambda: wgr(N=70, T=1, S=65), E_SHAPE), ("mmf_w2v_posconv_wgrad", lambda: wgr(C=64, G_=3), E_SHAPE),
        ("mmf_w2v_posconv_wgrad", lambda: wgr(C=48, G_=2), E_UNSUPPORTED), ("mmf_w2v_posconv_wgrad", lambda: wgr(C=128, G_=2, k=400), E_UNSUPPORTED),
        ("mmf_w2v_posconv_wgrad", lambda: wgr(dw=p(nan32, 4)), E_ALIGN), ("mmf_w2v_posconv_wgrad", lambda: wgr(x=p(b, 2)), E_ALIGN),
        ("mmf_w2v_weightnorm_bwd", lambda: wn(dv=None), E_SHAPE), ("mmf_w2v_weightnorm_bwd", lambda: wn(k=0), E_SHAPE),
        ("mmf_w2v_weightnorm_bwd", lambda: wn(C=40), E_SHAPE), ("mmf_w2v_weightnorm_bwd", lambda: wn(C=1 << 15, cg=1 << 15, k=4), E_UNSUPPORTED),
        ("mmf_w2v_weightnorm_bwd", lambda: wn(dw=p(f, 4)), E_ALIGN), ("mmf_w2v_weightnorm_bwd", lambda: wn(dg=p(nan32, 2)), E_ALIGN),
    ]
    for i, (name, fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, (i, name, rc, want, L.mmf_last_error())
        assert name.encode() in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all())           # nothing was launched
    assert F32_TOL < BOUND_A
