"""GPU: the positional-convolution kernels and ``mmf_w2v_weightnorm_bwd`` (csrc/wav2vec2.hip) on the random bf16 operands of
tests/test_w2v_finetune_kernels_gpu.py, bounded PER ELEMENT where that file bounds the relative L2.

  |got - exact| <= lead(exact) + G x gamma x sum|terms|          (tests/w2v_kernel_checks.py)
lead is one bf16 ulp of the float64 result (2^-24 |exact| for the wgrad's f32 output), sum|terms| the float64 convolution of |w| and
|x| (plus |b|), G the epilogue's derivative bound (1 for the dgrad, sup|gelu'| for the forward, |dy| sup|gelu''| for bwd_act) and gamma
the f32 summation error relative to sum|terms|.  gamma is not fixed in advance: it is measured per case on the CPU, the same
contraction in float32 in two orders against float64, the worst element taken four times over because the MFMA's own order is a third
one.  It is printed per case (profiles/w2v_kernel_pins.txt).

``mmf_w2v_weightnorm_bwd`` is f32 throughout: dg and dv per element within F32_TOL x max(|ref|, 1), in the overwriting and in the adding
form, two runs bit-equal.  At (768, 48, 128), where a tap's two reductions run over 36864 elements, the bound is four times the measured
error of the f32 CPU restatement if that itself exceeds F32_TOL."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_grad_ref as G  # noqa: E402
import w2v_kernel_checks as K  # noqa: E402
import w2v_ref  # noqa: E402
from helpers import _lib  # noqa: E402
from test_deberta_grad_gpu import F32_TOL  # noqa: E402
from test_w2v_finetune_kernels_gpu import CASES as FT_CASES, _case, _run_wgrad  # noqa: E402

BF16 = torch.bfloat16
GUARD = 4096
CASES = FT_CASES + [(2, 160, 2, 32, 16), (2, 129, 2, 16, 5)]
IDS = [f"T{c[1]}-cg{c[3]}-k{c[4]}" for c in CASES]
_refs = {}


def _ref(N, T, groups, cg, k):
    """per case, once: the three contractions in float64 with their sum|terms| and measured gamma"""
    key = (N, T, groups, cg, k)
    if key not in _refs:
        c = _case(N, T, groups, cg, k)
        x, w, dz16 = c["x"].double(), c["w"].double(), c["dz16"].double()
        conv, terms, gamma = K.gamma_conv(x, G.pack(w), cg, k, k // 2)
        r = dict(z=conv + c["bias"].double(), z_terms=terms + c["bias"].double().abs(), z_gamma=gamma)
        r["dconv"], r["d_terms"], r["d_gamma"] = K.gamma_conv(dz16, G.pack_transposed(w), cg, k, k - 1 - k // 2)
        r["dw"], r["w_terms"], r["w_gamma"] = K.gamma_wgrad(dz16, x, cg, k)
        assert float((r["z"] - w2v_ref.pos_conv(x, w, c["bias"].double(), groups)).abs().max()) < 1e-9
        assert float((r["dconv"] + c["dy"].double() - c["dx0"]).abs().max()) < 1e-9 and float((G.unpack(r["dw"], cg) - c["dw"]).abs().max()) < 1e-9
        _refs[key] = r
    return _refs[key]


def _nan(N, T, C):
    return torch.full((N * T * C + GUARD,), float("nan"), dtype=BF16, device="cuda")


def _got(what, buf, N, T, C):
    torch.cuda.synchronize()
    n = N * T * C
    assert not bool(torch.isnan(buf[:n]).any()) and bool(torch.isnan(buf[n:]).all()), f"{what}: NaN in the output, or the guard written"
    return buf[:n].view(N, T, C).cpu()


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_forward_per_element(N, T, groups, cg, k):
    lib, c, r = _lib(), _case(N, T, groups, cg, k), _ref(N, T, groups, cg, k)
    C = c["C"]
    buf = _nan(N, T, C)
    lib.w2v_posconv(c["x"].cuda(), c["packed"].cuda(), c["bias"].cuda(), buf, N, T, C, groups, k)
    want = c["x"].double() + w2v_ref.gelu_erf(r["z"])
    worst = K.worst(_got("posconv", buf, N, T, C), want, K.elementwise_bound(want, r["z_terms"], K.GELU_D1_SUP, r["z_gamma"]))
    print(f"PARITY posconv per element N={N} T={T} groups={groups} cg={cg} k={k}: worst error / bound {worst:.3f} (bound 1); gamma {r['z_gamma']:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_bwd_act_per_element(N, T, groups, cg, k):
    lib, c, r = _lib(), _case(N, T, groups, cg, k), _ref(N, T, groups, cg, k)
    C = c["C"]
    buf = _nan(N, T, C)
    lib.w2v_posconv_bwd_act(c["x"].cuda(), c["packed"].cuda(), c["bias"].cuda(), c["dy"].cuda(), buf, N, T, C, groups, k)
    dy = c["dy"].double()
    want = dy * K.gelu_grad(r["z"])
    assert float((want - c["dz"]).abs().max()) < 1e-9                                    # the closed form against autograd's
    worst = K.worst(_got("posconv_bwd_act", buf, N, T, C), want,
                    K.elementwise_bound(want, r["z_terms"], dy.abs() * K.GELU_D2_SUP, r["z_gamma"]))
    print(f"PARITY posconv_bwd_act per element N={N} T={T} groups={groups} cg={cg} k={k}: worst error / bound {worst:.3f} (bound 1); "
          f"gamma {r['z_gamma']:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_dgrad_per_element(N, T, groups, cg, k):
    lib, c, r = _lib(), _case(N, T, groups, cg, k), _ref(N, T, groups, cg, k)
    C = c["C"]
    buf = _nan(N, T, C)
    lib.w2v_posconv_dgrad(c["dz16"].cuda(), c["packed_t"].cuda(), c["dy"].cuda(), buf, N, T, C, groups, k)
    want = c["dy"].double() + r["dconv"]
    worst = K.worst(_got("posconv_dgrad", buf, N, T, C), want, K.elementwise_bound(want, r["d_terms"], 1.0, r["d_gamma"]))
    print(f"PARITY posconv_dgrad per element N={N} T={T} groups={groups} cg={cg} k={k}: worst error / bound {worst:.3f} (bound 1); "
          f"gamma {r['d_gamma']:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("slabs", [1, 2], ids=["plain", "two-slabs"])
@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_wgrad_per_element(N, T, groups, cg, k, slabs):
    c, r = _case(N, T, groups, cg, k), _ref(N, T, groups, cg, k)
    if slabs > N * ((T + 127) // 128):
        slabs = 1                                                                       # (one unit: the plain form again)
    raw = _run_wgrad(c, N, T, groups, k, slabs)
    assert bool((raw[:, k * cg:] == 0).all())
    worst = K.worst(raw[:, :k * cg], r["dw"], K.elementwise_bound(r["dw"], r["w_terms"], 1.0, r["w_gamma"], f32_out=True))
    print(f"PARITY posconv_wgrad per element N={N} T={T} groups={groups} cg={cg} k={k} slabs={slabs}: worst error / bound {worst:.3f} (bound 1); "
          f"gamma {r['w_gamma']:.3e}")
    assert worst <= 1.0


WN_CASES = [(96, 48, 15), (128, 64, 16), (768, 48, 128), (32, 16, 5)]


@pytest.mark.parametrize("C,cg,k", WN_CASES)
def test_weightnorm_bwd_per_element(C, cg, k):
    lib = _lib()
    g = torch.Generator().manual_seed(C + k)
    gain = 1.0 + torch.rand(1, 1, k, generator=g)
    v, dw = torch.randn(C, cg, k, generator=g), torch.randn(C, cg, k, generator=g)
    fill_g, fill_v = torch.randn(1, 1, k, generator=g), torch.randn(C, cg, k, generator=g)
    ref_g, ref_v = G.weightnorm_bwd(dw.double(), gain.double(), v.double())
    cpu_g, cpu_v = K.weightnorm_f32(dw, gain, v)
    cpu_err = max(K.scaled_err(cpu_g, ref_g), K.scaled_err(cpu_v, ref_v))
    tol = K.ORDER_MARGIN * cpu_err if (C, cg, k) == (768, 48, 128) and cpu_err > F32_TOL else F32_TOL
    packed = K.padded(G.pack(dw), K.kp_of(k, cg)).cuda()
    n, outs = C * cg * k, []
    for over in (True, False, True):
        dg, buf = fill_g.cuda().clone(), torch.full((n + GUARD,), float("nan"), device="cuda")
        buf[:n] = fill_v.cuda().view(-1)
        ins = packed, gain.cuda(), v.cuda()
        before = [K.bits(t).clone() for t in ins]
        lib.w2v_weightnorm_bwd(*ins, dg, buf[:n].view(C, cg, k), over)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[n:]).all()) and all(torch.equal(K.bits(t), b) for t, b in zip(ins, before))
        outs.append((dg.cpu(), buf[:n].view(C, cg, k).cpu()))
    (dg, dv), (dg_add, dv_add), (dg2, dv2) = outs
    assert torch.equal(K.bits(dg), K.bits(dg2)) and torch.equal(K.bits(dv), K.bits(dv2)), "two runs differ"
    want_g = fill_g.double() + ref_g
    errs = {"dg": K.scaled_err(dg, want_g), "dv": K.scaled_err(dv, ref_v), "dg, adding form": K.scaled_err(dg_add, want_g),
            "dv, adding form": K.scaled_err(dv_add, fill_v.double() + ref_v)}
    print(f"PARITY weightnorm_bwd per element C={C} cg={cg} k={k}: " + ", ".join(f"{n_} {e:.3e}" for n_, e in errs.items())
          + f" (bound {tol:.3e} x max(|ref|, 1)); the f32 CPU restatement's own error {cpu_err:.3e} (F32_TOL {F32_TOL})")
    assert all(e <= tol for e in errs.values())
