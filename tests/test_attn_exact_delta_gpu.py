"""GPU: ``mmf_attn_delta_f32`` (the softmax backward's row term by its definition, delta_i = sum_j p_ij dp_ij, in f32) and
``mmf_attn_bwd_grouped_delta`` (the fused attention backward with that delta as an input) against float64 on the same bf16
operands, on the fused q | k | v rows the backbones use.

Bounds.  delta: per row 1e-4 x sum_j p_ij |dO_i| |v_j|, the size of the terms it sums (f32 products and sums of 64 / 96 + T terms
and the forward's f32 LSE: a few 1e-6 of that, taken with a margin of one order of magnitude).  dV: relative L2 <= BOUND_A.
dQ / dK: ||got - want|| <= BOUND_A ||want|| + 2^-9 scale || |dS| |K| || (|dS|^T |Q| for dK): the MFMA takes dS as a bf16 operand,
and 2^-9 |dS_ij| per entry is that rounding's worst case; the term matters where the keys are alike, because the rows of dS sum to
zero exactly and those of bf16(dS) do not, so sum_j dS_ij K_j loses the cancellation that makes dQ small.
The "alike" cases are the ones the pair exists for: keys and values that are one row plus 2 % of noise, so that dS nearly vanishes
and dQ / dK are some 1e-4 of what |dO| |O| suggests; there ``mmf_attn_bwd_grouped``'s own delta = dO . O from the bf16 O leaves a
residue tens of times the gradient (printed, not asserted)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import BOUND_A, _lib, l2_rel  # noqa: E402

BF16 = torch.bfloat16
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5


def _case(B, H, T, dh, alike, seed):
    g = torch.Generator().manual_seed(seed)
    d = H * dh
    qkv = torch.randn(B * T, 3 * d, generator=g)
    if alike:                                            # every key / value row = one row per item + 2 % of noise
        base = torch.randn(B, 1, 2 * d, generator=g).expand(B, T, 2 * d).reshape(B * T, 2 * d)
        qkv[:, d:] = base + 0.02 * qkv[:, d:]
    return qkv.to(BF16), torch.randn(B * T, d, generator=g).to(BF16)


def _heads(t, B, T, H, dh):
    return t.double().reshape(B, T, H, dh).transpose(1, 2)


def _run(qkv, dout, B, H, T, dh, exact):
    lib = _lib()
    d, scale = H * dh, dh ** -0.5
    q, do = qkv.cuda(), dout.cuda()
    att = torch.empty(B * T, d, dtype=BF16, device="cuda")
    lse = torch.empty(B * H * T, device="cuda")
    delta = torch.full((B * H * T,), float("nan"), device="cuda")
    dqkv = torch.full((B * T, 3 * d), float("nan"), dtype=BF16, device="cuda")
    p, dp = q.data_ptr(), dqkv.data_ptr()
    prob = lambda: lib.AttnProblem(p, p + 2 * d, p + 4 * d, att.data_ptr(), lse.data_ptr(), do.data_ptr(), delta.data_ptr(), dp, dp + 2 * d,
                                   dp + 4 * d, B, H, T, T, 3 * d, 3 * d, 3 * d, d)
    lib.attn_fwd_grouped([prob()], dh, scale)
    (lib.attn_bwd_grouped_exact_delta if exact else lib.attn_bwd_grouped)([prob()], dh, scale)
    torch.cuda.synchronize()
    return delta.cpu(), dqkv.cpu()


@pytest.mark.parametrize("B,H,T,dh,alike", [(2, 2, 70, 64, False), (2, 2, 149, 64, True), (1, 2, 33, 96, True), (2, 1, 300, 96, False)])
def test_exact_delta_and_the_backward_on_it_against_float64(B, H, T, dh, alike):
    qkv, dout = _case(B, H, T, dh, alike, T + dh)
    d, scale = H * dh, dh ** -0.5
    Q, K, V = (_heads(qkv[:, i * d:(i + 1) * d], B, T, H, dh) for i in range(3))
    dO = _heads(dout, B, T, H, dh)
    P = torch.softmax(scale * Q @ K.transpose(-1, -2), dim=-1)
    dP = dO @ V.transpose(-1, -2)
    want_delta = (P * dP).sum(-1)
    dS = P * (dP - want_delta.unsqueeze(-1))
    flat = lambda t: t.transpose(1, 2).reshape(B * T, d)
    want = torch.cat([flat(scale * dS @ K), flat(scale * dS.transpose(-1, -2) @ Q), flat(P.transpose(-1, -2) @ dO)], dim=1)
    delta, dqkv = _run(qkv, dout, B, H, T, dh, True)
    _, plain = _run(qkv, dout, B, H, T, dh, False)
    size = (P * dO.norm(dim=-1, keepdim=True) * V.norm(dim=-1).unsqueeze(-2)).sum(-1)
    worst = float(((delta.double().reshape(B, H, T) - want_delta).abs() / (1e-4 * size)).max())
    print(f"attn_delta_f32 B={B} H={H} T={T} dh={dh} alike={alike}: worst |error| / (1e-4 x sum p |dO| |v|) = {worst:.3e}")
    assert worst <= 1.0
    assert not torch.isnan(dqkv.float()).any()
    rounding = (flat(scale * dS.abs() @ K.abs()), flat(scale * dS.abs().transpose(-1, -2) @ Q.abs()), torch.zeros(1, dtype=torch.float64))
    for i, name in enumerate(("dQ", "dK", "dV")):
        got, ref, old = (t[:, i * d:(i + 1) * d].double() for t in (dqkv, want, plain))
        err, bound = float((got - ref).norm()), BOUND_A * float(ref.norm()) + 2.0 ** -9 * float(rounding[i].norm())
        print(f"    {name}: error / bound {err / bound:.3e}; rel L2 {l2_rel(got, ref):.3e}, of which the bf16 dS term allows "
              f"{2.0 ** -9 * float(rounding[i].norm()) / float(ref.norm()):.3e}; mmf_attn_bwd_grouped with its own delta: rel L2 "
              f"{l2_rel(old, ref):.3e}; ||{name}|| {float(ref.norm()):.3e}")
        assert err <= bound, name
    assert torch.equal(dqkv[:, 2 * d:], plain[:, 2 * d:])          # dV does not read delta


def test_refusals():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    b = torch.zeros(1 << 14, dtype=BF16, device="cuda")
    f = torch.zeros(1 << 12, device="cuda")
    nan = torch.full((1 << 12,), float("nan"), device="cuda")
    p = b.data_ptr()

    def prob(**kw):
        a = dict(Q=p, K=p + 256, V=p + 512, O=p, LSE=f.data_ptr(), dO=p, delta=nan.data_ptr(), dQ=p, dK=p, dV=p, B=1, H=2, Tq=8, Tk=8, ldq=384,
                 ldk=384, ldv=384, ldo=128)
        a.update(kw)
        return (lib.AttnProblem * 1)(lib.AttnProblem(*[a[k] for k in ("Q", "K", "V", "O", "LSE", "dO", "delta", "dQ", "dK", "dV", "B", "H", "Tq",
                                                                     "Tk", "ldq", "ldk", "ldv", "ldo")]))
    for fn, name in ((L.mmf_attn_delta_f32, b"mmf_attn_delta_f32"), (L.mmf_attn_bwd_grouped_delta, b"mmf_attn_bwd_grouped_delta")):
        for kw, dh, want in ((dict(dO=None), 64, E_SHAPE), (dict(delta=None), 64, E_SHAPE), (dict(Tq=0), 64, E_SHAPE), (dict(LSE=None), 64, E_SHAPE),
                             (dict(dO=p + 8), 64, E_ALIGN), (dict(ldq=100), 64, E_ALIGN), ({}, 32, E_UNSUPPORTED)):
            rc = fn(prob(**kw), 1, dh, 0.125, s)
            assert rc == want and name in L.mmf_last_error(), (name, kw, rc, L.mmf_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan).all())                                                # nothing was launched
