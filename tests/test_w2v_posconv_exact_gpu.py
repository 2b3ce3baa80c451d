"""GPU: the positional-convolution kernels of csrc/wav2vec2.hip (``mmf_w2v_posconv`` and its two backward epilogues,
``mmf_w2v_posconv_wgrad``) on operands for which their f32 accumulation is EXACT, element by element.

Every operand is an integer or a small dyadic rational that bf16 holds exactly, and every partial sum of the contraction, in any order,
is an integer number of units below 2^24 (asserted per case: ``w2v_kernel_checks.exact_budget``).  The MFMA's own summation order then
cannot show, and one wrong row, tap, channel or column does:
  dgrad    dx = bf16(dy + conv) compared BIT FOR BIT with the float64 value rounded once
  wgrad    the f32 gradient bit for bit with the float64 contraction: one slab, two slabs and one slab per (clip, block) unit through
           ``sum_slabs``, a slab count that leaves the last slab empty, and ``accumulate`` onto an integer pre-fill; the columns
           [k cg, Kp) are zero, or under ``accumulate`` what they held
  forward  z = bias + conv is exact (weights in units of 2^-e, the bias in quarters over -3 .. 3, z over -6 .. 6 and at most -9 .. 9); every element within
           ``w2v_kernel_checks.fwd_bound`` of the float64 x + gelu(z): half a bf16 ulp, the f32 add and the allowance of tests/gelu_domain.py
  bwd_act  the same exact z; every element within one bf16 ulp of dy gelu'(z) plus |dy| times the f32 error of gelu', which is
           measured on the f32 CPU restatement of Phi(z) + z phi(z) against float64 over the case's z, four times over
Outputs are pre-filled with NaN and have a NaN guard behind them, inputs must come back bit-identical, and every clip and group is
filled at another scale or sign pattern, so that a read across a clip or group seam changes the result.  The shapes are the smallest
that reach each path: all four group widths, odd and even k (5, 15, 16, 128; k cg a multiple of 32 or not), and T on both sides of a
wave's 32 rows, of the 128-row tile and of k.  profiles/w2v_kernel_pins.txt holds the printed lines from an MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gelu_domain  # noqa: E402
import w2v_grad_ref as G  # noqa: E402
import w2v_kernel_checks as K  # noqa: E402
import w2v_ref  # noqa: E402
from helpers import _lib  # noqa: E402

BF16 = torch.bfloat16
GUARD = 4096
CASES = [                                   # (N, T, groups, cg, k): every T with an odd and an even k, every width on both sides of 128
    (2, 1, 2, 16, 5), (2, 1, 2, 32, 16),                  # one row: three of the four waves return at once
    (2, 9, 2, 48, 15), (2, 9, 2, 64, 128),                # T below k: every output row reads zero rows on both sides
    (2, 31, 2, 32, 5), (2, 31, 2, 16, 16),                # one row short of a wave
    (2, 32, 2, 64, 15), (2, 32, 2, 48, 16),               # exactly one wave
    (2, 33, 2, 16, 15), (2, 33, 2, 64, 16),               # one row into the second wave
    (2, 127, 2, 48, 5), (2, 127, 2, 32, 128),             # one row short of the tile
    (2, 128, 2, 32, 15), (2, 128, 2, 16, 128),            # exactly one tile
    (2, 129, 2, 16, 5), (2, 129, 3, 48, 128),             # one row into the second tile; the shipped k and width
    (2, 160, 2, 64, 5), (2, 160, 2, 32, 16),              # the second tile holds one wave
    (3, 257, 2, 48, 15), (2, 257, 2, 64, 128),            # three tiles; the largest LDS image
]
IDS = [f"T{c[1]}-cg{c[3]}-k{c[4]}" for c in CASES]
EMPTY_SLAB = [(5, 33, 2, 16, 5), (5, 9, 2, 64, 16)]     # 5 units in 4 slabs of 2: the last slab has none
_ints, _dyadic = {}, {}


def _fill(g, N, T, groups, cg, spread, scales):
    """integers: clip n scaled by scales[n % len], even groups drawn from -spread .. spread, odd groups from 0 .. spread + 1"""
    even = torch.randint(-spread, spread + 1, (N, T, groups, cg), generator=g)
    odd = torch.randint(0, spread + 2, (N, T, groups, cg), generator=g)
    x = torch.where((torch.arange(groups) % 2 == 0).view(1, 1, groups, 1), even, odd)
    s = torch.tensor([scales[n % len(scales)] for n in range(N)]).view(N, 1, 1, 1)
    return (x * s).reshape(N, T, groups * cg).double()


def _int_case(N, T, groups, cg, k):
    """integer operands of the dgrad and the wgrad and their float64 results, through autograd of the float64 restatement"""
    key = (N, T, groups, cg, k)
    if key not in _ints:
        C, g = groups * cg, torch.Generator().manual_seed(1000 * T + 10 * k + cg)
        x, dz = _fill(g, N, T, groups, cg, 2, (1, 2, 3)), _fill(g, N, T, groups, cg, 2, (3, 1, 2))
        w = torch.randint(-3, 4, (C, cg, k), generator=g).double()
        dy = torch.randint(-64, 65, (N, T, C), generator=g).double()
        fill = torch.randint(-100, 101, (C, K.kp_of(k, cg)), generator=g).double()
        xd, wd = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        dx, dw = torch.autograd.grad(w2v_ref.pos_conv(xd, wd, torch.zeros(C, dtype=torch.float64), groups), [xd, wd], dz)
        assert K.exact_budget(k * cg, dz, w, 1.0, extra=64.0) < K.EXACT_LIMIT            # the dgrad's sums
        assert K.exact_budget(N * T, dz, x, 1.0, extra=100.0) < K.EXACT_LIMIT            # the wgrad's, on top of the pre-fill
        assert all(bool((t.to(BF16).double() == t).all()) for t in (x, dz, w, dy))       # bf16 holds every operand
        _ints[key] = dict(C=C, Kp=K.kp_of(k, cg), x=x, dz=dz, w=w, dy=dy, fill=fill, dx=dy + dx, dw=G.pack(dw))
    return _ints[key]


def _dyadic_case(N, T, groups, cg, k):
    """operands of the forward and of bwd_act with an exact z: x integers, w in units of 2^-e, the bias in quarters"""
    key = (N, T, groups, cg, k)
    if key not in _dyadic:
        C, g = groups * cg, torch.Generator().manual_seed(2000 * T + 10 * k + cg)
        e = math.ceil(math.log2(2.0 * math.sqrt(k * cg)))                                 # the convolution's spread is then 1 to 1.5
        x = _fill(g, N, T, groups, cg, 1, (1, 2))
        m = torch.randint(1, 3, (C, cg, k), generator=g) * (2 * torch.randint(0, 2, (C, cg, k), generator=g) - 1)
        w = m.double() * 2.0 ** -e
        bias = torch.randint(-12, 13, (C,), generator=g).double() / 4.0
        dy = _fill(g, N, T, groups, cg, 8, (1, 3))
        unit = 2.0 ** -e
        assert e >= 2 and K.exact_budget(k * cg, x, w, unit, extra=3.0) < K.EXACT_LIMIT
        assert K.is_multiple(w, unit) and K.is_multiple(bias, unit)
        assert all(bool((t.to(BF16).double() == t).all()) for t in (x, w, dy)) and bool((bias.float().double() == bias).all())
        z = w2v_ref.pos_conv(x, w, bias, groups)
        assert K.is_multiple(z, unit) and bool((z.float().double() == z).all())
        _dyadic[key] = dict(C=C, Kp=K.kp_of(k, cg), x=x, w=w, bias=bias, dy=dy, z=z, e=e)
    return _dyadic[key]


def _nan(numel, dtype):
    return torch.full((numel + GUARD,), float("nan"), dtype=dtype, device="cuda")


def _done(what, buf, n, inputs, before):
    """after a launch: the output holds no NaN, the guard behind it is all NaN, the inputs are what they were"""
    torch.cuda.synchronize()
    assert not bool(torch.isnan(buf[:n]).any()), f"{what}: NaN left in the output"
    assert bool(torch.isnan(buf[n:]).all()), f"{what}: the guard behind the output was written"
    assert all(torch.equal(K.bits(t), b) for t, b in zip(inputs, before)), f"{what}: an input was changed"


def _dev(*ts):
    out = [t.cuda().contiguous() for t in ts]
    return out, [K.bits(t).clone() for t in out]


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_dgrad_bit_for_bit(N, T, groups, cg, k):
    lib, c = _lib(), _int_case(N, T, groups, cg, k)
    C, n = c["C"], N * T * c["C"]
    (dz, wt, dy), before = _dev(c["dz"].to(BF16), K.padded(G.pack_transposed(c["w"]), c["Kp"]).to(BF16), c["dy"].to(BF16))
    buf = _nan(n, BF16)
    lib.w2v_posconv_dgrad(dz, wt, dy, buf, N, T, C, groups, k)
    _done("posconv_dgrad", buf, n, (dz, wt, dy), before)
    got = buf[:n].view(N, T, C).cpu()
    bad = K.mismatches(got, c["dx"])
    print(f"PARITY posconv_dgrad exact N={N} T={T} groups={groups} cg={cg} k={k}: {bad} of {n} elements differ from bf16(float64) in their bits; "
          f"|dx| up to {float(c['dx'].abs().max()):.0f}")
    assert torch.equal(K.bits(got), K.bits(c["dx"].to(BF16)))


def _wgrad(c, N, T, groups, k, slabs, accumulate=False):
    """-> the (C, Kp) f32 result on the CPU, the slab partials summed by ``sum_slabs``, and the raw partials"""
    lib = _lib()
    C, Kp = c["C"], c["Kp"]
    (dz, x), before = _dev(c["dz"].to(BF16), c["x"].to(BF16))
    n = slabs * C * Kp
    buf = _nan(n, torch.float32)
    if accumulate:
        buf[:n] = c["fill"].float().cuda().view(-1)
    lib.w2v_posconv_wgrad(dz, x, buf[:n], N, T, C, groups, k, slabs=slabs, accumulate=accumulate)
    _done(f"posconv_wgrad slabs={slabs}", buf, n, (dz, x), before)
    parts = buf[:n].view(slabs, C, Kp)
    if slabs == 1:
        return parts[0].cpu(), parts.cpu()
    out = _nan(C * Kp, torch.float32)
    lib.sum_slabs(parts.view(slabs, -1), out[:C * Kp], False)
    _done("sum_slabs", out, C * Kp, (parts,), [K.bits(parts).clone()])
    return out[:C * Kp].view(C, Kp).cpu(), parts.cpu()


def _wgrad_check(what, got, c, cg, k, held=None):
    want = K.padded(c["dw"], c["Kp"]) + (0.0 if held is None else held)
    bad = K.mismatches(got, want)
    print(f"PARITY posconv_wgrad exact {what}: {bad} of {got.numel()} elements differ from f32(float64) in their bits; "
          f"|dW| up to {float(c['dw'].abs().max()):.0f}")
    pad_cols = got[:, k * cg:]
    assert bool((pad_cols == (0.0 if held is None else held[:, k * cg:].float())).all()), f"{what}: the columns [k cg, Kp)"
    assert torch.equal(K.bits(got), K.bits(want.float()))


@pytest.mark.parametrize("form", ["one-slab", "two-slabs", "slab-per-unit", "accumulate"])
@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_wgrad_bit_for_bit(N, T, groups, cg, k, form):
    c = _int_case(N, T, groups, cg, k)
    units = N * ((T + 127) // 128)
    slabs = {"one-slab": 1, "two-slabs": 2, "slab-per-unit": units, "accumulate": 1}[form]
    got, _ = _wgrad(c, N, T, groups, k, slabs, accumulate=form == "accumulate")
    _wgrad_check(f"N={N} T={T} groups={groups} cg={cg} k={k} {form} (slabs={slabs} of {units} units)", got, c, cg, k,
                 held=c["fill"] if form == "accumulate" else None)


@pytest.mark.parametrize("N,T,groups,cg,k", EMPTY_SLAB, ids=[f"T{c[1]}-cg{c[3]}-k{c[4]}" for c in EMPTY_SLAB])
def test_wgrad_empty_last_slab(N, T, groups, cg, k):
    """units = 5 in slabs = 4: three slabs of two units (the third of one) and a fourth of none, which must be WRITTEN, as zeros"""
    c = _int_case(N, T, groups, cg, k)
    assert N * ((T + 127) // 128) == 5
    got, parts = _wgrad(c, N, T, groups, k, 4)
    assert bool((parts[3] == 0).all()), "the empty slab's partial is not all zeros"
    _wgrad_check(f"N={N} T={T} groups={groups} cg={cg} k={k} empty last slab (slabs=4 of 5 units)", got, c, cg, k)


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_forward_within_one_ulp_of_exact_z(N, T, groups, cg, k):
    lib, c = _lib(), _dyadic_case(N, T, groups, cg, k)
    C, n = c["C"], N * T * c["C"]
    (x, w, bias), before = _dev(c["x"].to(BF16), K.padded(G.pack(c["w"]), c["Kp"]).to(BF16), c["bias"].float())
    buf = _nan(n, BF16)
    lib.w2v_posconv(x, w, bias, buf, N, T, C, groups, k)
    _done("posconv", buf, n, (x, w, bias), before)
    z = c["z"]
    want = c["x"] + gelu_domain.gelu64(z)
    r = K.worst(buf[:n].view(N, T, C).cpu(), want, K.fwd_bound(want, z))
    print(f"PARITY posconv exact-z N={N} T={T} groups={groups} cg={cg} k={k}: worst |got - exact| / allowance = {r:.3f} (bound 1); "
          f"z in {float(z.min()):.2f} .. {float(z.max()):.2f} in units of 2^-{c['e']}")
    assert r <= 1.0


@pytest.mark.parametrize("N,T,groups,cg,k", CASES, ids=IDS)
def test_bwd_act_within_one_ulp_of_exact_z(N, T, groups, cg, k):
    lib, c = _lib(), _dyadic_case(N, T, groups, cg, k)
    C, n = c["C"], N * T * c["C"]
    (x, w, bias, dy), before = _dev(c["x"].to(BF16), K.padded(G.pack(c["w"]), c["Kp"]).to(BF16), c["bias"].float(), c["dy"].to(BF16))
    buf = _nan(n, BF16)
    lib.w2v_posconv_bwd_act(x, w, bias, dy, buf, N, T, C, groups, k)
    _done("posconv_bwd_act", buf, n, (x, w, bias, dy), before)
    z = c["z"]
    want, margin = c["dy"] * K.gelu_grad(z), K.gelu_grad_margin(z)                      # the margin: reference against reference
    r = K.worst(buf[:n].view(N, T, C).cpu(), want, K.act_bound(want, c["dy"], margin))
    print(f"PARITY posconv_bwd_act exact-z N={N} T={T} groups={groups} cg={cg} k={k}: worst |got - exact| / (ulp + |dy| margin) = {r:.3f} "
          f"(bound 1); the f32 error of gelu' over this z, four times over: {margin:.3e}")
    assert r <= 1.0
