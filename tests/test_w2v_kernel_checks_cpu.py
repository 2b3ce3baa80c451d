"""CPU: the per-element checkers of the Wav2Vec2 convolution kernels' tests (tests/w2v_kernel_checks.py, and the cancelling-set
checker of tests/test_w2v_ln_gpu.py that tests/test_w2v_conv0_kernels_gpu.py uses) reject the errors they are there for.

Each test builds the float64 expectation of one kernel at one small case, restates the kernel's INDEXING in float64 (``_conv_model``:
the 128-row tiles, their halo rows and the zero rows outside the clip; ``_wgrad_units``: the (clip, block) units the slabs are made
of) and plants one error in it.  The planted result, rounded as the kernel rounds, must be REJECTED by the new checker and ACCEPTED by
the relative L2 <= BOUND_A that tests/test_w2v_gpu.py and tests/test_w2v_finetune_kernels_gpu.py held these kernels to; the second
assertion is the evidence that the gap existed.  The unmutated restatement must pass the new checker.

One of the eight is accepted by the whole-tensor L2 only where the residual outweighs the convolution: the dgrad padded by k / 2 at an
even k shifts the whole convolution by a row, which the old file's third figure, the L2 of the convolution's part alone, does see.  The
case here makes the residual dy a hundred times the convolution, where that file's first two figures accept the shift."""
import pytest
import torch

import w2v_grad_ref as G
import w2v_kernel_checks as K
import w2v_ref
from helpers import BOUND_A, _bf16_ulp, l2_rel
from test_w2v_conv0_kernels_gpu import CASES as CONV0_CASES, IDS as CONV0_IDS, conv0_case
from test_w2v_ln_gpu import CANCEL, GUARD, _check

BF16 = torch.bfloat16
TT = 128


def _conv_model(x, packed, cg, k, pad, fault=None):
    """w2v_posconv_kernel's index arithmetic in float64: per (clip, group, 128-row tile) the image of rows t0 - pad .. t0 + 127 + k - 1
    - pad, zero outside [0, T), and out[t0 + r] = sum over the k cg columns at image row r.  ``fault``:
      "seam"  clip 1, group 1, tile 1: the first halo row (t0 - 1, the neighbouring tile's last) is read as row t0
      "clip"  clip 1: rows t < 0 are read where the flat index lands, in clip 0's tail, instead of as zeros"""
    N, T, C = x.shape
    flat, out = x.reshape(N * T, C), torch.zeros_like(x)
    for n in range(N):
        for t0 in range(0, T, TT):
            t = t0 - pad + torch.arange(TT + k - 1)
            inside = (t >= 0) & (t < T)
            if fault == "clip" and n == 1:
                inside = t < T
            rows = min(TT, T - t0)
            for g in range(C // cg):
                ch = slice(g * cg, (g + 1) * cg)
                tg = torch.where(t == t0 - 1, t + 1, t) if fault == "seam" and (n, g, t0) == (1, 1, TT) else t
                img = torch.where(inside.unsqueeze(1), flat[(n * T + tg).clamp(0, N * T - 1)][:, ch], torch.zeros((), dtype=x.dtype))
                out[n, t0:t0 + rows, ch] = w2v_ref.window(img[None], k, 1)[0, :rows] @ packed[ch].T
    return out


def _random_case(N, T, groups, cg, k, seed=0):
    """the random bf16 operands of tests/test_w2v_finetune_kernels_gpu.py, as float64"""
    C, g = groups * cg, torch.Generator().manual_seed(seed + T + k)
    x = torch.randn(N, T, C, generator=g).to(BF16).double()
    w = (torch.randn(C, cg, k, generator=g) * (2.0 / (cg * k)) ** 0.5).to(BF16).double()
    bias = (0.1 * torch.randn(C, generator=g)).float().double()
    dy = torch.randn(N, T, C, generator=g).to(BF16).double()
    return x, w, bias, dy


def _forward(x, packed, bias, cg, k, fault=None):
    return x + w2v_ref.gelu_erf(_conv_model(x, packed, cg, k, k // 2, fault) + bias)


def _forward_verdicts(x, w, bias, cg, k, got):
    """-> (the new checker's worst error / bound, the old relative L2) of a forward result ``got`` (float64, before its rounding)"""
    conv, terms, gamma = K.gamma_conv(x, G.pack(w), cg, k, k // 2)
    want = x + w2v_ref.gelu_erf(conv + bias)
    got16 = got.to(BF16)
    return K.worst(got16, want, K.elementwise_bound(want, terms + bias.abs(), K.GELU_D1_SUP, gamma)), l2_rel(got16, want)


def test_the_model_is_the_convolution_and_passes_unmutated():
    N, T, groups, cg, k = 2, 160, 2, 16, 15
    x, w, bias, dy = _random_case(N, T, groups, cg, k)
    assert float((_conv_model(x, G.pack(w), cg, k, k // 2) + bias - w2v_ref.pos_conv(x, w, bias, groups)).abs().max()) < 1e-12
    for kk in (15, 16):                                                          # the dgrad's padding, odd and even k
        x, w, bias, dy = _random_case(N, T, groups, cg, kk)
        xd = x.clone().requires_grad_(True)
        (dx,) = torch.autograd.grad(w2v_ref.pos_conv(xd, w, bias, groups), xd, dy)
        assert float((_conv_model(dy, G.pack_transposed(w), cg, kk, kk - 1 - kk // 2) - dx).abs().max()) < 1e-12
    new, old = _forward_verdicts(x, w, bias, cg, 16, _forward(x, G.pack(w), bias, cg, 16))
    print(f"unmutated forward: worst error / bound {new:.3f}, rel L2 {old:.2e}")
    assert new <= 1.0 and old <= BOUND_A


def test_a_seam_row_from_the_neighbouring_tile_is_rejected():
    N, T, groups, cg, k = 4, 257, 2, 16, 15
    x, w, bias, _ = _random_case(N, T, groups, cg, k)
    new, old = _forward_verdicts(x, w, bias, cg, k, _forward(x, G.pack(w), bias, cg, k, "seam"))
    print(f"seam row: worst error / bound {new:.1f}, rel L2 {old:.2e} (BOUND_A {BOUND_A})")
    assert new > 1.0 and old <= BOUND_A


def test_rows_before_a_clip_read_from_the_previous_clip_are_rejected():
    N, T, groups, cg, k = 4, 1000, 2, 16, 15
    x, w, bias, _ = _random_case(N, T, groups, cg, k)
    new, old = _forward_verdicts(x, w, bias, cg, k, _forward(x, G.pack(w), bias, cg, k, "clip"))
    print(f"clip seam: worst error / bound {new:.1f}, rel L2 {old:.2e} (BOUND_A {BOUND_A})")
    assert new > 1.0 and old <= BOUND_A


def test_tap_k_minus_1_dropped_at_one_group_is_rejected():
    N, T, groups, cg, k = 2, 160, 16, 16, 128
    x, w, bias, _ = _random_case(N, T, groups, cg, k)
    short = w.clone()
    short[cg:2 * cg, :, k - 1] = 0.0
    new, old = _forward_verdicts(x, w, bias, cg, k, _forward(x, G.pack(short), bias, cg, k))
    print(f"dropped tap: worst error / bound {new:.1f}, rel L2 {old:.2e} (BOUND_A {BOUND_A})")
    assert new > 1.0 and old <= BOUND_A


def _int_dgrad(N, T, groups, cg, k, dy_scale):
    C, g = groups * cg, torch.Generator().manual_seed(T + k)
    dz = torch.randint(-2, 3, (N, T, C), generator=g).double()
    w = torch.randint(-3, 4, (C, cg, k), generator=g).double()
    dy = (torch.randint(-64, 65, (N, T, C), generator=g) * dy_scale).double()
    assert K.exact_budget(k * cg, dz, w, 1.0, extra=float(dy.abs().max())) < K.EXACT_LIMIT
    return dz, w, dy


def test_the_dgrad_padded_by_half_k_at_an_even_k_is_rejected():
    N, T, groups, cg, k = 2, 33, 2, 16, 16
    dz, w, dy = _int_dgrad(N, T, groups, cg, k, 128)                             # residual-dominated: module docstring
    assert bool((dy.to(BF16).double() == dy).all())
    wt = G.pack_transposed(w)
    want = dy + _conv_model(dz, wt, cg, k, k - 1 - k // 2)
    assert K.mismatches(want.to(BF16), want) == 0
    got = (dy + _conv_model(dz, wt, cg, k, k // 2)).to(BF16)
    bad, old = K.mismatches(got, want), l2_rel(got, want)
    print(f"dgrad pad: {bad} elements differ in their bits, rel L2 {old:.2e} (BOUND_A {BOUND_A})")
    assert bad > 0 and old <= BOUND_A


def _wgrad_units(dz, x, cg, k):
    """the packed weight gradient of every (clip, 128-row block) unit on its own: what a slab of one unit holds"""
    N, T, C = x.shape
    units = []
    for n in range(N):
        for t0 in range(0, T, TT):
            part = torch.zeros_like(dz)
            part[n, t0:t0 + TT] = dz[n, t0:t0 + TT]
            units.append(G.conv_weight_grad(part, x, cg, k))
    return units


def test_a_wgrad_slab_added_twice_and_a_nonzero_padding_column_are_rejected():
    N, T, groups, cg, k = 32, 129, 2, 16, 5
    C, Kp, g = groups * cg, K.kp_of(k, cg), torch.Generator().manual_seed(5)
    x, dz = (torch.randint(-2, 3, (N, T, C), generator=g).double() for _ in range(2))
    assert K.exact_budget(N * T, dz, x, 1.0) < K.EXACT_LIMIT
    want = G.conv_weight_grad(dz, x, cg, k)
    units = _wgrad_units(dz, x, cg, k)
    assert len(units) == 2 * N and K.mismatches(K.padded(sum(units), Kp).float(), K.padded(want, Kp)) == 0
    twice = K.padded(sum(units) + units[-1], Kp).float()                         # the last unit: clip 31's one-row block
    bad, old = K.mismatches(twice, K.padded(want, Kp)), l2_rel(G.unpack(twice[:, :k * cg], cg), G.unpack(want, cg))
    print(f"slab twice: {bad} elements differ in their bits, rel L2 {old:.2e} (BOUND_A {BOUND_A})")
    assert bad > 0 and old <= BOUND_A
    dirty = K.padded(want, Kp).float()
    dirty[3, k * cg + 1] = 1.0
    assert not bool((dirty[:, k * cg:] == 0).all()) and K.mismatches(dirty, K.padded(want, Kp)) == 1
    assert l2_rel(G.unpack(dirty[:, :k * cg], cg), G.unpack(want, cg)) <= BOUND_A   # the unpacked gradient never holds those columns


def _conv0_buf(t):
    return torch.cat([t.reshape(-1).to(BF16), torch.full((GUARD,), float("nan"), dtype=BF16)])


def test_a_conv0_frame_stored_one_tap_over_and_two_ulps_are_rejected():
    N, L, C0, k0, s0, k1, s1 = 1, 30000, 8, 10, 5, 3, 2
    c = conv0_case(N, L, C0, k0, s0, k1, s1, "spread")
    want, y, terms = c["want"], c["y"], c["terms"]                               # (N, T1, k1 C0)
    _check("unmutated conv0", _conv0_buf(want), want, y, terms)
    moved = want.clone()
    moved.view(N, -1, k1, C0)[0, 700, 2] = moved.view(N, -1, k1, C0)[0, 700, 1]  # frame 1401 stored at (700, 2) as well as at (700, 1)
    assert l2_rel(moved.to(BF16), want) <= BOUND_A
    with pytest.raises(AssertionError):
        _check("conv0 frame one tap over", _conv0_buf(moved), want, y, terms)
    off = want.to(BF16).double()
    flat = off.view(-1)
    at = int(torch.argmax(((y.abs() > 0.5) & (y.abs() < 2.0)).view(-1).int()))   # an output well outside the cancelling set
    flat[at] += 2.0 * float(_bf16_ulp(flat[at:at + 1]))
    assert l2_rel(off, want) <= BOUND_A
    with pytest.raises(AssertionError):
        _check("conv0 two ulps", _conv0_buf(off), want, y, terms)
    x, w, bias, _ = _random_case(2, 33, 2, 16, 5)                                # and through the positional convolution's bound
    conv, pterms, gamma = K.gamma_conv(x, G.pack(w), 16, 5, 2)
    pw = x + w2v_ref.gelu_erf(conv + bias)
    two = pw.to(BF16).double()
    two[1, 17, 5] += 2.0 * float(_bf16_ulp(two[1, 17, 5:6]))
    assert K.worst(two, pw, K.elementwise_bound(pw, pterms + bias.abs(), K.GELU_D1_SUP, gamma)) > 1.0 and l2_rel(two, pw) <= BOUND_A


@pytest.mark.parametrize("N,L,C0,k0,s0,k1,s1,affine", CONV0_CASES, ids=CONV0_IDS)
def test_conv0_cases_keep_their_cancelling_set_within_the_cap(N, L, C0, k0, s0, k1, s1, affine):
    """with the float64 reference alone: the GPU test relies on the checker's count cap, so every case is shown to respect it first"""
    c = conv0_case(N, L, C0, k0, s0, k1, s1, affine)
    n, count = c["y"].numel(), int((c["y"].abs() < CANCEL * c["terms"]).sum())
    cap = 0 if affine == "tail" else max(8, n >> 8)
    print(f"conv0 case L={L} C0={C0} k0={k0} {affine}: cancelling set {count} of {n} (cap {cap})")
    assert count <= cap and c["want"].shape == (N, (((L - k0) // s0 + 1) - k1) // s1 + 1, k1 * C0)


def test_exact_operand_rules():
    a, b = torch.full((4,), 3.0), torch.full((4,), 2.0 ** -8)
    assert K.exact_budget(8192, a, b, 2.0 ** -8) == 8192 * 3 and K.is_multiple(b, 2.0 ** -8) and not K.is_multiple(b, 2.0 ** -7)
    assert K.mismatches(torch.tensor([257.0]).to(BF16), torch.tensor([257.0], dtype=torch.float64)) == 0     # rounded once: 256
    assert K.mismatches(torch.tensor([258.0]).to(BF16), torch.tensor([257.0], dtype=torch.float64)) == 1
    assert abs(K.GELU_D1_SUP - 1.12890) < 1e-4 and abs(K.GELU_D2_SUP - 0.79788) < 1e-4
    z = torch.linspace(-6.0, 6.0, 49, dtype=torch.float64)
    zz = z.clone().requires_grad_(True)
    (d,) = torch.autograd.grad(w2v_ref.gelu_erf(zz).sum(), zz)
    assert float((K.gelu_grad(z) - d).abs().max()) < 1e-14 and 0.0 < K.gelu_grad_margin(z) < 1e-5
