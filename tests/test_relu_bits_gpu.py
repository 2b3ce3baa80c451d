"""GPU: the ReLU / dropout keep-mask as bits (MMF_EPI_RELU_BITS / MMF_EPI_MASK_BITS, csrc/gemm7.hip drain_tile).

The forward launch with RELU_BITS must store the same h as the launch without it and, next to it, one bit per element that is
(stored bf16 h > 0); the dgrad launch with MASK_BITS must equal the MASK_AUX launch on that h bit for bit.  The layout is keyed by
the problem's 32 x 32 blocks, so the bits a 256-wide launch writes are read by a 192-wide one and the other way round.  Problems:
M = 480 (ragged against the 256-row tile), 300 and 37 (no multiple of 32: the last block row is partial), N = 768 and 3072, one
launch for all three and one each; K = 160, the shortest reduction generation 7 takes.  Everything is bit equality: no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fused_seams_ref as old  # noqa: E402
from mmfusion import lib, ops  # noqa: E402
from mmfusion.lib import (EPI_BIAS, EPI_MASK_AUX, EPI_MASK_BITS, EPI_RELU, EPI_RELU_BITS, GEMM_NN, GEMM_NT)  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
K = 160
SHAPES = [(480, 768), (300, 3072), (37, 768)]
GROUPS = {"grouped": [[0, 1, 2]], "singly": [[0], [1], [2]]}
# output columns of problem 0 made NaN (a NaN weight row), +inf (a finite f32 bias that rounds to inf in bf16) and a positive f32
# that rounds to zero in bf16 (zero weights, a bias below half the smallest bf16 subnormal)
NAN_COL, INF_COL, TINY_COL = 5, 40, 77


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.fixture(scope="module")
def data():
    g = torch.Generator(device=DEV).manual_seed(11)
    out = []
    for i, (M, N) in enumerate(SHAPES):
        x = torch.randn(M, K, device=DEV, generator=g).to(BF16)
        w1 = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(BF16)
        b1 = torch.randn(N, device=DEV, generator=g) * 0.1
        if i == 0:                                          # the special values: NaN -> bit 0, +inf -> bit 1, like a0 > 0.f
            w1[NAN_COL] = float("nan")
            b1[INF_COL] = 3.4e38
            w1[TINY_COL] = 0
            b1[TINY_COL] = 1e-41
        dy = torch.randn(M, K, device=DEV, generator=g).to(BF16)
        w2 = (torch.randn(K, N, device=DEV, generator=g) * K ** -0.5).to(BF16)
        out.append((x, w1, b1, dy, w2))
    return out


class pinned:
    """generation 7 at one tile width for the launches inside"""

    def __init__(self, tile_n):
        self.tile_n = tile_n

    def __enter__(self):
        L = lib.load()
        lib.check(L.mmf_gemm_select_impl(7))
        lib.check(L.mmf_gemm7_set_tile_n(self.tile_n))

    def __exit__(self, *exc):
        L = lib.load()
        lib.check(L.mmf_gemm_select_impl(0))
        lib.check(L.mmf_gemm7_set_tile_n(0))


def nan_out(M, N):
    return torch.full((M, N), float("nan"), dtype=BF16, device=DEV)


def forward(data, ids, tile_n, dropout, with_bits):
    """ffn1 of the problems `ids` in one launch: h (and the bit buffers, pre-filled with a pattern)"""
    hs = [nan_out(*SHAPES[i]) for i in ids]
    bits = [ops.relu_bits_buffer(h).fill_(0xA5) for h in hs] if with_bits else [None] * len(ids)
    probs = [(data[i][0], data[i][1], h, data[i][2], b) for i, h, b in zip(ids, hs, bits)]
    epi = EPI_BIAS | EPI_RELU | (EPI_RELU_BITS if with_bits else 0)
    with pinned(tile_n):
        if dropout:
            ops.seed_dropout(2024)
        if with_bits:
            assert ops.relu_bits_available(GEMM_NT, probs, epi, dropout=dropout)
        ops.gemm_group(GEMM_NT, probs, epi, dropout=dropout)
        assert lib.load().mmf_gemm_last_impl() == 7 and lib.load().mmf_gemm7_last_tile_n() == tile_n
    torch.cuda.synchronize()
    return hs, bits


def dgrad(data, ids, tile_n, auxs, epi, alpha):
    dhs = [nan_out(*SHAPES[i]) for i in ids]
    probs = [(data[i][3], data[i][4], dh, None, a) for i, dh, a in zip(ids, dhs, auxs)]
    with pinned(tile_n):
        if epi == EPI_MASK_BITS:
            assert ops.relu_bits_available(GEMM_NN, probs, epi, alpha=alpha)
        ops.gemm_group(GEMM_NN, probs, epi, alpha=alpha)
        assert lib.load().mmf_gemm_last_impl() == 7 and lib.load().mmf_gemm7_last_tile_n() == tile_n
    torch.cuda.synchronize()
    return dhs


@pytest.mark.parametrize("widths", [(256, 192), (192, 256)], ids=["fwd256_dgrad192", "fwd192_dgrad256"])
@pytest.mark.parametrize("dropout", [None, (0.5, 3)], ids=["plain", "dropout"])
@pytest.mark.parametrize("grouping", sorted(GROUPS))
def test_bits_written_and_read(data, grouping, dropout, widths):
    for ids in GROUPS[grouping]:
        h_ref, _ = forward(data, ids, widths[0], dropout, with_bits=False)
        h, bits = forward(data, ids, widths[0], dropout, with_bits=True)
        for j, i in enumerate(ids):
            M, N = SHAPES[i]
            assert same_bits(h[j], h_ref[j]), f"problem {i}: h differs from the launch without RELU_BITS"
            want = h[j].float() > 0
            assert torch.equal(old.unpack_relu_bits(bits[j], M, N), want), f"problem {i}: bits != (h > 0)"
            if i == 0:
                assert not bool(want[:, NAN_COL].any()) and not bool(want[:, TINY_COL].any())
                assert bool(torch.isinf(h[j][:, INF_COL]).all() if dropout is None else torch.isinf(h[j][:, INF_COL]).any())
                assert torch.equal(want[:, INF_COL], torch.isinf(h[j][:, INF_COL]))
            if dropout is not None:                         # units dropout zeroed are exact zeros in h: their bit is 0
                h_plain = forward(data, [i], widths[0], None, with_bits=False)[0][0]
                zeroed = (h_plain.float() > 0) & (h[j].float() == 0)
                assert 0.3 < float(zeroed.sum()) / float((h_plain.float() > 0).sum()) < 0.7
                assert not bool(old.unpack_relu_bits(bits[j], M, N)[zeroed].any())
        for alpha in (1.0, 2.0):
            want = dgrad(data, ids, widths[1], h, EPI_MASK_AUX, alpha)
            got = dgrad(data, ids, widths[1], bits, EPI_MASK_BITS, alpha)
            for j, i in enumerate(ids):
                assert not bool(torch.isnan(got[j].float()).any()), f"problem {i}: unwritten dH"
                assert same_bits(got[j], want[j]), f"problem {i}, alpha {alpha}: MASK_BITS differs from MASK_AUX"


def test_bit_flags_outside_generation_7_are_refused():
    """a launch that goes to generation 2 has no bit form: the query says so and the launch itself is an error, not a fallback"""
    M, N = 64, 64
    x = torch.randn(M, K, device=DEV).to(BF16)
    w = torch.randn(N, K, device=DEV).to(BF16)
    b = torch.zeros(N, device=DEV)
    h = nan_out(M, N)
    probs = [(x, w, h, b, ops.relu_bits_buffer(h))]
    assert not ops.relu_bits_available(GEMM_NT, probs, EPI_BIAS | EPI_RELU | EPI_RELU_BITS)        # one tile: generation 2
    with pytest.raises(RuntimeError, match="generation 7 only"):
        ops.gemm_group(GEMM_NT, probs, EPI_BIAS | EPI_RELU | EPI_RELU_BITS)
    with pytest.raises(RuntimeError, match="RELU_BITS needs RELU"):
        ops.gemm_group(GEMM_NT, probs, EPI_BIAS | EPI_RELU_BITS)


def _ffn_grads(group_fn, mods, xs, gys, p, seed):
    for m in mods:
        m[0].weight.grad.zero_(), m[0].bias.grad.zero_(), m[1].weight.grad.zero_(), m[1].bias.grad.zero_()
    ops.seed_dropout(seed)
    ops.begin_training_forward()
    xin = [x.clone().requires_grad_(True) for x in xs]
    ys = group_fn([(x, m[0], m[1]) for x, m in zip(xin, mods)], dropout_p=p)
    torch.autograd.backward(ys, gys)
    torch.cuda.synchronize()
    return [y.detach() for y in ys], [x.grad for x in xin], [q.grad.clone() for m in mods for q in (m[0].weight, m[1].weight)]


@pytest.mark.parametrize("p", [0.0, 0.25], ids=["plain", "dropout"])
@pytest.mark.parametrize("d,rows,bits", [(64, [50, 7], False), (512, [300, 37, 480, 300, 260, 130], True)], ids=["gemm2", "gemm7"])
def test_ffn_residual_group_equals_the_aux_form(d, rows, bits, p):
    """``ops.ffn_residual_group`` against the same FFN with dH masked by h (fused_seams_ref): a small group that generation 7 cannot
    take (too few tiles: generation 2, the product keeps MASK_AUX) and one it takes with the bits (80 tiles of 256 x 256 in ffn1 and dH).
    Outputs, input gradients and weight gradients have one writer per element: bit-equal."""
    from mmfusion import arena as arena_mod
    torch.manual_seed(d)
    mods = [torch.nn.Sequential(torch.nn.Linear(d, 4 * d), torch.nn.Linear(4 * d, d)).cuda() for _ in rows]
    holder = torch.nn.ModuleList(mods)
    arena_mod.ensure(holder)
    xs = [torch.randn(r, d, device=DEV).to(BF16) for r in rows]
    gys = [torch.randn(r, d, device=DEV).to(BF16) for r in rows]
    seen = []
    real = ops.gemm_group

    def spy(layout, probs, epilogue, **kw):
        seen.append(epilogue)
        return real(layout, probs, epilogue, **kw)
    ops.gemm_group = spy
    try:
        got = _ffn_grads(ops.ffn_residual_group, mods, xs, gys, p, seed=5)
    finally:
        ops.gemm_group = real
    assert any(e & EPI_MASK_BITS for e in seen) == bits and any(e & EPI_RELU_BITS for e in seen) == bits
    want = _ffn_grads(old.ffn_residual_group, mods, xs, gys, p, seed=5)
    for name, a, b in zip(("y", "dx", "dW"), got, want):
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), f"{name}[{i}] differs from the aux form"
