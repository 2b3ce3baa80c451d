"""GPU: generation 7's two tile widths (csrc/gemm7.hip: 256 x 256 and 256 x 192) give every output element the same MFMA chain, so
the 192 form must equal the 256 form BIT FOR BIT — for every flag set generation 7 is instantiated for, on 1 / 3 / 8 / CU-count
persistent workgroups (a workgroup then crosses tile and problem boundaries with its ring running), on ragged M, on N that is a
multiple of 8 but not of 192 (edge tiles), on mixed K in one launch, and on the fusion step's own launch lists.  The automatic
choice must be the one tests/gemm7_step_launches.py lists for the step."""
import pytest
import torch

from gemm7_step_launches import STEP_LAUNCHES
from mmfusion import lib, ops
from mmfusion.lib import EPI_ADD_AUX, EPI_BIAS, EPI_DROPOUT, EPI_MASK_AUX, EPI_RELU, GEMM_NN, GEMM_NT

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRIDS = (1, 3, 8, 0)                  # 0: the CU count
FLAG_SETS = {GEMM_NT: (0, EPI_BIAS, EPI_BIAS | EPI_RELU, EPI_BIAS | EPI_ADD_AUX, EPI_BIAS | EPI_RELU | EPI_DROPOUT),
             GEMM_NN: (0, EPI_MASK_AUX, EPI_ADD_AUX)}
# ragged M, N % 8 == 0 but not % 192 (and not % 256), mixed K in one launch (the minimum of five stages up), wider leading dimensions
SMALL = [(520, 264, 160, 8), (300, 520, 768, 0), (257, 8, 192, 16), (1000, 392, 512, 8), (256, 200, 2048, 0), (40, 1032, 224, 24)]


def _operands(layout, shapes, epi, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    probs = []
    for M, N, K, pad in shapes:
        a = torch.randn(M, K + pad, device=DEV, generator=g).to(torch.bfloat16)[:, pad:]
        if layout == GEMM_NT:
            b = (torch.randn(N, K + 2 * pad, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16)[:, 2 * pad:]
        else:
            b = (torch.randn(K, N + 2 * pad, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16)[:, :N]
        bias = torch.randn(N, device=DEV, generator=g) if epi & EPI_BIAS else None
        aux = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16) if epi & (EPI_ADD_AUX | EPI_MASK_AUX) else None
        probs.append((a, b, bias, aux))
    return probs


def _run(layout, probs, epi, wgs, tile_n, alpha, dropout):
    L = lib.load()
    outs = [torch.full((a.shape[0], b.shape[0] if layout == GEMM_NT else b.shape[1]), float("nan"), dtype=torch.bfloat16, device=DEV)
            for a, b, _, _ in probs]
    try:
        lib.check(L.mmf_gemm_select_impl(7))
        lib.check(L.mmf_gemm_set_persistent_workgroups(wgs))
        lib.check(L.mmf_gemm7_set_tile_n(tile_n))
        if dropout:
            ops.seed_dropout(4321)
        ops.gemm_group(layout, [(a, b, c, bias, aux) for (a, b, bias, aux), c in zip(probs, outs)], epi, alpha=alpha,
                       dropout=dropout)
        assert L.mmf_gemm_last_impl() == 7
        width = L.mmf_gemm7_last_tile_n()
        torch.cuda.synchronize()
    finally:
        lib.check(L.mmf_gemm_select_impl(0))
        lib.check(L.mmf_gemm_set_persistent_workgroups(0))
        lib.check(L.mmf_gemm7_set_tile_n(0))
    return outs, width


def _same_bits(layout, shapes, epi, wgs, seed):
    alpha = 1.0 / 0.75 if (layout == GEMM_NN and epi == EPI_MASK_AUX) else 1.0
    dropout = (0.25, 3) if epi & EPI_DROPOUT else None
    probs = _operands(layout, shapes, epi & ~EPI_DROPOUT, seed)
    c256, w256 = _run(layout, probs, epi & ~EPI_DROPOUT, wgs, 256, alpha, dropout)
    c192, w192 = _run(layout, probs, epi & ~EPI_DROPOUT, wgs, 192, alpha, dropout)
    assert (w256, w192) == (256, 192)
    for i, (x, y) in enumerate(zip(c256, c192)):
        assert not bool(torch.isnan(y.float()).any()), f"epi {epi} wgs {wgs} problem {i}: unwritten output at 192"
        assert torch.equal(x, y), f"epi {epi} wgs {wgs} problem {i}: the 192 form differs from the 256 form"


@pytest.mark.parametrize("layout", [GEMM_NT, GEMM_NN])
@pytest.mark.parametrize("wgs", GRIDS)
def test_192_form_bit_identical_to_256_form(layout, wgs):
    for epi in FLAG_SETS[layout]:
        _same_bits(layout, SMALL, epi, wgs, seed=100 + epi)


@pytest.mark.parametrize("wgs", GRIDS)
@pytest.mark.parametrize("case", range(len(STEP_LAUNCHES)), ids=[s[0] for s in STEP_LAUNCHES])
def test_192_form_bit_identical_on_the_step_launches(case, wgs):
    _name, layout, epi, shapes, _want = STEP_LAUNCHES[case]
    _same_bits(layout, [(M, N, K, 0) for M, N, K in shapes], epi, wgs, seed=7 + case)


def test_automatic_width_of_the_step_launches():
    """on the CU-count grid the automatic rule runs the launches the step table marks at 192 and keeps ffn1, dH and a 4096^3 launch
    at 256"""
    L = lib.load()
    assert L.mmf_device_cu_count() == 256                         # the MI355X: the table's widths are for 256 workgroups
    cases = [(s[1], s[2], s[3], s[4]) for s in STEP_LAUNCHES] + [(GEMM_NT, 0, [(4096, 4096, 4096)], 256)]
    for layout, epi, shapes, want in cases:
        probs = _operands(layout, [(M, N, K, 0) for M, N, K in shapes], epi, seed=1)
        outs = [torch.empty((a.shape[0], b.shape[0] if layout == GEMM_NT else b.shape[1]), dtype=torch.bfloat16, device=DEV)
                for a, b, _, _ in probs]
        ops.gemm_group(layout, [(a, b, c, bias, aux) for (a, b, bias, aux), c in zip(probs, outs)], epi)
        assert L.mmf_gemm_last_impl() == 7
        assert L.mmf_gemm7_last_tile_n() == want, (shapes[0], L.mmf_gemm7_last_tile_n(), want)
    torch.cuda.synchronize()
