"""GPU: generation 7's K-segment chains (csrc/gemm7.hip, CHAIN; mmf_gemm_grouped_chain).  A chain's output tile runs its MFMA
chain over the segments in order — bias start, then the k-substeps of segment 0, 1, .. — so the launch must equal, BIT FOR BIT,
mmf_gemm_grouped on one problem whose A is the segments' A side by side and whose B is the segments' B stacked: for 1..4
segments, segment K from {160, 192, 768} (160 is the kernel's minimum: the operand switch falls into a segment's second stage), ragged
and multi-tile M, N that takes the 256-wide and the 192-wide tile, every flag set the chain form has, both forced tile widths, a
few persistent workgroups (a workgroup then walks several tiles, each with its segments) and launches of two and three chains
of different segment counts.  The error against a float64 product is reported and held to the bound of the gemm form pins
(test_kernel_forms_gpu.py: 2^-8 of the result's scale for a bf16 output)."""
import math

import pytest
import torch

from mmfusion import lib, ops
from mmfusion.lib import EPI_ADD_AUX, EPI_BIAS, GEMM_NN

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16_TOL = 2 ** -8
KS = (160, 192, 768)
MS = (33, 256, 257, 480)
NS = (192, 256, 768)
EPIS = (0, EPI_BIAS, EPI_ADD_AUX)


def _segment_ks(nseg, salt):
    """nseg segment lengths from KS; over the salts every length appears in every position"""
    return [KS[(salt + 2 * j) % 3] for j in range(nseg)]


def _chain(M, N, ks, epi, g, pad=0):
    """operands of one chain, the segments in buffers of their own (A_s with a wider leading dimension when pad > 0)"""
    segs = []
    ktot = sum(ks)
    for K in ks:
        a = torch.randn(M, K + pad, device=DEV, generator=g).to(torch.bfloat16)[:, pad:]
        b = (torch.randn(K, N + pad, device=DEV, generator=g) * ktot ** -0.5).to(torch.bfloat16)[:, :N]
        segs.append((a, b))
    bias = torch.randn(N, device=DEV, generator=g) if epi & EPI_BIAS else None
    aux = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16) if epi & EPI_ADD_AUX else None
    return segs, bias, aux


def _nan(M, N):
    return torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)


def _run_chains(chains, epi, wgs=0, tile_n=0):
    L = lib.load()
    outs = [_nan(segs[0][0].shape[0], segs[0][1].shape[1]) for segs, _, _ in chains]
    args = [(c, bias, aux, segs) for c, (segs, bias, aux) in zip(outs, chains)]
    try:
        lib.check(L.mmf_gemm_set_persistent_workgroups(wgs))
        lib.check(L.mmf_gemm7_set_tile_n(tile_n))
        assert ops.gemm_chain_available(args, epi)
        ops.gemm_chain_group(args, epi)
        assert L.mmf_gemm_last_impl() == 7
        width = L.mmf_gemm7_last_tile_n()
        torch.cuda.synchronize()
    finally:
        lib.check(L.mmf_gemm_set_persistent_workgroups(0))
        lib.check(L.mmf_gemm7_set_tile_n(0))
    return outs, width


def _run_concatenated(chains, epi):
    """mmf_gemm_grouped (generation 7) on the physically concatenated operands, one problem per chain"""
    L = lib.load()
    probs, outs = [], []
    for segs, bias, aux in chains:
        a = torch.cat([s[0] for s in segs], dim=1).contiguous()
        b = torch.cat([s[1] for s in segs], dim=0).contiguous()
        c = _nan(a.shape[0], b.shape[1])
        probs.append((a, b, c, bias, aux))
        outs.append(c)
    try:
        lib.check(L.mmf_gemm_select_impl(7))
        ops.gemm_group(GEMM_NN, probs, epi)
        assert L.mmf_gemm_last_impl() == 7
        torch.cuda.synchronize()
    finally:
        lib.check(L.mmf_gemm_select_impl(0))
    return outs


def _fp64(chains, epi):
    refs = []
    for segs, bias, aux in chains:
        r = sum(a.double().cpu() @ b.double().cpu() for a, b in segs)
        if epi & EPI_BIAS:
            r = r + bias.double().cpu()
        if epi & EPI_ADD_AUX:
            r = r + aux.double().cpu()
        refs.append(r)
    return refs


def _rel(c, ref):
    c = c.double().cpu()
    if not bool(torch.isfinite(c).all()):
        return math.inf
    return float((c - ref).abs().max() / float(ref.abs().max()))


def _check(chains, epi, what, grids=(0,), widths=(0,)):
    want = _run_concatenated(chains, epi)
    refs = _fp64(chains, epi)
    worst = 0.0
    seen = set()
    for wgs in grids:
        for tile_n in widths:
            got, width = _run_chains(chains, epi, wgs, tile_n)
            seen.add(width)
            for i, (x, y, r) in enumerate(zip(got, want, refs)):
                assert not bool(torch.isnan(x.float()).any()), f"{what} wgs {wgs} width {width} chain {i}: unwritten output"
                assert torch.equal(x, y), f"{what} wgs {wgs} width {width} chain {i}: differs from the concatenated GEMM"
                worst = max(worst, _rel(x, r))
    print(f"{what}: widths {sorted(seen)}, worst error against float64 {worst:.3e} of the result's scale (bound {BF16_TOL:.3e})")
    assert worst < BF16_TOL, worst
    return seen


@pytest.mark.parametrize("epi", EPIS, ids=["plain", "bias", "add_aux"])
@pytest.mark.parametrize("M", MS)
def test_chain_bit_equal_to_concatenated_gemm(M, epi):
    """every segment count and N at this M and flag set, at both tile widths (on launches this small the automatic rule always
    takes the narrower tile, so the widths are forced)"""
    g = torch.Generator(device=DEV).manual_seed(1000 + 10 * M + epi)
    seen = set()
    for nseg in (1, 2, 3, 4):
        for ni, N in enumerate(NS):
            ks = _segment_ks(nseg, nseg + ni + M)
            seen |= _check([_chain(M, N, ks, epi, g, pad=8 * (ni % 2))], epi, f"M {M} N {N} K {ks} epi {epi}", widths=(256, 192))
    assert seen == {192, 256}


@pytest.mark.parametrize("epi", EPIS, ids=["plain", "bias", "add_aux"])
def test_chain_forced_widths_and_few_workgroups(epi):
    """both tile widths on 1, 3 and the CU count of persistent workgroups: with one workgroup every tile of the launch and each
    tile's segments are consecutive entries of ONE walk (480 x 768: 2 x 3 / 2 x 4 tiles, four segments each)"""
    g = torch.Generator(device=DEV).manual_seed(77 + epi)
    chains = [_chain(480, 768, [768, 160, 192, 160], epi, g)]
    assert _check(chains, epi, f"forced widths epi {epi}", grids=(1, 3, 0), widths=(256, 192)) == {192, 256}


@pytest.mark.parametrize("epi", EPIS, ids=["plain", "bias", "add_aux"])
@pytest.mark.parametrize("wgs", (2, 0))
def test_launch_of_chains_with_different_segment_counts(wgs, epi):
    """two and three chains in one launch, segment counts 1..4 mixed, different M and N per chain: a workgroup's walk crosses from
    one chain's tile into another's, whose segment count differs"""
    g = torch.Generator(device=DEV).manual_seed(300 + epi)
    two = [_chain(257, 768, [768, 192, 160], epi, g), _chain(33, 256, [160], epi, g, pad=8)]
    three = [_chain(480, 192, [192, 768], epi, g), _chain(256, 768, [160, 160, 768, 192], epi, g), _chain(33, 192, [768], epi, g)]
    _check(two, epi, f"two chains epi {epi}", grids=(wgs,), widths=(0, 256, 192))
    _check(three, epi, f"three chains epi {epi}", grids=(wgs,), widths=(0, 256, 192))


def test_refused_launches():
    """what the chain form does not take: _available is 0 and the call returns MMF_E_SHAPE, nothing is launched"""
    g = torch.Generator(device=DEV).manual_seed(5)
    segs, _, _ = _chain(64, 256, [160, 192], 0, g)
    c = _nan(64, 256)
    short = (torch.zeros(64, 128, dtype=torch.bfloat16, device=DEV), torch.zeros(128, 256, dtype=torch.bfloat16, device=DEV))
    odd = (torch.zeros(64, 176, dtype=torch.bfloat16, device=DEV), torch.zeros(176, 256, dtype=torch.bfloat16, device=DEV))
    for bad in ([segs[0], short], [odd]):
        assert not ops.gemm_chain_available([(c, None, None, bad)], 0)
        with pytest.raises(RuntimeError, match="mmf_gemm_grouped_chain"):
            ops.gemm_chain_group([(c, None, None, bad)], 0)
    assert not ops.gemm_chain_available([(c, None, None, segs)], EPI_BIAS)          # the flag without its operand
    assert not ops.gemm_chain_available([(c, None, None, segs)], EPI_BIAS | EPI_ADD_AUX)
    torch.cuda.synchronize()
    assert bool(torch.isnan(c.float()).all())
