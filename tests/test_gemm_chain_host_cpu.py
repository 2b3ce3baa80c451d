"""CPU: the host side of generation 7's K-segment chains (mmf_gemm_chain_available / mmf_gemm_grouped_chain /
mmf_gemm7_chain_tile_n).  Validation launches nothing, so it runs without a GPU on made-up (aligned) addresses: the chain form
takes NN launches of 1..12 chains of 1..4 segments, every segment's K a multiple of 32 and at least 160, with the flag sets none /
bias / residual; everything else is answered 0 by _available and MMF_E_SHAPE by the call.  The tile walk sees a chain as ONE tile
list of K = the sum of its segments' K: the width rule must give a chain launch the width it gives the summed problems."""
import ctypes as C

from mmfusion import lib
from mmfusion.lib import EPI_ADD_AUX, EPI_BIAS, EPI_MASK_AUX, EPI_RELU, GEMM_NN, GEMM_NT, GEMM_TN

MMF_E_SHAPE = -1
BASE = 0x7F0000000000                       # addresses are only looked at (alignment), never followed


def _chain(M=480, N=768, ks=(768, 768, 1536, 1536), **kw):
    c = lib.GemmChain()
    c.C, c.bias, c.aux = BASE, BASE + 0x1000000, BASE + 0x2000000
    c.M, c.N, c.ldc, c.ldaux, c.num_segments = M, N, N, N, len(ks)
    for j, K in enumerate(ks[:lib.GEMM_CHAIN_MAX_SEGMENTS]):
        s = c.seg[j]
        s.A, s.B, s.K, s.lda, s.ldb = BASE + 0x10000000 * (j + 1), BASE + 0x10000000 * (j + 1) + 0x8000000, K, K, N
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _available(chains, layout=GEMM_NN, epi=0):
    arr = (lib.GemmChain * len(chains))(*chains)
    return lib.load().mmf_gemm_chain_available(arr, len(chains), layout, epi, None)


def _call(chains, layout=GEMM_NN, epi=0):
    arr = (lib.GemmChain * len(chains))(*chains)
    return lib.load().mmf_gemm_grouped_chain(arr, len(chains), layout, epi, None)


def test_struct_sizes_match_c_layout():
    assert C.sizeof(lib.GemmSegment) == 32
    assert C.sizeof(lib.GemmChain) == 48 + 4 * 32


def test_what_the_chain_form_takes():
    for epi in (0, EPI_BIAS, EPI_ADD_AUX):
        for nseg in (1, 2, 3, 4):
            assert _available([_chain(ks=(160, 192, 768, 1536)[:nseg])], epi=epi) == 1
    assert _available([_chain(M=m) for m in (8192, 6400, 480)], epi=EPI_ADD_AUX) == 1        # the step's launch
    assert _available([_chain(M=33, N=8, ks=(160,))] * lib.GEMM_MAX_CHAINS) == 1
    assert _available([_chain(ldc=776, ldaux=1024)], epi=EPI_ADD_AUX) == 1


def test_what_it_refuses():
    def seg(c, j, **kw):
        for k, v in kw.items():
            setattr(c.seg[j], k, v)
        return c
    refused = [
        ([_chain()], GEMM_NT, 0), ([_chain()], GEMM_TN, 0),                                   # NN only
        ([_chain()], GEMM_NN, EPI_RELU), ([_chain()], GEMM_NN, EPI_MASK_AUX), ([_chain()], GEMM_NN, EPI_BIAS | EPI_ADD_AUX),
        ([_chain(ks=(768, 128))], GEMM_NN, 0),                                                # K < (NS + 1) * 32 = 160
        ([_chain(ks=(176,))], GEMM_NN, 0),                                                    # K % 32
        ([_chain(num_segments=0)], GEMM_NN, 0), ([_chain(num_segments=5)], GEMM_NN, 0),
        ([_chain(M=0)], GEMM_NN, 0), ([_chain(N=772, ldc=776)], GEMM_NN, 0),                  # N % 8
        ([_chain(ldc=760)], GEMM_NN, 0), ([_chain(ldc=772)], GEMM_NN, 0),                     # ldc < N, ldc % 8
        ([_chain(C=BASE + 8)], GEMM_NN, 0), ([_chain(C=None)], GEMM_NN, 0),
        ([_chain(bias=None)], GEMM_NN, EPI_BIAS), ([_chain(aux=None)], GEMM_NN, EPI_ADD_AUX),
        ([_chain(ldaux=760)], GEMM_NN, EPI_ADD_AUX), ([_chain(aux=BASE + 8)], GEMM_NN, EPI_ADD_AUX),
        ([seg(_chain(), 2, lda=1528)], GEMM_NN, 0), ([seg(_chain(), 1, ldb=760)], GEMM_NN, 0),   # a row shorter than the segment
        ([seg(_chain(), 3, A=BASE + 2)], GEMM_NN, 0), ([seg(_chain(), 0, B=None)], GEMM_NN, 0),
        ([_chain(M=33, N=8, ks=(160,))] * (lib.GEMM_MAX_CHAINS + 1), GEMM_NN, 0),
        ([_chain(M=1 << 20, ks=(1536,))], GEMM_NN, 0),                                        # an operand of 2 GiB and more
    ]
    for chains, layout, epi in refused:
        assert _available(chains, layout, epi) == 0, (layout, epi)
        assert _call(chains, layout, epi) == MMF_E_SHAPE, (layout, epi)
        assert b"mmf_gemm_grouped_chain" in lib.load().mmf_last_error()
    assert _available([_chain(ldaux=0, aux=None, bias=None)]) == 1                            # unused operands are not looked at


def test_pinned_generation_has_no_chain_form():
    L = lib.load()
    try:
        for impl, want in ((6, 0), (2, 0), (7, 1), (0, 1)):
            lib.check(L.mmf_gemm_select_impl(impl))
            assert _available([_chain()]) == want, impl
    finally:
        lib.check(L.mmf_gemm_select_impl(0))


def _width_of_sums(shapes, workgroups):
    arr = (lib.GemmProblem * len(shapes))()
    for p, (M, N, K) in zip(arr, shapes):
        p.M, p.N, p.K = M, N, K
    return lib.load().mmf_gemm7_tile_n(arr, len(shapes), workgroups)


def test_the_walk_sees_a_chain_as_one_tile_list_of_summed_k():
    L = lib.load()
    cases = [
        ([(8192, 768, (768, 768, 1536, 1536)), (6400, 768, (768, 768, 1536, 1536)), (480, 768, (768, 768, 1536, 1536))], 256),
        ([(4096, 4096, (2048, 2048))], 256), ([(8192, 3072, (192, 192, 192, 192))], 256), ([(8192, 3072, (768,))], 128),
        ([(256, 768, (160, 608))], 1), ([(1000, 264, (768, 160)), (300, 520, (3072,)), (257, 8, (192, 192, 192))], 8),
    ]
    for chains, wgs in cases:
        arr = (lib.GemmChain * len(chains))(*[_chain(M, N, ks) for M, N, ks in chains])
        got = L.mmf_gemm7_chain_tile_n(arr, len(chains), wgs)
        assert got in (192, 256)
        assert got == _width_of_sums([(M, N, sum(ks)) for M, N, ks in chains], wgs), (chains, wgs)
    # the step's launch: three outputs of K = 4608, 236 tiles at the 192-wide form on 256 workgroups (one round), 177 at 256
    arr = (lib.GemmChain * 3)(*[_chain(M=m) for m in (8192, 6400, 480)])
    assert L.mmf_gemm7_chain_tile_n(arr, 3, 256) == 192
    assert L.mmf_gemm7_chain_tile_n(arr, 0, 256) == MMF_E_SHAPE
