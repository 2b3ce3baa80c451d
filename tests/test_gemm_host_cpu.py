"""CPU: the host side of mmf_gemm_grouped / mmf_gemm_grouped_ex and of the pure predicates beside them (mmf_gemm_relu_bits_available,
mmf_gemm7_tile_n).  Validation launches nothing, so it runs without a GPU on made-up (aligned) addresses.  Only refused calls and
predicates are here: every call below is answered by the entry point's validation or by a launch function's table fill (the "operand
larger than 2 GiB" rule) BEFORE a kernel is enqueued — a case that got past them would launch on addresses nobody owns.  The
answers are the ones the library gave before the three generations' launch functions shared one table fill and one statement of
what generation 7 takes of a problem (profiles/gemm_shared_parts.txt)."""
import ctypes as C

from mmfusion import lib
from mmfusion.lib import (EPI_ACCUM, EPI_ADD_AUX, EPI_BIAS, EPI_COLSUM_A, EPI_DROPOUT, EPI_MASK_AUX, EPI_MASK_BITS, EPI_RELU,
                          EPI_RELU_BITS, GEMM_NN, GEMM_NT, GEMM_TN)

E_SHAPE, E_ALIGN, E_LAUNCH, E_UNSUPPORTED = -1, -3, -4, -5
BASE = 0x7F0000000000                       # addresses are only looked at (null, alignment), never followed
RNG = BASE + 0x70000000


def _problem(M=8192, N=768, K=768, layout=GEMM_NT, **kw):
    p = lib.GemmProblem()
    p.A, p.B, p.C, p.bias, p.aux = (BASE + 0x10000000 * i for i in range(1, 6))
    p.M, p.N, p.K = M, N, K
    p.lda = M if layout == GEMM_TN else K
    p.ldb = K if layout == GEMM_NT else N
    p.ldc = p.ldaux = N
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _extra(alpha=1.0, p=0.0, rng=None, site=3):
    return lib.GemmExtra(alpha, p, rng, site)


def _refused(problems, layout=GEMM_NT, epi=0, out_f32=0, extra=None, n=None):
    """the call's return code and message; the plain entry point where there is no extra"""
    L = lib.load()
    arr = (lib.GemmProblem * max(1, len(problems)))(*problems) if problems is not None else None
    n = len(problems) if n is None else n
    if extra is None:
        rc = L.mmf_gemm_grouped(arr, n, layout, epi, out_f32, None)
    else:
        rc = L.mmf_gemm_grouped_ex(arr, n, layout, epi, out_f32, C.byref(extra), None)
    assert rc not in (0, E_LAUNCH), "a case of this file reached a launch"
    return rc, L.mmf_last_error().decode()


def _bits_available(problems, layout, epi, out_f32=0, extra=None, n=None):
    arr = (lib.GemmProblem * max(1, len(problems)))(*problems) if problems is not None else None
    return lib.load().mmf_gemm_relu_bits_available(arr, len(problems) if n is None else n, layout, epi, out_f32,
                                                   C.byref(extra if extra is not None else _extra()))


def _pinned(impls=(0, 2, 6, 7)):
    L = lib.load()
    for impl in impls:
        lib.check(L.mmf_gemm_select_impl(impl))
        yield impl


def test_problem_count():
    for n in (0, -1, lib.GEMM_MAX_PROBLEMS + 1):
        rc, msg = _refused([_problem()] * max(n, 1), n=n)
        assert rc == E_SHAPE and "num_problems=%d out of range [1,48]" % n in msg
    rc, msg = _refused(None, n=1)
    assert rc == E_SHAPE and "out of range" in msg


def test_layout_and_flag_combinations():
    for layout in (5, 3, -1):
        rc, msg = _refused([_problem()], layout=layout)
        assert rc == E_UNSUPPORTED and "unknown layout %d" % layout in msg
    tn = [_problem(layout=GEMM_TN)]
    cases = [
        ([_problem()], GEMM_NT, EPI_ACCUM, 0, "MMF_EPI_ACCUM needs f32 output"),
        ([_problem()], GEMM_NT, EPI_MASK_AUX | EPI_ADD_AUX, 0, "MASK_AUX and ADD_AUX are exclusive"),
        ([_problem()], GEMM_NT, EPI_COLSUM_A, 1, "COLSUM_A is a TN (wgrad) epilogue and excludes BIAS"),
        ([_problem(layout=GEMM_NN)], GEMM_NN, EPI_COLSUM_A, 1, "COLSUM_A is a TN"),
        (tn, GEMM_TN, EPI_COLSUM_A | EPI_BIAS, 1, "COLSUM_A is a TN"),
        ([_problem()], GEMM_NT, EPI_RELU_BITS | EPI_MASK_BITS | EPI_RELU, 0, "RELU_BITS needs RELU"),
        ([_problem()], GEMM_NT, EPI_RELU_BITS, 0, "RELU_BITS needs RELU"),
        ([_problem()], GEMM_NT, EPI_RELU_BITS | EPI_BIAS, 0, "RELU_BITS needs RELU"),
        ([_problem(layout=GEMM_NN)], GEMM_NN, EPI_MASK_BITS | EPI_MASK_AUX, 0, "exclusive (one aux pointer)"),
        ([_problem(layout=GEMM_NN)], GEMM_NN, EPI_MASK_BITS | EPI_ADD_AUX, 0, "exclusive (one aux pointer)"),
        ([_problem()], GEMM_NT, EPI_RELU | EPI_RELU_BITS | EPI_ADD_AUX, 0, "exclusive (one aux pointer)"),
    ]
    try:
        for _ in _pinned():
            for problems, layout, epi, f32, want in cases:
                rc, msg = _refused(problems, layout, epi, f32)
                assert rc == E_UNSUPPORTED and want in msg, (epi, msg)
            # dropout: the plain entry point has no extra; with one, a state and 0 <= p < 1
            epi = EPI_BIAS | EPI_RELU | EPI_DROPOUT
            for extra in (None, _extra(p=0.1), _extra(p=-0.1, rng=RNG), _extra(p=1.0, rng=RNG), _extra(p=float("nan"), rng=RNG)):
                rc, msg = _refused([_problem()], GEMM_NT, epi, 0, extra)
                assert rc == E_SHAPE and "MMF_EPI_DROPOUT needs rng_state and 0 <= p < 1" in msg
    finally:
        lib.check(lib.load().mmf_gemm_select_impl(0))


def test_bit_forms_exist_in_generation_7_only():
    bits_nt, bits_nn = EPI_RELU | EPI_RELU_BITS | EPI_BIAS, EPI_MASK_BITS
    try:
        for impl in _pinned((2, 6)):
            rc, msg = _refused([_problem()], GEMM_NT, bits_nt)
            assert rc == E_UNSUPPORTED and "exist in generation 7 only and this launch goes to generation %d" % impl in msg
            assert _bits_available([_problem()], GEMM_NT, bits_nt) == 0
        for _ in _pinned((0, 7)):
            # what generation 7 does not take falls back to 6 (K % 32 == 0) or 2, where the bits do not exist
            for p, layout, epi, extra, gen in [
                (_problem(K=128), GEMM_NT, bits_nt, None, 6), (_problem(K=776), GEMM_NT, bits_nt, None, 2),
                (_problem(N=772, ldc=776), GEMM_NT, bits_nt, None, 6), (_problem(ldc=772), GEMM_NT, bits_nt, None, 6),
                (_problem(layout=GEMM_NN, aux=None), GEMM_NN, bits_nn, None, 6),
                (_problem(layout=GEMM_NN, aux=BASE + 8), GEMM_NN, bits_nn, None, 6),
                (_problem(), GEMM_NT, bits_nt, _extra(alpha=2.0), 6),               # alpha rides on the NN mask only
                (_problem(layout=GEMM_NN), GEMM_NN, EPI_MASK_BITS | EPI_BIAS, None, 6),   # a flag set generation 7 does not instantiate
                (_problem(layout=GEMM_TN), GEMM_TN, bits_nn, None, None),
            ]:
                rc, msg = _refused([p], layout, epi, 0, extra)
                assert rc == E_UNSUPPORTED and "this launch goes to generation" + (" %d" % gen if gen else "") in msg, msg
                assert _bits_available([p], layout, epi, 0, extra) == 0
            rc, msg = _refused([_problem()], GEMM_NT, bits_nt, out_f32=1)
            assert rc == E_UNSUPPORTED and "generation 7 only" in msg
    finally:
        lib.check(lib.load().mmf_gemm_select_impl(0))


def test_relu_bits_available_is_generation_7s_answer():
    bits_nt, nn = EPI_RELU | EPI_RELU_BITS, dict(layout=GEMM_NN)
    try:
        for _ in _pinned((0, 7)):
            for epi in (bits_nt, bits_nt | EPI_BIAS):
                assert _bits_available([_problem()], GEMM_NT, epi) == 1
                assert _bits_available([_problem()], GEMM_NT, epi | EPI_DROPOUT, extra=_extra(p=0.1, rng=RNG)) == 1
                assert _bits_available([_problem()], GEMM_NT, epi | EPI_DROPOUT, extra=_extra(p=0.1)) == 0     # no state
            assert _bits_available([_problem(**nn)], GEMM_NN, EPI_MASK_BITS) == 1
            assert _bits_available([_problem(**nn)], GEMM_NN, EPI_MASK_BITS, extra=_extra(alpha=1.25)) == 1
            assert _bits_available([_problem(**nn), _problem(M=6400, K=1536, **nn), _problem(M=480, K=160, **nn)], GEMM_NN, EPI_MASK_BITS) == 1
            assert _bits_available([_problem(K=160)], GEMM_NT, bits_nt) == 1                      # K >= (NS + 1) * 32
            assert _bits_available([_problem(K=128)], GEMM_NT, bits_nt) == 0
            assert _bits_available([_problem(), _problem(K=176)], GEMM_NT, bits_nt) == 0          # K % 32, second problem
            assert _bits_available([_problem(ldc=776)], GEMM_NT, bits_nt) == 1
            assert _bits_available([_problem(ldaux=3, **nn)], GEMM_NN, EPI_MASK_BITS) == 1        # a bit buffer has no ldaux
            # aux at 8-byte but not 16-byte alignment: the entry point's own rule accepts it, generation 7 does not take it
            assert _bits_available([_problem(aux=BASE + 8, **nn)], GEMM_NN, EPI_MASK_BITS) == 0
            assert _bits_available([_problem(aux=BASE + 16, **nn)], GEMM_NN, EPI_MASK_BITS) == 1
            assert _bits_available([_problem(aux=BASE + 8)], GEMM_NT, bits_nt) == 0
            # not a question about the bit forms
            assert _bits_available([_problem()], GEMM_NT, EPI_BIAS | EPI_RELU) == 0
            assert _bits_available([_problem()], GEMM_NT, EPI_RELU_BITS) == 0
            assert _bits_available([_problem()], GEMM_NT, bits_nt, n=0) == 0
            assert _bits_available([_problem()] * 2, GEMM_NT, bits_nt, n=lib.GEMM_MAX_PROBLEMS + 1) == 0
            assert _bits_available(None, GEMM_NT, bits_nt, n=1) == 0
            assert _bits_available([_problem()], GEMM_NT, bits_nt, out_f32=1) == 0
        # automatic: a launch too small for the 256 x 256 tile goes to generation 2
        lib.check(lib.load().mmf_gemm_select_impl(0))
        assert _bits_available([_problem(M=256)], GEMM_NT, bits_nt) == 0
        lib.check(lib.load().mmf_gemm_select_impl(7))
        assert _bits_available([_problem(M=256)], GEMM_NT, bits_nt) == 1
    finally:
        lib.check(lib.load().mmf_gemm_select_impl(0))


def test_each_problem_is_validated():
    nn, tn = dict(layout=GEMM_NN), dict(layout=GEMM_TN)
    cases = [
        # (problem, layout, epilogue, out_f32, code, message)
        (_problem(M=0), GEMM_NT, 0, 0, E_SHAPE, "empty problem M=0 N=768 K=768"),
        (_problem(N=0), GEMM_NT, 0, 0, E_SHAPE, "empty problem"), (_problem(K=-8), GEMM_NT, 0, 0, E_SHAPE, "empty problem"),
        (_problem(A=None), GEMM_NT, 0, 0, E_SHAPE, "null operand"), (_problem(B=None), GEMM_NT, 0, 0, E_SHAPE, "null operand"),
        (_problem(C=None), GEMM_NT, 0, 0, E_SHAPE, "null operand"),
        (_problem(bias=None), GEMM_NT, EPI_BIAS, 0, E_SHAPE, "bias is null"),
        (_problem(bias=None, **tn), GEMM_TN, EPI_COLSUM_A, 1, E_SHAPE, "bias is null"),
        (_problem(aux=None), GEMM_NT, EPI_BIAS | EPI_ADD_AUX, 0, E_SHAPE, "aux is null"),
        (_problem(aux=None, **nn), GEMM_NN, EPI_MASK_AUX, 0, E_SHAPE, "aux is null"),
        (_problem(K=772), GEMM_NT, 0, 0, E_ALIGN, "violate the 8-element (operands) / 4-element (output) granularity"),
        (_problem(lda=772), GEMM_NT, 0, 0, E_ALIGN, "violate the 8-element"), (_problem(ldb=772), GEMM_NT, 0, 0, E_ALIGN, "violate the 8-element"),
        (_problem(M=772, **tn), GEMM_TN, 0, 1, E_ALIGN, "violate the 8-element"), (_problem(N=772, ldc=776, **nn), GEMM_NN, 0, 0, E_ALIGN, "violate the 8-element"),
        (_problem(N=770, ldc=776), GEMM_NT, 0, 0, E_ALIGN, "violate the 8-element"), (_problem(ldc=770), GEMM_NT, 0, 0, E_ALIGN, "violate the 8-element"),
        (_problem(ldaux=770), GEMM_NT, EPI_BIAS | EPI_ADD_AUX, 0, E_ALIGN, "ldaux=770 violate the 8-element"),
        (_problem(lda=760), GEMM_NT, 0, 0, E_SHAPE, "leading dimension smaller than the row"),
        (_problem(ldb=760), GEMM_NT, 0, 0, E_SHAPE, "leading dimension smaller than the row"),
        (_problem(ldb=760, **nn), GEMM_NN, 0, 0, E_SHAPE, "leading dimension smaller than the row"),
        (_problem(lda=8184, **tn), GEMM_TN, 0, 1, E_SHAPE, "leading dimension smaller than the row"),
        (_problem(ldc=760), GEMM_NT, 0, 0, E_SHAPE, "leading dimension smaller than the row"),
        (_problem(A=BASE + 8), GEMM_NT, 0, 0, E_ALIGN, "operand pointers must be 16-byte aligned"),
        (_problem(B=BASE + 2), GEMM_NT, 0, 0, E_ALIGN, "16-byte aligned"), (_problem(C=BASE + 8), GEMM_NT, 0, 0, E_ALIGN, "16-byte aligned"),
        (_problem(bias=BASE + 8), GEMM_NT, 0, 0, E_ALIGN, "16-byte aligned"),              # looked at whether or not a flag reads it
        (_problem(aux=BASE + 4), GEMM_NT, 0, 0, E_ALIGN, "16-byte aligned"),
    ]
    try:
        for _ in _pinned():
            for p, layout, epi, f32, code, want in cases:
                rc, msg = _refused([p], layout, epi, f32)
                assert rc == code and want in msg and "mmf_gemm_grouped[0]" in msg, (rc, msg)
                good = _problem(layout=layout)
                rc, msg = _refused([good, good, p], layout, epi, f32)                    # the message names the caller's problem
                assert rc == code and "mmf_gemm_grouped[2]" in msg, (rc, msg)
    finally:
        lib.check(lib.load().mmf_gemm_select_impl(0))


def test_operands_behind_buffer_descriptors_stay_below_2_gib():
    """A and B sit behind 32-bit buffer descriptors in every generation; C and aux (or the bit buffer) only in generation 7's drain.
    A call whose first problem has only a large C (aux) and whose second has a large A is therefore refused at problem 0 where
    generation 7 takes the launch and at problem 1 everywhere else (both problems have one K: generation 7 walks them by K)."""
    big = 1 << 20                                                                        # 2^20 x 1536 x 2 bytes = 3 GiB
    nn, tn = dict(layout=GEMM_NN), dict(layout=GEMM_TN)
    want = "operand larger than 2 GiB"
    try:
        for impl in _pinned():
            for p, layout, f32 in [
                (_problem(M=big, K=1536), GEMM_NT, 0), (_problem(M=256, N=big, K=1536), GEMM_NT, 0),               # A, B of NT
                (_problem(M=big, K=1536, **nn), GEMM_NN, 0), (_problem(M=256, N=1536, K=big, **nn), GEMM_NN, 0),   # A, B of NN
                (_problem(M=1536, N=256, K=big, **tn), GEMM_TN, 1), (_problem(M=256, N=1536, K=big, **tn), GEMM_TN, 1),
            ]:
                rc, msg = _refused([p], layout, 0, f32)
                assert rc == E_UNSUPPORTED and want in msg and "mmf_gemm_grouped[0]" in msg, (impl, msg)
            big_c = _problem(M=big, N=1536, K=160)
            big_x = _problem(M=big, N=8, K=160, ldaux=1536)
            big_a = _problem(M=big, N=8, K=160, lda=1536)
            at = 0 if impl in (0, 7) else 1
            rc, msg = _refused([big_c, big_a], GEMM_NT, 0)
            assert rc == E_UNSUPPORTED and want in msg and "mmf_gemm_grouped[%d]" % at in msg, (impl, msg)
            rc, msg = _refused([big_x, big_a], GEMM_NT, EPI_BIAS | EPI_ADD_AUX)
            assert rc == E_UNSUPPORTED and want in msg and "mmf_gemm_grouped[%d]" % at in msg, (impl, msg)
            rc, msg = _refused([big_c, big_a], GEMM_NT, 0, 1)          # f32 output never goes to generation 7: C is not looked at
            assert rc == E_UNSUPPORTED and want in msg and "mmf_gemm_grouped[1]" in msg, (impl, msg)
    finally:
        lib.check(lib.load().mmf_gemm_select_impl(0))


def _width(shapes, workgroups):
    arr = (lib.GemmProblem * len(shapes))()
    for p, (M, N, K) in zip(arr, shapes):
        p.M, p.N, p.K = M, N, K
    return lib.load().mmf_gemm7_tile_n(arr, len(shapes), workgroups)


def test_gemm7_tile_n():
    """the chain test's shapes as plain problems of the summed K (tests/test_gemm_chain_host_cpu.py), with the widths the rule gave them"""
    cases = [
        ([(8192, 768, 4608), (6400, 768, 4608), (480, 768, 4608)], 256, 192),
        ([(4096, 4096, 4096)], 256, 256), ([(8192, 3072, 768)], 256, 192), ([(8192, 3072, 768)], 128, 256),
        ([(256, 768, 768)], 1, 256), ([(1000, 264, 928), (300, 520, 3072), (257, 8, 576)], 8, 192),
    ]
    for shapes, wgs, want in cases:
        assert _width(shapes, wgs) == want, (shapes, wgs)
    arr = (lib.GemmProblem * 1)()
    L = lib.load()
    assert L.mmf_gemm7_tile_n(arr, 0, 256) == E_SHAPE
    assert L.mmf_gemm7_tile_n(arr, lib.GEMM_MAX_PROBLEMS + 1, 256) == E_SHAPE
    assert L.mmf_gemm7_tile_n(arr, 1, -1) == E_SHAPE
    assert L.mmf_gemm7_tile_n(None, 1, 256) == E_SHAPE
    assert b"mmf_gemm7_tile_n" in L.mmf_last_error()

