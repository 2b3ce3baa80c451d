"""GPU: every dropout mask of the fusion path against the host restatement of its keying (tests/keyed_dropout_ref.py, itself
pinned by tests/test_keyed_dropout_ref_cpu.py): the GEMM epilogues of generations 2, 6 and 7, the skinny forward and dgrad, the
dense GAT layer, ModalityDropout's draw, mmf_dropout past one grid pass, and the site / state arithmetic of mmfusion.ops.

No mask is read off the launch it checks: the expected mask comes from the restated hash of (state, site, sub-stream, index), and
with positive operands (|randn| rounded to bf16: every pre-dropout value is > 0) the zero pattern of the WHOLE output must equal
it.  Signed operands check the arithmetic around the mask against the float64 epilogue restatement, elementwise, within
  one rounding of the result to bf16 (2^-8 relative; bf16 outputs)  +  K 2^-24 sum|a||b| (f32 accumulation, evaluated in float64),
the second term carried through the epilogue's own factors (keyed_dropout_ref.epilogue_bound).

Conventions: calls go through mmfusion.lib on raw tensors; the state has a non-zero high word; outputs are pre-filled with NaN
(known values where the kernel accumulates) and row-strided outputs keep NaN guard columns; the process-wide GEMM hooks are set
inside try / finally and the generation (and tile width) that ran is asserted after each launch.  Each case prints `KEYED` lines:
elements whose mask was compared / disagreed, and the worst error / bound ratio of each arithmetic comparison
(profiles/keyed_masks_parity.txt is those lines from an MI355X run).

One-line mutations of the keying, each built and run once on an MI355X, and the case here that fails under it:
  idx = n for m * N + n in gemm2.hip                      test_gemm_epilogue_nt_every_flag_set[2-*], test_gemm_epilogue_nn_tn[2-*]
  pi for args.orig[pi] in gemm7.hip                       test_gemm7_mask_follows_the_callers_problem_index[*]
  P.ldy for N in the skinny forward's index               test_skinny_fwd_mask_and_twin[M >= 16]  (M = 1 has one row: idx = n either way)
  idx for idx + e in the skinny dgrad                     test_skinny_dgrad_regenerates_the_forward_mask[*]
  0 for the modality fallback's % 3u pick                 test_modality_dropout_draw[*]
  (j * 3 + i) for (i * 3 + j) in the gat3 backward only   test_gat3_coefficient_dropout[*]
  _site = 1 in ops.begin_training_forward                 test_ops_sites_and_state"""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fused_seams_ref as seams  # noqa: E402
import keyed_dropout_ref as K  # noqa: E402
import small_ref as R  # noqa: E402
from mmfusion import lib, ops  # noqa: E402
from mmfusion.lib import (EPI_ACCUM, EPI_ADD_AUX, EPI_BIAS, EPI_DROPOUT, EPI_MASK_AUX, EPI_RELU, EPI_RELU_BITS, GEMM_NN, GEMM_NT,
                          GEMM_TN)  # noqa: E402
from test_kernel_forms_gpu import DEV, F32_TOL, bf, expected_strip, f32, host, nan_like, rnd  # noqa: E402
from test_streaming_small_gpu import bits, bound_ok, hold  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
STATE = (0x1234567 << 32) | 0x89ABCDEF
P = 0.25
THRESH = K.mmf_drop_thresh(P)
INV = K.inv_keep_of(THRESH)
LAYOUT = {GEMM_NT: "NT", GEMM_NN: "NN", GEMM_TN: "TN"}


class Record:
    """rec(name, ratio): the worst error / bound ratio per name; rec.mask(name, got, keep): counts the compared / disagreeing
    elements of a mask and fails on the first disagreement"""

    def __init__(self):
        self.ratio, self.masks = {}, {}

    def __call__(self, name, ratio):
        self.ratio[name] = max(self.ratio.get(name, 0.0), float(ratio))

    def mask(self, name, got, keep):
        got = got.detach().cpu().numpy().astype(bool)
        assert got.shape == keep.shape, (name, got.shape, keep.shape)
        bad = got != keep
        c = self.masks.setdefault(name, [0, 0])
        c[0] += keep.size
        c[1] += int(bad.sum())
        assert not bad.any(), f"{name}: {int(bad.sum())} of {keep.size} elements disagree with the restated mask, first at {tuple(np.argwhere(bad)[0])}"


@pytest.fixture
def rec(request):
    r = Record()
    yield r
    test = request.node.nodeid.split("::")[-1]
    for name, (n, bad) in r.masks.items():
        print(f"KEYED {test} {name}: mask elements {n} disagreed {bad}")
    for name, x in r.ratio.items():
        print(f"KEYED {test} {name}: worst error/bound {x:.4f}")


@pytest.fixture(scope="module")
def state():
    return K.state_tensor(STATE, DEV)


def operand(shape, seed, positive):
    x = rnd(*shape, seed=seed)
    return x.abs() if positive else x


def same(a, b):
    return bool(torch.equal(bits(a).cpu(), bits(b).cpu()))


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


@contextlib.contextmanager
def pinned(impl, workgroups=0, tile_n=0):
    """one GEMM generation (and, for generation 7, grid and tile width) for the launches inside; always reset"""
    L = lib.load()
    try:
        lib.check(L.mmf_gemm_select_impl(impl))
        lib.check(L.mmf_gemm_set_persistent_workgroups(workgroups))
        lib.check(L.mmf_gemm7_set_tile_n(tile_n))
        yield L
    finally:
        L.mmf_gemm_select_impl(0)
        L.mmf_gemm_set_persistent_workgroups(0)
        L.mmf_gemm7_set_tile_n(0)


# =============================================================================================== a / b: GEMM epilogues
class GemmData:
    """operands of one problem on the device and, in float64 on the host, the exact product of the rounded operands and
    sum|a||b|; aux is row-strided (ldaux = N + 8)"""

    def __init__(self, layout, M, N, K_, seed, positive):
        self.M, self.N, self.K = M, N, K_
        a_shape = (K_, M) if layout == GEMM_TN else (M, K_)
        b_shape = (N, K_) if layout == GEMM_NT else (K_, N)
        self.A, self.B = bf(operand(a_shape, seed, positive)), bf(operand(b_shape, seed + 1, positive))
        self.bias = f32(operand((N,), seed + 2, positive))
        self.aux = bf(operand((M, N + 8), seed + 3, positive))[:, :N]
        self.cold = f32(operand((M, N), seed + 4, positive))
        a, b = host(self.A), host(self.B)
        a = a.t() if layout == GEMM_TN else a
        b = b.t() if layout == GEMM_NT else b
        self.acc, self.abs_acc = a @ b, a.abs() @ b.abs()


def gemm_data(layout, shapes, seed, positive):
    return [GemmData(layout, M, N, K_, seed + 10 * i, positive) for i, (M, N, K_) in enumerate(shapes)]


def gemm_problems(data, epi, out_f32, with_bits=False):
    """-> (GemmProblem list, output buffers, bit buffers): problem 0 has ldc = N + 8 with NaN guard columns; an accumulating
    output starts from the known old C"""
    ps, bufs, bitbufs = [], [], []
    for i, d in enumerate(data):
        ldc = d.N + (8 if i == 0 else 0)
        buf = nan_like((d.M, ldc), F32 if out_f32 else BF16)
        if epi & EPI_ACCUM:
            buf[:, :d.N] = d.cold
        bb = ops.relu_bits_buffer(buf[:, :d.N]).fill_(0xA5) if with_bits else None
        aux = bb if with_bits else d.aux if epi & (EPI_MASK_AUX | EPI_ADD_AUX) else None
        ps.append(lib.GemmProblem(d.A.data_ptr(), d.B.data_ptr(), buf.data_ptr(), d.bias.data_ptr() if epi & EPI_BIAS else None,
                                  None if aux is None else aux.data_ptr(), d.M, d.N, d.K, d.A.stride(0), d.B.stride(0), ldc,
                                  0 if (aux is None or with_bits) else aux.stride(0)))
        bufs.append(buf), bitbufs.append(bb)
    return ps, bufs, bitbufs


def gemm_expected(d, epi, out_f32, alpha, keep):
    """(float64 reference, elementwise bound, what a dropped element holds) under the restated mask"""
    aux = host(d.aux)
    kw = dict(keep=keep, inv_keep=INV, alpha=alpha, mask_aux=aux if epi & EPI_MASK_AUX else None)
    bias = host(d.bias) if epi & EPI_BIAS else None
    ref = K.epilogue(d.acc, bias=bias, relu=bool(epi & EPI_RELU), add_aux=aux if epi & EPI_ADD_AUX else None,
                     c_old=host(d.cold) if epi & EPI_ACCUM else None, **kw)
    abs_acc = d.abs_acc if bias is None else d.abs_acc + bias.abs()
    bound = K.epilogue_bound(ref, abs_acc, d.K, not out_f32, **kw)
    base = aux if epi & EPI_ADD_AUX else host(d.cold) if epi & EPI_ACCUM else torch.zeros_like(ref)
    return ref, bound, base


def check_gemm(rec, label, data, bufs, epi, out_f32, alpha, site, positive):
    for i, (d, buf) in enumerate(zip(data, bufs)):
        keep = K.gemm_keep(STATE, site, i, d.M, d.N, THRESH)                    # sub-stream: the CALLER's problem index
        ref, bound, base = gemm_expected(d, epi, out_f32, alpha, keep)
        c = buf[:, :d.N]
        assert all_nan(buf[:, d.N:]), f"{label}[{i}]: wrote past N"
        if positive:      # every pre-dropout value is > 0 (the residual / old C comes back unchanged where dropped)
            rec.mask(f"{label} mask", host(c) != base, keep)
        bound_ok(rec, f"{label} {'positive' if positive else 'signed'}", c, ref, bound)


FLAG_SETS = [("DROPOUT", EPI_DROPOUT, False, 1.0),
             ("BIAS|DROPOUT", EPI_BIAS | EPI_DROPOUT, False, 1.0),
             ("BIAS|RELU|DROPOUT", EPI_BIAS | EPI_RELU | EPI_DROPOUT, False, 1.0),
             ("BIAS|RELU|DROPOUT|ADD_AUX", EPI_BIAS | EPI_RELU | EPI_DROPOUT | EPI_ADD_AUX, False, 1.0),
             ("DROPOUT|MASK_AUX alpha=2", EPI_DROPOUT | EPI_MASK_AUX, False, 2.0),
             ("f32 DROPOUT", EPI_DROPOUT, True, 1.0),
             ("f32 DROPOUT|ACCUM", EPI_DROPOUT | EPI_ACCUM, True, 1.0)]
# one launch = these problems in this order: a ragged M and N against every tile (256 x 128, 256 x 256), one tiny problem
GEN_SHAPES = {2: [(200, 136, 40), (130, 260, 72), (8, 8, 8)], 6: [(300, 264, 160), (257, 520, 96), (40, 8, 32)]}


def launch_gemm(L, impl, ps, layout, epi, out_f32, alpha, state, site):
    lib.gemm_grouped(ps, layout, epi, out_f32, alpha, P, state.data_ptr(), site)
    assert L.mmf_gemm_last_impl() == impl, f"generation {L.mmf_gemm_last_impl()} ran, not {impl}"
    torch.cuda.synchronize()


def raw_gemm_rc(L, ps, layout, epi, out_f32, alpha, state, site):
    arr = (lib.GemmProblem * len(ps))(*ps)
    ex = lib.GemmExtra(alpha, P, state.data_ptr(), site)
    return L.mmf_gemm_grouped_ex(arr, len(ps), layout, epi, int(out_f32), C.byref(ex), lib.stream_ptr())


@pytest.mark.parametrize("positive", [True, False], ids=["positive", "signed"])
@pytest.mark.parametrize("impl", [2, 6])
def test_gemm_epilogue_nt_every_flag_set(impl, positive, state, rec):
    """NT, every flag set, one grouped launch each; the run-time-flag epilogue of generation 6 must take every DROPOUT launch
    (none of its compile-time forms has dropout)"""
    data = gemm_data(GEMM_NT, GEN_SHAPES[impl], 100 * impl, positive)
    with pinned(impl) as L:
        for j, (name, epi, out_f32, alpha) in enumerate(FLAG_SETS):
            site = 5 + j
            ps, bufs, _ = gemm_problems(data, epi, out_f32)
            launch_gemm(L, impl, ps, GEMM_NT, epi, out_f32, alpha, state, site)
            check_gemm(rec, f"gemm{impl} NT {name}", data, bufs, epi, out_f32, alpha, site, positive)
        # ACCUM exists for f32 output only: the bf16 launch is refused, nothing is written
        ps, bufs, _ = gemm_problems(data, EPI_DROPOUT, False)
        assert raw_gemm_rc(L, ps, GEMM_NT, EPI_DROPOUT | EPI_ACCUM, False, 1.0, state, 5) == E_UNSUPPORTED
        torch.cuda.synchronize()
        assert all(all_nan(b) for b in bufs)


def aligned_shapes(shapes, layout):
    """the nearest shapes the layout's 8-element operand granularity takes: NN needs N % 8 == 0, TN also M % 8 == 0"""
    up = lambda v: (v + 7) // 8 * 8     # noqa: E731
    return [(up(M) if layout == GEMM_TN else M, up(N), K_) for M, N, K_ in shapes]


@pytest.mark.parametrize("layout,sets", [(GEMM_NN, FLAG_SETS[:2]), (GEMM_TN, FLAG_SETS[:1])], ids=["NN", "TN"])
@pytest.mark.parametrize("impl", [2, 6])
def test_gemm_epilogue_nn_tn(impl, layout, sets, state, rec):
    """NN (B is K x N: N % 8 == 0) and TN (A is K x M: M % 8 == 0 too).  Where the NT shapes break that granularity the launch
    is refused with MMF_E_ALIGN and writes nothing; the case then runs at the nearest shapes the layout takes (still ragged
    against the tiles)."""
    listed, shapes = GEN_SHAPES[impl], aligned_shapes(GEN_SHAPES[impl], layout)
    with pinned(impl) as L:
        if shapes != listed:
            ps, bufs, _ = gemm_problems(gemm_data(layout, listed, 7, True), EPI_DROPOUT, False)
            assert raw_gemm_rc(L, ps, layout, EPI_DROPOUT, False, 1.0, state, 5) == E_ALIGN, L.mmf_last_error()
            torch.cuda.synchronize()
            assert all(all_nan(b) for b in bufs)
        for positive in (True, False):
            data = gemm_data(layout, shapes, 100 * impl + layout, positive)
            for j, (name, epi, out_f32, alpha) in enumerate(sets):
                site = 20 + j
                ps, bufs, _ = gemm_problems(data, epi, out_f32)
                launch_gemm(L, impl, ps, layout, epi, out_f32, alpha, state, site)
                check_gemm(rec, f"gemm{impl} {LAYOUT[layout]} {name}", data, bufs, epi, out_f32, alpha, site, positive)


# the caller's order is NOT the kernel's (longest K first): 3, 1, 2, 0
G7_SHAPES = [(520, 264, 160), (300, 520, 768), (1000, 392, 512), (256, 256, 2048)]


@pytest.fixture(scope="module")
def g7_data():
    assert sorted(range(4), key=lambda i: -G7_SHAPES[i][2]) != [0, 1, 2, 3]
    return {positive: gemm_data(GEMM_NT, G7_SHAPES, 700, positive) for positive in (True, False)}


@pytest.mark.parametrize("tile_n", [256, 192])
@pytest.mark.parametrize("workgroups", [3, 0])
def test_gemm7_mask_follows_the_callers_problem_index(workgroups, tile_n, g7_data, state, rec):
    """generation 7 sorts its problems by K and walks them on persistent workgroups; the mask of each is still keyed by the
    caller's index.  BIAS|RELU|DROPOUT with and without RELU_BITS; the written bits are (stored value > 0): with positive
    operands exactly the restated mask."""
    epi, site = EPI_BIAS | EPI_RELU | EPI_DROPOUT, 31
    with pinned(7, workgroups, tile_n) as L:
        for positive in (True, False):
            data = g7_data[positive]
            for with_bits in (False, True):
                e = epi | (EPI_RELU_BITS if with_bits else 0)
                ps, bufs, bitbufs = gemm_problems(data, e, False, with_bits)
                if with_bits:
                    assert lib.gemm_relu_bits_available(ps, GEMM_NT, e, 1.0, P, state.data_ptr(), site)
                launch_gemm(L, 7, ps, GEMM_NT, e, False, 1.0, state, site)
                assert L.mmf_gemm7_last_tile_n() == tile_n
                check_gemm(rec, f"gemm7 NT BIAS|RELU|DROPOUT{'|RELU_BITS' if with_bits else ''}", data, bufs, epi, False, 1.0, site, positive)
                if with_bits:
                    for i, (d, buf, bb) in enumerate(zip(data, bufs, bitbufs)):
                        got = seams.unpack_relu_bits(bb, d.M, d.N)
                        assert bool(torch.equal(got, buf[:, :d.N].float() > 0)), f"problem {i}: bits != (stored value > 0)"
                        if positive:
                            rec.mask("gemm7 NT RELU_BITS bits", got, K.gemm_keep(STATE, site, i, d.M, d.N, THRESH))


# =============================================================================================== c / d: skinny forward and dgrad
SK_N = (8, 264, 520)                                   # the three problems of every skinny group (W rows)
SK_SITE = 11


def skinny_keep(i, M):
    """the mask of problem i of a skinny group: the forward's (M, N) output and the dgrad's (M, N_out) gradient share it"""
    return K.gemm_keep(STATE, SK_SITE, i, M, SK_N[i], THRESH)


@pytest.mark.parametrize("K_", [64, 1536])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_skinny_fwd_mask_and_twin(M, K_, state, rec):
    """y = dropout(act(x W^T + b)): bf16 and f32 x (narrowed while loaded), both output dtypes with the Y2 twin in the other one,
    BIAS|DROPOUT and BIAS|RELU|DROPOUT; x, Y and Y2 row-strided"""
    ws = [bf(operand((N, K_), 40 + i, True)) for i, N in enumerate(SK_N)]
    bs = [f32(operand((N,), 50 + i, True)) for i, N in enumerate(SK_N)]
    for x_f32 in (False, True):
        xb = [(f32 if x_f32 else bf)(operand((M, K_ + 8), 60 + i, True)) for i in range(3)]
        xs = [x[:, :K_] for x in xb]
        x64 = [K.bf16r(host(x)) for x in xs]
        accs = [(x @ host(w).t(), x.abs() @ host(w).abs().t() + host(b).abs()) for x, w, b in zip(x64, ws, bs)]
        for out_f32 in (False, True):
            for flags in (EPI_BIAS | EPI_DROPOUT, EPI_BIAS | EPI_RELU | EPI_DROPOUT):
                ybuf = [nan_like((M, N + 8), F32 if out_f32 else BF16) for N in SK_N]
                y2buf = [nan_like((M, N + 4), BF16 if out_f32 else F32) for N in SK_N]
                probs = [lib.SkinnyProblemEx(lib.SkinnyProblem(xs[i].data_ptr(), ws[i].data_ptr(), ybuf[i].data_ptr(), bs[i].data_ptr(), None,
                                                               M, N, K_, xb[i].stride(0), ws[i].stride(0), ybuf[i].stride(0), 0),
                                             y2buf[i].data_ptr(), None, None, y2buf[i].stride(0), 0, 0, 0) for i, N in enumerate(SK_N)]
                lib.skinny_fwd_ex(probs, flags, out_f32, lib.SkinnyExtra(int(x_f32), 0, 1.0, P, state.data_ptr(), SK_SITE, 0))
                torch.cuda.synchronize()
                tag = f"skinny fwd x {'f32' if x_f32 else 'bf16'} y {'f32' if out_f32 else 'bf16'}"
                for i, N in enumerate(SK_N):
                    keep = skinny_keep(i, M)
                    y, y2 = ybuf[i][:, :N], y2buf[i][:, :N]
                    assert all_nan(ybuf[i][:, N:]) and all_nan(y2buf[i][:, N:])
                    rec.mask(f"{tag} mask", y != 0, keep)
                    rec.mask(f"{tag} Y2 mask", y2 != 0, keep)
                    y32, y16 = (y, y2) if out_f32 else (y2, y)
                    assert same(y32.to(BF16), y16), f"{tag}[{i}]: Y2 is not the rounded twin"
                    ref = K.epilogue(accs[i][0], bias=host(bs[i]), relu=bool(flags & EPI_RELU), keep=keep, inv_keep=INV)
                    for out, is16 in ((y32, False), (y16, True)):
                        bound_ok(rec, f"{tag} {'bf16' if is16 else 'f32'} values", out, ref,
                                 K.epilogue_bound(ref, accs[i][1], K_, is16, keep=keep, inv_keep=INV))


STRIP_KIN = {1: 72, 2: 1032, 4: 2760}                   # dx columns per problem: three problems give the strip width named


@pytest.mark.parametrize("M", [1, 64])
@pytest.mark.parametrize("ct", [1, 2, 4])
def test_skinny_dgrad_regenerates_the_forward_mask(ct, M, state, rec):
    """dz = dy * (gate > 0) * gate_scale * keep / (1 - p), dx = dz W [* (aux > 0) * alpha] at every strip width.
    (1) DROPOUT alone on dy = 1: the written dz is keep * bf16(inv_keep) exactly — the regenerated mask, the one skinny_keep gives the
    forward of the same (site, problem, M, N) — and dx, formed per strip from masks each workgroup regenerates, follows it;
    (2) gate, MASK_AUX and alpha on signed data against the float64 restatement (dx from the dz the kernel wrote, once that is held)."""
    Kin = STRIP_KIN[ct]
    assert expected_strip([Kin] * 3) == ct
    L = lib.load()
    inv16 = float(K.bf16r(torch.tensor(INV, dtype=F64)))
    for dy_f32 in (False, True):
        tag = f"skinny dgrad strip {ct} dy {'f32' if dy_f32 else 'bf16'}"
        for gated in (False, True):
            wb = [bf(operand((N, Kin + 8), 70 + i, not gated)) for i, N in enumerate(SK_N)]
            ws = [w[:, :Kin] for w in wb]
            dys = [(f32 if dy_f32 else bf)(rnd(M, N, seed=80 + i) if gated else torch.ones(M, N, dtype=F64)) for i, N in enumerate(SK_N)]
            gates = [bf(rnd(M, N, seed=90 + i)) for i, N in enumerate(SK_N)]
            auxs = [bf(rnd(M, Kin, seed=95 + i)) for i in range(3)]
            out_f32 = not gated
            dzb = [nan_like((M, N + 8), BF16) for N in SK_N]
            dxb = [nan_like((M, Kin + 8), F32 if out_f32 else BF16) for _ in SK_N]
            probs = [lib.SkinnyProblemEx(lib.SkinnyProblem(dys[i].data_ptr(), ws[i].data_ptr(), dxb[i].data_ptr(), None,
                                                           auxs[i].data_ptr() if gated else None, M, N, Kin, dys[i].stride(0), wb[i].stride(0),
                                                           dxb[i].stride(0), auxs[i].stride(0) if gated else 0),
                                         None, gates[i].data_ptr() if gated else None, dzb[i].data_ptr(), 0, gates[i].stride(0) if gated else 0,
                                         dzb[i].stride(0), 0) for i, N in enumerate(SK_N)]
            alpha, gate_scale = (1.5, 2.0) if gated else (1.0, 1.0)
            extra = lib.SkinnyExtra(int(dy_f32), 0, gate_scale, P, state.data_ptr(), SK_SITE, 0)
            lib.skinny_dgrad_ex(probs, EPI_DROPOUT | (EPI_MASK_AUX if gated else 0), alpha, out_f32, extra)
            assert L.mmf_skinny_last_strip() == ct
            torch.cuda.synchronize()
            for i, N in enumerate(SK_N):
                keep = skinny_keep(i, M)
                keep_t = torch.from_numpy(keep).to(F64)
                dz, dx, w64 = host(dzb[i][:, :N]), dxb[i][:, :Kin], host(ws[i])
                assert all_nan(dzb[i][:, N:]) and all_nan(dxb[i][:, Kin:])
                if not gated:
                    rec.mask(f"{tag} dz mask", dz != 0, keep)
                    assert bool(torch.equal(dz, keep_t * inv16)), f"{tag}[{i}]: dz is not keep * bf16(inv_keep)"
                    dx_ref = dz @ w64
                    rec.mask(f"{tag} dx of all-dropped rows", host(dx) != 0, np.repeat(keep.any(axis=1)[:, None], Kin, axis=1))
                    bound_ok(rec, f"{tag} dx", dx, dx_ref, N * K.U24 * (dz.abs() @ w64.abs()))
                else:
                    dz_ref = torch.where(host(gates[i]) > 0, host(dys[i]) * gate_scale, torch.zeros(M, N, dtype=F64)) * keep_t * INV
                    bound_ok(rec, f"{tag} gated dz", dz, dz_ref, K.BF16_RN * dz_ref.abs())
                    live = (host(auxs[i]) > 0).to(F64)
                    dx_ref = (dz @ w64) * live * alpha
                    bound_ok(rec, f"{tag} gated dx", dx, dx_ref, N * K.U24 * (dz.abs() @ w64.abs()) * live * alpha + K.BF16_RN * dx_ref.abs())


# =============================================================================================== e: dense GAT layer
GAT_P, GAT_SITE = 0.5, 7


def gat_run_fwd(L, h, a_s, a_d, bias, B, H, C_, state):
    prm = lib.Gat3Params(B, H, C_, 0, 0.2, GAT_P, state.data_ptr(), GAT_SITE)
    y, alpha, sd = nan_like((B, 3, C_), BF16), nan_like((B, 3, 3, H)), nan_like((B, 2, 3, H))
    lib.check(L.mmf_gat3_dense_fwd(h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), y.data_ptr(), None, alpha.data_ptr(),
                                   sd.data_ptr(), C.byref(prm), lib.stream_ptr()))
    torch.cuda.synchronize()
    return prm, y, alpha, sd


@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_gat3_coefficient_dropout(H, state, rec):
    """forward: node features that are distinct unit vectors (h[b][j][hh] = e_{j H + hh}), zero bias, no ReLU: entry (i, j H + hh)
    of y IS the dropped coefficient alpha[i][j][hh] keep inv_keep / H; the saved alpha stays undropped.  backward: random h, every
    gradient against float64 autograd of the documented formula under the restated mask."""
    L = lib.load()
    thresh = K.mmf_drop_thresh(GAT_P)
    inv = K.inv_keep_of(thresh)
    for B in (1, 5):
        keep = K.gat3_keep(STATE, GAT_SITE, B, H, thresh)
        keep_t = torch.from_numpy(keep).to(F64)
        # ---- forward, C = 3 H + 5: the last five columns see no node
        C_ = 3 * H + 5
        h64 = torch.zeros(B, 3, H, C_, dtype=F64)
        for j in range(3):
            for hh in range(H):
                h64[:, j, hh, j * H + hh] = 1.0
        a_s, a_d = f32(rnd(H, C_, seed=H + B)), f32(rnd(H, C_, seed=H + B + 1))
        bias = torch.zeros(C_, dtype=F32, device=DEV)
        _, y, alpha, _ = gat_run_fwd(L, f32(h64), a_s, a_d, bias, B, H, C_, state)
        ra = R.gat3_fwd(h64, host(a_s), host(a_d), torch.zeros(C_, dtype=F64), 0.2, False)[2]
        hold(rec, "gat3 saved alpha (undropped)", alpha, ra, F32_TOL)
        coef = host(y)[:, :, :3 * H].reshape(B, 3, 3, H)                      # [b][i][j H + hh] -> (b, i, j, hh)
        rec.mask(f"gat3 fwd heads {H} mask", coef != 0, keep)
        want = ra * keep_t * inv / H
        bound_ok(rec, "gat3 fwd dropped coefficients", coef, want, K.BF16_RN * want.abs())
        assert bool((host(y)[:, :, 3 * H:] == 0).all())
        # ---- backward, C = 136, gradient through y and the pooled output
        C_ = 136
        hb = f32(rnd(B, 3, H, C_, seed=3 * H + B))
        sc = 2 * C_ ** -0.5
        a_s, a_d, bias = f32(rnd(H, C_, seed=1, scale=sc)), f32(rnd(H, C_, seed=2, scale=sc)), f32(rnd(C_, seed=3, scale=0.3))
        prm, y, alpha, sd = gat_run_fwd(L, hb, a_s, a_d, bias, B, H, C_, state)
        dy, dp = bf(rnd(B, 3, C_, seed=4)), bf(rnd(B, C_, seed=5))
        dh = nan_like((B, 3, H, C_))
        das, dad, db = (torch.zeros(s, dtype=F32, device=DEV) for s in ((H, C_), (H, C_), (C_,)))
        lib.check(L.mmf_gat3_dense_bwd(hb.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), y.data_ptr(), alpha.data_ptr(), sd.data_ptr(),
                                       dy.data_ptr(), dp.data_ptr(), dh.data_ptr(), das.data_ptr(), dad.data_ptr(), db.data_ptr(),
                                       C.byref(prm), lib.stream_ptr()))
        torch.cuda.synchronize()
        hr, asr, adr, br = (host(t).requires_grad_(True) for t in (hb, a_s, a_d, bias))
        s_src, s_dst = (hr * asr).sum(-1), (hr * adr).sum(-1)
        z = s_dst.unsqueeze(2) + s_src.unsqueeze(1)                            # (B, i, j, H)
        e = torch.where(z > 0, z, z * 0.2)
        ex = torch.exp(e - e.max(dim=2, keepdim=True).values)
        al = ex / (ex.sum(dim=2, keepdim=True) + 1e-16)
        out = torch.einsum("bijh,bjhc->bic", al * keep_t * inv, hr) / H + br
        ((out * host(dy)).sum() + (out.mean(1) * host(dp)).sum()).backward()
        hold(rec, "gat3 y under the restated mask", y, out.detach(), 2.0 ** -8)
        hold(rec, "gat3 bwd dh", dh, hr.grad, F32_TOL)
        hold(rec, "gat3 bwd datt_src", das, asr.grad, F32_TOL)
        hold(rec, "gat3 bwd datt_dst", dad, adr.grad, F32_TOL)
        hold(rec, "gat3 bwd dbias", db, br.grad, F32_TOL)


# =============================================================================================== f: ModalityDropout's draw
FALLBACK_ROWS = {(0.8, 257): 125, (0.5, 257): 29}      # tests/test_keyed_dropout_ref_cpu.py


@pytest.mark.parametrize("d", [4, 2052])
@pytest.mark.parametrize("B", [33, 257])
@pytest.mark.parametrize("p", [0.5, 0.8])
def test_modality_dropout_draw(p, B, d, state, rec):
    """keep[b][m] = the hash's keep of index 3 b + m in sub-stream 0; a sample left with nothing gets modality
    mmf_mix32(key ^ (0x51ed270b + b)) % 3 back; y = x * keep exactly (no rescale)"""
    site = 9
    keep, fell = K.modality_keep(STATE, site, B, K.mmf_drop_thresh(p))
    assert int(fell.sum()) == FALLBACK_ROWS.get((p, B), int(fell.sum())) and int(fell.sum()) >= 2, "the case must contain fallback rows"
    picks = np.bincount(keep[fell].argmax(axis=1), minlength=3)
    assert B < 257 or int(picks.min()) >= 6, picks                                # every fallback pick occurs
    xs = [f32(rnd(B, d, seed=10 + m) + 0.01) for m in range(3)]
    ys = [nan_like((B, d)) for _ in range(3)]
    kd = nan_like((B, 3))
    P3 = C.c_void_p * 3
    lib.check(lib.load().mmf_modality_dropout(P3(*[x.data_ptr() for x in xs]), P3(*[y.data_ptr() for y in ys]), kd.data_ptr(), B, d, p,
                                              state.data_ptr(), site, 1, lib.stream_ptr()))
    torch.cuda.synchronize()
    want = torch.from_numpy(keep.astype(np.float32))
    rec.mask("modality keep", kd == 1, keep)
    rec.mask("modality keep, fallback rows", kd.cpu()[torch.from_numpy(fell)] == 1, keep[fell])
    assert same(kd, want), "keep is not 0 / 1 as restated"
    for m in range(3):
        assert same(ys[m], xs[m].cpu() * want[:, m:m + 1]), f"modality {m}: y != x * keep"


# =============================================================================================== g: mmf_dropout past one grid pass
EW_THREADS, EW_GRID_CAP = 256, 2048                    # elementwise.hip / mmf_stream_grid


@pytest.mark.parametrize("is_f32", [1, 0], ids=["f32", "bf16"])
def test_dropout_second_grid_pass(is_f32, state, rec):
    """n = 2048 x 256 + 1: the capped grid covers 2048 x 256 elements per pass, so exactly one thread runs the grid-stride loop of
    dropout_kernel a second time — the smallest such n.  (The key twist at i >= 2^32 needs an 8 GiB tensor: out of reach of a test.)"""
    n, site = EW_THREADS * EW_GRID_CAP + 1, 3
    x = (rnd(n, seed=5).abs() + 0.5).to(F32 if is_f32 else BF16).to(DEV)
    y = nan_like((n + 8,), F32 if is_f32 else BF16)
    lib.check(lib.load().mmf_dropout(x.data_ptr(), y.data_ptr(), n, is_f32, P, state.data_ptr(), site, lib.stream_ptr()))
    torch.cuda.synchronize()
    keep = K.elementwise_keep(STATE, site, n, THRESH)
    assert all_nan(y[n:])
    rec.mask(f"mmf_dropout {'f32' if is_f32 else 'bf16'}", y[:n] != 0, keep)
    want = torch.from_numpy(x.float().cpu().numpy() * np.float32(INV)) * torch.from_numpy(keep)
    assert same(y[:n], want.to(y.dtype)), "kept values are not x * inv_keep"


# =============================================================================================== h: ops' site and state arithmetic
def _ops_sequence(rec, tag, state_value, first_site, mods, thresh):
    """ops.dropout, ffn_residual_group (generation 2), linear_group (the fused row linear), ops.dropout: four sites in call
    order; every forward mask and, after backward, every gradient's zero pattern against the restatement"""
    ffn, lin = mods
    M, d = 200, 64
    seen = []
    real = ops.gemm_group

    def spy(layout, probs, epilogue, **kw):
        seen.append((layout, epilogue, [q[2] for q in probs]))
        return real(layout, probs, epilogue, **kw)

    x1 = torch.ones(5000, device=DEV, requires_grad=True)
    y1 = ops.dropout(x1, P, True)
    xf = bf(operand((M, d), 1, True)).requires_grad_(True)
    ops.gemm_group = spy
    try:
        yf = ops.ffn_residual_group([(xf, ffn[0], ffn[1])], dropout_p=P)[0]
        assert lib.load().mmf_gemm_last_impl() == 2
        xl = bf(operand((16, 72), 2, True)).requires_grad_(True)
        yl, yl16 = ops.linear_group([(xl, ops.LinearSpec(ops.W(lin.weight), ops.W(lin.bias), False), None)], out_f32=True, dropout_p=P,
                                    dual=True)[0]
        x4 = torch.ones(4096, device=DEV, dtype=BF16, requires_grad=True)
        y4 = ops.dropout(x4, P, True)
        h = seen[0][2][0]                                                           # ffn1's output: dropout(relu(x W1^T + b1))
        assert seen[0][1] & EPI_RELU and h.shape == (M, 4 * d)
        nfwd = len(seen)
        torch.autograd.backward([y1.sum(), yf, yl, y4.sum()],
                                [None, bf(operand((M, d), 3, True)), f32(operand((16, 40), 4, True)), None])
        torch.cuda.synchronize()
        dh = next(c[0] for lay, e, c in seen[nfwd:] if lay == GEMM_NN and e & EPI_MASK_AUX)   # dH = (dY W2) * (h > 0) / (1 - p)
    finally:
        ops.gemm_group = real
    s = first_site
    k1, k2 = K.elementwise_keep(state_value, s, 5000, thresh), K.gemm_keep(state_value, s + 1, 0, M, 4 * d, thresh)
    k3, k4 = K.gemm_keep(state_value, s + 2, 0, 16, 40, thresh), K.elementwise_keep(state_value, s + 3, 4096, thresh)
    rec.mask(f"{tag} site {s} ops.dropout f32", y1 != 0, k1)
    rec.mask(f"{tag} site {s} ops.dropout f32 grad", x1.grad != 0, k1)
    rec.mask(f"{tag} site {s + 1} ffn hidden", h != 0, k2)
    rec.mask(f"{tag} site {s + 1} ffn hidden grad", dh != 0, k2)
    rec.mask(f"{tag} site {s + 2} row linear", yl != 0, k3)
    rec.mask(f"{tag} site {s + 2} row linear bf16 twin", yl16 != 0, k3)
    rec.mask(f"{tag} site {s + 2} row linear grad", xl.grad[:, :40] != 0, k3)         # W = [I | 0]: dx = dz in its first 40 columns
    assert bool((xl.grad[:, 40:] == 0).all())
    rec.mask(f"{tag} site {s + 3} ops.dropout bf16", y4 != 0, k4)
    rec.mask(f"{tag} site {s + 3} ops.dropout bf16 grad", x4.grad != 0, k4)


def test_ops_sites_and_state(rec):
    """state = (seed & 0x7FFFFFFF) << 20, + 1 per begin_training_forward; sites 1, 2, ... in call order; dropout_state swaps in another
    state with a numbering of its own and gives the outer one back"""
    from mmfusion import arena as arena_mod
    seed, d = 0x7654321, 64
    torch.manual_seed(0)
    ffn = torch.nn.Sequential(torch.nn.Linear(d, 4 * d), torch.nn.Linear(4 * d, d))
    lin = torch.nn.Linear(72, 40)
    with torch.no_grad():
        for q in ffn.parameters():
            q.copy_(q.abs() + 1e-3)
        lin.weight.copy_(torch.eye(40, 72))
        lin.bias.copy_(lin.bias.abs() + 1e-3)
    mods = torch.nn.ModuleList([ffn, lin]).cuda()
    arena_mod.ensure(mods).zero_grad()
    ops.seed_dropout(seed)
    ops.begin_training_forward()
    ops.begin_training_forward()
    outer = K.ops_state(seed, 2)
    assert outer >> 32 != 0 and int(ops.rng_state().item()) == outer
    _ops_sequence(rec, "outer", outer, 1, (mods[0], mods[1]), THRESH)
    other_value = STATE ^ 0x5555
    with ops.dropout_state(K.state_tensor(other_value, DEV)):
        _ops_sequence(rec, "dropout_state", other_value, 1, (mods[0], mods[1]), THRESH)
    assert int(ops.rng_state().item()) == outer                                     # the outer state did not move
    y5 = ops.dropout(torch.ones(5000, device=DEV), P, True)
    rec.mask("outer site 5 ops.dropout", y5 != 0, K.elementwise_keep(outer, 5, 5000, THRESH))
