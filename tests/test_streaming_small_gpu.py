"""GPU: the streaming kernels (csrc/elementwise.hip), the small fused branch kernels (csrc/small.hip) and the optimiser tail
(csrc/optim.hip), each called through the C ABI and compared with a float64 CPU restatement (tests/small_ref.py, plain torch
for the one-line operations) of the same operation on the same rounded operands.

Sizes come from the kernels' own constants, so that a case names the path it is for: 256 threads, grids capped at 2048
workgroups (512 per range in zero_ranges), 4 / 8 elements per vector, unrolled multi-stride loop + single-stride remainder
loop + scalar tail owned by workgroup 0, per-problem block ranges of the grouped launches, compile-time head counts, waves
of four similarities with clamped rows, per-thread key slots.

Conventions (those of tests/test_kernel_forms_gpu.py): operands from a seeded float64 generator; every output lives in an
`Out` buffer pre-filled with NaN (or with known non-zero values where the kernel accumulates: the expected value includes
them) between two guard regions that must come back bit-identical, as must every gap of a row-strided output; rel() is inf
on any non-finite output.  Tolerances: BF16_TOL / F32_TOL of that file; bit equality where the operation is exact; for long
f32 reductions an elementwise bound k 2^-24 sum|terms| computed by the reference, k = the additions on the longest chain of
the kernel's reduction order (written beside each case).  Every worst error / bound ratio is printed as a `PARITY` line
(profiles/streaming_small_parity.txt is those lines from an MI355X run)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import small_ref as R  # noqa: E402
from helpers import ptr3, within_bound  # noqa: E402
from mmfusion import lib  # noqa: E402
from test_kernel_forms_gpu import BF16_TOL, DEV, F32_TOL, NAN, bf, f32, host, rel, rnd  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E_SHAPE, E_UNSUPPORTED = -1, -5
THREADS, CAP = 256, 2048                 # EW_THREADS / SM_THREADS / OPT_THREADS; the grid cap of every streaming kernel
U24 = 2.0 ** -24                         # unit roundoff of f32
GUARD = 64                               # elements of each guard region (a multiple of 16 bytes for every dtype used)
SENTINEL = 777.0


def gamma(k):
    """the bound of k chained roundings: k u / (1 - k u)"""
    return k * U24 / (1.0 - k * U24)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


class Out:
    """n output elements at `off` elements past a 16-byte boundary, between two guard regions.  fill: NaN, a number, or a
    tensor of known values (an accumulating output)."""

    def __init__(self, n, dtype=F32, fill=NAN, off=0):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.full((n + off + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.v = self.buf[self.lo:self.lo + n]
        if isinstance(fill, torch.Tensor):
            self.v.copy_(fill.reshape(-1).to(dtype))
        else:
            self.v.fill_(fill)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.v.data_ptr()

    def intact(self, written=None):
        """the guards, and every element of the output the kernel does not own (written: bool mask over the n elements,
        on the CPU), are bit-identical to what they were"""
        a, b = bits(self.buf).cpu(), bits(self.before).cpu()
        keep = torch.ones(a.numel(), dtype=torch.bool)
        keep[self.lo:self.lo + self.n] = False if written is None else ~written.reshape(-1)
        return bool(torch.equal(a[keep], b[keep]))

    def untouched(self):
        return bool(torch.equal(bits(self.buf).cpu(), bits(self.before).cpu()))


@pytest.fixture
def rec(request):
    """rec(name, ratio): keeps the worst error / bound ratio per output name and prints them when the test ends"""
    worst = {}

    def put(name, ratio):
        worst[name] = max(worst.get(name, 0.0), float(ratio))
    yield put
    for name, r in worst.items():
        print(f"PARITY {request.node.nodeid.split('::')[-1]} {name} {r:.4f}")


def hold(rec, name, got, ref, tol, scale=None):
    """max |got - ref| <= tol x the reference's largest magnitude (or the given scale); a NaN left in got fails"""
    r = rel(got, ref) if scale is None else (float((host(got) - ref).abs().max()) / scale if bool(torch.isfinite(host(got)).all()) else math.inf)
    rec(name, r / tol)
    assert r < tol, (name, r, tol)


def bound_ok(rec, name, got, want, bound):
    w = [0.0, ""]
    try:
        within_bound(got, want, bound, name, w)
    finally:
        rec(name, w[0] if bool(torch.isfinite(host(got)).all()) else math.inf)


def same_bits(rec, name, got, want):
    ok = bool(torch.equal(bits(got).cpu(), bits(want).cpu()))
    rec(name, 0.0 if ok else math.inf)
    assert ok, (name, int((bits(got).cpu() != bits(want).cpu()).sum()), "elements differ")


def bf16_ulp(x):
    """the spacing of bf16 at |x| (float64 tensor); the smallest subnormal step at zero"""
    e = torch.frexp(x.abs().clamp_min(2.0 ** -126))[1]
    return torch.ldexp(torch.ones_like(x), e - 8)


def refused(rc, code, *outs):
    L = lib.load()
    assert rc == code, (rc, L.mmf_last_error().decode())
    assert L.mmf_last_error(), "a refusal names its reason"
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


def run(rc):
    lib.check(rc)


def S():
    return lib.stream_ptr()


# =============================================================================================== elementwise.hip: casts
N_CAP = 16 * THREADS * CAP                                   # ew_grid(n >> 4) reaches 2048: one unrolled iteration per thread
CAST_NS = [1, 3, 4, 5, 1023, 771000, N_CAP, N_CAP + 4, N_CAP + 2 * 4 * THREADS * CAP + 3]
TIE_DOWN, TIE_UP = 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8      # halfway between two bf16 values: to even
F32_MAX = float(np.finfo(np.float32).max)                           # rounds to inf in bf16
SPECIALS = [0.0, -0.0, math.inf, -math.inf, 1e-45, -1e-45, 2.0 ** -130, -(2.0 ** -133), 1e-40, TIE_DOWN, -TIE_DOWN, TIE_UP,
            -TIE_UP, F32_MAX, -F32_MAX, 2.0 ** -126, 3.0e38, NAN]


def check_f32_to_bf16(rec, name, got, x_cpu):
    """bit-identical to torch's round-to-nearest-even wherever x is not NaN; NaN stays NaN (any payload)"""
    want = x_cpu.to(BF16)
    nan = torch.isnan(x_cpu)
    g = got.cpu()
    assert bool(torch.isnan(g[nan]).all()), name
    same_bits(rec, name, g[~nan], want[~nan])


@pytest.mark.parametrize("n", CAST_NS)
def test_cast_f32_to_bf16_paths(n, rec):
    """n = 1, 3: tail only; 4: one vector; 5: vector + tail; 771000: uncapped grid, unrolled for some threads only;
    16 x 256 x 2048: capped grid, exactly one unrolled iteration per thread; + 4: one remainder vector;
    + 2 x 4 x 256 x 2048 + 3: unrolled iteration, two remainder iterations and a 3-element tail in one launch"""
    x = rnd(n, seed=n % 1000).float()
    k = min(n, len(SPECIALS))
    x[:k] = torch.tensor(SPECIALS[:k], dtype=F32)                 # body (or the tail when n < 4)
    if n >= 8:
        x[-3:] = torch.tensor([TIE_UP, -1e-40, F32_MAX])          # the last elements: the tail when n % 4 != 0
    o, xd = Out(n, BF16), x.to(DEV)
    run(lib.load().mmf_cast_f32_to_bf16(xd.data_ptr(), o.ptr, n, S()))
    torch.cuda.synchronize()
    check_f32_to_bf16(rec, "bf16", o.v, x)
    assert o.intact()


def test_cast_f32_to_bf16_special_values_in_body_and_tail(rec):
    """n = 7: elements 0..3 go through the vector body (pack_bf16x2), 4..6 through workgroup 0's tail
    (f32_to_bf16_bits); every special value is placed in both.  Body, tail and torch must agree bit for bit."""
    L = lib.load()
    for i in range(0, len(SPECIALS), 3):
        chunk = (SPECIALS[i:i + 3] + [1.0, 1.0])[:3]
        x = torch.tensor(chunk + [2.5] + chunk, dtype=F32)
        o, xd = Out(7, BF16), x.to(DEV)
        run(L.mmf_cast_f32_to_bf16(xd.data_ptr(), o.ptr, 7, S()))
        torch.cuda.synchronize()
        check_f32_to_bf16(rec, "bf16", o.v, x)
        g = bits(o.v).cpu()
        nan = torch.isnan(x[:3])
        assert bool(torch.equal(g[:3][~nan], g[4:][~nan])), ("body and tail disagree", chunk, g.tolist())
        assert o.intact()


@pytest.mark.parametrize("n", CAST_NS)
def test_cast_bf16_to_f32_paths(n, rec):
    """widening is exact and the scale is one IEEE multiplication: bit-identical to the same product in f32 on the CPU"""
    L = lib.load()
    x = rnd(n, seed=1 + n % 1000).to(BF16)
    sp = torch.tensor([0.0, -0.0, math.inf, -math.inf, 2.0 ** -133, -(2.0 ** -130), 3.0e38, 2.0 ** -126], dtype=F32).to(BF16)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n >= 8:
        x[-3:] = sp[4:7]
    xd = x.to(DEV)
    for scale in ((None, 0.125, 3.0) if n <= 771000 else (3.0,)):
        o = Out(n, F32)
        if scale is None:
            run(L.mmf_cast_bf16_to_f32(xd.data_ptr(), o.ptr, n, S()))
        else:
            run(L.mmf_cast_bf16_to_f32_scaled(xd.data_ptr(), o.ptr, n, scale, S()))
        torch.cuda.synchronize()
        same_bits(rec, "f32", o.v, x.float() * (1.0 if scale is None else scale))
        assert o.intact()


@pytest.mark.parametrize("rows", [1, 1000])
@pytest.mark.parametrize("cols", [4, 12, 772])
def test_cast_f32_to_bf16_2d_strided_source(rows, cols, rec):
    """ld_src > cols with NaN beyond the columns; the destination is 8-byte, not 16-byte, aligned"""
    for ld in (cols + 4, cols + 28):
        src = torch.full((rows, ld), NAN, dtype=F32)
        x = rnd(rows, cols, seed=cols + rows).float()
        x[0, :4] = torch.tensor([TIE_DOWN, TIE_UP, -0.0, F32_MAX])
        src[:, :cols] = x
        o, srcd = Out(rows * cols, BF16, off=4), src.to(DEV)
        assert o.ptr % 16 == 8
        run(lib.load().mmf_cast_f32_to_bf16_2d(srcd.data_ptr(), o.ptr, rows, cols, ld, S()))
        torch.cuda.synchronize()
        same_bits(rec, "bf16", o.v, x.to(BF16).reshape(-1))
        assert o.intact()


# =============================================================================================== add3 / addn
N_VEC8_CAP = 8 * THREADS * CAP                               # ew_grid(n >> 3) reaches its cap


def sum_check(rec, name, o, xs, out_f32=False):
    """f32 sum of the bf16 operands (len(xs) - 1 additions), then one rounding: the f32 form to F32_TOL, the bf16 form
    within one bf16 ulp of the float64 sum beyond the f32 sum's own error bound"""
    terms = torch.stack([host(x) for x in xs])
    ref = terms.sum(0)
    if out_f32:
        hold(rec, name, o.v, ref, F32_TOL)
    else:
        e32 = gamma(len(xs) - 1) * terms.abs().sum(0)
        bound_ok(rec, name, o.v, ref, bf16_ulp(ref.abs() + e32) + e32)
    assert o.intact()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 999, N_VEC8_CAP + 8 * THREADS * 3 + 5])
def test_add3_bf16_with_and_without_c(n, rec):
    L = lib.load()
    a, b, c = (bf(rnd(n, seed=s)) for s in (2, 3, 4))
    for ops_ in ((a, b, c), (a, b)):
        o = Out(n, BF16)
        run(L.mmf_add3_bf16(a.data_ptr(), b.data_ptr(), c.data_ptr() if len(ops_) == 3 else None, o.ptr, n, S()))
        torch.cuda.synchronize()
        sum_check(rec, f"y{len(ops_)}", o, ops_)


def test_add3_grouped_unequal_problems(rec):
    """MMF_ADD3_MAX problems in one launch: 1, 7 (tail only), 8, 9, one above the per-problem cap of 2048 blocks (its
    grid-stride loop iterates), and three ordinary ones"""
    ns = [1, 7, 8, 9, N_VEC8_CAP + 8 * 300 + 3, 1000, 17, 4096]
    assert len(ns) == lib.ADD3_MAX
    ins = [[bf(rnd(n, seed=10 * i + j)) for j in range(3)] for i, n in enumerate(ns)]
    outs = [Out(n, BF16) for n in ns]
    probs = (lib.Add3Problem * len(ns))(*[lib.Add3Problem(x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), o.ptr, n)
                                          for x, o, n in zip(ins, outs, ns)])
    run(lib.load().mmf_add3_grouped(probs, len(ns), S()))
    torch.cuda.synchronize()
    for i, (x, o) in enumerate(zip(ins, outs)):
        sum_check(rec, f"y[{i}]", o, x)


@pytest.mark.parametrize("k", range(2, lib.ADDN_MAX + 1))
def test_addn_bf16_every_count(k, rec):
    L = lib.load()
    for numel in ([8 * THREADS * 5 + 3] + ([N_VEC8_CAP + 8 * THREADS + 3] if k == 3 else [])):
        xs = [bf(rnd(numel, seed=20 * k + j)) for j in range(k)]
        ptrs = (C.c_void_p * k)(*[x.data_ptr() for x in xs])
        for out_f32 in (0, 1):
            o = Out(numel, F32 if out_f32 else BF16)
            run(L.mmf_addn_bf16(ptrs, k, o.ptr, numel, out_f32, S()))
            torch.cuda.synchronize()
            sum_check(rec, "f32" if out_f32 else "bf16", o, xs, bool(out_f32))


def test_addn_grouped_different_counts(rec):
    ks, ns = [2, 8, 3, 5], [1, 4099, 8, N_VEC8_CAP + 8 * 77 + 7]
    assert len(ks) == lib.ADDN_GROUP_MAX
    ins = [[bf(rnd(n, seed=50 * i + j)) for j in range(k)] for i, (k, n) in enumerate(zip(ks, ns))]
    outs = [Out(n, BF16) for n in ns]
    probs = (lib.AddNProblem * 4)()
    for i, (x, o) in enumerate(zip(ins, outs)):
        for j, t in enumerate(x):
            probs[i].x[j] = t.data_ptr()
        probs[i].y, probs[i].numel, probs[i].n = o.ptr, ns[i], ks[i]
    run(lib.load().mmf_addn_grouped(probs, 4, S()))
    torch.cuda.synchronize()
    for i, (x, o) in enumerate(zip(ins, outs)):
        sum_check(rec, f"y[{i}]", o, x)


# =============================================================================================== relu backward
EDGE_Y16 = [0x0000, 0x8000, 0x0001, 0x8001, 0x3f80, 0xbf80, 0x0080, 0x7f7f]    # +0 -0 +-smallest subnormal +-1 min normal max


def from_bits16(v):
    return torch.tensor(v, dtype=torch.int32).to(torch.int16).view(BF16) if not isinstance(v, torch.Tensor) else v.view(BF16)


def relu_operands(n, seed):
    """dy, y as bf16 CPU tensors; y carries +0, -0, the smallest positive subnormal and negatives at both ends.
    NaN in y is left out on purpose: the bit-pattern test of relu_bwd_kernel passes a positive-signed NaN and the float
    compare of relu_bwd_mixed_kernel does not, and neither is asserted here."""
    dy, y = rnd(n, seed=seed).to(BF16), rnd(n, seed=seed + 1).to(BF16)
    e = from_bits16([b - 65536 if b >= 32768 else b for b in EDGE_Y16])
    k = min(n, e.numel())
    y[:k] = e[:k]
    if n >= 16:
        y[-8:] = e.flip(0)
    if n > 2:
        dy[1] = -0.0
    return dy, y


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 999, N_VEC8_CAP + 8 * THREADS + 5])
def test_relu_bwd_bf16_aligned_and_scalar_branch(n, off, rec):
    """dx = where(y > 0, dy, +0) bit for bit.  off = 1: all three pointers one element past a 16-byte boundary, the
    scalar-only branch; the large n is above the grid cap (the vector loop, or the scalar loop, iterates)"""
    dy, y = relu_operands(n, seed=7 + n % 100)
    dyd, yd = Out(n, BF16, fill=dy, off=off), Out(n, BF16, fill=y, off=off)
    o = Out(n, BF16, off=off)
    assert (o.ptr % 16 == 0) == (off == 0)
    run(lib.load().mmf_relu_bwd_bf16(dyd.ptr, yd.ptr, o.ptr, n, S()))
    torch.cuda.synchronize()
    same_bits(rec, "dx", o.v, torch.where(y.float() > 0, dy, torch.zeros_like(dy)))
    assert o.intact() and dyd.untouched() and yd.untouched()


@pytest.mark.parametrize("y_f32", [0, 1])
@pytest.mark.parametrize("dy_f32", [0, 1])
def test_relu_bwd_mixed_all_type_combinations(dy_f32, y_f32, rec):
    L = lib.load()
    for n in (1, 999, THREADS * CAP + 300):
        dy, y = relu_operands(n, seed=3 + n % 100)
        dyh = rnd(n, seed=9).float() if dy_f32 else dy
        yh = y.float() if y_f32 else y
        if y_f32 and n > 2:
            yh[2] = 1e-45                                         # the smallest positive f32
        o, dyd, yd = Out(n, BF16), dyh.to(DEV), yh.to(DEV)
        run(L.mmf_relu_bwd_mixed(dyd.data_ptr(), dy_f32, yd.data_ptr(), y_f32, o.ptr, n, S()))
        torch.cuda.synchronize()
        want = torch.where(yh.float() > 0, dyh.to(BF16), torch.zeros(n, dtype=BF16))
        same_bits(rec, "dx", o.v, want)
        assert o.intact()


# =============================================================================================== mean pooling
POOL_T = [1, 15, 16, 17, 63, 64, 65, 500]
POOL_D = [8, 120, 128, 136, 768]


@pytest.mark.parametrize("T", POOL_T)
def test_meanpool_fwd_bwd(T, rec):
    """T < 16: row groups with no rows; d = 120 / 136: a partly filled 128-column block; ldy, lddy wider than d with NaN in
    the gap of the input and the gap of the output left as it was"""
    L, B = lib.load(), 3
    for d in POOL_D:
        ld = d + (8 if d != 128 else 24)
        x = bf(rnd(B, T, d, seed=T + d))
        col = (torch.arange(ld) < d).repeat(B)
        o = Out(B * ld, BF16)
        run(L.mmf_meanpool_fwd(x.data_ptr(), o.ptr, B, T, d, ld, S()))
        dy = torch.full((B, ld), NAN, dtype=BF16)
        dy[:, :d] = rnd(B, d, seed=T + d + 1).to(BF16)
        dx, dyd = Out(B * T * d, BF16), dy.to(DEV)
        run(L.mmf_meanpool_bwd(dyd.data_ptr(), dx.ptr, B, T, d, ld, S()))
        torch.cuda.synchronize()
        hold(rec, "y", o.v.view(B, ld)[:, :d], host(x).mean(1), BF16_TOL)
        hold(rec, "dx", dx.v.view(B, T, d), (host(dy[:, :d]) / T).unsqueeze(1).expand(B, T, d), BF16_TOL)
        assert o.intact(col) and dx.intact()


@pytest.mark.parametrize("Ts", [(1, 63, 65, 500), (15, 16, 17, 64), (64,), (500, 1)], ids=str)
def test_meanpool_cat_fwd_bwd(Ts, rec):
    """the grouped form (up to MMF_POOL_MAX problems, 64 row groups): T below, at and above 64 mixed in one launch"""
    L, B, n = lib.load(), 3, len(Ts)
    assert n <= lib.POOL_MAX
    for d in POOL_D:
        ld = n * d + 8
        xs = [bf(rnd(B, T, d, seed=T + d + i)) for i, T in enumerate(Ts)]
        xp = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        tp = (C.c_int * n)(*Ts)
        o = Out(B * ld, BF16)
        run(L.mmf_meanpool_cat_fwd(xp, tp, n, o.ptr, B, d, ld, S()))
        dy = torch.full((B, ld), NAN, dtype=BF16)
        dy[:, :n * d] = rnd(B, n * d, seed=d + 5).to(BF16)
        dxs = [Out(B * T * d, BF16) for T in Ts]
        dp, dyd = (C.c_void_p * n)(*[t.ptr for t in dxs]), dy.to(DEV)
        run(L.mmf_meanpool_cat_bwd(dyd.data_ptr(), dp, tp, n, B, d, ld, S()))
        torch.cuda.synchronize()
        hold(rec, "y", o.v.view(B, ld)[:, :n * d], torch.cat([host(x).mean(1) for x in xs], 1), BF16_TOL)
        assert o.intact((torch.arange(ld) < n * d).repeat(B))
        for i, T in enumerate(Ts):
            want = (host(dy[:, i * d:(i + 1) * d]) / T).unsqueeze(1).expand(B, T, d)
            hold(rec, f"dx[{i}]", dxs[i].v.view(B, T, d), want, BF16_TOL)
            assert dxs[i].intact()


# =============================================================================================== column sums
COLSUM_SHAPES = [(1, 8, 8), (3, 520, 528), (64, 512, 512), (65, 1032, 2048), (4097, 264, 264)]


def colsum_case(M, N, ldx, seed):
    x = bf(rnd(M, ldx, seed=seed))
    out0 = rnd(N, seed=seed + 1).float()
    return x, out0, Out(N, F32, fill=out0, off=1)                # 4-byte, not 16-byte, aligned


def colsum_check(rec, name, x, out0, o, M, N):
    """k: 16 additions per thread (64 rows over 4 waves), 3 across the waves, one atomic per 64-row workgroup, the value
    already in `out` among the terms"""
    k = 16 + 3 + (M + 63) // 64
    terms = host(x)[:, :N]
    bound_ok(rec, name, o.v, terms.sum(0) + out0.double(), gamma(k) * (terms.abs().sum(0) + out0.double().abs()))
    assert o.intact()


@pytest.mark.parametrize("M,N,ldx", COLSUM_SHAPES)
def test_colsum_bf16_shapes(M, N, ldx, rec):
    """M < 4: waves without a row; N > 512: several column chunks, the last one partial; ldx > N; M = 4097: 65 adders"""
    x, out0, o = colsum_case(M, N, ldx, seed=M + N)
    assert o.ptr % 16 == 4
    run(lib.load().mmf_colsum_bf16(x.data_ptr(), o.ptr, M, N, ldx, S()))
    torch.cuda.synchronize()
    colsum_check(rec, "out", x, out0, o, M, N)


def test_colsum_grouped_mixed_problems(rec):
    shapes = [COLSUM_SHAPES[i % 4] for i in range(lib.COLSUM_MAX_PROBLEMS)]
    shapes[5], shapes[22] = COLSUM_SHAPES[4], (130, 8, 16)
    cases = [colsum_case(M, N, ldx, seed=100 + 3 * i) for i, (M, N, ldx) in enumerate(shapes)]
    probs = (lib.ColsumProblem * len(shapes))(*[lib.ColsumProblem(c[0].data_ptr(), c[2].ptr, M, N, ldx)
                                                for c, (M, N, ldx) in zip(cases, shapes)])
    run(lib.load().mmf_colsum_grouped(probs, len(shapes), S()))
    torch.cuda.synchronize()
    for i, ((x, out0, o), (M, N, _)) in enumerate(zip(cases, shapes)):
        colsum_check(rec, f"out[{i}]", x, out0, o, M, N)


# =============================================================================================== zero_ranges
ZR_BIG = (3, 3 + 4 * THREADS * 512 * 2 + 2)                  # above the 512-block cap of a range: two iterations + both edges


def zero_ranges_case(ranges):
    hi = max(e for _, e in ranges)
    o = Out(hi + 37, F32, fill=1.0)
    n = len(ranges)
    st, en = (C.c_int64 * n)(*[s for s, _ in ranges]), (C.c_int64 * n)(*[e for _, e in ranges])
    run(lib.load().mmf_zero_ranges_f32(o.ptr, st, en, n, S()))
    torch.cuda.synchronize()
    want = torch.ones(hi + 37)
    for s, e in ranges:
        want[s:e] = 0
    return o, want


@pytest.mark.parametrize("rng", [(5, 6), (5, 8), (5, 11), (4, 8), (7, 7), (0, 4), (1, 3), ZR_BIG], ids=str)
def test_zero_ranges_single_range_edges(rng, rec):
    """shorter than 4 floats, inside one 16-byte group, leading / trailing scalar edges, empty, and above the block cap:
    zeros inside, ones (bit for bit) everywhere else"""
    o, want = zero_ranges_case([rng])
    same_bits(rec, "buffer", o.v, want)
    assert o.intact(torch.zeros(o.n, dtype=torch.bool) | (want == 0))


def test_zero_ranges_max_ranges_in_one_call(rec):
    lens = [0, 1, 2, 3, 4, 5, 9, 33, 64, 65, 1023, 4 * THREADS + 1]
    ranges, at = [], 1
    for r in range(lib.ZERO_MAX_RANGES):
        n = lens[r % len(lens)] if r != 17 else 4 * THREADS * 512 + 4 * THREADS + 3
        ranges.append((at, at + n))
        at += n + 1 + r % 5                                      # 1..5 ones between neighbours
    o, want = zero_ranges_case(ranges)
    same_bits(rec, "buffer", o.v, want)
    assert o.intact(want == 0)


# =============================================================================================== dropout
def test_dropout_f32_and_bf16_draw_the_same_mask(rec):
    """same (state, site) => same mask in both forms; another site => another mask; above 2048 x 256 elements the loop
    iterates; kept fraction within 4 sigma of 1 - p; kept values = x * scale, scale from the threshold as the host
    computes it (f32 arithmetic).  The statistics of the generator are tests/test_dropout_gpu.py's."""
    L, n, p = lib.load(), THREADS * CAP + 1000, 0.3
    x = (rnd(n, seed=5).abs() + 0.5).to(BF16)                      # never zero: a zero output is a dropped element
    x16, x32 = x.to(DEV), x.float().to(DEV)
    state = torch.tensor([(1234 << 20) + 7], dtype=torch.int64, device=DEV)
    thresh = min(int(float(np.float32(p)) * 4294967296.0), 4294967295)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(thresh) * np.float32(1.0 / 4294967296.0))
    res = {}
    for site in (3, 4):
        for is_f32 in (1, 0):
            o = Out(n, F32 if is_f32 else BF16)
            run(L.mmf_dropout((x32 if is_f32 else x16).data_ptr(), o.ptr, n, is_f32, p, state.data_ptr(), site, S()))
            torch.cuda.synchronize()
            assert o.intact()
            res[site, is_f32] = o.v.cpu()
    keep = res[3, 1] != 0
    assert bool(torch.equal(keep, res[3, 0] != 0)) and bool(torch.equal(res[4, 1] != 0, res[4, 0] != 0))
    assert not bool(torch.equal(keep, res[4, 1] != 0))
    sigma = math.sqrt(p * (1 - p) / n)
    for site in (3, 4):
        frac = float((res[site, 1] != 0).double().mean())
        rec(f"kept fraction site {site}", abs(frac - (1 - p)) / (4 * sigma))
        assert abs(frac - (1 - p)) <= 4 * sigma, frac
    want32 = torch.from_numpy(x.float().numpy() * scale)
    same_bits(rec, "f32 kept values", res[3, 1][keep], want32[keep])
    same_bits(rec, "bf16 kept values", res[3, 0][keep], want32.to(BF16)[keep])


# =============================================================================================== small.hip: GAT3
def gat_params(B, H, C, relu):
    return lib.Gat3Params(B, H, C, int(relu), 0.2, 0.0, None, 0)


@pytest.mark.parametrize("C_", [8, 136, 768, 1032])
@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_gat3_fwd_bwd_every_head_count(H, C_, rec):
    """C = 8: most threads idle; 136: the old single shape; 768, 1032: two and three columns per thread.  B = 1 and 5,
    ReLU on and off, gradient through y only / the pooled output only / both.  The backward's reference reads what the
    kernel reads: its saved alpha and dots, and the ReLU mask of its own bf16 y (a unit within bf16 rounding of zero may be
    on in one and off in the other; the kernel's mask is the one its backward is consistent with)."""
    L = lib.load()
    for B in (1, 5):
        h = f32(rnd(B, 3, H, C_, seed=H + C_ + B))
        sc = 2 * C_ ** -0.5                                     # attention logits of a few units at every C
        a_s, a_d, bias = f32(rnd(H, C_, seed=1, scale=sc)), f32(rnd(H, C_, seed=2, scale=sc)), f32(rnd(C_, seed=3, scale=0.3))
        for relu in (True, False):
            prm = gat_params(B, H, C_, relu)
            y, pooled = Out(B * 3 * C_, BF16), Out(B * C_, BF16)
            alpha, sd = Out(B * 9 * H), Out(B * 6 * H)
            run(L.mmf_gat3_dense_fwd(h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), y.ptr, pooled.ptr, alpha.ptr,
                                     sd.ptr, C.byref(prm), S()))
            y2, al2, sd2 = Out(B * 3 * C_, BF16), Out(B * 9 * H), Out(B * 6 * H)     # without the pooled output
            run(L.mmf_gat3_dense_fwd(h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), y2.ptr, None, al2.ptr, sd2.ptr,
                                     C.byref(prm), S()))
            torch.cuda.synchronize()
            ro, rp, ra, rs = R.gat3_fwd(host(h), host(a_s), host(a_d), host(bias), 0.2, relu)
            hold(rec, "y", y.v.view(B, 3, C_), ro, BF16_TOL)
            hold(rec, "pooled", pooled.v.view(B, C_), rp, BF16_TOL)
            hold(rec, "alpha", alpha.v.view(B, 3, 3, H), ra, F32_TOL)
            hold(rec, "sdots", sd.v.view(B, 2, 3, H), rs, F32_TOL)
            same_bits(rec, "y (no pool)", y2.v, y.v)
            assert all(o.intact() for o in (y, pooled, alpha, sd, y2, al2, sd2))
            live = (host(y.v).view(B, 3, C_) > 0).double() if relu else torch.ones(B, 3, C_, dtype=F64)
            dy, dp = bf(rnd(B, 3, C_, seed=4)), bf(rnd(B, C_, seed=5))
            for gy, gp, tag in ((dy, None, "dy"), (None, dp, "dpool"), (dy, dp, "both")):
                pre = [rnd(H, C_, seed=6).float(), rnd(H, C_, seed=7).float(), rnd(C_, seed=8).float()]
                dh, das, dad, db = Out(B * 3 * H * C_), Out(H * C_, fill=pre[0]), Out(H * C_, fill=pre[1]), Out(C_, fill=pre[2])
                run(L.mmf_gat3_dense_bwd(h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), y.ptr, alpha.ptr, sd.ptr,
                                         gy.data_ptr() if gy is not None else None, gp.data_ptr() if gp is not None else None,
                                         dh.ptr, das.ptr, dad.ptr, db.ptr, C.byref(prm), S()))
                torch.cuda.synchronize()
                want = R.gat3_bwd(host(h), host(a_s), host(a_d), host(alpha.v).view(B, 3, 3, H), host(sd.v).view(B, 2, 3, H), live,
                                  None if gy is None else host(gy), None if gp is None else host(gp), 0.2)
                hold(rec, f"dh/{tag}", dh.v.view(B, 3, H, C_), want[0], F32_TOL)
                hold(rec, f"datt_src/{tag}", das.v.view(H, C_), want[1] + pre[0].double(), F32_TOL)
                hold(rec, f"datt_dst/{tag}", dad.v.view(H, C_), want[2] + pre[1].double(), F32_TOL)
                hold(rec, f"dbias/{tag}", db.v, want[3] + pre[2].double(), F32_TOL)
                assert all(o.intact() for o in (dh, das, dad, db))


def test_gat3_refuses_three_heads():
    L, B, C_ = lib.load(), 2, 16
    h, a = f32(rnd(B, 3, 3, C_)), f32(rnd(3, C_))
    bias = f32(rnd(C_))
    y, pooled, alpha, sd = Out(B * 3 * C_, BF16), Out(B * C_, BF16), Out(B * 27), Out(B * 18)
    prm = gat_params(B, 3, C_, True)
    rc = L.mmf_gat3_dense_fwd(h.data_ptr(), a.data_ptr(), a.data_ptr(), bias.data_ptr(), y.ptr, pooled.ptr, alpha.ptr, sd.ptr,
                              C.byref(prm), S())
    refused(rc, E_UNSUPPORTED, y, pooled, alpha, sd)
    dh, da, db = Out(B * 9 * C_), Out(3 * C_), Out(C_)
    rc = L.mmf_gat3_dense_bwd(h.data_ptr(), a.data_ptr(), a.data_ptr(), y.ptr, alpha.ptr, sd.ptr, y.ptr, None, dh.ptr, da.ptr, da.ptr,
                              db.ptr, C.byref(prm), S())
    refused(rc, E_UNSUPPORTED, dh, da, db)


# =============================================================================================== small.hip: InfoNCE
NCE_SHAPES = [(1, 4), (2, 252), (3, 256), (5, 260), (16, 384), (17, 1024), (33, 4), (63, 260), (64, 1024), (64, 384)]


def nce_forward(zs, B, D, temp, with_loss=True):
    L = lib.load()
    ns, inv = [Out(B * D) for _ in range(3)], Out(3 * B)
    losses, lse = Out(3), Out(6 * B)
    run(L.mmf_infonce_fwd(ptr3(zs), ptr3([o.ptr for o in ns]), inv.ptr, losses.ptr if with_loss else None,
                          lse.ptr if with_loss else None, B, D, temp, S()))
    torch.cuda.synchronize()
    return ns, inv, losses, lse


def nce_backward(ns, inv, lse, dn, dloss, B, D, temp):
    dz = [Out(B * D) for _ in range(3)]
    run(lib.load().mmf_infonce_bwd(ptr3([o.ptr for o in ns]), inv.ptr, lse.ptr if lse is not None else None,
                                   ptr3(dn if dn is not None else [None] * 3), ptr3(dloss), ptr3([o.ptr for o in dz]), B, D, temp, S()))
    torch.cuda.synchronize()
    return dz


@pytest.mark.parametrize("B,D", NCE_SHAPES)
def test_infonce_fwd_bwd_shapes(B, D, rec):
    """B not a multiple of 4 (the clamped rows of a wave's four similarities), B = 1, B > 16 (more rows than waves),
    B = 64 (NCE_MAXB); D < 256 (most lanes idle), D not a multiple of 256.  Temperature 0.07 and 1.0; all three losses, one
    and two pairs without a loss gradient, no gradient of the normalised outputs, normalise-only.
    Every output is held to F32_TOL of its own largest magnitude, with two exceptions, both at B = 1 only, where the
    exact result is a complete cancellation and has no magnitude of its own:
      * the loss is lse - sim = 0: held to F32_TOL of |sim|, the operand it is the difference of;
      * the loss part of dz is dsim n_other / ||z|| with dsim = dl (p_row + p_col - 2) = 0, dl = |dloss| / (2 B T): a
        difference of numbers of size 2 dl, so the error scales with 2 dl |n|max / ||z||min even though the sum is zero
        (the forward and the backward each compute the similarity, and their last bits need not agree).  That scale,
        capped so that the absolute bound stays at or below the 1e-4 of test_normalize_infonce_matches_torch, replaces
        the gradient's own magnitude where it is larger.  Measured on MI355X at (1, 4), T = 0.07: the error is 30.7 x
        F32_TOL of the gradient's own magnitude (the rounding of one similarity of size 14 against |dn| = 0.01), and
        0.022 of this bound (worst / bound; 0.0001 at T = 1.0)."""
    for temp in (0.07, 1.0):
        zs = [f32(rnd(B, D, seed=B + D + m)) for m in range(3)]
        zh = [host(z) for z in zs]
        ns, inv, losses, lse = nce_forward(zs, B, D, temp)
        rn, rinv, rl, rlse, sims = R.infonce_fwd(zh, temp)
        dl1 = 0.5 / (B * temp) * max(float(t.abs().max()) for t in rn) * float(rinv.max())      # used at B = 1 only
        for m in range(3):
            hold(rec, "n", ns[m].v.view(B, D), rn[m], F32_TOL)
        hold(rec, "inv_norm", inv.v.view(3, B), rinv, F32_TOL)
        hold(rec, f"losses/T={temp}", losses.v, rl, F32_TOL, scale=max(float(s.abs().max()) for s in sims) if B == 1 else None)
        hold(rec, f"lse/T={temp}", lse.v.view(3, 2, B), rlse, F32_TOL)
        assert all(o.intact() for o in (*ns, inv, losses, lse))
        n0, i0, l0, s0 = nce_forward(zs, B, D, temp, with_loss=False)        # normalise-only: no loss, no lse written
        for m in range(3):
            same_bits(rec, "n (normalise-only)", n0[m].v, ns[m].v)
        assert l0.untouched() and s0.untouched() and i0.intact()
        dn = [f32(rnd(B, D, seed=40 + m, scale=0.01)) for m in range(3)]
        w = f32(torch.tensor([0.3, 1.1, 0.7], dtype=F64))
        wp = [w.data_ptr() + 4 * p for p in range(3)]
        # the reference differentiates the float64 loss of the kernel's own operand z; the kernel's saved n / inv_norm /
        # lse are f32 roundings of the same quantities
        for tag, gn, gl in (("all", dn, (0, 1, 2)), ("dn null", None, (0, 1, 2)), ("one null loss", dn, (0, 2)),
                            ("two null losses", dn, (1,)), ("normalise-only", dn, ())):
            dz = nce_backward(ns, inv, lse if gl else None, gn, [wp[p] if p in gl else None for p in range(3)], B, D, temp)
            want = R.infonce_bwd(zh, temp, None if gn is None else [host(g) for g in gn],
                                 [float(host(w)[p]) if p in gl else None for p in range(3)])
            for m in range(3):
                sc = None                                      # F32_TOL of the gradient's own largest magnitude
                if B == 1 and gl:
                    sc = min(max(float(want[m].abs().max()), 2 * dl1 * max(abs(float(host(w)[p])) for p in gl)), 1e-4 / F32_TOL)
                hold(rec, f"dz/{tag}/T={temp}" + ("/B=1" if sc else ""), dz[m].v.view(B, D), want[m], F32_TOL, scale=sc)
                assert dz[m].intact()


def test_infonce_zero_row_is_clamped(rec):
    """A row of zeros in z: max(norm, 1e-12) keeps n, the losses and every gradient finite, and the clamped row's own
    gradient is zero.  Everything else is held to the float64 reference, whose gradient for that one row is autograd's
    dn / 1e-12 (tests/test_small_ref_cpu.py::test_infonce_zero_row_is_what_autograd_gives): the kernel deliberately does not
    follow it there (csrc/small.hip nce_clamped)."""
    B, D, temp = 5, 260, 0.07
    z = [rnd(B, D, seed=70 + m) for m in range(3)]
    z[1][2] = 0
    zs = [f32(t) for t in z]
    zh = [host(t) for t in zs]
    ns, inv, losses, lse = nce_forward(zs, B, D, temp)
    dn = [f32(rnd(B, D, seed=80 + m, scale=0.01)) for m in range(3)]
    w = f32(torch.tensor([0.3, 1.1, 0.7], dtype=F64))
    dz = nce_backward(ns, inv, lse, dn, [w.data_ptr() + 4 * p for p in range(3)], B, D, temp)
    rn, rinv, rl, rlse, sims = R.infonce_fwd(zh, temp)
    want = R.infonce_bwd(zh, temp, [host(g) for g in dn], [float(x) for x in host(w)])
    for o in (*ns, inv, losses, lse, *dz):
        assert bool(torch.isfinite(o.v).all()) and o.intact()
    assert float(ns[1].v.view(B, D)[2].abs().max()) == 0.0
    hold(rec, "losses", losses.v, rl, F32_TOL)
    rows = torch.ones(B, dtype=torch.bool)
    rows[2] = False
    sc = max(float(want[0].abs().max()), float(want[1][rows].abs().max()), float(want[2].abs().max()))
    for m in range(3):
        keep = rows if m == 1 else torch.ones(B, dtype=torch.bool)
        hold(rec, "dz (other rows)", dz[m].v.view(B, D)[keep.to(DEV)], want[m][keep], F32_TOL, scale=sc)
    got = host(dz[1].v.view(B, D)[2])
    rec("dz (zero row)", 0.0 if float(got.abs().max()) == 0.0 else math.inf)
    assert float(got.abs().max()) == 0.0
    dz = nce_backward(ns, inv, None, dn, [None] * 3, B, D, temp)          # through the normalised outputs alone
    want = R.infonce_bwd(zh, temp, [host(g) for g in dn], None)
    for m in range(3):
        keep = rows if m == 1 else torch.ones(B, dtype=torch.bool)
        hold(rec, "dz (other rows, dn only)", dz[m].v.view(B, D)[keep.to(DEV)], want[m][keep], F32_TOL)
    assert float(dz[1].v.view(B, D)[2].abs().max()) == 0.0


def test_infonce_refuses_large_batch_and_odd_width():
    L = lib.load()
    for B, D in ((65, 8), (4, 6)):
        zs = [f32(rnd(B, D + 2, seed=m)) for m in range(3)]
        ns, inv, losses, lse, dz = [Out(B * D) for _ in range(3)], Out(3 * B), Out(3), Out(6 * B), [Out(B * D) for _ in range(3)]
        rc = L.mmf_infonce_fwd(ptr3(zs), ptr3([o.ptr for o in ns]), inv.ptr, losses.ptr, lse.ptr, B, D, 0.07, S())
        refused(rc, E_UNSUPPORTED, *ns, inv, losses, lse)
        rc = L.mmf_infonce_bwd(ptr3([o.ptr for o in ns]), inv.ptr, lse.ptr, ptr3([None] * 3), ptr3([None] * 3),
                               ptr3([o.ptr for o in dz]), B, D, 0.07, S())
        refused(rc, E_UNSUPPORTED, *dz)


# =============================================================================================== small.hip: adaptive combine
@pytest.mark.parametrize("B,d", [(1, 4), (16, 200), (3, 256), (7, 1000)])
def test_adaptive_combine_fwd_bwd(B, d, rec):
    """d below, at and above 256 (one to four columns per thread, the last pass partial); backward with both gradients,
    without dweighted, without daw; dW2 / db2 accumulate into non-zero values.
    dW2 / db2: elementwise bound from the reference.  da[b][m] = sum_c g att is a sum of d products: per thread
    ceil(d / 256) additions, 6 in the wave, 4 across waves and one for daw, k1 = ceil(d / 256) + 12 roundings on
    sum|g att| + |daw|; dl = aw (da - sum aw da) carries e_dl = aw (e_da + sum aw e_da) + 8 u (|aw da| + aw sum|aw da|);
    dW2 = pre + sum_b dl x: e_dl |x| per term plus the B atomics and the product, k2 = B + 2 roundings on the terms."""
    L = lib.load()
    hp, att = f32(rnd(B, d, seed=B + d)), f32(rnd(B, 3, d, seed=B + d + 1))
    W2, b2 = f32(rnd(3, d, seed=3, scale=0.3)), f32(rnd(3, seed=4, scale=0.3))
    aw, wt = Out(B * 3), Out(B * d, BF16)
    run(L.mmf_adaptive_combine_fwd(hp.data_ptr(), W2.data_ptr(), b2.data_ptr(), att.data_ptr(), aw.ptr, wt.ptr, B, d, S()))
    torch.cuda.synchronize()
    raw, rwt = R.adaptive_fwd(host(hp), host(W2), host(b2), host(att))
    hold(rec, "aw", aw.v.view(B, 3), raw, F32_TOL)
    hold(rec, "weighted", wt.v.view(B, d), rwt, BF16_TOL)
    assert aw.intact() and wt.intact()
    gw, ga = bf(rnd(B, d, seed=5)), f32(rnd(B, 3, seed=6))
    awk = host(aw.v).view(B, 3)                                    # the backward reads the forward's saved weights
    for tag, w_, a_ in (("both", gw, ga), ("dweighted null", None, ga), ("daw null", gw, None)):
        pre = [rnd(3, d, seed=7).float(), rnd(3, seed=8).float()]
        datt, dhp, dW2, db2 = Out(B * 3 * d), Out(B * d), Out(3 * d, fill=pre[0]), Out(3, fill=pre[1])
        run(L.mmf_adaptive_combine_bwd(hp.data_ptr(), W2.data_ptr(), att.data_ptr(), aw.ptr, w_.data_ptr() if w_ is not None else None,
                                       a_.data_ptr() if a_ is not None else None, datt.ptr, dhp.ptr, dW2.ptr, db2.ptr, B, d, S()))
        torch.cuda.synchronize()
        g = None if w_ is None else host(w_)
        da_ext = None if a_ is None else host(a_)
        want = R.adaptive_bwd(host(hp), host(W2), host(att), awk, g, da_ext)
        hold(rec, f"dattended/{tag}", datt.v.view(B, 3, d), want[0], F32_TOL)
        hold(rec, f"dhp/{tag}", dhp.v.view(B, d), want[1], F32_TOL)
        gz = torch.zeros(B, d, dtype=F64) if g is None else g
        abs_da = (gz.unsqueeze(1) * host(att)).abs().sum(-1) + (0 if da_ext is None else da_ext.abs())
        da = (gz.unsqueeze(1) * host(att)).sum(-1) + (0 if da_ext is None else da_ext)
        e_da = gamma((d + 255) // 256 + 12) * abs_da
        e_dl = awk * (e_da + (awk * e_da).sum(1, keepdim=True)) + 8 * U24 * ((awk * da).abs() + awk * (awk * da).abs().sum(1, keepdim=True))
        dl = awk * (da - (awk * da).sum(1, keepdim=True))
        xa = host(hp).abs()
        bW = e_dl.t() @ xa + gamma(B + 2) * (dl.abs().t() @ xa + pre[0].double().abs())
        bb = e_dl.sum(0) + gamma(B + 1) * (dl.abs().sum(0) + pre[1].double().abs())
        bound_ok(rec, f"dW2/{tag}", dW2.v.view(3, d), want[2] + pre[0].double(), bW)
        bound_ok(rec, f"db2/{tag}", db2.v, want[3] + pre[1].double(), bb)
        assert all(o.intact() for o in (datt, dhp, dW2, db2))


@pytest.mark.parametrize("heads", [1, 8, 16])
def test_adaptive_attn_weights_heads(heads, rec):
    """the 3-token head-averaged attention weights: 9 x heads score threads (144 at ADAW_MAXH = 16)"""
    B, dh = 3, 8
    qkv = bf(rnd(B * 3, 3 * heads * dh, seed=heads))
    w = Out(B * 9)
    run(lib.load().mmf_adaptive_attn_weights(qkv.data_ptr(), w.ptr, B, heads, dh, S()))
    torch.cuda.synchronize()
    want = R.attn_weights_mean(host(qkv), B, 3, heads, dh)
    hold(rec, "w", w.v.view(B, 3, 3), want, F32_TOL)
    hold(rec, "row sums", w.v.view(B, 3, 3).double().sum(-1), torch.ones(B, 3, dtype=F64), F32_TOL)
    assert w.intact()


@pytest.mark.parametrize("heads,dh", [(1, 8), (8, 96), (12, 64)])
@pytest.mark.parametrize("T", [1, 3, 255, 256, 257, 2048])
def test_attn_weights_mean_key_slots(T, heads, dh, rec):
    """T = 255 / 256 / 257: the first key slot partly used, full, and the second one begun; 2048: every AWM_MAXK slot"""
    B = 2 if T <= 257 else 1
    qkv = bf(rnd(B * T, 3 * heads * dh, seed=T + heads))
    w = Out(B * T * T)
    run(lib.load().mmf_attn_weights_mean(qkv.data_ptr(), w.ptr, B, T, heads, dh, S()))
    torch.cuda.synchronize()
    want = R.attn_weights_mean(host(qkv), B, T, heads, dh)
    hold(rec, "w", w.v.view(B, T, T), want, F32_TOL)
    hold(rec, "row sums", w.v.view(B, T, T).double().sum(-1), torch.ones(B, T, dtype=F64), F32_TOL)
    assert w.intact()


def test_attn_weights_refusals():
    L = lib.load()
    qkv = bf(rnd(2049, 3 * 16))
    w = Out(4096)
    refused(L.mmf_attn_weights_mean(qkv.data_ptr(), w.ptr, 1, 2049, 2, 8, S()), E_SHAPE, w)
    refused(L.mmf_attn_weights_mean(qkv.data_ptr(), w.ptr, 1, 4, 1, 12, S()), E_SHAPE, w)
    refused(L.mmf_adaptive_attn_weights(qkv.data_ptr(), w.ptr, 1, 17, 8, S()), E_SHAPE, w)


# =============================================================================================== small.hip: narrow linear
@pytest.mark.parametrize("N", [1, 7, 16])
def test_narrow_linear_fwd_bwd(N, rec):
    """K = 1, 255, 256, 257, 1000: one to four columns per thread / one to four workgroups of the backward; M = 1, 16, 70;
    b / db / dx absent in turn; dW, db accumulate into non-zero values.
    dW[n][k] = pre + sum_m dy x, added in order by one thread: k = M + 2 roundings (M additions, the product, the final
    add) on |pre| + sum|dy x|; db: k = M + 1 on |pre| + sum|dy|."""
    L, case = lib.load(), 0
    for K in (1, 255, 256, 257, 1000):
        for M in (1, 16, 70):
            no_b, no_db, no_dx = case % 3 == 1, case % 4 == 2, case % 3 == 2
            case += 1
            x, W, b = f32(rnd(M, K, seed=K + M)), f32(rnd(N, K, seed=K + N, scale=K ** -0.5)), f32(rnd(N, seed=N))
            y = Out(M * N)
            run(L.mmf_linear_narrow_fwd(x.data_ptr(), W.data_ptr(), None if no_b else b.data_ptr(), y.ptr, M, N, K, S()))
            dy = f32(rnd(M, N, seed=K + M + 1))
            pre = [rnd(N, K, seed=1).float(), rnd(N, seed=2).float()]
            dx, dW, db = Out(M * K), Out(N * K, fill=pre[0]), Out(N, fill=pre[1])
            run(L.mmf_linear_narrow_bwd(x.data_ptr(), W.data_ptr(), dy.data_ptr(), None if no_dx else dx.ptr, dW.ptr,
                                        None if no_db else db.ptr, M, N, K, S()))
            torch.cuda.synchronize()
            hold(rec, "y", y.v.view(M, N), R.narrow_fwd(host(x), host(W), None if no_b else host(b)), F32_TOL)
            rdx, rdW, rdb = R.narrow_bwd(host(x), host(W), host(dy))
            if no_dx:
                assert dx.untouched()
            else:
                hold(rec, "dx", dx.v.view(M, K), rdx, F32_TOL)
            bound_ok(rec, "dW", dW.v.view(N, K), rdW + pre[0].double(), gamma(M + 2) * (host(dy).abs().t() @ host(x).abs() + pre[0].double().abs()))
            if no_db:
                assert db.untouched()
            else:
                bound_ok(rec, "db", db.v, rdb + pre[1].double(), gamma(M + 1) * (host(dy).abs().sum(0) + pre[1].double().abs()))
            assert all(o.intact() for o in (y, dx, dW, db))


def test_narrow_linear_refuses_seventeen_outputs():
    L = lib.load()
    x, W = f32(rnd(4, 32)), f32(rnd(17, 32))
    y, dx, dW = Out(4 * 17), Out(4 * 32), Out(17 * 32)
    refused(L.mmf_linear_narrow_fwd(x.data_ptr(), W.data_ptr(), None, y.ptr, 4, 17, 32, S()), E_SHAPE, y)
    refused(L.mmf_linear_narrow_bwd(x.data_ptr(), W.data_ptr(), y.ptr, dx.ptr, dW.ptr, None, 4, 17, 32, S()), E_SHAPE, dx, dW)


# =============================================================================================== small.hip: stack3, rowmask
@pytest.mark.parametrize("B,d", [(6, 72), (700, 256)], ids=["small", "above_cap"])
def test_stack3_embed_fwd_bwd(B, d, rec):
    """row-strided features / gradients (ldf, ldd > d, NaN in the gaps of the inputs, the gaps of the outputs left alone);
    with and without the embedding; d1 absent; 700 x 3 x 256 elements are above 2048 x 256 (the forward's loop iterates).
    demb = pre + sum_b dx, one thread in order: k = B + 1 roundings on |pre| + sum|dx|."""
    L, ld = lib.load(), d + 8
    fs = []
    for m in range(3):
        t = torch.full((B, ld), NAN, dtype=F32)
        t[:, :d] = rnd(B, d, seed=m + d).float()
        fs.append(t.to(DEV))
    emb = f32(rnd(3, d, seed=9, scale=0.3))
    for e in (emb, None):
        x = Out(B * 3 * d, BF16)
        run(L.mmf_stack3_embed_fwd(fs[0].data_ptr(), fs[1].data_ptr(), fs[2].data_ptr(), e.data_ptr() if e is not None else None,
                                   x.ptr, B, d, ld, S()))
        torch.cuda.synchronize()
        want = R.stack3_fwd(*[host(f[:, :d]) for f in fs], None if e is None else host(e))
        if e is None:
            same_bits(rec, "x (no emb)", x.v.view(B, 3, d), want.to(BF16))        # f32 -> bf16 of the feature itself
        else:
            hold(rec, "x", x.v.view(B, 3, d), want, BF16_TOL)
        assert x.intact()
    dx = bf(rnd(B, 3, d, seed=11))
    col = (torch.arange(ld) < d).repeat(B)
    for skip, with_emb in ((None, True), (1, True), (None, False)):
        pre = rnd(3, d, seed=12).float()
        ds, demb = [Out(B * ld) for _ in range(3)], Out(3 * d, fill=pre)
        run(L.mmf_stack3_embed_bwd(dx.data_ptr(), *[None if m == skip else ds[m].ptr for m in range(3)],
                                   demb.ptr if with_emb else None, B, d, ld, S()))
        torch.cuda.synchronize()
        r = R.stack3_bwd(host(dx))
        for m in range(3):
            if m == skip:
                assert ds[m].untouched()
            else:
                same_bits(rec, f"d{m}", ds[m].v.view(B, ld)[:, :d], r[m].float())
                assert ds[m].intact(col)
        if with_emb:
            bound_ok(rec, "demb", demb.v.view(3, d), r[3] + pre.double(), gamma(B + 1) * (host(dx).abs().sum(0) + pre.double().abs()))
            assert demb.intact()
        else:
            assert demb.untouched()


@pytest.mark.parametrize("B,d", [(6, 72), (600, 1000)], ids=["small", "above_cap"])
def test_rowmask_exact(B, d, rec):
    x = rnd(B, d, seed=B).float()
    mask = torch.tensor([0.0, 1.0, 1.0, 0.5, 0.0, 1.0], dtype=F32).repeat(B // 6)
    y, xd, md = Out(B * d), x.to(DEV), mask.to(DEV)
    run(lib.load().mmf_rowmask_apply(xd.data_ptr(), md.data_ptr(), y.ptr, B, d, S()))
    torch.cuda.synchronize()
    same_bits(rec, "y", y.v.view(B, d), x * mask[:, None])
    assert y.intact()


# =============================================================================================== optim.hip
OPT_VEC = 4 * THREADS * CAP                                  # floats one pass of the capped grid covers
N_SQ = 4 * OPT_VEC + OPT_VEC + 3                             # capped grid: one 4-way unrolled iteration, one remainder, tail of 3
N_ADAM = 5_000_003                                           # capped grid: one 2-way unrolled iteration, remainder for some, tail of 3


@pytest.mark.parametrize("n", [1, 3, 4, 1027, N_SQ, 20_000_003])
def test_sqnorm_accumulates(n, rec):
    """out += sum x^2.  k: 4 additions per vector x ceil(vectors / threads) per thread, the tail element, 6 in the wave, 3
    across the waves, the product's rounding, and one atomic per workgroup onto the value already there"""
    x = f32(rnd(n, seed=n % 97))
    out = Out(1, fill=3.5)
    run(lib.load().mmf_sqnorm_f32(x.data_ptr(), n, out.ptr, S()))
    torch.cuda.synchronize()
    grid = min(max(((n >> 2) + THREADS - 1) // THREADS, 1), CAP)
    k = 4 * -(-(n >> 2) // (grid * THREADS)) + 1 + 6 + 3 + 1 + grid
    s = (host(x) ** 2).sum()
    bound_ok(rec, "out", out.v, (s + 3.5).reshape(1), (gamma(k) * (s + 3.5)).reshape(1))
    assert out.intact()


def hp_tensor(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, t=1, max_norm=1.0, gs=1.0):
    return torch.tensor([lr, b1, b2, eps, wd, 1 - b1 ** t, 1 - b2 ** t, max_norm, gs], dtype=F32)


ADAM_CASES = {
    # name: (hp, later step (non-zero moments), pass gnorm_sq, clipping expected)
    "clip_active_wd": (dict(t=7, max_norm=1.0, wd=1e-2), True, True, True),
    "clip_inactive_scale_eighth_step1": (dict(t=1, max_norm=1e9, wd=0.0, gs=0.125), False, True, False),
    "clip_off_negative_scale": (dict(t=3, max_norm=0.0, wd=1e-2, gs=-0.5), True, True, False),
    "no_norm_pointer": (dict(t=3, max_norm=1.0, wd=0.0), True, False, False),
    "clip_active_negative_scale": (dict(t=2, max_norm=1.0, wd=1e-2, gs=-0.125), True, True, True),
}


ADAM_RUNS = [(n, c) for n in (1, 3, 4, 1027) for c in ("clip_active_wd", "clip_inactive_scale_eighth_step1")] + \
            [(N_ADAM, c) for c in ADAM_CASES]


@pytest.mark.parametrize("n,case", ADAM_RUNS)
def test_adamw_step_every_element(n, case, rec):
    """masters, both moments and the bf16 shadow of every element.  The non-temporal unrolled body, the plain remainder loop
    and the scalar tail all run on the same tensors at n = 5 000 003 (every hyper-parameter set; the small sizes run two).
    The parameters are small (0.05 N(0, 1)) so that the update (lr = 1e-2) is as large as they are and F32_TOL of their
    scale is a bound on the update itself.  The shadow is the bf16 rounding of the f32 master the kernel wrote: bit-exact
    from the kernel's own master."""
    kw, later, with_norm, clips = ADAM_CASES[case]
    hp = hp_tensor(**kw)
    p0, g = rnd(n, seed=1, scale=0.05).float(), rnd(n, seed=2, scale=0.3).float()
    m0 = (rnd(n, seed=3, scale=0.1).float() if later else torch.zeros(n))
    v0 = ((rnd(n, seed=4, scale=0.1) ** 2).float() if later else torch.zeros(n))
    gn = (g.double() ** 2).sum().float().reshape(1)
    coef = R.clip_coef(hp.double().tolist(), float(gn) if with_norm else None)
    if n == N_ADAM:
        assert (abs(coef) < abs(kw.get("gs", 1.0)) * 0.999) == clips        # the case is the branch it says it is
    p, m, v, sh = Out(n, fill=p0), Out(n, fill=m0), Out(n, fill=v0), Out(n, BF16, off=4)
    gd, hpd, gnd = g.to(DEV), hp.to(DEV), gn.to(DEV)
    run(lib.load().mmf_adamw_step(p.ptr, gd.data_ptr(), m.ptr, v.ptr, sh.ptr, n, hpd.data_ptr(),
                                  gnd.data_ptr() if with_norm else None, S()))
    torch.cuda.synchronize()
    rp, rm, rv = R.adamw(p0.double(), g.double(), m0.double(), v0.double(), hp.double().tolist(), float(gn) if with_norm else None)
    hold(rec, "master", p.v, rp, F32_TOL)
    hold(rec, "exp_avg", m.v, rm, F32_TOL)
    hold(rec, "exp_avg_sq", v.v, rv, F32_TOL)
    # the step itself, to F32_TOL of the largest step plus the rounding of the stored master (half an f32 ulp of |p|max)
    upd = rp - p0.double()
    hold(rec, "update", host(p.v) - p0.double(), upd, F32_TOL, scale=float(upd.abs().max()) + U24 * float(rp.abs().max()) / F32_TOL)
    same_bits(rec, "shadow", sh.v, p.v.cpu().to(BF16))
    assert all(o.intact() for o in (p, m, v, sh))
    assert bool(torch.equal(gd.cpu(), g)) and bool(torch.equal(hpd.cpu(), hp))


@pytest.mark.parametrize("mode", ["onecycle_cycle_momentum", "onecycle_fixed_momentum", "constant"])
def test_adamw_advance_schedule(mode, rec):
    """steps 1 .. total + 2 (past the end of the schedule: held at the final value): the step counter exactly, hp[0], [1],
    [5], [6] against the float64 restatement fed the hp the kernel read — double arithmetic rounded once to f32, so
    2^-23 relative — and every other entry of hp untouched"""
    L, total = lib.load(), 10
    sched = [0.0 if mode == "constant" else 1.0, 3e-3, float(total), 0.3, 25.0, 1e4, 1.0 if mode == "onecycle_cycle_momentum" else 0.0,
             0.85, 0.95]
    sd = torch.tensor(sched, dtype=F64, device=DEV)
    hp = Out(9, fill=hp_tensor(lr=7e-4, t=1))
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for t in range(1, total + 3):
        before = hp.v.cpu()
        run(L.mmf_adamw_advance(step.data_ptr(), hp.ptr, sd.data_ptr(), S()))
        torch.cuda.synchronize()
        want_t, want = R.adamw_advance(t - 1, before.double().tolist(), sched)
        assert int(step.item()) == want_t == t
        got = hp.v.cpu()
        for i in (0, 1, 5, 6):
            r = abs(float(got[i]) - want[i]) / abs(want[i])
            rec(f"hp[{i}]", r / 2.0 ** -23)
            assert r <= 2.0 ** -23, (t, i, float(got[i]), want[i])
        for i in (2, 3, 4, 7, 8):
            assert bits(got)[i] == bits(before)[i]
        assert hp.intact()
