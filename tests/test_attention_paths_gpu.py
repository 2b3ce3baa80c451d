"""GPU: the twelve fused-attention instantiations of csrc/attention2.hip (forward, dQ, dK/dV; head_dim 64 / 96; with and
without dropout), path by path, against the float64 restatement of tests/attn_ref.py.

The kernels are called through lib.attn_fwd_grouped / lib.attn_bwd_grouped with hand-built problems, so strides, guards, LSE
and delta are the test's.  The three kernels are isolated: the forward is checked on its own (O, and LSE per (b, h, q)); the
backward is then handed O (rounded to bf16) and LSE (f32) of the REFERENCE, so a forward error can neither mask nor mimic a
backward one.  One case per head_dim goes through ops.attention_group for the wiring.

Conventions (tests/test_kernel_forms_gpu.py): operands from a seeded float64 generator, rounded to bf16; every output pre-filled
with NaN; guard rows behind row B*T, guard columns beside the head range of a strided buffer and guard elements behind
LSE / delta hold a sentinel and must come back bit-identical, as must every input.

Bounds.  O, dQ, dK, dV against staged():  BF16_TOL x max|ref| + N, N = max|staged - staged with scores perturbed by 2^-22|
for that case and output (the reference's own sensitivity to f32-sized score errors, computed here on the CPU); for dQ and
dK, N also takes attn_ref.f32_noise(): the f32 summation noise of dP - delta, each sum held to F32_TOL x the sum of its terms'
magnitudes (the delta output's own bound), carried through dS = P (dP - delta) into the two products.  Without it the cases
whose softmax is one-hot failed on an MI355X with nothing wrong in the kernels: at Tk = 1, and with one key 40 log2 units
above the rest, dP - delta cancels to 0, the true dQ / dK are 0 (the reference gives 1e-10), and the kernels return the
rounding noise of two 64- or 96-term f32 sums times |K|, 1e-7 to 1.3e-5.  On random operands the term adds 2 - 6 % to the bound.  LSE:
F32_TOL x max(|ref|, 1).  delta: per row F32_TOL x sum|O dO| of the operands the kernel was given.  Every error / bound
ratio is printed as a PARITY line before anything is asserted (profiles/attention_parity.txt is those lines from an MI355X).

Shapes are read off fill_args2 and the kernels: the forward splits Tq into ceil(Tq / 128) balanced chunks of a multiple of 32
rows (129 -> 2 x 96, 257 -> 3 x 96), dQ into fixed 128-row chunks, dK/dV splits Tk into 128-key chunks; one wave per 32 rows,
waves past the end only stage tiles; the swept axis moves in 64-row tiles of two 32-row blocks through a 2-stage ring whose
free stage (tile count parity) takes the epilogue; dK/dV with Tk <= 32 gives query block w of every tile to wave w (sweep
split) and adds wave 1's partial sums through LDS."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as R  # noqa: E402
from mmfusion import lib, ops  # noqa: E402
from test_kernel_forms_gpu import BF16_TOL, DEV, F32_TOL, NAN  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
SENTINEL = 777.0
GROWS, GELEMS = 2, 16                      # guard rows behind a matrix, guard elements behind LSE / delta
STATE = (0x5EED1234 << 32) | 0x9ABCDEF1    # dropout state with a non-zero high word
SITE = 5
DHS = (64, 96)


def scale_of(dh):
    return R.f32r_scale(1.0 / math.sqrt(dh))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


class Mat:
    """rows x d bf16 values at column `off` of a (rows + GROWS, ld) buffer; values None = an output, NaN-filled.  Everything
    outside the rows x d window is guard (sentinel)."""

    def __init__(self, rows, d, ld, off, values=None):
        self.rows, self.d, self.off = rows, d, off
        self.buf = torch.full((rows + GROWS, ld), SENTINEL, dtype=BF16, device=DEV)
        self.v = self.buf[:rows, off:off + d]
        if values is None:
            self.v.fill_(NAN)
        else:
            self.v.copy_(values.reshape(rows, d).to(BF16))
        self.mark()

    def mark(self):
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 2 * self.off

    def guards_intact(self):
        a, b = bits(self.buf), bits(self.before)
        keep = torch.ones(a.shape, dtype=torch.bool)
        keep[:self.rows, self.off:self.off + self.d] = False
        return bool(torch.equal(a[keep], b[keep]))

    def untouched(self):
        return bool(torch.equal(bits(self.buf), bits(self.before)))

    def host(self):
        return self.v.detach().cpu().double()


class Vec:
    """n f32 values followed by GELEMS guard elements"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + GELEMS,), SENTINEL, dtype=F32, device=DEV)
        self.v = self.buf[:n]
        self.v.fill_(NAN)
        self.mark()

    mark = Mat.mark
    untouched = Mat.untouched

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def guards_intact(self):
        return bool(torch.equal(bits(self.buf)[self.n:], bits(self.before)[self.n:]))

    def host(self):
        return self.v.detach().cpu().double()


def operands(dh, B, H, Tq, Tk, seed, qs=1.0, dos=1.0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda T, s: R.bf16r(torch.randn(B, T, H * dh, generator=g, dtype=F64) * s)
    return mk(Tq, qs), mk(Tk, 1.0), mk(Tk, 1.0), mk(Tq, dos)


class Case:
    """one attention problem: device buffers, reference, checks.  strided: ldq, ldk, ldv, ldo distinct, above H*dh, multiples
    of 8, every operand at a non-zero column offset of its buffer."""

    def __init__(self, dh, B, H, Tq, Tk, seed=0, strided=False, ops_=None, qs=1.0, dos=1.0):
        self.dh, self.B, self.H, self.Tq, self.Tk = dh, B, H, Tq, Tk
        d = self.d = H * dh
        self.q, self.k, self.v, self.do = ops_ if ops_ is not None else operands(dh, B, H, Tq, Tk, seed, qs, dos)
        (self.ldq, oq), (self.ldk, ok), (self.ldv, ov), (self.ldo, oo) = \
            ((d + 8, 8), (d + 24, 16), (d + 40, 8), (d + 16, 8)) if strided else ((d, 0),) * 4
        self.Q, self.dQ = Mat(B * Tq, d, self.ldq, oq, self.q), Mat(B * Tq, d, self.ldq, oq)
        self.K, self.dK = Mat(B * Tk, d, self.ldk, ok, self.k), Mat(B * Tk, d, self.ldk, ok)
        self.V, self.dV = Mat(B * Tk, d, self.ldv, ov, self.v), Mat(B * Tk, d, self.ldv, ov)
        self.O, self.dO = Mat(B * Tq, d, self.ldo, oo), Mat(B * Tq, d, self.ldo, oo, self.do)
        self.LSE, self.delta = Vec(B * H * Tq), Vec(B * H * Tq)

    def problem(self):
        return lib.AttnProblem(self.Q.ptr, self.K.ptr, self.V.ptr, self.O.ptr, self.LSE.ptr, self.dO.ptr, self.delta.ptr,
                               self.dQ.ptr, self.dK.ptr, self.dV.ptr, self.B, self.H, self.Tq, self.Tk,
                               self.ldq, self.ldk, self.ldv, self.ldo)

    def reference(self, scale, keep=None, inv_keep=1.0):
        a = (self.q, self.k, self.v, self.do, self.H, scale, keep, inv_keep)
        self.ref = R.staged(*a)
        self.noisy = R.staged(*a, perturb=R.PERTURB, seed=1)
        self.o16 = R.bf16r(self.ref["o"])
        self.lse32 = R.f32r(self.ref["lse"])
        self.noise32 = R.f32_noise(self.q, self.k, self.v, self.do, self.H, scale, self.o16, self.lse32, F32_TOL, keep, inv_keep)

    def _mat(self, rec, fails, tag, name, mat, key):
        ref, got = self.ref[key].reshape(-1, self.d), mat.host()
        noise = float((self.ref[key] - self.noisy[key]).abs().max()) + self.noise32.get(key, 0.0)
        bound = BF16_TOL * float(ref.abs().max()) + noise
        err = float((got - ref).abs().max()) if bool(torch.isfinite(got).all()) else math.inf
        rec(f"{tag}{name}", err / max(bound, 1e-300))
        if not err <= bound:
            bad = (~((got - ref).abs() <= bound)).nonzero()
            fails.append(f"{tag}{name}: err {err:.4g} > bound {bound:.4g} (noise {noise:.3g}); {len(bad)} elements, first (row, col) {bad[0].tolist()}")
        if not mat.guards_intact():
            fails.append(f"{tag}{name}: guard rows / columns changed")

    def check_forward(self, rec, fails, tag=""):
        self._mat(rec, fails, tag, "O", self.O, "o")
        ref, got = self.ref["lse"].reshape(-1), self.LSE.host()
        bound = F32_TOL * max(float(ref.abs().max()), 1.0)
        err = float((got - ref).abs().max()) if bool(torch.isfinite(got).all()) else math.inf
        rec(f"{tag}LSE", err / bound)
        if not err <= bound:
            fails.append(f"{tag}LSE: err {err:.4g} > bound {bound:.4g}, first (b*H + h)*Tq + q = {int((~((got - ref).abs() <= bound)).nonzero()[0])}")
        for name, x in (("LSE", self.LSE), ("Q", self.Q), ("K", self.K), ("V", self.V)):
            if not (x.guards_intact() if name == "LSE" else x.untouched()):
                fails.append(f"{tag}{name}: changed by the forward")

    def hand_reference_forward_to_backward(self):
        self.O.v.copy_(self.o16.reshape(-1, self.d).to(BF16))
        self.LSE.v.copy_(self.lse32.reshape(-1).to(F32))
        self.O.mark(), self.LSE.mark()

    def check_backward(self, rec, fails, tag=""):
        self._mat(rec, fails, tag, "dQ", self.dQ, "dq")
        self._mat(rec, fails, tag, "dK", self.dK, "dk")
        self._mat(rec, fails, tag, "dV", self.dV, "dv")
        o16 = self.O.host().reshape(self.B, self.Tq, self.d)       # the O this backward was given
        ref = (R.heads(o16, self.H) * R.heads(self.do, self.H)).sum(-1).reshape(-1)
        bound = F32_TOL * R.delta_bound(o16, self.do, self.H).reshape(-1)
        got = self.delta.host()
        err = (got - ref).abs()
        ok = err <= bound
        rec(f"{tag}delta", float((err / bound.clamp_min(1e-300)).max()) if bool(torch.isfinite(got).all()) else math.inf)
        if not bool(ok.all()):
            fails.append(f"{tag}delta: {int((~ok).sum())} rows outside F32_TOL x sum|O dO|, first {int((~ok).nonzero()[0])}")
        if not self.delta.guards_intact():
            fails.append(f"{tag}delta: guard elements changed")
        for name, x in (("O", self.O), ("LSE", self.LSE), ("Q", self.Q), ("K", self.K), ("V", self.V), ("dO", self.dO)):
            if not x.untouched():
                fails.append(f"{tag}{name}: changed by the backward")

    def outputs(self):
        return [bits(x.buf) for x in (self.O, self.LSE, self.delta, self.dQ, self.dK, self.dV)]


@pytest.fixture
def rec(request):
    """rec(name, ratio): the worst error / bound per output name, printed when the test ends (also when it fails)"""
    worst = {}

    def put(name, ratio):
        worst[name] = max(worst.get(name, 0.0), float(ratio))
    yield put
    for name, r in worst.items():
        print(f"PARITY {request.node.nodeid.split('::')[-1]} {name} {r:.4f}")


@pytest.fixture(scope="module")
def rng_state():
    return torch.tensor([STATE], dtype=torch.int64, device=DEV)


def run_group(rec, dh, cases, scale=None, p=0.0, state=None, tags=None, refs=True):
    """one grouped forward, checked; then one grouped backward on the reference's O and LSE, checked.  Under dropout the
    masks come from the host restatement, keyed by each case's index in `cases`."""
    scale = scale_of(dh) if scale is None else scale
    thresh = R.mmf_drop_thresh(p) if p > 0 else 0
    inv = R.inv_keep_of(thresh)
    tags = tags or ([""] if len(cases) == 1 else [f"p{i}." for i in range(len(cases))])
    if refs:
        for i, c in enumerate(cases):
            keep = R.attention_keep(STATE, SITE, i, c.B, c.H, c.Tq, c.Tk, thresh) if thresh else None
            c.reference(scale, keep, inv)
    drop = (p, state.data_ptr(), SITE) if p > 0 else (0.0, None, 0)
    fails = []
    probs = [c.problem() for c in cases]
    lib.attn_fwd_grouped(probs, dh, scale, *drop)
    torch.cuda.synchronize()
    for c, t in zip(cases, tags):
        c.check_forward(rec, fails, t)
        c.fwd_bits = [bits(c.O.buf), bits(c.LSE.buf)]
        c.hand_reference_forward_to_backward()
    lib.attn_bwd_grouped(probs, dh, scale, *drop)
    torch.cuda.synchronize()
    for c, t in zip(cases, tags):
        c.check_backward(rec, fails, t)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ shapes, path by path
# forward / dQ: query chunking (Tq 1..257: one chunk of 1-4 blocks, 2 x 96 with a 33-row last chunk, 3 x 96 with 65) x key
# sweep (1-4 tiles of both parities, ragged first / second block, second block pure padding)
FWD_PAIRS = [(1, 1), (31, 31), (32, 32), (33, 33), (96, 64), (97, 65), (128, 96), (129, 97), (257, 128), (1, 129), (31, 193),
             (33, 1), (129, 31), (257, 33), (96, 129), (128, 193), (32, 65)]
# dK/dV general path: key chunks with inactive waves x query tiles of both parities, rows past Tq inside a tile, empty second block
DKV_PAIRS = [(1, 33), (32, 64), (33, 65), (64, 128), (65, 129), (97, 257), (129, 33), (193, 65), (64, 257), (1, 64), (193, 129)]
# dK/dV sweep split (Tk <= 32) with B*H in {1, 3, 9}; (200, 33) is the first shape that does not split
SPLIT = [(1, 1, 1, 1), (30, 30, 3, 1), (32, 32, 3, 3), (33, 32, 1, 1), (64, 17, 1, 3), (65, 32, 3, 3), (97, 5, 1, 1),
         (129, 32, 3, 1), (200, 32, 3, 3), (200, 33, 1, 3)]


@pytest.mark.parametrize("Tq,Tk", FWD_PAIRS, ids=lambda x: str(x))
@pytest.mark.parametrize("dh", DHS)
def test_query_chunks_and_key_sweep(rec, dh, Tq, Tk):
    run_group(rec, dh, [Case(dh, 2, 2, Tq, Tk, seed=Tq * 1000 + Tk)])


@pytest.mark.parametrize("Tq,Tk", DKV_PAIRS, ids=lambda x: str(x))
@pytest.mark.parametrize("dh", DHS)
def test_dkv_key_chunks_and_query_sweep(rec, dh, Tq, Tk):
    run_group(rec, dh, [Case(dh, 1, 2, Tq, Tk, seed=Tq * 1000 + Tk + 1)])


@pytest.mark.parametrize("Tq,Tk,B,H", SPLIT, ids=lambda x: str(x))
@pytest.mark.parametrize("dh", DHS)
def test_dkv_sweep_split(rec, dh, Tq, Tk, B, H):
    run_group(rec, dh, [Case(dh, B, H, Tq, Tk, seed=Tq * 1000 + Tk + 2)])


# ------------------------------------------------------------------------------------------------ deferred running maximum
def halfway_pair(c):
    """bf16 a, b with E = a b c just over DEFER and 2^E within 1 % of the midpoint of two bf16 neighbours in [64, 128): a P
    that the unraised maximum would feed to the matrix pipe with the largest rounding error bf16 has (1 / 257)"""
    m = np.arange(128, 256, dtype=np.float64) / 128.0
    a = np.concatenate([4.0 * m, 8.0 * m])[:, None]
    b = np.concatenate([m, 2.0 * m, 4.0 * m])[None, :]
    E = a * b * c
    pos = np.mod((np.exp2(E) - 64.0) / 0.5, 1.0)
    ok = (E > 6.02) & (E < 6.9) & (np.abs(pos - 0.5) < 0.01)
    i, j = np.argwhere(ok)[0]
    return float(a[i, 0]), float(b[0, j]), float(E[i, j])


def max_operands(dh, kind):
    """scores on one coordinate: q[.., 0] = a in every row, k[j, 0] = b_j, so s[i][j] = a b_j exactly.  Block 0 (keys 0..31)
    has its maximum 0 at key 3, the rest at -4 a; key 70 (block 2) carries the case."""
    B, H, Tq, Tk = 1, 2, 40, 101
    scale = scale_of(dh)
    c = float(np.float32(scale) * np.float32(1.4426950408889634))
    q, k, v, do = operands(dh, B, H, Tq, Tk, seed=77)
    a = 8.0
    kc = torch.zeros_like(k)
    b = torch.full((Tk,), -4.0, dtype=F64)
    b[3] = 0.0
    if kind == "under6":
        b[70] = float(R.bf16r(torch.tensor(5.9 / (a * c), dtype=F64)))
    elif kind == "over6":
        a, b70, E = halfway_pair(c)
        assert 6.0 < E < 7.0
        b[70] = b70
        g = torch.Generator().manual_seed(3)            # |V| of the dominant key in [1.5, 2): every O element is near the maximum
        mag = 1.5 + 0.5 * torch.rand(H * dh, generator=g, dtype=F64)
        v[0, 70] = R.bf16r(mag * torch.sign(torch.randn(H * dh, generator=g, dtype=F64)))
        v[0, :70] *= 0.25
        v[0, 71:] *= 0.25
        v = R.bf16r(v)
    elif kind == "about40":
        b[70] = float(R.bf16r(torch.tensor(40.0 / (a * c), dtype=F64)))
    elif kind == "first_block":
        b[3] = float(R.bf16r(torch.tensor(9.0 / (a * c), dtype=F64)))
    elif kind == "minus200":
        b[:] = float(R.bf16r(torch.tensor(-200.0 / (a * scale), dtype=F64)))
        b = b + R.bf16r(torch.randn(Tk, generator=torch.Generator().manual_seed(4), dtype=F64))
        b = R.bf16r(b)
    for h in range(H):
        q[..., h * dh] = a
        kc[0, :, h * dh] = b
    if kind == "equal_keys":
        kc = k[:, :1].expand(B, Tk, H * dh).clone()
        q = R.bf16r(q * 0.25)
    return (B, H, Tq, Tk), (q, kc, v, do)


@pytest.mark.parametrize("kind", ["under6", "over6", "about40", "first_block", "minus200", "equal_keys"])
@pytest.mark.parametrize("dh", DHS)
def test_deferred_running_maximum(rec, dh, kind):
    """a block maximum just under DEFER above the running one (no rescale: P about 60 goes to the matrix pipe), just over
    (rescale: that P becomes exactly 1 — held at a P the unraised form would round worst), far over, the maximum in the
    first block, every score near -200, all keys equal (P = 1 / Tk, LSE = s + ln Tk); the same operands go to the backward"""
    shape, operands_ = max_operands(dh, kind)
    c = Case(dh, *shape, ops_=operands_)
    run_group(rec, dh, [c])
    if kind == "equal_keys":
        want = ((R.heads(c.q, c.H) @ R.heads(c.k, c.H).transpose(-1, -2))[..., 0] * scale_of(dh) + math.log(c.Tk)).reshape(-1)
        got = c.fwd_bits[1][:c.LSE.n].view(F32).double()
        assert float((got - want).abs().max()) <= F32_TOL * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("dh", DHS)
def test_large_statistics(rec, dh):
    """LSE near +60 (b = 0) and -60 (b = 1) at the head_dim's scale (1/8, 1/sqrt(96)), dO scaled by 50: the dK/dV kernel
    spreads -LSE / scale (about 480 / 590) and -delta through a three-way bf16 split that is claimed to be exact"""
    B, H, Tq, Tk = 2, 2, 70, 45
    q, k, v, do = operands(dh, B, H, Tq, Tk, seed=88, dos=50.0)
    big = 30.0 if dh == 64 else 36.75                # 16 x big x scale = 60
    for h in range(H):
        q[..., h * dh] = 16.0
        k[0, :, h * dh] = big
        k[1, :, h * dh] = -big
    c = Case(dh, B, H, Tq, Tk, ops_=(q, k, v, do))
    run_group(rec, dh, [c])
    lse = c.ref["lse"]
    assert 55 < float(lse[0].mean()) < 70 and -70 < float(lse[1].mean()) < -50


# ------------------------------------------------------------------------------------------------ strides and guards
@pytest.mark.parametrize("Tq,Tk", [(33, 65), (129, 32), (97, 129), (1, 1)], ids=lambda x: str(x))
@pytest.mark.parametrize("dh", DHS)
def test_strides_offsets_and_guards(rec, dh, Tq, Tk):
    """ldq, ldk, ldv, ldo distinct, above H*dh, multiples of 8; Q / K / V at non-zero column offsets of wider buffers; O, dQ,
    dK, dV into strided buffers; guard columns beside every head range, guard rows behind row B*T and guard elements behind
    LSE / delta must come back bit-identical (checked inside every Case; here the strides make the columns exist)"""
    c = Case(dh, 2, 3, Tq, Tk, seed=5, strided=True)
    assert len({c.ldq, c.ldk, c.ldv, c.ldo}) == 4 and min(c.ldq, c.ldk, c.ldv, c.ldo) > c.d
    run_group(rec, dh, [c])


# ------------------------------------------------------------------------------------------------ workgroup table
@pytest.mark.parametrize("B,H,T", [(1, 1, 100), (3, 1, 100), (3, 3, 100), (17, 1, 40), (3, 1, 300), (1, 17, 33)],
                         ids=["1", "3", "9", "17", "3x3chunks", "17heads"])
@pytest.mark.parametrize("dh", DHS)
def test_workgroup_counts(rec, dh, B, H, T):
    """B*H*nchunk in {1, 3, 9, 17} (and 3 x 3 chunks): the XCD remap of a range padded to a multiple of 8 and the
    item >= nwg exit; every (b, h, chunk) must be written (NaN pre-fill)"""
    run_group(rec, dh, [Case(dh, B, H, T, T + 3, seed=B * 100 + H)])


MIXED = [(33, 65, 1, 2), (33, 65, 2, 1), (64, 17, 1, 1), (129, 32, 1, 2), (1, 1, 1, 1), (97, 129, 1, 1), (30, 30, 2, 2),
         (64, 30, 1, 1), (200, 32, 1, 1), (65, 64, 1, 2), (32, 32, 1, 1), (129, 97, 1, 1)]


@pytest.mark.parametrize("dh", DHS)
def test_twelve_mixed_problems_match_their_solo_launches(rec, dh):
    """MMF_ATTN_MAX_PROBLEMS problems of mixed shapes in one launch, with equal keys in the heaviest-first sort of all three
    kernels ((33, 65) twice; (64, 17) and (64, 30)): each problem against the reference, and bit for bit against its own
    solo launch"""
    assert len(MIXED) == lib.ATTN_MAX_PROBLEMS
    mk = lambda: [Case(dh, B, H, Tq, Tk, seed=50 + i) for i, (Tq, Tk, B, H) in enumerate(MIXED)]
    group = mk()
    run_group(rec, dh, group)
    for i, c in enumerate(mk()):
        run_group(rec, dh, [c], tags=[f"solo{i}."])
        for name, a, b in zip(("O", "LSE"), c.fwd_bits, group[i].fwd_bits):
            assert torch.equal(a, b), (i, name)
        for name, a, b in zip(("O", "LSE", "delta", "dQ", "dK", "dV"), c.outputs(), group[i].outputs()):
            assert torch.equal(a, b), (i, name)


# ------------------------------------------------------------------------------------------------ dropout
DROP_GROUP = [(30, 30, 1, 2), (129, 193, 1, 2), (64, 17, 2, 2), (97, 65, 1, 3), (33, 129, 1, 2)]     # caller's order
OTHER_COMPANY = [(257, 64, 1, 2), (31, 33, 1, 2), (64, 17, 2, 2), (20, 200, 1, 2)]                   # index 2 is the same problem


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dh", DHS)
def test_dropout_grouped_masks_follow_the_callers_index(rec, rng_state, dh, p):
    """five problems whose launch order (forward / dQ: longest key sweep first; dK/dV: longest query sweep first) differs from
    the caller's; state with a non-zero high word, site 5, H >= 2.  The masks are the host restatement's, keyed by the
    caller's index; the bounds are those of the runs without dropout.  The problem at index 2 gives the same bits in other
    company."""
    mk = lambda shapes: [Case(dh, B, H, Tq, Tk, seed=70 + i) for i, (Tq, Tk, B, H) in enumerate(shapes)]
    group = mk(DROP_GROUP)
    run_group(rec, dh, group, p=p, state=rng_state)
    other = mk(OTHER_COMPANY)
    run_group(rec, dh, other, p=p, state=rng_state, tags=[f"o{i}." for i in range(len(other))])
    for name, a, b in zip(("O", "LSE"), other[2].fwd_bits, group[2].fwd_bits):
        assert torch.equal(a, b), name
    for name, a, b in zip(("O", "LSE", "delta", "dQ", "dK", "dV"), other[2].outputs(), group[2].outputs()):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("dh", DHS)
def test_dropout_threshold_zero_is_no_dropout(rec, rng_state, dh):
    """p so small that its 2^-32 quantisation is 0 gives the bits of p = 0"""
    assert R.mmf_drop_thresh(1e-11) == 0
    a, b = Case(dh, 1, 2, 70, 40, seed=9), Case(dh, 1, 2, 70, 40, seed=9)
    run_group(rec, dh, [a])
    run_group(rec, dh, [b], p=1e-11, state=rng_state, tags=["tiny_p."])
    assert all(torch.equal(x, y) for x, y in zip(a.outputs() + a.fwd_bits, b.outputs() + b.fwd_bits))


def test_counter_hash_restatement_matches_the_device():
    """the hash is device-only code: mmf_dropout (sub-stream 0) over 5000 ones, state with a non-zero high word, site 7; the
    zero pattern must equal the restated mask exactly"""
    n, p, site = 5000, 0.3, 7
    st = torch.tensor([STATE], dtype=torch.int64, device=DEV)
    x = torch.ones(n, dtype=F32, device=DEV)
    y = torch.full((n,), NAN, dtype=F32, device=DEV)
    lib.check(lib.load().mmf_dropout(x.data_ptr(), y.data_ptr(), n, 1, p, st.data_ptr(), site, lib.stream_ptr()))
    torch.cuda.synchronize()
    keep = torch.from_numpy(R.elementwise_keep(STATE, site, n, R.mmf_drop_thresh(p)))
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y.cpu() != 0, keep)
    assert 0.65 < float(keep.double().mean()) < 0.75
    assert not torch.equal(keep, torch.from_numpy(R.elementwise_keep(STATE & 0xFFFFFFFF, site, n, R.mmf_drop_thresh(p))))
    assert not torch.equal(keep, torch.from_numpy(R.elementwise_keep(STATE, 0, n, R.mmf_drop_thresh(p))))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("dh", DHS)
def test_end_to_end_through_attention_group(rec, dh):
    """ops.attention_group on packed sources (q; k | v), forward and autograd backward: the wiring of pointers, strides, LSE
    and delta.  The backward reference takes the O the op returned (checked first)."""
    B, H, Tq, Tk = 2, 2, 70, 45
    d = H * dh
    q, k, v, do = operands(dh, B, H, Tq, Tk, seed=21)
    qd = q.reshape(B * Tq, d).to(BF16).to(DEV).requires_grad_(True)
    kvd = torch.cat([k, v], -1).reshape(B * Tk, 2 * d).to(BF16).to(DEV).requires_grad_(True)
    o = ops.attention_group([ops.AttnSpec(B, Tq, Tk, q=(0, 0), k=(1, 0), v=(1, d))], H, dh, [qd, kvd])[0]
    o.backward(do.reshape(B * Tq, d).to(BF16).to(DEV))
    torch.cuda.synchronize()
    og = o.detach().cpu().double().reshape(B, Tq, d)
    a = (q, k, v, do, H, scale_of(dh))
    ref, noisy = R.staged(*a, o_bwd=og), R.staged(*a, o_bwd=og, perturb=R.PERTURB, seed=1)
    n32 = R.f32_noise(*a, og, R.f32r(ref["lse"]), F32_TOL)
    kvg = kvd.grad.cpu().double().reshape(B, Tk, 2 * d)
    for name, got, key in (("O", og, "o"), ("dQ", qd.grad.cpu().double().reshape(B, Tq, d), "dq"), ("dK", kvg[..., :d], "dk"),
                           ("dV", kvg[..., d:], "dv")):
        bound = BF16_TOL * float(ref[key].abs().max()) + float((ref[key] - noisy[key]).abs().max()) + n32.get(key, 0.0)
        err = float((got - ref[key]).abs().max())
        rec(name, err / bound)
        assert err <= bound, (name, err, bound)


# ------------------------------------------------------------------------------------------------ host refusals
def test_host_refusals(rng_state):
    """each returns its code and message before any launch: the NaN-filled outputs stay NaN"""
    L = lib.load()
    c = Case(64, 1, 2, 8, 8)
    st = rng_state.data_ptr()

    def call(bwd, probs, n=None, dh=64, p=0.0, state=None, **over):
        arr = (lib.AttnProblem * max(len(probs), 1))(*probs)
        for key, val in over.items():
            setattr(arr[0], key, val)
        fn = L.mmf_attn_bwd_grouped_ex if bwd else L.mmf_attn_fwd_grouped_ex
        rc = fn(arr, len(probs) if n is None else n, dh, 0.125, p, state, 0, lib.stream_ptr())
        return rc, L.mmf_last_error().decode()

    for bwd in (False, True):
        one = [c.problem()]
        assert call(bwd, one, n=0)[0] == E_SHAPE and "num_problems=0" in call(bwd, one, n=0)[1]
        rc, msg = call(bwd, [c.problem()] * 13)
        assert rc == E_SHAPE and "num_problems=13" in msg
        for dh in (32, 128):
            rc, msg = call(bwd, one, dh=dh)
            assert rc == E_UNSUPPORTED and f"head_dim={dh}" in msg
        for key in ("ldq", "ldk", "ldv", "ldo"):
            rc, msg = call(bwd, one, **{key: 120})
            assert rc == E_ALIGN and "row strides must be >= H*head_dim" in msg
            rc, msg = call(bwd, one, **{key: 132})
            assert rc == E_ALIGN and "multiples of 8" in msg
        for key in ("Q", "K", "V", "O"):
            rc, msg = call(bwd, one, **{key: getattr(c, key).ptr + 8})
            assert rc == E_ALIGN and "16-byte aligned" in msg
        rc, msg = call(bwd, one, LSE=None)
        assert rc == E_SHAPE and "null operand" in msg
        for p, state in ((-0.1, st), (1.0, st), (1.5, st), (float("nan"), st), (0.2, None)):
            rc, msg = call(bwd, one, p=p, state=state)
            assert rc == E_SHAPE and "dropout needs 0 <= p < 1" in msg, (p, msg)
        # T * ld * 2 >= 2 GiB, as sizes only (nothing is dereferenced before the check)
        for over in (dict(Tq=1 << 20, ldq=1024), dict(Tq=1 << 20, ldo=1024), dict(Tk=1 << 20, ldk=1024), dict(Tk=1 << 20, ldv=1024)):
            rc, msg = call(bwd, one, **over)
            assert rc == E_SHAPE and "2 GiB" in msg, over
        # the dropout stream id is problem * 4096 + b*H + h: B*H > 4096 would run into the next problem's streams
        rc, msg = call(bwd, one, p=0.2, state=st, B=4097, H=1, ldq=64, ldk=64, ldv=64, ldo=64)
        assert rc == E_SHAPE and "B*H <= 4096" in msg
        rc, msg = call(bwd, one, p=0.2, state=st, B=1, H=4097, ldq=4097 * 64, ldk=4097 * 64, ldv=4097 * 64, ldo=4097 * 64)
        assert rc == E_SHAPE and "B*H <= 4096" in msg
    rc, msg = call(True, [c.problem()], delta=None)
    assert rc == E_SHAPE and "null gradient operand" in msg
    rc, msg = call(True, [c.problem()], dQ=c.dQ.ptr + 8)
    assert rc == E_ALIGN and "gradient pointers" in msg
    torch.cuda.synchronize()
    for x in (c.O, c.LSE, c.delta, c.dQ, c.dK, c.dV, c.Q, c.K, c.V, c.dO):
        assert x.untouched()
