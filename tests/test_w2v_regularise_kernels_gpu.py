"""GPU: the kernels behind ``NativeWav2Vec2``'s training-mode regularisers against float64 under the masks
tests/w2v_regularise_ref.py restates on the host: the fused attention with dropped probabilities on the exact-delta route
(``mmf_attn_fwd_grouped_keyed`` / ``mmf_attn_delta_f32_keyed`` / ``mmf_attn_bwd_grouped_delta_keyed``), the GELU with activation dropout
(``mmf_bias_gelu_drop_bf16_to`` / ``_bwd_bf16``), the span draw (``mmf_w2v_mask_spans``) and masking + feature-projection dropout with
its backward (``mmf_w2v_mask_drop`` / ``mmf_w2v_mask_embed_grad``).

Bounds.  The attention is one launch of 3 clips of T = 149 (odd, past one 128-row block) whose first clip is clip ITEM0 of a batch, so
the stream-id base is ITEM0 * H.  The mask is held to the restatement EXACTLY (one-hot V rows turn the forward's output into the
mask).  O, dQ, dK, dV: the bounds of tests/test_attention_paths_gpu.py's dropout cases (``Case._mat``: BF16_TOL x max|ref| + the
reference's own sensitivity + the f32 noise of dP - delta), the staged reference taking its delta from the unrounded O, which is what the
delta route's sum_j p w dp is.  LSE: that file's bound, and bit-equal to the plain forward's.  delta: tests/test_attn_exact_delta_gpu.py's
per-row 1e-4 x sum_j p_ij w_ij |dO_i| |v_j|.  The streaming kernels are one f32 expression and one rounding.  Where the expression is a
product of a bf16 value and the f32 factor c it is restated exactly (float64, rounded to f32, then to bf16); the GELU's
forward is held to float64 under the allowance of tests/gelu_domain.py; its backward, which goes through erfc, to half a bf16 ulp of the
float64 value (at most BF16_TOL = 2^-8 |want|), plus F32_TOL |want| for its f32 arithmetic and f32 erfc's absolute error
(``_one_rounding``); both to an exact zero where the restated mask drops.  The embedding gradient is an f32 sum of n bf16 terms in a fixed
order: |got - want| <= n 2^-23 sum |terms|, and the same bits on every run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as A  # noqa: E402
import gelu_domain  # noqa: E402
import w2v_regularise_ref as R  # noqa: E402
from helpers import _lib  # noqa: E402
from test_attention_paths_gpu import E_ALIGN, E_SHAPE, E_UNSUPPORTED, Case, bits, rec, scale_of  # noqa: E402,F401
from test_kernel_forms_gpu import BF16_TOL, F32_TOL  # noqa: E402

BF16 = torch.bfloat16
STATE, SITE, ITEM0 = (77 << 20) + 3, 9, 5
B, H, T = 3, 2, 149
_cases = {}


def _state(v=STATE):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


class DeltaCase(Case):
    """tests/test_attention_paths_gpu.py's problem with the reference of the delta route: delta = sum_j p w dp = dO . O of the
    UNROUNDED O under the mask"""

    def reference(self, scale, keep=None, inv_keep=1.0):
        a = (self.q, self.k, self.v, self.do, self.H, scale, keep, inv_keep)
        o = A.exact(*a)["o"]
        self.ref = A.staged(*a, o_bwd=o)
        self.noisy = A.staged(*a, o_bwd=o, perturb=A.PERTURB, seed=1)
        self.o16 = A.bf16r(self.ref["o"])
        self.lse32 = A.f32r(self.ref["lse"])
        self.noise32 = A.f32_noise(self.q, self.k, self.v, self.do, self.H, scale, o, self.lse32, F32_TOL, keep, inv_keep)


def _attn_case(dh, p):
    """the 3-clip problem, its restated mask and its reference; once per (dh, p)"""
    if (dh, p) not in _cases:
        c = DeltaCase(dh, B, H, T, T, seed=dh + 1)
        th = A.mmf_drop_thresh(p)
        keep = R.probs_keep(STATE, SITE, ITEM0, B, H, T, th) if th else None
        c.reference(scale_of(dh), keep, A.inv_keep_of(th))
        _cases[(dh, p)] = (c, keep, A.inv_keep_of(th))
    return _cases[(dh, p)]


def _drop(p, item0=ITEM0, state=None, site=SITE):
    return (p, _state() if state is None else state, site, item0 * H)


def _run(c, dh, drop, fails, rec_=None, check=True):
    """forward, delta, backward through the keyed entries on ``c``'s buffers -> the six outputs' bits"""
    lib = _lib()
    scale = scale_of(dh)
    lib.attn_fwd_grouped_keyed([c.problem()], dh, scale, drop)
    torch.cuda.synchronize()
    if check:
        c.check_forward(rec_, fails)
    fwd = [bits(c.O.buf), bits(c.LSE.buf)]
    if check:
        c.hand_reference_forward_to_backward()
    lib.attn_delta_keyed([c.problem()], dh, scale, drop)
    lib.attn_bwd_grouped_delta_keyed([c.problem()], dh, scale, drop)
    torch.cuda.synchronize()
    return fwd + [bits(x.buf) for x in (c.delta, c.dQ, c.dK, c.dV)]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dh", [64, 96])
def test_attention_with_dropout_on_the_delta_route_against_float64(rec, dh, p):
    lib = _lib()
    c, keep, inv = _attn_case(dh, p)
    scale, fails = scale_of(dh), []
    out = _run(c, dh, _drop(p), fails, rec)
    # LSE is the undropped one: the plain forward's bits
    plain = Case(dh, B, H, T, T, ops_=(c.q, c.k, c.v, c.do))
    lib.attn_fwd_grouped([plain.problem()], dh, scale)
    torch.cuda.synchronize()
    assert torch.equal(out[1], bits(plain.LSE.buf)), "lse must be the plain forward's bits"
    assert not torch.equal(out[0], bits(plain.O.buf))
    # delta against float64 sum_j p w dp, p from the LSE the kernel was given
    qh, kh, vh, doh = (A.heads(t, H) for t in (c.q, c.k, c.v, c.do))
    P = torch.exp(qh @ kh.transpose(-1, -2) * scale - c.lse32[..., None])
    w = keep.double() * inv
    want = (P * w * (doh @ vh.transpose(-1, -2))).sum(-1)
    size = (P * w * doh.norm(dim=-1, keepdim=True) * vh.norm(dim=-1).unsqueeze(-2)).sum(-1)
    worst = float(((c.delta.host().reshape(B, H, T) - want).abs() / (1e-4 * size)).max())
    rec("delta", worst)
    print(f"attn_delta_f32_keyed dh={dh} p={p}: worst |error| / (1e-4 x sum p w |dO| |v|) = {worst:.3e}")
    assert worst <= 1.0 and c.delta.guards_intact()
    for name, mat, key in (("dQ", c.dQ, "dq"), ("dK", c.dK, "dk"), ("dV", c.dV, "dv")):
        c._mat(rec, fails, "", name, mat, key)
    for name, x in (("O", c.O), ("LSE", c.LSE), ("Q", c.Q), ("K", c.K), ("V", c.V), ("dO", c.dO)):
        if not x.untouched():
            fails.append(f"{name}: changed by the backward")
    assert not fails, "\n".join(fails)
    # two runs give the same bits
    first, second = _run(c, dh, _drop(p), [], check=False), _run(c, dh, _drop(p), [], check=False)
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(first[0], out[0])


@pytest.mark.parametrize("dh", [64, 96])
def test_the_attention_mask_is_the_restated_one_exactly(dh):
    """one-hot V rows, key j -> column j mod dh, the keys taken dh at a time: output element (i, head, j mod dh) is c P_ij where the
    kernel kept pair (i, j) and exactly 0 where it dropped it (P_ij > 0 everywhere: no padding)"""
    lib = _lib()
    p = 0.5
    c, keep, _ = _attn_case(dh, p)
    for j0 in range(0, T, dh):
        keys = torch.arange(j0, min(j0 + dh, T))
        v = torch.zeros(B, T, H, dh, dtype=torch.float64)
        v[:, keys, :, keys - j0] = 1.0
        one = Case(dh, B, H, T, T, ops_=(c.q, c.k, v.reshape(B, T, H * dh), c.do))
        lib.attn_fwd_grouped_keyed([one.problem()], dh, scale_of(dh), _drop(p))
        torch.cuda.synchronize()
        got = one.O.host().reshape(B, T, H, dh).permute(0, 2, 1, 3)[..., :len(keys)] != 0          # [clip, h, i, key - j0]
        want = keep[..., keys]
        assert torch.equal(got, want), f"keys {j0}..: {int((got != want).sum())} of {want.numel()} pairs differ from the restated mask"
        assert bool(want.any()) and not bool(want.all())


@pytest.mark.parametrize("dh", [64, 96])
def test_a_one_clip_launch_at_its_base_is_the_batchs_clip_and_threshold_zero_is_plain(dh):
    lib = _lib()
    p = 0.1
    c, _, _ = _attn_case(dh, p)
    c.hand_reference_forward_to_backward()
    whole = _run(c, dh, _drop(p), [], check=False)
    d = H * dh
    for i in (0, 2):
        one = Case(dh, 1, H, T, T, ops_=tuple(t[i:i + 1] for t in (c.q, c.k, c.v, c.do)))
        one.LSE.v.copy_(c.LSE.v[i * H * T:(i + 1) * H * T])
        got = _run(one, dh, _drop(p, item0=ITEM0 + i), [], check=False)
        rows = lambda m: bits(m.buf[i * T:(i + 1) * T])
        vec = lambda m: bits(m.buf[i * H * T:(i + 1) * H * T])
        want = [rows(c.O), vec(c.LSE), vec(c.delta), rows(c.dQ), rows(c.dK), rows(c.dV)]
        for name, a, b in zip(("O", "LSE", "delta", "dQ", "dK", "dV"), got, want):
            n = b.shape[0]
            assert torch.equal(a[:n], b), f"clip {i}: {name} of the one-clip launch at base (ITEM0 + {i}) H differs from the batch's"
        if i == 2:                                               # another base: another mask
            moved = _run(one, dh, _drop(p, item0=ITEM0), [], check=False)
            assert not torch.equal(moved[0], got[0]) and not torch.equal(moved[3], got[3])
    for other in (_drop(p, site=SITE + 1), _drop(p, state=_state(STATE + 1))):
        assert not torch.equal(_run(c, dh, other, [], check=False)[0], whole[0])
    # threshold 0 through the keyed entries: the plain entries' bits, with or without a state
    scale = scale_of(dh)
    lib.attn_fwd_grouped([c.problem()], dh, scale)
    lib.attn_bwd_grouped_exact_delta([c.problem()], dh, scale)
    torch.cuda.synchronize()
    plain = c.outputs()
    for drop in ((0.0, None, SITE, ITEM0 * H), _drop(0.0)):
        got = _run(c, dh, drop, [], check=False)
        assert all(torch.equal(a, b) for a, b in zip(got, [plain[0], plain[1], plain[2], plain[3], plain[4], plain[5]]))


# ---- the GELU with activation dropout ---------------------------------------------------------------------------------------
def _gelu_grad64(v):
    return 0.5 * (1.0 + torch.erf(v / 2.0 ** 0.5)) + v * torch.exp(-0.5 * v * v) / (2.0 * torch.pi) ** 0.5


def _one_rounding(got, want, keep, erf_term, what):
    """a dropped element is exactly 0; a kept one is within half a bf16 ulp of the float64 value (8 significant bits: half an ulp is
    between 2^-9 and 2^-8 of the value, BF16_TOL = 2^-8 is its worst case), plus F32_TOL of it for the f32 arithmetic, plus ``erf_term``: 2^-22 times what multiplies Phi in the expression
    (the backward's f32 erfc and exp, and the cancellation of its two terms at the derivative's root)"""
    got, want = got.double(), want.double()
    assert bool((got[~keep] == 0).all()), f"{what}: a dropped element is not 0"
    err = (got - want).abs()[keep]
    bound = ((BF16_TOL + F32_TOL) * want.abs() + 2.0 ** -22 * erf_term + 1e-30)[keep]
    print(f"{what}: worst |error| / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("items,Tr,cols", [(3, 149, 512), (2, 5, 8), (1, 33, 3072)])
def test_gelu_with_activation_dropout_forward_and_backward(items, Tr, cols, p):
    lib = _lib()
    th = A.mmf_drop_thresh(p)
    c = A.inv_keep_of(th)
    keep = R.hidden_keep(STATE, SITE, ITEM0, items, Tr * cols, th).reshape(items * Tr, cols)
    g = torch.Generator().manual_seed(items * Tr + cols)
    h = (2.0 * torch.randn(items * Tr, cols, generator=g)).to(BF16)
    bias = 0.3 * torch.randn(cols, generator=g)
    dg = torch.randn(items * Tr, cols, generator=g).to(BF16)
    hd, bd, dgd = h.cuda(), bias.cuda(), dg.cuda()
    drop = (p, _state(), SITE, ITEM0)
    out = torch.full_like(hd, float("nan"))
    lib.bias_gelu_drop_to(hd, bd, out, items, drop)
    v32 = h.float() + bias                                       # the f32 sum the kernel forms, exactly
    got = out.cpu()
    assert bool((got[~keep].float() == 0).all()), "gelu-dropout forward: a dropped element is not 0"
    worst, at, over = gelu_domain.report(f"gelu-dropout forward {items} x {Tr} x {cols} p={p}", gelu_domain.ratio_fwd(got, v32, scale=c)[keep], v32[keep])
    assert over == 0
    v = h.double() + bias.double()
    assert torch.equal(bits(hd), bits(h)), "h must stay raw"
    inplace = hd.clone()
    lib.bias_gelu_drop_to(inplace, bd, inplace, items, drop)
    assert torch.equal(bits(inplace), bits(out))
    dh = torch.full_like(hd, float("nan"))
    lib.bias_gelu_drop_bwd(dgd, hd, bd, dh, items, drop)
    _one_rounding(dh.cpu(), dg.double() * c * _gelu_grad64(v), keep, dg.double().abs() * c, f"gelu-dropout backward {items} x {Tr} x {cols} p={p}")
    # the kept elements are the plain kernels' values times c up to the two roundings; p = 0 IS the plain kernels
    plain, zero = torch.empty_like(hd), torch.empty_like(hd)
    lib.bias_gelu_to(hd, bd, plain)
    lib.bias_gelu_drop_to(hd, bd, zero, items, (0.0, None, SITE, ITEM0))
    assert torch.equal(bits(zero), bits(plain))
    lib.bias_gelu_bwd(dgd, hd, bd, plain)
    lib.bias_gelu_drop_bwd(dgd, hd, bd, zero, items, (0.0, _state(), SITE, ITEM0))
    assert torch.equal(bits(zero), bits(plain))
    if items > 1:                                                # a chunk draws what the batch draws
        part = torch.empty_like(hd[Tr:])
        lib.bias_gelu_drop_to(hd[Tr:], bd, part, items - 1, (p, _state(), SITE, ITEM0 + 1))
        assert torch.equal(bits(part), bits(out[Tr:]))
    torch.cuda.synchronize()


# ---- the span draw ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_,prob,length,mn", [(10, 0.5, 10, 2), (11, 1.0, 10, 0), (149, 0.2, 10, 0), (149, 0.05, 10, 2), (12, 1.0, 1, 0),
                                                 (149, 0.65, 2, 0)])
def test_span_draw_is_the_host_restatement(T_, prob, length, mn):
    """(12, 1.0, 1) fills every place, (149, 0.65, 2) 48 or 49 of 148: both go through the redraws, the first through the probe too"""
    lib = _lib()
    from mmfusion.wav2vec2 import span_slots
    N, item0 = 5, 3
    S = span_slots(T_, prob, length, mn)
    for state in (STATE, STATE + 1, (0x5EED1234 << 32) | 0x9ABCDEF1):
        starts = torch.full((N, S + 1), -7, dtype=torch.int32, device="cuda")          # one slot more than needed: it must read -1
        lib.w2v_mask_spans(starts, T_, prob, length, mn, _state(state), SITE, item0)
        torch.cuda.synchronize()
        want = R.span_table(state, SITE, item0, N, T_, prob, length, mn, S + 1)
        assert torch.equal(starts.cpu(), want), (state, starts.cpu().tolist(), want.tolist())
        assert bool((want[:, 0] >= 0).all()) and bool((want[:, S] == -1).all())


# ---- masking + feature-projection dropout -----------------------------------------------------------------------------------------
def _scale_bf16(x, c):
    """bf16(x c) of a bf16 x and an f32 c: the product is exact in float64, so rounding it to f32 and then to bf16 is the kernel's f32
    multiply and its one rounding"""
    return (x.double() * c).float().to(BF16)


@pytest.mark.parametrize("mask,p", [(True, 0.0), (False, 0.1), (True, 0.1), (True, 0.5)], ids=["mask", "dropout", "both", "both-half"])
def test_mask_and_feature_projection_dropout_forward_and_backward(mask, p):
    lib = _lib()
    items, Tm, d, length = 3, 149, 256, 10
    th = A.mmf_drop_thresh(p)
    c = A.inv_keep_of(th)
    keep = R.hidden_keep(STATE, SITE, ITEM0, items, Tm * d, th).reshape(items * Tm, d) if th else torch.ones(items * Tm, d, dtype=torch.bool)
    table = R.span_table(STATE, SITE + 1, ITEM0, items, Tm, 0.2, length, 2, 4) if mask else None
    span = R.rows_of(table, Tm, length).reshape(-1) if mask else torch.zeros(items * Tm, dtype=torch.bool)
    assert not mask or (bool(span.any()) and not bool(span.all()))
    g = torch.Generator().manual_seed(5)
    x = (1.0 + torch.rand(items * Tm, d, generator=g)).to(BF16)                       # never 0: a zero is a dropped element
    embed = torch.randn(d, generator=g) * 1.2345
    dx = torch.randn(items * Tm, d, generator=g).to(BF16)
    starts = table.cuda() if mask else None
    drop = (p, _state() if th else None, SITE, ITEM0)
    out = torch.full_like(x.cuda(), float("nan"))
    lib.w2v_mask_drop(x.cuda(), out, items, Tm, length, drop, starts, embed.cuda())
    want = torch.where(span[:, None], embed.to(BF16)[None, :], torch.where(keep, _scale_bf16(x, c), torch.zeros_like(x)))
    assert torch.equal(bits(out), bits(want))
    assert torch.equal(bits(out.cpu()[span]), bits(embed.to(BF16)[None, :].expand(int(span.sum()), d))), "a masked row is bf16(embed)"
    inplace = x.cuda()
    lib.w2v_mask_drop(inplace, inplace, items, Tm, length, drop, starts, embed.cuda())
    assert torch.equal(bits(inplace), bits(out))
    # the gradient form: dproj = in_span ? 0 : dx keep c
    dproj = torch.full_like(out, float("nan"))
    lib.w2v_mask_drop(dx.cuda(), dproj, items, Tm, length, drop, starts)
    want = torch.where(span[:, None] | ~keep, torch.zeros_like(dx), _scale_bf16(dx, c))
    assert torch.equal(bits(dproj), bits(want))
    if mask:
        for slabs in (1, 6, 64):
            partial = torch.full((slabs, d), float("nan"), device="cuda")
            lib.w2v_mask_embed_grad(dx.cuda(), starts, partial, items, Tm, length)
            acc = torch.full((d,), 0.5, device="cuda")
            lib.sum_slabs(partial, acc, True)
            again = torch.full((slabs, d), float("nan"), device="cuda")
            lib.w2v_mask_embed_grad(dx.cuda(), starts, again, items, Tm, length)
            torch.cuda.synchronize()
            assert torch.equal(bits(again), bits(partial)), "two runs of the embedding gradient differ"
            rows = dx.double()[span]
            err = (acc.cpu().double() - 0.5 - rows.sum(0)).abs()
            bound = (rows.shape[0] + 1) * 2.0 ** -23 * (rows.abs().sum(0) + 0.5)
            assert bool((err <= bound).all()), float((err / bound).max())
        part = torch.full_like(out[Tm:], float("nan"))                                # a chunk is the batch's clips
        lib.w2v_mask_drop(x.cuda()[Tm:], part, items - 1, Tm, length, (p, drop[1], SITE, ITEM0 + 1), starts[1:], embed.cuda())
        assert torch.equal(bits(part), bits(out[Tm:]))
    torch.cuda.synchronize()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    nan32 = torch.full((1 << 14,), float("nan"), device="cuda")
    b = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    f = torch.zeros(1 << 12, device="cuda")
    ints = torch.full((64,), -5, dtype=torch.int32, device="cuda")
    st = _state()
    P = lambda t, off=0: t.data_ptr() + off

    def prob(**kw):
        a = dict(Q=P(b), K=P(b, 256), V=P(b, 512), O=P(nan16), LSE=P(nan32), dO=P(b), delta=P(nan32, 4096), dQ=P(nan16, 8192), dK=P(nan16, 16384),
                 dV=P(nan16, 32768), B=1, H=2, Tq=8, Tk=8, ldq=384, ldk=384, ldv=384, ldo=128)
        a.update(kw)
        return (lib.AttnProblem * 1)(lib.AttnProblem(*[a[k] for k in ("Q", "K", "V", "O", "LSE", "dO", "delta", "dQ", "dK", "dV", "B", "H", "Tq",
                                                                     "Tk", "ldq", "ldk", "ldv", "ldo")]))
    cases = []
    for fn, name in ((L.mmf_attn_fwd_grouped_keyed, "mmf_attn_fwd_grouped_keyed"), (L.mmf_attn_delta_f32_keyed, "mmf_attn_delta_f32_keyed"),
                     (L.mmf_attn_bwd_grouped_delta_keyed, "mmf_attn_bwd_grouped_delta_keyed")):
        call = lambda pr=0.1, state=P(st), base=0, dh=64, fn=fn, **kw: fn(prob(**kw), 1, dh, 0.125, pr, state, 3, base, s)
        cases += [(name, lambda c=call: c(pr=1.0), E_SHAPE), (name, lambda c=call: c(pr=-0.5), E_SHAPE), (name, lambda c=call: c(state=None), E_SHAPE),
                  (name, lambda c=call: c(state=P(st, 4)), E_ALIGN), (name, lambda c=call: c(Q=P(b, 2)), E_ALIGN), (name, lambda c=call: c(dh=32), E_UNSUPPORTED),
                  (name, lambda c=call: c(base=0xFFFFFFFF), E_SHAPE), (name, lambda c=call: c(Tq=0), E_SHAPE)]
    gelu = lambda pr=0.1, state=P(st), h=P(b), out=P(nan16), rows=8, items=2, cols=64, item0=0, bias=P(f): L.mmf_bias_gelu_drop_bf16_to(
        h, bias, out, rows, cols, cols, items, pr, state, 3, item0, s)
    gelu_bwd = lambda pr=0.1, state=P(st), dg=P(b), out=P(nan16), rows=8, items=2: L.mmf_bias_gelu_drop_bwd_bf16(
        dg, P(b), P(f), out, rows, 64, 64, items, pr, state, 3, 0, s)
    G, Gb = "mmf_bias_gelu_drop_bf16_to", "mmf_bias_gelu_drop_bwd_bf16"
    cases += [(G, lambda: gelu(pr=1.0), E_SHAPE), (G, lambda: gelu(state=None), E_SHAPE), (G, lambda: gelu(state=P(st, 4)), E_ALIGN),
              (G, lambda: gelu(items=3), E_SHAPE), (G, lambda: gelu(item0=-1), E_SHAPE), (G, lambda: gelu(bias=None), E_SHAPE),
              (G, lambda: gelu(out=P(nan16, 2)), E_ALIGN), (G, lambda: gelu(cols=60), E_UNSUPPORTED),
              (Gb, lambda: gelu_bwd(pr=2.0), E_SHAPE), (Gb, lambda: gelu_bwd(state=None), E_SHAPE), (Gb, lambda: gelu_bwd(dg=P(b, 2)), E_ALIGN),
              (Gb, lambda: gelu_bwd(items=0), E_SHAPE)]
    spans = lambda starts=P(ints), N=2, S=4, T_=20, prob_=0.2, length=10, mn=2, state=P(st), item0=0: L.mmf_w2v_mask_spans(
        starts, N, S, T_, prob_, length, mn, state, 3, item0, s)
    Sp = "mmf_w2v_mask_spans"
    cases += [(Sp, lambda: spans(state=None), E_SHAPE), (Sp, lambda: spans(starts=None), E_SHAPE), (Sp, lambda: spans(length=21), E_SHAPE),
              (Sp, lambda: spans(length=0), E_SHAPE), (Sp, lambda: spans(prob_=0.0), E_SHAPE), (Sp, lambda: spans(prob_=1.5), E_SHAPE),
              (Sp, lambda: spans(S=1), E_SHAPE), (Sp, lambda: spans(state=P(st, 4)), E_ALIGN), (Sp, lambda: spans(starts=P(ints, 2)), E_ALIGN),
              (Sp, lambda: spans(item0=-1), E_SHAPE)]
    md = lambda x=P(b), embed=P(f), starts=P(ints), out=P(nan16), items=2, T_=20, d=64, S=4, length=10, pr=0.1, state=P(st), item0=0: L.mmf_w2v_mask_drop(
        x, embed, starts, out, items, T_, d, S, length, pr, state, 3, item0, s)
    Md = "mmf_w2v_mask_drop"
    cases += [(Md, lambda: md(pr=1.0), E_SHAPE), (Md, lambda: md(state=None), E_SHAPE), (Md, lambda: md(x=None), E_SHAPE),
              (Md, lambda: md(length=21), E_SHAPE), (Md, lambda: md(starts=None, pr=0.0), E_SHAPE), (Md, lambda: md(d=60), E_UNSUPPORTED),
              (Md, lambda: md(out=P(nan16, 2)), E_ALIGN), (Md, lambda: md(state=P(st, 4)), E_ALIGN), (Md, lambda: md(embed=P(f, 2)), E_ALIGN),
              (Md, lambda: md(item0=-2), E_SHAPE)]
    eg = lambda dx=P(b), starts=P(ints), partial=P(nan32), items=2, T_=20, d=64, S=4, length=10, slabs=4: L.mmf_w2v_mask_embed_grad(
        dx, starts, partial, items, T_, d, S, length, slabs, s)
    Eg = "mmf_w2v_mask_embed_grad"
    cases += [(Eg, lambda: eg(starts=None), E_SHAPE), (Eg, lambda: eg(slabs=0), E_SHAPE), (Eg, lambda: eg(slabs=65), E_SHAPE),
              (Eg, lambda: eg(length=0), E_SHAPE), (Eg, lambda: eg(partial=P(nan32, 2)), E_ALIGN), (Eg, lambda: eg(dx=P(b, 1)), E_ALIGN)]
    for name, call, want in cases:
        rc = call()
        assert rc == want, (name, rc, want, L.mmf_last_error())
        assert name.encode() in L.mmf_last_error(), (name, L.mmf_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all()) and bool((ints == -5).all())      # nothing was launched
    assert int(st.item()) == STATE
