"""GPU: the three kernels of csrc/bert.hip against float64 / exact host restatements (tests/bert_ref.py).

``mmf_attn_fwd_keymask`` against ``bert_ref.keymask_staged`` (tests/attn_ref.py's staged forward with masked keys dropped, the
empty-item rule and skipped blocks): B = 3 items, H = 2, Q / K / V in one fused (rows, 3 d) buffer, one mask family per item.  The
K and V rows of masked keys hold 3e4, which the restatement never reads, so a leak of any size shows.  The bounds are the plain
forward's (tests/test_attention_paths_gpu.py): O within BF16_TOL x max|ref| plus the restatement's own sensitivity to scores
perturbed by 2^-22; LSE within F32_TOL x max(|ref|, 1).  Every masked case must differ from the unmasked restatement by more than
10 x BF16_TOL x max|ref|.  With all ones (and with no mask at all) the same bounds hold against the PLAIN restatement.  T: one key,
a ragged block, exactly one block, one block and a key, one tile, a tile and a key, a ragged second tile, two query chunks (129 ->
a wave that only stages), a fourth tile (193).
``mmf_mask_pack`` against ``bert_ref.pack_ref``, exactly.  ``mmf_bert_embed`` against float64 at the bound of
tests/test_deberta_gpu.py's embedding test (one bf16 ulp of the reference).
Outputs are pre-filled with NaN; guard rows, guard columns and guard elements must come back bit-identical, as must the inputs."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as R  # noqa: E402
import bert_ref  # noqa: E402
from mmfusion import lib  # noqa: E402
from test_attention_paths_gpu import E_ALIGN, E_SHAPE, E_UNSUPPORTED, Mat, Vec, bits, scale_of  # noqa: E402
from test_deberta_gpu import _bf16_ulp  # noqa: E402
from test_kernel_forms_gpu import BF16_TOL, DEV, F32_TOL  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TS = (1, 31, 32, 33, 64, 65, 97, 129, 193)
B, H = 3, 2
BIG = 3.0e4
GUARD = 0x5A5A5A5A


# ---- the mask families -------------------------------------------------------------------------------------------
def _ones(T):
    return torch.ones(T, dtype=torch.bool)


def _tail(T, L):
    v = torch.zeros(T, dtype=torch.bool)
    v[:L] = True
    return v


def _tail_mid_block(T):
    L = (2 * T) // 3
    L -= 1 if L % 32 == 0 else 0
    return _tail(T, L) if 1 <= L < T else None


def _tail_on_boundary(T):
    L = 32 * ((T - 1) // 32)
    return _tail(T, L) if L >= 32 else None


def _tail_whole_tile(T):
    return _tail(T, 40) if T >= 129 else None                  # tiles 1 .. are behind the last valid key


def _hole_one(T):
    if T < 2:
        return None
    v = _ones(T)
    v[T // 2] = False
    return v


def _hole_block(T):
    if T < 65:
        return None
    v = _ones(T)
    v[32:64] = False
    return v


def _first_masked(T):
    if T < 2:
        return None
    v = _ones(T)
    v[0] = False
    return v


def _last_only(T):
    if T < 2:
        return None
    v = torch.zeros(T, dtype=torch.bool)
    v[T - 1] = True
    return v


def _empty(T):
    return torch.zeros(T, dtype=torch.bool)


FAMILIES = (_tail_mid_block, _tail_on_boundary, _tail_whole_tile, _hole_one, _hole_block, _first_masked, _last_only, _empty)


def mask_groups(T):
    """the families that exist at ``T``, three per case (one per item); a short last group is filled with all ones, and the empty
    item always stands beside a full one"""
    rows = [(f.__name__, f(T)) for f in FAMILIES if f(T) is not None]
    groups = []
    for i in range(0, len(rows), 3):
        g = rows[i:i + 3]
        while len(g) < 3:
            g.append(("_ones", _ones(T)))
        groups.append(g)
    if not any(n == "_ones" for n, _ in groups[-1]) and any(n == "_empty" for n, _ in groups[-1]):
        groups[-1][0], extra = ("_ones", _ones(T)), groups[-1][0]
        groups.append([extra, ("_ones", _ones(T)), ("_ones", _ones(T))])
    return groups


CASES = [(T, g) for T in TS for g in range(len(mask_groups(T)))]


def test_every_family_is_exercised():
    seen = {n for T in TS for g in mask_groups(T) for n, _ in g}
    assert seen == {f.__name__ for f in FAMILIES} | {"_ones"}
    for T in TS:
        for g in mask_groups(T):
            assert len(g) == 3 and (not any(n == "_empty" for n, _ in g) or any(n == "_ones" for n, _ in g))
    assert int(_tail_mid_block(97).sum()) == 63 and int(_tail_on_boundary(97).sum()) == 96 and int(_tail_whole_tile(193).sum()) == 40


class IntVec:
    """n int32 values followed by guard elements"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 16,), GUARD, dtype=torch.int32, device=DEV)
        self.v = self.buf[:n]

    def guards_intact(self):
        return bool((self.buf[self.n:] == GUARD).all())


class Masked:
    """one self-attention problem read from a fused (B T, 3 d) buffer under a (B, T) key mask, with guards around everything"""

    def __init__(self, dh, T, valid, seed, kind):
        self.dh, self.T, self.valid, self.kind = dh, T, valid, kind
        d = self.d = H * dh
        g = torch.Generator().manual_seed(seed)
        qkv = R.bf16r(torch.randn(B, T, 3 * d, generator=g, dtype=F64))
        dead = ~valid & valid.any(dim=1, keepdim=True)         # masked keys of an item that has valid ones
        qkv[..., d:][dead] = R.bf16r(torch.tensor(BIG, dtype=F64))
        self.qkv = qkv
        self.QKV = Mat(B * T, 3 * d, 3 * d + 8, 8, qkv)
        self.O, self.LSE = Mat(B * T, d, d + 16, 8), Vec(B * H * T)
        self.mask = None if kind == "none" else valid.to(F32 if kind == "f32" else torch.uint8).to(DEV)
        if kind == "f32":
            self.mask = self.mask * 2.5                        # any non-zero value is valid
        self.mask_before = None if self.mask is None else self.mask.clone()
        self.P = IntVec(B * lib.mask_pack_words(T))
        lib.mask_pack(self.mask, self.P.v, B, T)

    def problem(self, **over):
        d, ld = self.d, 3 * self.d + 8
        f = dict(Q=self.QKV.ptr, K=self.QKV.ptr + 2 * d, V=self.QKV.ptr + 4 * d, O=self.O.ptr, LSE=self.LSE.ptr, B=B, H=H,
                 Tq=self.T, Tk=self.T, ldq=ld, ldk=ld, ldv=ld, ldo=d + 16)
        f.update(over)
        return lib.AttnProblem(f["Q"], f["K"], f["V"], f["O"], f["LSE"], None, None, None, None, None, f["B"], f["H"], f["Tq"], f["Tk"],
                               f["ldq"], f["ldk"], f["ldv"], f["ldo"])

    def run(self):
        lib.attn_fwd_keymask(self.problem(), self.dh, scale_of(self.dh), self.P.v)

    def qkv_parts(self):
        d = self.d
        return self.qkv[..., :d], self.qkv[..., d:2 * d], self.qkv[..., 2 * d:]

    def check(self, ref, noisy, tag):
        fails = []
        o, got = ref["o"].reshape(-1, self.d), self.O.host()
        bound = BF16_TOL * float(o.abs().max()) + float((ref["o"] - noisy["o"]).abs().max())
        err = float((got - o).abs().max()) if bool(torch.isfinite(got).all()) else math.inf
        print(f"PARITY {tag} O: err / bound {err / bound:.3f}")
        if not err <= bound:
            bad = (~((got - o).abs() <= bound)).nonzero()
            fails.append(f"{tag} O: err {err:.4g} > bound {bound:.4g}; {len(bad)} elements, first (row, col) {bad[0].tolist()}")
        lse, got = ref["lse"].reshape(-1), self.LSE.host()
        bound = F32_TOL * max(float(lse.abs().max()), 1.0)
        err = float((got - lse).abs().max()) if bool(torch.isfinite(got).all()) else math.inf
        print(f"PARITY {tag} LSE: err / bound {err / bound:.3f}")
        if not err <= bound:
            fails.append(f"{tag} LSE: err {err:.4g} > bound {bound:.4g}, first {int((~((got - lse).abs() <= bound)).nonzero()[0])}")
        if not (self.O.guards_intact() and self.LSE.guards_intact() and self.P.guards_intact()):
            fails.append(f"{tag}: guards around O / LSE / the packed mask changed")
        if not (self.QKV.untouched() and (self.mask is None or torch.equal(self.mask, self.mask_before))):
            fails.append(f"{tag}: an input changed")
        return fails


# ---- mmf_attn_fwd_keymask ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("dh", [64, 96])
@pytest.mark.parametrize("T,g", CASES)
def test_keymask_forward_against_staged_float64(T, g, dh, kind):
    group = mask_groups(T)[g]
    valid = torch.stack([v for _, v in group])
    c = Masked(dh, T, valid, seed=7 * T + dh + 1000 * g, kind=kind)
    scale = scale_of(dh)
    c.run()
    first = bits(c.O.buf).clone(), bits(c.LSE.buf).clone()
    q, k, v = c.qkv_parts()
    ref = bert_ref.keymask_staged(q, k, v, H, scale, valid)
    noisy = bert_ref.keymask_staged(q, k, v, H, scale, valid, perturb=R.PERTURB, seed=1)
    tag = f"keymask dh={dh} T={T} {kind} [{', '.join(n for n, _ in group)}]"
    assert bool(torch.isfinite(ref["o"]).all()) and bool(torch.isfinite(ref["lse"]).all())
    if T > 1:                                                                  # the mask matters in this case
        plain = R.staged(q, k, v, torch.zeros_like(q), H, scale)
        assert float((ref["o"] - plain["o"]).abs().max()) > 10 * BF16_TOL * float(ref["o"].abs().max()), tag
    for b, (name, _) in enumerate(group):
        if name == "_empty":                                                   # the uniform row: the mean of the T value rows, ln T
            assert float((ref["o"][b] - v[b].mean(dim=0)).abs().max()) <= 2 ** -7 * float(v[b].abs().max())
            assert float((ref["lse"][b] - math.log(T)).abs().max()) <= 1e-9
    fails = c.check(ref, noisy, tag)
    assert not fails, "\n".join(fails)
    c.run()                                                                    # no atomics: the same bits again
    assert torch.equal(bits(c.O.buf), first[0]) and torch.equal(bits(c.LSE.buf), first[1])


@pytest.mark.parametrize("kind", ["none", "f32", "u8"])
@pytest.mark.parametrize("dh", [64, 96])
@pytest.mark.parametrize("T", TS)
def test_keymask_forward_with_all_ones_is_the_plain_attention(T, dh, kind):
    c = Masked(dh, T, torch.ones(B, T, dtype=torch.bool), seed=11 * T + dh, kind=kind)
    scale = scale_of(dh)
    c.run()
    q, k, v = c.qkv_parts()
    z = torch.zeros_like(q)
    ref, noisy = R.staged(q, k, v, z, H, scale), R.staged(q, k, v, z, H, scale, perturb=R.PERTURB, seed=1)
    fails = c.check(ref, noisy, f"all ones ({kind}) dh={dh} T={T}")
    assert not fails, "\n".join(fails)


# ---- mmf_mask_pack --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "f32", "u8", "bool"])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 65, 193])
def test_mask_pack_is_exactly_the_host_restatement(T, kind):
    n = 5
    g = torch.Generator().manual_seed(100 + T)
    valid = torch.rand(n, T, generator=g) > 0.4
    valid[1] = True
    valid[2] = False                                           # an empty item
    valid[3] = False
    valid[3, T - 1] = True                                     # only the last key
    valid[4, T // 2:] = False                                  # a tail
    if kind == "none":
        mask, valid = None, torch.ones(n, T, dtype=torch.bool)
    elif kind == "f32":
        mask = torch.where(valid, torch.randn(n, T, generator=g).abs() + 0.5, torch.zeros(n, T)).to(DEV)
        mask[1, 0] = -1.0                                      # any non-zero value is valid
    else:
        mask = valid.to(torch.uint8 if kind == "u8" else torch.bool).to(DEV)
        if kind == "u8":
            mask[1, 0] = 255
    words = lib.mask_pack_words(T)
    out, again = IntVec(n * words), IntVec(n * words)
    before = None if mask is None else mask.clone()
    for o in (out, again):
        lib.mask_pack(mask, o.v, n, T)
    want = bert_ref.pack_ref(valid, n, T)
    got = out.v.cpu().to(torch.int64).reshape(n, words) & 0xffffffff
    assert torch.equal(got, want), (got, want)
    if kind != "none":
        assert want[2].tolist() == [0] * words and want[3, :2].tolist() == [T, 1]
    assert torch.equal(out.buf, again.buf) and out.guards_intact()
    assert mask is None or torch.equal(mask, before)


# ---- mmf_bert_embed -----------------------------------------------------------------------------------------------------
def _ids_with_pads(n, T, vocab, pad, g):
    """item 0: pads at the front and in the middle, ids beyond the vocabulary on both sides; item 1: pads at the end; item 2 (where
    there is one): a whole item of pads"""
    ids = torch.randint(0, vocab, (n, T), generator=g)
    ids[ids == pad] = (pad + 1) % vocab
    ids[0, :max(1, T // 5)] = pad
    if T > 4:
        ids[0, T // 2:T // 2 + max(1, T // 7)] = pad
        ids[0, T // 2 - 1], ids[0, T - 2], ids[0, T - 1] = vocab + 7, -3, 1 << 40     # clamped to the table's ends
    ids[1, T - max(1, T // 4):] = pad
    if n > 2:
        ids[2] = pad
    return ids


@pytest.mark.parametrize("route", ["ids", "embeds"])
@pytest.mark.parametrize("rule", ["bert", "roberta"])
@pytest.mark.parametrize("T,d,n", [(1, 256, 5), (33, 132, 5), (65, 768, 5), (130, 1024, 5)])
def test_embed_within_one_bf16_ulp_of_float64_and_bit_repeatable(T, d, n, rule, route):
    """Shapes: T = 1, 65 and 130 (one, two and three 64-id loads of RoBERTa's count) and every column form of the row (one
    256-column chunk, a partial one, three, four).  The bound is relative to the bf16 spacing AT THE REFERENCE VALUE, so among
    the 665,600 outputs of the largest case it also holds the kernel at outputs that fall within 1e-6 of zero, where a float32
    LayerNorm (torch's own too) is several spacings off: the kernel carries the row in f64 for that reason."""
    vocab, ntype, pad = 37, 3, 1 if rule == "roberta" else 0
    npos = T + pad + 1 if route == "embeds" or rule == "bert" else T + pad - 2        # RoBERTa ids route: the last positions clamp
    npos = max(npos, 1)
    g = torch.Generator().manual_seed(17 * T + d)
    word, pos, typ = (torch.randn(r, d, generator=g) * s + 0.1 for r, s in ((vocab, 2.0), (npos, 1.0), (ntype, 1.0)))
    gamma, beta = 1.0 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    eps = 1e-5 if rule == "roberta" else 1e-12
    ids = _ids_with_pads(n, T, vocab, pad, g)
    tt = torch.randint(0, ntype, (n, T), generator=g)
    tt[0, 0] = ntype + 2                                       # clamped
    emb = torch.randn(n, T, d, generator=g)
    if route == "ids":
        rows = word[bert_ref.clamp_ids(ids, vocab)]
        p = bert_ref.position_ids(ids, rule, pad)
    else:
        rows, p = emb, bert_ref.embeds_position_ids(n, T, rule, pad)
    pc = bert_ref.clamp_ids(p, npos)
    if rule == "roberta" and route == "ids" and T > 4:
        assert bool((p != pc).any()) and (n < 3 or int(p[2].max()) == pad)     # positions clamp; a whole item of pads sits at pad
    for types_ in (tt, None):
        trow = typ[bert_ref.clamp_ids(tt, ntype)] if types_ is not None else typ[0].expand(n, T, d)
        want = bert_ref.embed_ref(rows.double(), pos[pc].double(), trow.double(), gamma.double(), beta.double(), eps).reshape(n * T, d)
        out = [torch.full((n * T + 2, d), float("nan"), dtype=BF16, device=DEV) for _ in range(2)]
        c = lambda t: None if t is None else t.to(DEV)
        ins = [c(word), c(pos), c(typ), c(gamma), c(beta), c(ids.reshape(-1)), c(emb), c(None if types_ is None else types_.reshape(-1))]
        keep = [None if t is None else t.clone() for t in ins]
        for o in out:
            lib.bert_embed(o[:n * T], ins[0], ins[1], ins[2], ins[3], ins[4], eps, T, rule, pad,
                           ids=ins[5] if route == "ids" else None, embeds=ins[6] if route == "embeds" else None, token_type_ids=ins[7])
        got = out[0][:n * T].cpu().double()
        worst = float(((got - want).abs() / _bf16_ulp(want.float()).double()).max()) if bool(torch.isfinite(got).all()) else math.inf
        print(f"bert embed ({rule}, {route}, types {'given' if types_ is not None else 'null'}) T={T} d={d}: worst error / bf16 ulp = {worst:.3f}")
        assert worst <= 1.0
        assert torch.equal(bits(out[0]), bits(out[1])) and bool(torch.isnan(out[0][n * T:]).all())
        assert all(a is None or torch.equal(a, b) for a, b in zip(ins, keep))


def test_embed_position_rules_differ_where_they_should():
    """a position table whose rows are far apart: BERT and RoBERTa positions, and ids against embeds, give different rows exactly
    where the rules differ"""
    n, T, d, vocab, pad = 2, 70, 256, 9, 1
    g = torch.Generator().manual_seed(3)
    word, typ = torch.randn(vocab, d, generator=g), torch.zeros(1, d)
    pos = torch.randn(T + 4, d, generator=g) * 3.0
    ids = torch.randint(2, vocab, (n, T), generator=g)
    ids[0, 10:20] = pad
    ones, zeros = torch.ones(d), torch.zeros(d)
    run = {}
    for rule in ("bert", "roberta"):
        out = torch.empty(n * T, d, dtype=BF16, device=DEV)
        lib.bert_embed(out, word.to(DEV), pos.to(DEV), typ.to(DEV), ones.to(DEV), zeros.to(DEV), 1e-5, T, rule, pad, ids=ids.reshape(-1).to(DEV))
        run[rule] = out.cpu().float().reshape(n, T, d)
    for rule in ("bert", "roberta"):
        p = bert_ref.position_ids(ids, rule, pad)
        want = bert_ref.layer_norm((word[ids] + pos[p]).double(), ones.double(), zeros.double(), 1e-5)
        assert float((run[rule].double() - want).abs().max()) <= 2 ** -7 * float(want.abs().max())
    assert not torch.equal(run["bert"], run["roberta"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_documented_codes_and_launch_nothing():
    import ctypes
    L = lib.load()
    s = lib.stream_ptr()
    c = Masked(64, 40, torch.ones(B, 40, dtype=torch.bool), seed=3, kind="u8")
    packed_before = c.P.buf.clone()
    pp = c.P.buf.data_ptr()
    att = lambda p, dh=64, packed=pp: L.mmf_attn_fwd_keymask(p, dh, 0.125, packed, s)
    ref = lambda **over: ctypes.byref(c.problem(**over))
    pout = IntVec(B * lib.mask_pack_words(40))
    m8, m32 = torch.ones(B * 40 + 8, dtype=torch.uint8, device=DEV), torch.ones(B * 40 + 8, device=DEV)
    P = lambda t, off=0: t.data_ptr() + off
    pack = lambda mask=P(m8), kind=2, out=pout.buf.data_ptr(), n=B, T=40: L.mmf_mask_pack(mask, kind, out, n, T, s)
    f = torch.zeros(1 << 14, device=DEV)
    ids = torch.zeros(64, dtype=torch.int64, device=DEV)
    eout = torch.full((1 << 14,), float("nan"), dtype=BF16, device=DEV)

    def embed(ids_=P(ids), emb=None, tt=None, word=P(f), pos=P(f), typ=P(f), gamma=P(f), out=P(eout), rows=8, T=4, d=256, vocab=16, npos=8,
              ntype=2, rule=0):
        return L.mmf_bert_embed(ids_, emb, tt, word, pos, typ, gamma, P(f), 1e-5, rule, 0, out, rows, T, d, vocab, npos, ntype, s)
    cases = [
        ("mmf_attn_fwd_keymask", lambda: att(None), E_SHAPE),
        ("mmf_attn_fwd_keymask", lambda: att(ref(Q=None)), E_SHAPE),
        ("mmf_attn_fwd_keymask", lambda: att(ref(O=None)), E_SHAPE),
        ("mmf_attn_fwd_keymask", lambda: att(ref(LSE=None)), E_SHAPE),
        ("mmf_attn_fwd_keymask", lambda: att(ref(), packed=None), E_SHAPE),
        ("mmf_attn_fwd_keymask", lambda: att(ref(Tk=39)), E_SHAPE),
        ("mmf_attn_fwd_keymask", lambda: att(ref(Tq=41)), E_SHAPE),
        ("mmf_attn_fwd_keymask", lambda: att(ref(B=0)), E_SHAPE),
        ("mmf_attn_fwd_keymask", lambda: att(ref(K=c.QKV.ptr + 2 * c.d + 2)), E_ALIGN),
        ("mmf_attn_fwd_keymask", lambda: att(ref(ldq=3 * c.d + 4)), E_ALIGN),
        ("mmf_attn_fwd_keymask", lambda: att(ref(ldo=c.d - 8)), E_ALIGN),
        ("mmf_attn_fwd_keymask", lambda: att(ref(), packed=pp + 4), E_ALIGN),
        ("mmf_attn_fwd_keymask", lambda: att(ref(), dh=128), E_UNSUPPORTED),
        ("mmf_attn_fwd_keymask", lambda: att(ref(), dh=32), E_UNSUPPORTED),
        ("mmf_mask_pack", lambda: pack(mask=None), E_SHAPE),                   # a kind without a mask
        ("mmf_mask_pack", lambda: pack(kind=0), E_SHAPE),                      # a mask without a kind
        ("mmf_mask_pack", lambda: pack(kind=3), E_SHAPE),
        ("mmf_mask_pack", lambda: pack(out=None), E_SHAPE),
        ("mmf_mask_pack", lambda: pack(n=0), E_SHAPE),
        ("mmf_mask_pack", lambda: pack(T=0), E_SHAPE),
        ("mmf_mask_pack", lambda: pack(mask=P(m32, 2), kind=1), E_ALIGN),
        ("mmf_mask_pack", lambda: pack(out=pout.buf.data_ptr() + 4), E_ALIGN),
        ("mmf_bert_embed", lambda: embed(emb=P(f)), E_SHAPE),                  # both ids and embeds
        ("mmf_bert_embed", lambda: embed(ids_=None), E_SHAPE),                 # neither
        ("mmf_bert_embed", lambda: embed(word=None), E_SHAPE),                 # ids without a table
        ("mmf_bert_embed", lambda: embed(pos=None), E_SHAPE),
        ("mmf_bert_embed", lambda: embed(typ=None), E_SHAPE),
        ("mmf_bert_embed", lambda: embed(rows=0), E_SHAPE),
        ("mmf_bert_embed", lambda: embed(rows=7), E_SHAPE),                    # not a multiple of T
        ("mmf_bert_embed", lambda: embed(rule=2), E_SHAPE),
        ("mmf_bert_embed", lambda: embed(npos=0), E_SHAPE),
        ("mmf_bert_embed", lambda: embed(d=2048), E_UNSUPPORTED),
        ("mmf_bert_embed", lambda: embed(d=250), E_UNSUPPORTED),
        ("mmf_bert_embed", lambda: embed(ids_=None, emb=P(f, 4)), E_ALIGN),
        ("mmf_bert_embed", lambda: embed(out=P(eout, 2)), E_ALIGN),
        ("mmf_bert_embed", lambda: embed(ids_=P(ids, 4)), E_ALIGN),
        ("mmf_bert_embed", lambda: embed(tt=P(ids, 4)), E_ALIGN),
    ]
    for name, call, want in cases:
        rc = call()
        assert rc == want, (name, rc, want, L.mmf_last_error())
        assert name.encode() in L.mmf_last_error()
    torch.cuda.synchronize()
    assert c.O.untouched() and c.LSE.untouched()                                       # still NaN: nothing was launched
    assert bool(torch.isnan(c.O.v).all()) and bool(torch.isnan(c.LSE.v).all()) and bool(torch.isnan(eout).all())
    assert bool((pout.buf == GUARD).all()) and torch.equal(c.P.buf, packed_before)
