"""GPU: the seven entry points on the disentangled-attention body of csrc/deberta.hip (mmf_deberta_attn_fwd, _fwd_lse, _fwd_drop;
_bwd, _bwd_drop; _bwd_pos, _bwd_pos_drop), element by element against the staged float64 restatement of
tests/deberta_attn_staged_ref.py.  That module's docstring lists the staging points with their lines in deberta.hip and derives
every bound; tests/test_deberta_attn_staged_cpu.py shows that the bounds see a fault confined to one window, which the
whole-tensor norms of the older DeBERTa tests do not.

Each kernel is checked in isolation: the forward's O and lse on their own; the backward is handed the REFERENCE's O (bf16) and lse
(f32), so a forward error can neither mask nor mimic a backward one.

Conventions (tests/test_attention_paths_gpu.py): operands from a seeded generator, rounded to bf16; every output pre-filled with
NaN; guard rows behind qkv / out / dout / dqkv, guard elements behind lse / delta_ws / the position workspace, guard columns beside
posq | posk and dposq | dposk, which are column slices of wider buffers (ld_pos = 2 d + 24, ld_dpos = 2 d + 12: neither is H 64;
every view 16-byte aligned); all guards and all inputs come back bit-identical; two runs are bit-equal; the position workspace is
handed over NaN-filled (lib.deberta_attn_bwd_pos: it need not be initialised).

Bounds, element-wise (deberta_attn_staged_ref.bounds; BF16_TOL = 2^-8 and F32_TOL = 1e-5 are tests/test_kernel_forms_gpu.py's):
  O, dQ, dK, dV   BF16_TOL max|ref| over the (item, head) slice + N (N: the reference's sensitivity to a relative 2^-22 on every
                  score; for dQ / dK also the element's f32 summation noise of dP - delta)
  lse             F32_TOL max(|ref|, 1), unmasked query rows only
  delta_ws        per row F32_TOL sum|O dO| of the operands given
  dposQ, dposK    per element BF16_TOL sum|bucket sum| |own vector element| + the element's f32-noise term; where the entry adds
                  to something (a non-zero fill; a chunk after the first), one f32 rounding of that sum: 2^-24 (|fill| + |ref|)
A table row no unmasked pair reaches keeps the bits it held.  Every worst error / bound ratio is printed as a PARITY line before
anything is asserted (profiles/deberta_attention_parity.txt is those lines from an MI355X).  No term was added beyond these.  Measured
there, worst error / bound: dQ 0.95, dV 0.87, O 0.87, dK 0.86 (outputs the kernels round to bf16 once: half an ulp of a slice's
largest element is by itself up to 1.0 of BF16_TOL max|ref|), dposQ 0.23, dposK 0.13, lse 0.012, delta 0.007.

Every index table handed to a kernel satisfies the contract (deberta_attn_staged_ref.contract_ok, asserted per problem)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref  # noqa: E402
import deberta_attn_staged_ref as R  # noqa: E402
import deberta_dropout_ref as D  # noqa: E402
from mmfusion import lib  # noqa: E402
from test_attention_paths_gpu import GELEMS, GROWS, SENTINEL, SITE, STATE, rec  # noqa: E402,F401  (rec: the PARITY fixture)
from test_deberta_grad_gpu import _bits, _heads  # noqa: E402
from test_kernel_forms_gpu import BF16_TOL, DEV, F32_TOL, NAN  # noqa: E402

assert (BF16_TOL, F32_TOL) == (R.BF16_TOL, R.F32_TOL)
BF16, F32 = torch.bfloat16, torch.float32
ITEM0 = 3                                   # the index, in a larger batch, of a dropout call's first item
_refs = {}


def reference(name, mask_kind=None, p=0.0, item0=ITEM0):
    """the problem and its staged reference with bounds, computed once; p > 0: the keep mask of the host restatement"""
    key = (name, mask_kind, p, item0 if p else 0)
    if key not in _refs:
        pr = R.problem(name, mask_kind)
        w = None
        if p:
            thresh = attn_ref.mmf_drop_thresh(p)
            w = D.probs_keep(STATE, SITE, item0, pr.n, pr.H, pr.T, thresh).to(torch.float64) * attn_ref.inv_keep_of(thresh)
        _refs[key] = (pr, dict(R.reference(*pr.args, pr.dO, w), w=w))
    return _refs[key]


class Buf:
    """a SENTINEL-filled buffer whose windows (tuples of slices) are the live regions: ``values`` copied in, or ``fill``"""

    def __init__(self, shape, dtype, wins, values=None, fill=NAN):
        self.buf = torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
        self.wins = wins
        self.views = [self.buf[w] for w in wins]
        for i, v in enumerate(self.views):
            if values is None:
                v.fill_(fill)
            else:
                v.copy_(values[i].reshape(v.shape).to(dtype))
        self.mark()

    def mark(self):
        self.before = _bits(self.buf)

    def untouched(self):
        return bool(torch.equal(_bits(self.buf), self.before))

    def guards_intact(self):
        guard = torch.ones(self.buf.shape, dtype=torch.bool)
        for w in self.wins:
            guard[w] = False
        return bool(torch.equal(_bits(self.buf)[guard], self.before[guard]))

    def host(self, i=0):
        return self.views[i].detach().cpu().double()


class Dev:
    """the device side of one problem; ``lo:hi`` an item range (a chunk of the batch: row slices of the same operands)"""

    def __init__(self, pr, ref, mask_dtype=F32, dpos_fill=None):
        self.pr, self.ref = pr, ref
        n, H, T, S, d = pr.n, pr.H, pr.T, pr.S, pr.d
        rows = (slice(0, n * T), slice(None))
        mat = lambda cols, values=None: Buf((n * T + GROWS, cols), BF16, [rows], None if values is None else [values])
        vec = lambda values=None: Buf((n * H * T + GELEMS,), F32, [(slice(0, n * H * T),)], None if values is None else [values])
        self.qkv, self.dout = mat(3 * d, pr.qkv), mat(d, pr.dout)
        self.out, self.dqkv = mat(d), mat(3 * d)
        self.o16 = mat(d, R.rows_of(ref["o16"]))
        self.lse, self.delta, self.lse32 = vec(), vec(), vec(ref["lse32"])
        r2 = slice(0, 2 * S)
        self.pos = Buf((2 * S + GROWS, 2 * d + 24), BF16, [(r2, slice(8, 8 + d)), (r2, slice(16 + d, 16 + 2 * d))], [pr.posq, pr.posk])
        self.fill = torch.zeros(2, 2 * S, d) if dpos_fill is None else dpos_fill
        self.dpos = Buf((2 * S + GROWS, 2 * d + 12), F32, [(r2, slice(4, 4 + d)), (r2, slice(8 + d, 8 + 2 * d))], list(self.fill))
        need = lib.deberta_attn_bwd_pos_workspace_bytes(n, H, T, S)
        self.ws = Buf((need // 4 + GELEMS,), F32, [(slice(0, need // 4),)])
        self.idx = pr.idx.to(DEV)
        self.mask = None if pr.mask is None else pr.mask.to(mask_dtype).to(DEV)
        assert self.pos.buf.stride(0) % 8 == 0 and self.pos.buf.stride(0) != d and self.dpos.buf.stride(0) % 4 == 0 and self.dpos.buf.stride(0) != d
        for v in self.pos.views + self.dpos.views + [self.qkv.buf, self.out.buf, self.dqkv.buf, self.dout.buf, self.o16.buf, self.ws.buf]:
            assert v.data_ptr() % 16 == 0
        self.inputs_fwd = [("qkv", self.qkv), ("pos", self.pos)]
        self.inputs_bwd = self.inputs_fwd + [("dout", self.dout), ("o16", self.o16), ("lse32", self.lse32)]

    def _chunk(self, lo, hi):
        pr = self.pr
        T, H = pr.T, pr.H
        r = lambda b: b.buf[lo * T:]
        e = lambda b: b.buf[lo * H * T:]
        return r, e, None if self.mask is None else self.mask[lo:hi].contiguous(), (hi - lo, H, T, pr.S, R.SCALE)

    def forward(self, lse=True, drop=None, lo=0, hi=None):
        r, e, m, dims = self._chunk(lo, self.pr.n if hi is None else hi)
        lib.deberta_attn_fwd(r(self.qkv), self.pos.views[0], self.pos.views[1], self.idx, m, r(self.out), *dims,
                             lse=e(self.lse) if lse else None, drop=drop)
        torch.cuda.synchronize()

    def backward(self, pos=True, drop=None, lo=0, hi=None):
        r, e, m, dims = self._chunk(lo, self.pr.n if hi is None else hi)
        a = (r(self.qkv), self.pos.views[0], self.pos.views[1], self.idx, m, r(self.o16), e(self.lse32), r(self.dout), e(self.delta), r(self.dqkv))
        if pos:
            lib.deberta_attn_bwd_pos(*a, self.dpos.views[0], self.dpos.views[1], self.ws.buf, *dims, drop=drop)
        else:
            lib.deberta_attn_bwd(*a, *dims, drop=drop)
        torch.cuda.synchronize()

    def inputs_untouched(self, which, fails, tag):
        for name, b in which:
            if not b.untouched():
                fails.append(f"{tag}{name}: an input changed")
        if not torch.equal(self.idx.cpu(), self.pr.idx):
            fails.append(f"{tag}idx changed")
        if self.mask is not None and not torch.equal(self.mask.cpu().double(), self.pr.mask.double()):
            fails.append(f"{tag}mask changed")

    def forward_bits(self):
        return [_bits(self.out.buf), _bits(self.lse.buf)]

    def backward_bits(self):
        return [_bits(self.dqkv.buf), _bits(self.delta.buf), _bits(self.dpos.buf)]


def _held(rec, fails, name, got, want, bound, where=None):
    """element-wise |got - want| <= bound (on ``where``); the worst ratio goes to ``rec`` whatever happens"""
    ok_el = torch.isfinite(got) & ((got - want).abs() <= bound)
    ratio = (got - want).abs() / bound.clamp_min(1e-300)
    ratio = torch.where((got - want).abs() == 0, torch.zeros_like(ratio), ratio)
    if where is not None:
        ok_el, ratio = ok_el | ~where, torch.where(where, ratio, torch.zeros_like(ratio))
    rec(name, float(ratio.max()) if bool(torch.isfinite(got if where is None else got[where]).all()) else float("inf"))
    if not bool(ok_el.all()):
        bad = (~ok_el).nonzero()
        i = tuple(bad[0].tolist())
        fails.append(f"{name}: {len(bad)} elements outside the bound, first {i}: got {float(got[i]):.6g} want {float(want[i]):.6g} "
                     f"bound {float(bound[i]):.3g}")


def check_forward(rec, fails, dv, tag="", lse=True):
    pr, ref = dv.pr, dv.ref
    got = _heads(dv.out.host(), pr.n, pr.T, pr.H)
    _held(rec, fails, tag + "O", got, ref["o"], ref["bound"]["o"])
    on = ref["on"]
    if not bool(on.all()):                                         # a masked query row is the plain mean of V over all T keys
        mean = pr.args[2].mean(dim=2, keepdim=True).expand_as(got)  # (under dropout: of the kept keys' c V, still over T)
        if ref["w"] is not None:
            mean = ref["w"] @ pr.args[2] / pr.T
        rows = (~on)[:, None, :, None].expand_as(got)
        _held(rec, fails, tag + "O.masked_rows_vs_mean_V", got, mean, ref["bound"]["o"], rows)
    if lse:
        got_lse = dv.lse.host().reshape(pr.n, pr.H, pr.T)
        _held(rec, fails, tag + "lse", got_lse, ref["lse"], ref["bound"]["lse"], on[:, None, :].expand_as(got_lse))
        if bool(torch.isnan(got_lse).any()):
            fails.append(f"{tag}lse: an element was not written")
    elif not dv.lse.untouched():
        fails.append(f"{tag}lse: written by the form without lse")
    for name, b in (("out", dv.out), ("lse", dv.lse)):
        if not b.guards_intact():
            fails.append(f"{tag}{name}: guards changed")
    dv.inputs_untouched(dv.inputs_fwd, fails, tag)


def reached_rows(pr):
    """(2S,) bool: the table rows some unmasked (i, j) pair of some item maps to"""
    T = pr.T
    ix = R.pair_index(pr.idx, T)
    hit = torch.zeros(2 * pr.S, dtype=torch.bool)
    for item in range(pr.n):
        on = torch.ones(T, dtype=torch.bool) if pr.mask is None else pr.mask[item] != 0
        hit[ix[on][:, on].reshape(-1)] = True
    return hit


def check_backward(rec, fails, dv, tag="", pos=True, adds=1):
    pr, ref = dv.pr, dv.ref
    n, H, T, d = pr.n, pr.H, pr.T, pr.d
    dqkv = dv.dqkv.host()
    parts = {key: _heads(dqkv[:, i * d:(i + 1) * d], n, T, H) for i, key in enumerate(("dq", "dk", "dv"))}
    for key, got in parts.items():
        _held(rec, fails, tag + {"dq": "dQ", "dk": "dK", "dv": "dV"}[key], got, ref[key], ref["bound"][key])
    on = ref["on"]
    if not bool(on.all()):
        off = (~on)[:, None, :, None].expand_as(parts["dq"])
        for key in ("dq", "dk"):                                   # exactly 0: no unmasked pair has that token
            if not bool((parts[key][off] == 0).all()):
                fails.append(f"{tag}{key}: a masked token's row is not exactly 0")
        # dV of a masked key: only the masked query rows (P = 1 / T, rounded to bf16 as the operand) reach it
        # (under dropout the operand is bf16(w / T), w = keep c)
        w = torch.ones(n, H, T, T, dtype=torch.float64) if ref["w"] is None else ref["w"]
        want = attn_ref.bf16r(w * R.ROUND.inv(float(T))).transpose(-1, -2) @ (pr.dO * (~on)[:, None, :, None])
        _held(rec, fails, tag + "dV.masked_keys_vs_mean_dO", parts["dv"], want, ref["bound"]["dv"], off)
    got_delta = dv.delta.host().reshape(n, H, T)
    _held(rec, fails, tag + "delta", got_delta, (pr.dO * ref["o16"]).sum(-1), ref["bound"]["delta"])
    if pos:
        hit = reached_rows(pr)
        for i, key in enumerate(("dposq", "dposk")):
            got = dv.dpos.host(i).reshape(2 * pr.S, H, 64).transpose(0, 1)
            fill = dv.fill[i].double().reshape(2 * pr.S, H, 64).transpose(0, 1)
            # the entry ADDS: one f32 rounding per call that adds to something (a non-zero fill; every chunk after the first)
            bound = ref["bound"][key] + 2.0 ** -24 * (fill.abs() + ref[key].abs()) * ((fill != 0).double() + (adds - 1))
            _held(rec, fails, tag + {"dposq": "dposQ", "dposk": "dposK"}[key], got - fill, ref[key], bound)
            same = _bits(dv.dpos.views[i].reshape(2 * pr.S, H * 64))[~hit] == _bits(dv.fill[i].to(DEV))[~hit]
            if not bool(same.all()):
                fails.append(f"{tag}{key}: a row no unmasked pair reaches changed")
    elif not dv.dpos.untouched() or not dv.ws.untouched():
        fails.append(f"{tag}dpos / workspace: written by the form without table gradients")
    for name, b in (("dqkv", dv.dqkv), ("delta", dv.delta), ("dpos", dv.dpos), ("workspace", dv.ws)):
        if not b.guards_intact():
            fails.append(f"{tag}{name}: guards changed")
    dv.inputs_untouched(dv.inputs_bwd, fails, tag)


def run_all(rec, name, mask_kind=None, mask_dtype=F32, p=0.0, dpos_fill=None):
    """the forward with lse, then the backward with table gradients on the reference's O and lse: each checked, each run twice"""
    pr, ref = reference(name, mask_kind, p)
    state = torch.tensor([STATE], dtype=torch.int64, device=DEV)
    drop = (p, state, SITE, ITEM0) if p else None
    fails, runs = [], []
    for again in range(2):
        dv = Dev(pr, ref, mask_dtype, dpos_fill)
        dv.forward(drop=drop)
        dv.backward(drop=drop)
        runs.append(dv.forward_bits() + dv.backward_bits())
        if not again:
            check_forward(rec, fails, dv)
            check_backward(rec, fails, dv)
    if not all(torch.equal(a, b) for a, b in zip(*runs)):
        fails.append("two runs differ")
    assert not fails, "\n".join(fails)
    return dv


# ------------------------------------------------------------------------------------------------ shapes and index tables
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_case_element_by_element(rec, name):
    """T = 1; one key past a tile; both clamps with a ragged second query block; every C2P count on a small table; the real
    geometry; T > max_position with all nine chunk counts; full-width, one-row and division-edge windows on synthetic tables;
    both far-end clamps binding between rows that differ (deberta_attn_staged_ref.CASES)"""
    run_all(rec, name)


def test_table_gradients_on_top_of_a_non_zero_fill(rec):
    pr, _ = reference("d")
    g = torch.Generator().manual_seed(11)
    fill = torch.randn(2, 2 * pr.S, pr.d, generator=g)
    run_all(rec, "d", dpos_fill=fill)


# ------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.uint8, torch.bool], ids=["f32", "u8", "bool"])
@pytest.mark.parametrize("kind", R.MASKS)
def test_masks_on_the_ragged_geometry(rec, kind, mask_dtype):
    """tail padding; 40 tokens of left padding (the first key tile fully masked: the running maximum starts at -FLT_MAX and is
    rescaled away); a hole; one unmasked token (a one-hot softmax); an item whose mask is all zero next to a normal one.  Masked
    query rows of O are the mean of V, their dQ and the masked keys' dK exactly 0, the masked keys' dV the 1 / T sum of the masked
    rows' dO (check_forward / check_backward)."""
    dv = run_all(rec, "c", kind, mask_dtype)
    if kind == "empty_item":                       # the fully masked item adds exactly 0: the bits of the normal item alone
        pr, ref = dv.pr, dv.ref
        alone = Dev(pr, ref, mask_dtype)
        alone.backward(lo=0, hi=1)
        assert torch.equal(_bits(alone.dpos.buf), _bits(dv.dpos.buf))
        assert bool(ref["on"][0].all()) and not bool(ref["on"][1].any())


# ------------------------------------------------------------------------------------------------ forms
FORM_CASES = [("c", None), ("e", None), ("c", "left")]


@pytest.mark.parametrize("name,kind", FORM_CASES, ids=["c", "e", "c-left"])
def test_plain_forms_agree_bit_for_bit(rec, name, kind):
    """_fwd against _fwd_lse: O; _bwd against _bwd_pos: dqkv and delta; p = 0 through the three _drop entries: the plain bits"""
    pr, ref = reference(name, kind)
    full = Dev(pr, ref)
    full.forward()
    full.backward()
    fails = []
    bare = Dev(pr, ref)
    bare.forward(lse=False)
    bare.backward(pos=False)
    check_forward(rec, fails, bare, "no_lse.", lse=False)
    check_backward(rec, fails, bare, "no_pos.", pos=False)
    assert not fails, "\n".join(fails)
    assert torch.equal(_bits(bare.out.buf), _bits(full.out.buf)), "O of _fwd and _fwd_lse"
    assert torch.equal(_bits(bare.dqkv.buf), _bits(full.dqkv.buf)) and torch.equal(_bits(bare.delta.buf), _bits(full.delta.buf))
    state = torch.tensor([STATE], dtype=torch.int64, device=DEV)
    for st in (state, None):                       # a threshold of 0 takes the plain kernels; the state may be NULL
        z = Dev(pr, ref)
        z.forward(drop=(0.0, st, SITE, ITEM0))
        z.backward(drop=(0.0, st, SITE, ITEM0))
        assert all(torch.equal(a, b) for a, b in zip(z.forward_bits() + z.backward_bits(), full.forward_bits() + full.backward_bits()))
        z2 = Dev(pr, ref)
        z2.forward(lse=False, drop=(0.0, st, SITE, ITEM0))
        z2.backward(pos=False, drop=(0.0, st, SITE, ITEM0))
        assert torch.equal(_bits(z2.out.buf), _bits(full.out.buf)) and torch.equal(_bits(z2.dqkv.buf), _bits(full.dqkv.buf))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name,kind", FORM_CASES, ids=["c", "e", "c-left"])
def test_dropout_forms(rec, name, kind, p):
    """the three DROP forms: keep masks from deberta_dropout_ref.probs_keep, a non-zero item0, a state with a non-zero high word;
    lse bit-equal to the undropped forward's; the form without lse / without table gradients gives the same O / dqkv bits"""
    dv = run_all(rec, name, kind, p=p)
    pr, ref = dv.pr, dv.ref
    assert STATE >> 32 and ITEM0
    keep = D.probs_keep(STATE, SITE, ITEM0, pr.n, pr.H, pr.T, attn_ref.mmf_drop_thresh(p))
    assert abs(float(keep.double().mean()) - (1 - p)) < 0.02           # (the reference really dropped that share)
    plain = Dev(*reference(name, kind))
    plain.forward()
    assert torch.equal(_bits(plain.lse.buf), _bits(dv.lse.buf)), "lse under dropout"
    assert not torch.equal(_bits(plain.out.buf), _bits(dv.out.buf))
    state = torch.tensor([STATE], dtype=torch.int64, device=DEV)
    bare = Dev(pr, ref)
    bare.forward(lse=False, drop=(p, state, SITE, ITEM0))
    bare.backward(pos=False, drop=(p, state, SITE, ITEM0))
    assert torch.equal(_bits(bare.out.buf), _bits(dv.out.buf)) and bare.lse.untouched()
    assert torch.equal(_bits(bare.dqkv.buf), _bits(dv.dqkv.buf)) and torch.equal(_bits(bare.delta.buf), _bits(dv.delta.buf))


# ------------------------------------------------------------------------------------------------ chunked calls
@pytest.mark.parametrize("name,kind,p", [("c", None, 0.1), ("e", None, 0.5), ("c", "left", 0.0), ("c", "empty_item", 0.1)],
                         ids=["c-p0.1", "e-p0.5", "c-left", "c-empty-p0.1"])
def test_chunked_calls_give_the_whole_batch(rec, name, kind, p):
    """items [0, 1) then [1, 2) with item0 advanced: the whole-batch call's bits for O, lse, delta and dqkv (a mask is a function of
    the element, never of the launch); dposq / dposk: the entry adds, so the chunked sum is (fill + first) + second in f32, each
    chunk's own sum being what a call on that chunk alone into zeros gives"""
    pr, ref = reference(name, kind, p)
    assert pr.n == 2
    state = torch.tensor([STATE], dtype=torch.int64, device=DEV)
    drop = lambda item0: (p, state, SITE, item0) if p else None
    whole = Dev(pr, ref)
    whole.forward(drop=drop(ITEM0))
    whole.backward(drop=drop(ITEM0))
    chunked, alone = Dev(pr, ref), []
    for lo in (0, 1):
        chunked.forward(drop=drop(ITEM0 + lo), lo=lo, hi=lo + 1)
        chunked.backward(drop=drop(ITEM0 + lo), lo=lo, hi=lo + 1)
        one = Dev(pr, ref)
        one.backward(drop=drop(ITEM0 + lo), lo=lo, hi=lo + 1)
        alone.append(one.dpos.buf.clone())
    fails = []
    check_forward(rec, fails, chunked, "chunked.")
    check_backward(rec, fails, chunked, "chunked.", adds=2)
    assert not fails, "\n".join(fails)
    for a, b, what in zip(chunked.forward_bits() + chunked.backward_bits()[:2], whole.forward_bits() + whole.backward_bits()[:2],
                          ("O", "lse", "dqkv", "delta")):
        assert torch.equal(a, b), what
    live = torch.zeros(chunked.dpos.buf.shape, dtype=torch.bool)
    for wnd in chunked.dpos.wins:
        live[wnd] = True
    want = (alone[0] + alone[1])                                   # f32 on the device: IEEE addition, (0 + first) + second
    assert torch.equal(_bits(chunked.dpos.buf)[live], _bits(want)[live]), "dpos: the chunks' sums added in call order"
