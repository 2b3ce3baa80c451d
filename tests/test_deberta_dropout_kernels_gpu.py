"""GPU: the dropout kernels of csrc/deberta.hip and csrc/elementwise.hip against float64 under the masks tests/deberta_dropout_ref.py restates on the host:
the attention forward and backward with dropped probabilities (``mmf_deberta_attn_fwd_drop`` / ``_bwd_drop`` / ``_bwd_pos_drop``) and
the streaming hidden dropout (``mmf_hidden_dropout``).

The mask is held to the restatement EXACTLY (one-hot V rows turn the forward's output into the mask; the streaming kernel's zeros
are the mask), values to the bounds of tests/test_deberta_grad_gpu.py: the forward's O within BOUND_A relative L2 of float64, its
lse bit-equal to the plain forward's (the softmax statistics run over the undropped probabilities); a gradient within
BOUND_A ||want|| + ||N||, N the f32 summation noise of dP - delta (that file's docstring), the reference handed the reference's
own O (rounded to bf16) and lse (f32).  The streaming kernel is one f32 multiply-add and one rounding: exact.

Shapes are tests/test_deberta_grad_gpu.py's smallest four: T = 1; one key past a tile; two query blocks with a ragged tile and a
padded item; linear and log buckets over four query blocks.  Every call has a non-zero first-item index."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref  # noqa: E402
import deberta_dropout_ref as D  # noqa: E402
from helpers import BOUND_A, _lib, l2_rel  # noqa: E402
from test_deberta_gpu import _attn_case  # noqa: E402
from test_deberta_grad_gpu import E_ALIGN, E_SHAPE, E_UNSUPPORTED, F32_TOL, SCALE, _bits, _heads, _rows  # noqa: E402

BF16 = torch.bfloat16
CASES = [
    (1, 3, 1, 8, 32, None),              # T = 1: the output is 0 or c V
    (1, 2, 33, 8, 32, None),             # one key past a tile
    (2, 2, 70, 8, 32, 50),               # two query blocks, a ragged tile and a padded item
    (2, 2, 200, 256, 512, None),         # linear and log buckets
]
PS = [0.1, 0.5]
STATE, SITE, ITEM0 = (77 << 20) + 3, 9, 5
_cache = {}


def _state():
    return torch.tensor([STATE], dtype=torch.int64, device="cuda")


def _drop(p, item0=ITEM0, site=SITE, state=None):
    return (p, _state() if state is None else state, site, item0)


def _weights(n, H, T, p, item0=ITEM0):
    """(keep (n, H, T, T) bool, w = keep * c float64) as the kernels draw them for a call whose first item is ``item0``"""
    th = attn_ref.mmf_drop_thresh(p)
    keep = D.probs_keep(STATE, SITE, item0, n, H, T, th)
    return keep, keep.double() * attn_ref.inv_keep_of(th)


def _case(n, H, T, S, max_pos, pad, p):
    """operands, the restated mask, the float64 O / lse under it and the float64 gradients for the reference's own O (bf16) and lse
    (f32); computed once per (case, p) and shared"""
    key = (n, H, T, S, max_pos, pad, p)
    if key not in _cache:
        qkv, posq, posk, idx, mask = _attn_case(n, H, T, S, max_pos, pad)
        d = H * 64
        g = torch.Generator().manual_seed(11 * T + S)
        dout = torch.randn(n * T, d, generator=g).to(BF16)
        q, k, v = (_heads(qkv.double()[:, i * d:(i + 1) * d], n, T, H) for i in range(3))
        pq, pk = (t.double().reshape(2 * S, H, 64).transpose(0, 1) for t in (posq, posk))
        keep, w = _weights(n, H, T, p)
        O, lse = D.attention_stats(q, k, v, pq, pk, idx, mask, SCALE, w)
        o16, lse32 = _rows(O, n, T, H).to(BF16), lse.float()
        want, noise = D.attention_backward(q, k, v, pq, pk, idx, mask, SCALE, _heads(dout.double(), n, T, H), w,
                                           _heads(o16.double(), n, T, H), lse32.double(), F32_TOL)
        tab = lambda t: t.transpose(0, 1).reshape(2 * S, d)
        shape = [lambda t: _rows(t, n, T, H)] * 3 + [tab, tab]
        _cache[key] = dict(qkv=qkv, posq=posq, posk=posk, idx=idx, mask=mask, dout=dout, keep=keep, O64=_rows(O, n, T, H), o16=o16,
                           lse32=lse32, want=[f(t) for f, t in zip(shape, want)], noise=[float(f(t).norm()) for f, t in zip(shape, noise)])
    return _cache[key]


def _dev(c):
    dev = {k: c[k].cuda() for k in ("qkv", "posq", "posk", "idx", "dout", "o16", "lse32")}
    dev["mask"] = None if c["mask"] is None else c["mask"].cuda()
    return dev


def _fwd(dev, n, H, T, S, drop, lse=True, plain=False):
    lib = _lib()
    out = torch.full((n * T, H * 64), float("nan"), dtype=BF16, device="cuda")
    l = torch.full((n, H, T), float("nan"), device="cuda") if lse else None
    kw = {} if plain else dict(drop=drop)
    lib.deberta_attn_fwd(dev["qkv"], dev["posq"], dev["posk"], dev["idx"], dev["mask"], out, n, H, T, S, SCALE, lse=l, **kw)
    torch.cuda.synchronize()
    return out, l


def _bwd(dev, n, H, T, S, drop, pos, plain=False):
    lib = _lib()
    d = H * 64
    dqkv = torch.full((n * T, 3 * d), float("nan"), dtype=BF16, device="cuda")
    delta = torch.empty(n * H * T, device="cuda")
    kw = {} if plain else dict(drop=drop)
    args = (dev["qkv"], dev["posq"], dev["posk"], dev["idx"], dev["mask"], dev["o16"], dev["lse32"].reshape(-1), dev["dout"], delta, dqkv)
    if not pos:
        lib.deberta_attn_bwd(*args, n, H, T, S, SCALE, **kw)
        torch.cuda.synchronize()
        return dqkv.cpu(), None
    dpos = torch.zeros((2 * S, 2 * d), device="cuda")
    ws = torch.full((lib.deberta_attn_bwd_pos_workspace_bytes(n, H, T, S) // 4,), float("nan"), device="cuda")
    lib.deberta_attn_bwd_pos(*args, dpos[:, :d], dpos[:, d:], ws, n, H, T, S, SCALE, **kw)
    torch.cuda.synchronize()
    return dqkv.cpu(), dpos.cpu()


# ---- forward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n,H,T,S,max_pos,pad", CASES)
def test_forward_against_float64_and_lse_is_the_undropped_one(n, H, T, S, max_pos, pad, p):
    c = _case(n, H, T, S, max_pos, pad, p)
    dev = _dev(c)
    out, lse = _fwd(dev, n, H, T, S, _drop(p))
    no_lse, _ = _fwd(dev, n, H, T, S, _drop(p), lse=False)
    plain, plain_lse = _fwd(dev, n, H, T, S, None, plain=True)
    assert not torch.isnan(out.float()).any() and not torch.isnan(lse).any()
    err = l2_rel(out.cpu().double(), c["O64"])
    print(f"deberta attention forward with dropout p={p} n={n} H={H} T={T} S={S} pad={pad}: O rel L2 {err:.3e} (bound {BOUND_A}); "
          f"the plain forward is {l2_rel(plain.cpu().double(), c['O64']):.3e} away")
    assert err <= BOUND_A
    assert torch.equal(_bits(lse), _bits(plain_lse)), "lse must be the plain forward's bits"
    assert torch.equal(_bits(no_lse), _bits(out))
    assert not torch.equal(_bits(out), _bits(plain))
    if T == 1:                                       # one key: every output row is 0 (dropped) or c V (kept)
        d = H * 64
        keep = c["keep"].reshape(n, H)
        v = c["qkv"].float()[:, 2 * d:].reshape(n, H, 64)
        got = out.cpu().float().reshape(n, H, 64)
        assert bool((got[~keep] == 0).all()) and bool((got[keep] != 0).all())
        assert l2_rel(got[keep], v[keep] * attn_ref.inv_keep_of(attn_ref.mmf_drop_thresh(p))) <= BOUND_A


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n,H,T,S,max_pos,pad", [CASES[1], CASES[2]])
def test_the_mask_is_the_restated_one_exactly(n, H, T, S, max_pos, pad, p):
    """one-hot V rows, key j -> column j mod 64, the keys taken 64 at a time: the output element (i, head, j mod 64) is c P_ij where
    the kernel kept pair (i, j) and exactly 0 where it dropped it.  P_ij > 0 on unmasked pairs and on every key of a masked query
    (the uniform row); a masked key of an unmasked query is 0 either way."""
    c = _case(n, H, T, S, max_pos, pad, p)
    d = H * 64
    on = torch.ones(n, T, dtype=torch.bool) if c["mask"] is None else c["mask"] != 0
    alive = (on[:, None, :] | ~on[:, :, None])[:, None].expand(n, H, T, T)              # [item, h, i, j]: P_ij > 0
    for j0 in range(0, T, 64):
        keys = torch.arange(j0, min(j0 + 64, T))
        v = torch.zeros(n, T, H, 64)
        v[:, keys, :, keys - j0] = 1.0
        qkv = c["qkv"].clone()
        qkv[:, 2 * d:] = v.reshape(n * T, d).to(BF16)
        dev = _dev(dict(c, qkv=qkv))
        out, _ = _fwd(dev, n, H, T, S, _drop(p), lse=False)
        got = out.cpu().float().reshape(n, T, H, 64).permute(0, 2, 1, 3)[..., :len(keys)] != 0      # [item, h, i, key - j0]
        want = (c["keep"] & alive)[..., keys]
        assert torch.equal(got, want), f"keys {j0}..: {int((got != want).sum())} of {want.numel()} pairs differ from the restated mask"
        assert bool(want.any()) and not bool(want.all())


def test_a_chunk_draws_what_the_batch_draws_and_a_state_or_site_changes_it():
    n, H, T, S, max_pos, pad = CASES[2]
    c = _case(n, H, T, S, max_pos, pad, 0.1)
    dev = _dev(c)
    d = H * 64
    both, _ = _fwd(dev, n, H, T, S, _drop(0.1))
    last = {k: (v[T:] if k in ("qkv", "dout", "o16") else v) for k, v in dev.items()}
    last["mask"] = dev["mask"][1:].contiguous()
    one, _ = _fwd(last, 1, H, T, S, _drop(0.1, item0=ITEM0 + 1))
    assert torch.equal(_bits(one), _bits(both[T:])), "item 1 of the call at item0 must be item 0 of a call at item0 + 1"
    moved, _ = _fwd(last, 1, H, T, S, _drop(0.1, item0=ITEM0))
    assert not torch.equal(_bits(moved), _bits(one))
    for other in (_drop(0.1, site=SITE + 1), _drop(0.1, state=torch.tensor([STATE + 1], dtype=torch.int64, device="cuda"))):
        assert not torch.equal(_bits(_fwd(dev, n, H, T, S, other)[0]), _bits(both))
    # and the backward of the chunk is the batch's rows
    dq_both, _ = _bwd(dev, n, H, T, S, _drop(0.1), False)
    last["lse32"] = dev["lse32"][1:].contiguous()
    dq_one, _ = _bwd(last, 1, H, T, S, _drop(0.1, item0=ITEM0 + 1), False)
    assert torch.equal(_bits(dq_one), _bits(dq_both[T:]))


# ---- backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n,H,T,S,max_pos,pad", CASES)
def test_backward_against_float64(n, H, T, S, max_pos, pad, p):
    c = _case(n, H, T, S, max_pos, pad, p)
    dev = _dev(c)
    d = H * 64
    dqkv, _ = _bwd(dev, n, H, T, S, _drop(p), False)
    again, _ = _bwd(dev, n, H, T, S, _drop(p), False)
    with_pos, dpos = _bwd(dev, n, H, T, S, _drop(p), True)
    with_pos2, dpos2 = _bwd(dev, n, H, T, S, _drop(p), True)
    plain, _ = _bwd(dev, n, H, T, S, None, False, plain=True)
    assert not torch.isnan(dqkv.float()).any(), "an element of dqkv was not written"
    assert torch.equal(_bits(dqkv), _bits(again)) and torch.equal(_bits(dpos), _bits(dpos2)), "two runs differ"
    assert torch.equal(_bits(with_pos), _bits(dqkv)) and torch.equal(_bits(with_pos2), _bits(dqkv)), "the POS form's dqkv differs"
    assert not torch.equal(_bits(plain), _bits(dqkv))
    got = [dqkv[:, i * d:(i + 1) * d].double() for i in range(3)] + [dpos[:, :d].double(), dpos[:, d:].double()]
    errs = [float((g - w).norm()) for g, w in zip(got, c["want"])]
    bounds = [BOUND_A * float(w.norm()) + nz for w, nz in zip(c["want"], c["noise"])]
    names = ("dQ", "dK", "dV", "dposQ", "dposK")
    print(f"deberta attention backward with dropout p={p} n={n} H={H} T={T} S={S} pad={pad}: error / bound "
          + " ".join(f"{nm} {e / max(b, 1e-300):.3e}" for nm, e, b in zip(names, errs, bounds))
          + "; rel L2 " + " ".join(f"{l2_rel(g, w):.3e}" for g, w in zip(got, c["want"]))
          + "; f32 noise term / BOUND_A ||want|| " + " ".join(f"{nz / max(BOUND_A * float(w.norm()), 1e-300):.1e}" for w, nz in zip(c["want"], c["noise"])))
    assert all(e <= b for e, b in zip(errs, bounds)), (errs, bounds)
    if pad is not None:
        masked = torch.arange(T + pad, 2 * T)
        assert bool((got[0][masked] == 0).all()) and bool((got[1][masked] == 0).all()), "dQ of a masked query / dK of a masked key"


@pytest.mark.parametrize("n,H,T,S,max_pos,pad", [CASES[1], CASES[2]])
def test_threshold_zero_takes_the_plain_kernels(n, H, T, S, max_pos, pad):
    """p = 0 through the new entry points: the existing entry points' bits, forward and backward, with or without a state"""
    c = _case(n, H, T, S, max_pos, pad, 0.1)
    dev = _dev(c)
    for drop in ((0.0, None, SITE, ITEM0), _drop(0.0)):
        out, lse = _fwd(dev, n, H, T, S, drop)
        plain, plain_lse = _fwd(dev, n, H, T, S, None, plain=True)
        assert torch.equal(_bits(out), _bits(plain)) and torch.equal(_bits(lse), _bits(plain_lse))
        assert torch.equal(_bits(_fwd(dev, n, H, T, S, drop, lse=False)[0]), _bits(plain))
        for pos in (False, True):
            a, ap = _bwd(dev, n, H, T, S, drop, pos)
            b, bp = _bwd(dev, n, H, T, S, None, pos, plain=True)
            assert torch.equal(_bits(a), _bits(b)) and (not pos or torch.equal(_bits(ap), _bits(bp)))


# ---- the streaming kernel --------------------------------------------------------------------------------------------
def _fma_bf16(y, c, resid):
    """bf16(fma(y, c, resid)) of bf16 y / resid and an f32 c: the product and the sum are exact in float64 (8 + 24 bits, then
    operands within 2^20 of each other), so rounding that to f32 and then to bf16 is the kernel's f32 fma and its one rounding"""
    return (y.double() * c + resid.double()).float().to(BF16)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("items,per", [(3, 24 * 256), (2, 8), (5, 1000), (1, 16 * 768)])
def test_streaming_dropout_is_the_restated_mask_and_exact(items, per, p):
    lib = _lib()
    th = attn_ref.mmf_drop_thresh(p)
    cf = attn_ref.inv_keep_of(th)
    keep = D.hidden_keep(STATE, SITE, ITEM0, items, per, th)
    g = torch.Generator().manual_seed(items * per)
    y = (1.0 + torch.rand(items, per, generator=g)).to(BF16) * torch.where(torch.rand(items, per, generator=g) < 0.5, -1.0, 1.0).to(BF16)
    resid = torch.randn(items, per, generator=g).to(BF16)
    yd, rd = y.cuda(), resid.cuda()
    # without a residual: zeros exactly where the restatement drops (y is never 0), bf16(y c) elsewhere; the gradient form
    out = torch.full_like(yd, float("nan"))
    lib.hidden_dropout(yd, out, items, _drop(p))
    got = out.cpu()
    assert torch.equal(got.float() != 0, keep), "the kept set is not the restated one"
    assert torch.equal(_bits(got), _bits(torch.where(keep, _fma_bf16(y, cf, torch.zeros_like(y)), torch.zeros_like(y))))
    # with the residual: one multiply-add, one rounding; a dropped element is the residual itself
    out2 = torch.full_like(yd, float("nan"))
    lib.hidden_dropout(yd, out2, items, _drop(p), resid=rd)
    assert torch.equal(_bits(out2.cpu()), _bits(torch.where(keep, _fma_bf16(y, cf, resid), resid)))
    inplace = yd.clone()
    lib.hidden_dropout(inplace, inplace, items, _drop(p), resid=rd)
    assert torch.equal(_bits(inplace), _bits(out2)) and torch.equal(_bits(yd), _bits(y)) and torch.equal(_bits(rd), _bits(resid))
    # f32 (the gradient of an f32 buffer): the same mask, y c in f32
    y32 = y.float() * 1.2345
    out3 = torch.full((items, per), float("nan"), device="cuda")
    lib.hidden_dropout(y32.cuda(), out3, items, _drop(p))
    assert torch.equal(_bits(out3.cpu()), _bits(torch.where(keep, (y32.double() * cf).float(), torch.zeros_like(y32))))
    # another first item: another mask, and the batch's rows when it is a chunk of it
    if items > 1:
        out4 = torch.full_like(yd[1:], float("nan"))
        lib.hidden_dropout(yd[1:].contiguous(), out4, items - 1, _drop(p, item0=ITEM0 + 1))
        assert torch.equal(_bits(out4), _bits(out[1:]))
        lib.hidden_dropout(yd[1:].contiguous(), out4, items - 1, _drop(p, item0=ITEM0))
        assert not torch.equal(_bits(out4), _bits(out[1:]))
    torch.cuda.synchronize()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    nan32 = torch.full((1 << 16,), float("nan"), device="cuda")
    f = torch.zeros(1 << 14, device="cuda")
    b = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    idx = torch.zeros(4096, dtype=torch.int32, device="cuda")
    st = _state()
    p = lambda t, off=0: t.data_ptr() + off
    fwd = lambda prob, state, item0=0, qkv=None, hd=64, T=16, lse=None: L.mmf_deberta_attn_fwd_drop(
        p(b) if qkv is None else qkv, p(b), p(b), 128, p(idx), None, 0, p(nan16), lse, 1, 2, T, 8, hd, SCALE, prob, state, 3, item0, s)
    bwd = lambda prob, state, item0=0, dqkv=None, hd=64, lse="f": L.mmf_deberta_attn_bwd_drop(
        p(b), p(b), p(b), 128, p(idx), None, 0, p(b), p(f) if lse == "f" else lse, p(b), p(nan32), p(nan16) if dqkv is None else dqkv,
        1, 2, 16, 8, hd, SCALE, prob, state, 3, item0, s)
    bwd_pos = lambda prob, state, ws_bytes=1 << 18, ld=128: L.mmf_deberta_attn_bwd_pos_drop(
        p(b), p(b), p(b), 128, p(idx), None, 0, p(b), p(f), p(b), p(nan32), p(nan16), 1, 2, 16, 8, 64, SCALE, p(nan32), p(nan32, 4096 * 4), ld,
        p(nan32, 8192 * 4), ws_bytes, prob, state, 3, 0, s)
    drop = lambda prob, state, y="b", resid=None, out=None, f32=0, items=4, per=64, item0=0: L.mmf_hidden_dropout(
        p(b) if y == "b" else y, resid, p(nan16) if out is None else out, f32, items, per, prob, state, 3, item0, s)
    A, B_, C_, D_ = "mmf_deberta_attn_fwd_drop", "mmf_deberta_attn_bwd_drop", "mmf_deberta_attn_bwd_pos_drop", "mmf_hidden_dropout"
    cases = [
        (A, lambda: fwd(1.0, p(st)), E_SHAPE), (A, lambda: fwd(-0.1, p(st)), E_SHAPE), (A, lambda: fwd(float("nan"), p(st)), E_SHAPE),
        (A, lambda: fwd(0.1, None), E_SHAPE), (A, lambda: fwd(0.1, p(st), item0=-1), E_SHAPE), (A, lambda: fwd(0.1, p(st, 4)), E_ALIGN),
        (A, lambda: fwd(0.1, p(st), hd=96), E_UNSUPPORTED), (A, lambda: fwd(0.1, p(st), T=1025), E_UNSUPPORTED),
        (A, lambda: fwd(0.1, p(st), qkv=p(b, 2)), E_ALIGN), (A, lambda: fwd(0.1, p(st), lse=p(nan32, 2)), E_ALIGN),
        (A, lambda: fwd(0.0, None, hd=96), E_UNSUPPORTED),                                        # p = 0 keeps the plain entry's rules
        (B_, lambda: bwd(1.0, p(st)), E_SHAPE), (B_, lambda: bwd(0.1, None), E_SHAPE), (B_, lambda: bwd(0.1, p(st, 4)), E_ALIGN),
        (B_, lambda: bwd(0.1, p(st), item0=-3), E_SHAPE), (B_, lambda: bwd(0.1, p(st), lse=None), E_SHAPE),
        (B_, lambda: bwd(0.1, p(st), hd=96), E_UNSUPPORTED), (B_, lambda: bwd(0.1, p(st), dqkv=p(nan16, 2)), E_ALIGN),
        (C_, lambda: bwd_pos(1.5, p(st)), E_SHAPE), (C_, lambda: bwd_pos(0.1, None), E_SHAPE), (C_, lambda: bwd_pos(0.1, p(st), ws_bytes=16), E_SHAPE),
        (C_, lambda: bwd_pos(0.1, p(st), ld=64), E_SHAPE), (C_, lambda: bwd_pos(0.1, p(st), ld=130), E_ALIGN),
        (D_, lambda: drop(1.0, p(st)), E_SHAPE), (D_, lambda: drop(0.1, None), E_SHAPE), (D_, lambda: drop(0.0, None), E_SHAPE),
        (D_, lambda: drop(0.1, p(st), y=None), E_SHAPE), (D_, lambda: drop(0.1, p(st), items=0), E_SHAPE),
        (D_, lambda: drop(0.1, p(st), resid=p(b), f32=1), E_SHAPE), (D_, lambda: drop(0.1, p(st), item0=-1), E_SHAPE),
        (D_, lambda: drop(0.1, p(st), per=60), E_UNSUPPORTED), (D_, lambda: drop(0.1, p(st), out=p(nan16, 2)), E_ALIGN),
        (D_, lambda: drop(0.1, p(st), resid=p(b, 2)), E_ALIGN), (D_, lambda: drop(0.1, p(st, 4)), E_ALIGN),
    ]
    for name, call, want in cases:
        rc = call()
        assert rc == want, (name, rc, want, L.mmf_last_error())
        assert name.encode() in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all())                 # nothing was launched
    assert int(st.item()) == STATE
