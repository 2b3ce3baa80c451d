"""GPU, through the C ABI: ``mmf_deberta_embed_bwd_params`` (the embedding backward with the LayerNorm parameters' gradients, on
the ids and the embeds route) and ``mmf_embedding_scatter_add_f32`` (gradient rows into the word-embedding table's gradient)
against the float64 closed forms tests/deberta_embed_grad_ref.py.

Bounds.  The operands are exact (f32 inputs; a bf16 ``dy`` the reference reads as the same values), so what separates a kernel
from float64 is f32 rounding alone.  Kernel A: the f32-noise form of this project's kernel tests (tests/deberta_grad_ref.py's
term), ||got - want|| <= F32_TOL x || the summed magnitudes of each element's terms ||, with tests/test_deberta_grad_gpu.py's
F32_TOL.  Kernel B: per element |got - want| <= n 2^-23 sum |terms|, n the number of occurrences added, the standard bound of an
f32 sum in any fixed order."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_embed_grad_ref as R  # noqa: E402
from helpers import _lib  # noqa: E402
from test_deberta_grad_gpu import E_ALIGN, E_SHAPE, E_UNSUPPORTED, F32_TOL, _bits  # noqa: E402

BF16 = torch.bfloat16
EPS = 1e-7
MASKS = (None, torch.float32, torch.uint8, torch.bool)
_cases = {}


def _embed_case(rows, d):
    """operands on the CPU and the float64 results with and without the mask, once per (rows, d): ids over a table of 37 rows,
    some outside it on both sides; the embeds route reads the same source rows"""
    key = (rows, d)
    if key not in _cases:
        g = torch.Generator().manual_seed(rows + d)
        vocab = 37
        table = torch.randn(vocab, d, generator=g) * 2.0 + 0.3
        ids = torch.randint(0, vocab, (rows,), generator=g)
        ids[0] = -3
        if rows > 2:
            ids[1], ids[2] = vocab + 5, vocab - 1
        gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
        mask = (torch.rand(rows, generator=g) > 0.3).float()
        mask[0] = 1.0
        if rows > 1:
            mask[-1] = 0.0
        dy = torch.randn(rows, d, generator=g).to(BF16)
        fill = torch.randn(2, d, generator=g)
        c = dict(vocab=vocab, table=table, ids=ids, gamma=gamma, mask=mask, dy=dy, fill=fill, embeds=table[R.clamp_ids(ids, vocab)].contiguous())
        for tag, mk in (("plain", None), ("masked", mask)):
            c[tag] = R.embed_bwd_params(dy, gamma, EPS, mk, ids=ids, table=table)
        _cases[key] = c
    return _cases[key]


def _embed_run(c, route, mask_dtype, accumulate=None, ws_fill=float("nan")):
    """-> (d_rows, dgamma | dbeta (2, d)) on the CPU; ``accumulate``: what d_rows holds before an accumulating call"""
    lib = _lib()
    rows, d = c["dy"].shape
    dev = {k: c[k].cuda() for k in ("table", "ids", "gamma", "dy", "embeds")}
    m = None if mask_dtype is None else c["mask"].to(mask_dtype).cuda()
    before = {k: _bits(v) for k, v in dev.items()}
    d_rows = torch.full((rows, d), float("nan"), device="cuda") if accumulate is None else accumulate.cuda().clone()
    dgb = c["fill"].cuda().clone()
    nbytes = lib.deberta_embed_bwd_params_workspace_bytes(rows, d)
    assert nbytes == min((rows + 3) // 4, 512) * 2 * d * 4
    ws = torch.full((nbytes // 4,), ws_fill, device="cuda")                            # it need not be initialised
    kw = dict(ids=dev["ids"], table=dev["table"]) if route == "ids" else dict(embeds=dev["embeds"])
    lib.deberta_embed_bwd_params(dev["gamma"], EPS, m, dev["dy"], d_rows, dgb[0], dgb[1], ws, accumulate=accumulate is not None, **kw)
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(_bits(dev[k]), b), f"{k} was written"
    return d_rows.cpu(), dgb.cpu()


# d: the LayerNorm lane forms' widths and the widest the embed kernel takes; rows: one, a partial workgroup, and 2053 = more rows
# than the 512 workgroups' 2048 waves (every wave walks a second row or not) with a partial last workgroup
@pytest.mark.parametrize("d", [256, 768, 1024])
@pytest.mark.parametrize("rows", [1, 5, 2053])
def test_embed_backward_with_parameter_gradients_against_float64(rows, d):
    lib = _lib()
    c = _embed_case(rows, d)
    for mask_dtype in MASKS:
        (w_rows, w_g, w_b), (m_rows, m_g, m_b) = c["plain" if mask_dtype is None else "masked"]
        got = {route: _embed_run(c, route, mask_dtype) for route in ("ids", "embeds")}
        again = _embed_run(c, "ids", mask_dtype, ws_fill=3.0)
        old = torch.full((rows, d), float("nan"), device="cuda")
        lib.deberta_embed_bwd(c["embeds"].cuda(), c["gamma"].cuda(), EPS, None if mask_dtype is None else c["mask"].to(mask_dtype).cuda(),
                              c["dy"].cuda(), old)
        torch.cuda.synchronize()
        # the embeds route's d_rows bits are mmf_deberta_embed_bwd's; the ids route reads the same source rows: the same bits again
        assert torch.equal(_bits(got["embeds"][0]), _bits(old.cpu())), "d_rows differs from mmf_deberta_embed_bwd's"
        assert torch.equal(_bits(got["ids"][0]), _bits(got["embeds"][0])) and torch.equal(_bits(got["ids"][1]), _bits(got["embeds"][1]))
        # two runs give the same bits, whatever the workspace held
        assert torch.equal(_bits(again[0]), _bits(got["ids"][0])) and torch.equal(_bits(again[1]), _bits(got["ids"][1])), "two runs differ"
        d_rows, dgb = got["ids"]
        assert bool(torch.isfinite(d_rows).all()) and bool(torch.isfinite(dgb).all())
        if mask_dtype is not None:
            assert bool((d_rows[c["mask"] == 0] == 0).all()), "a masked row is not exactly 0"
        fill = c["fill"].double()
        for name, g, w, mag in (("d_rows", d_rows.double(), w_rows, m_rows), ("dgamma", dgb[0].double() - fill[0], w_g, m_g + fill[0].abs()),
                                ("dbeta", dgb[1].double() - fill[1], w_b, m_b + fill[1].abs())):
            err, bound = float((g - w).norm()), F32_TOL * float(mag.norm())
            print(f"deberta embed backward with parameters rows={rows} d={d} mask={mask_dtype} {name}: ||got - want|| {err:.3e}, "
                  f"bound F32_TOL ||magnitudes|| {bound:.3e} (ratio {err / bound:.3e}), ||want|| {float(w.norm()):.3e}")
            assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("rows,d", [(5, 256), (2053, 768)])
def test_embed_backward_accumulates_onto_what_d_rows_holds(rows, d):
    c = _embed_case(rows, d)
    want = c["masked"][0][0]
    g = torch.Generator().manual_seed(rows)
    fill = torch.randn(rows, d, generator=g) * float(want.abs().max())
    for route in ("ids", "embeds"):
        zero, _ = _embed_run(c, route, torch.float32)
        got, dgb = _embed_run(c, route, torch.float32, accumulate=fill)
        tol = F32_TOL * torch.maximum(fill.abs().double(), want.abs())
        worst = float((((got - fill).double() - zero.double()).abs() - tol).max())
        print(f"accumulating d_rows rows={rows} d={d} ({route}): worst (|(got - c) - from zero| - F32_TOL max(|c|, |want|)) = {worst:.3e}")
        assert worst <= 0
        assert torch.equal(got[c["mask"] == 0], fill[c["mask"] == 0])                  # nothing is added to a masked row
        assert torch.equal(_bits(dgb), _bits(_embed_run(c, route, torch.float32)[1]))  # the parameter sums do not depend on the flag


# ---- the scatter ---------------------------------------------------------------------------------------------
def _scatter_ids(kind, rows, vocab, g):
    if kind == "equal":
        return torch.full((rows,), 7, dtype=torch.int64)
    if kind == "distinct":
        return torch.randperm(vocab, generator=g)[:rows]
    ids = torch.randint(0, vocab, (rows,), generator=g)
    for at, v in zip(range(rows), (0, vocab - 1, -3, vocab + 5)):                     # both ends of the table, and past them
        ids[at] = v
    if rows >= 65:
        ids[ids == vocab // 2] = vocab // 2 + 1
        ids[63] = ids[64] = vocab // 2                                                # a duplicate straddling a 64-lane scan step
    return ids


SCATTER = [("random", 300, 50), ("equal", 130, 50), ("distinct", 70, 100)] + [("random", r, 50) for r in (1, 63, 64, 65, 130)]


def _scatter_run(ids, d_rows, fill, mask):
    lib = _lib()
    dev = dict(ids=ids.cuda(), d_rows=d_rows.cuda())
    before = {k: _bits(v) for k, v in dev.items()}
    out = fill.cuda().clone()
    lib.embedding_scatter_add(dev["ids"], dev["d_rows"], out, mask=None if mask is None else mask.cuda())
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(_bits(dev[k]), b), f"{k} was written"
    return out.cpu()


@pytest.mark.parametrize("d", [256, 768])
@pytest.mark.parametrize("kind,rows,vocab", SCATTER)
def test_scatter_add_against_float64(kind, rows, vocab, d):
    g = torch.Generator().manual_seed(rows + d + vocab)
    ids = _scatter_ids(kind, rows, vocab, g)
    d_rows, fill = torch.randn(rows, d, generator=g), torch.randn(vocab, d, generator=g)
    mask = (torch.rand(rows, generator=g) > 0.3).float()
    named = R.clamp_ids(ids, vocab)
    only = int(named[rows // 2])
    if kind != "equal":
        mask[named == only] = 0                                                       # the only occurrences of one table row are masked
        if rows >= 65:
            mask[63] = mask[64] = 1.0
    for mk in (None, mask, mask.to(torch.uint8), mask.bool()):
        want, count, mag = R.scatter_add(ids, d_rows, vocab, mk, fill)
        got = _scatter_run(ids, d_rows, fill, mk)
        assert torch.equal(_bits(got), _bits(_scatter_run(ids, d_rows, fill, mk))), "two runs differ"
        assert bool(torch.isfinite(got).all())
        bound = count.double().unsqueeze(-1) * 2.0 ** -23 * mag
        worst = float(((got.double() - want).abs() - bound).max())
        print(f"scatter-add {kind} rows={rows} vocab={vocab} d={d} mask={None if mk is None else mk.dtype}: most occurrences "
              f"{int(count.max())}, worst (|got - want| - n 2^-23 sum|terms|) = {worst:.3e}, max error {float((got.double() - want).abs().max()):.3e}")
        assert worst <= 0
        assert torch.equal(_bits(got[count == 0]), _bits(fill[count == 0])), "a table row no unmasked id names was touched"
        if mk is not None and kind != "equal":
            assert int(count[only]) == 0
    if rows >= 4 and kind == "random":
        assert int(named[2]) == 0 and int(named[3]) == vocab - 1                      # the ids outside the table name its nearest rows


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    rows, d, vocab = 8, 256, 16
    nan32 = torch.full((1 << 14,), float("nan"), device="cuda")
    f = torch.zeros(1 << 14, device="cuda")
    b = torch.zeros(1 << 14, dtype=BF16, device="cuda")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    need = lib.deberta_embed_bwd_params_workspace_bytes(rows, d)
    ws = torch.full((need // 4 + 4,), float("nan"), device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    dg, db = p(nan32, 4 * 8192), p(nan32, 4 * 12288)

    def a(i=p(ids), e=None, t=p(f), v=vocab, gm=p(f), mk=None, kind=0, dy=p(b), dr=p(nan32), g=dg, bt=db, w=p(ws), wb=need, r=rows, dd=d):
        return L.mmf_deberta_embed_bwd_params(i, e, t, v, gm, EPS, mk, kind, dy, dr, 0, g, bt, w, wb, r, dd, s)
    cases = [
        (lambda: a(gm=None), E_SHAPE), (lambda: a(dy=None), E_SHAPE), (lambda: a(dr=None), E_SHAPE), (lambda: a(g=None), E_SHAPE),
        (lambda: a(bt=None), E_SHAPE), (lambda: a(w=None), E_SHAPE), (lambda: a(t=None), E_SHAPE), (lambda: a(v=0), E_SHAPE),
        (lambda: a(r=0), E_SHAPE), (lambda: a(e=p(f)), E_SHAPE), (lambda: a(i=None), E_SHAPE),            # both, neither
        (lambda: a(wb=need - 4), E_SHAPE), (lambda: a(wb=0), E_SHAPE), (lambda: a(kind=1), E_SHAPE), (lambda: a(kind=3, mk=p(f)), E_SHAPE),
        (lambda: a(dr=p(nan32, 4)), E_ALIGN), (lambda: a(g=dg + 8), E_ALIGN), (lambda: a(bt=db + 4), E_ALIGN), (lambda: a(w=p(ws, 4)), E_ALIGN),
        (lambda: a(t=p(f, 4)), E_ALIGN), (lambda: a(i=None, e=p(f, 8)), E_ALIGN), (lambda: a(gm=p(f, 4)), E_ALIGN),
        (lambda: a(dy=p(b, 2)), E_ALIGN), (lambda: a(i=p(ids) + 4), E_ALIGN), (lambda: a(mk=p(f) + 2, kind=1), E_ALIGN),
        (lambda: a(dd=1028, wb=1 << 30), E_UNSUPPORTED), (lambda: a(dd=254), E_UNSUPPORTED),
    ]
    for i, (fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, ("embed_bwd_params", i, rc, want, L.mmf_last_error())
        assert b"mmf_deberta_embed_bwd_params" in L.mmf_last_error()
    assert lib.deberta_embed_bwd_params_workspace_bytes(0, d) == 0 and lib.deberta_embed_bwd_params_workspace_bytes(rows, 0) == 0

    def sc(i=p(ids), mk=None, kind=0, dr=p(f), t=p(nan32), r=rows, dd=d, v=vocab):
        return L.mmf_embedding_scatter_add_f32(i, mk, kind, dr, t, r, dd, v, s)
    cases = [
        (lambda: sc(i=None), E_SHAPE), (lambda: sc(dr=None), E_SHAPE), (lambda: sc(t=None), E_SHAPE), (lambda: sc(r=0), E_SHAPE),
        (lambda: sc(v=0), E_SHAPE), (lambda: sc(kind=2), E_SHAPE), (lambda: sc(mk=p(f)), E_SHAPE),
        (lambda: sc(dr=p(f, 4)), E_ALIGN), (lambda: sc(t=p(nan32, 8)), E_ALIGN), (lambda: sc(i=p(ids) + 4), E_ALIGN),
        (lambda: sc(mk=p(f) + 1, kind=1), E_ALIGN),
        (lambda: sc(dd=1028), E_UNSUPPORTED), (lambda: sc(dd=6), E_UNSUPPORTED), (lambda: sc(r=(1 << 30) + 1), E_UNSUPPORTED),
    ]
    for i, (fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, ("scatter_add", i, rc, want, L.mmf_last_error())
        assert b"mmf_embedding_scatter_add_f32" in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan32).all()) and bool(torch.isnan(ws).all())              # nothing was launched
