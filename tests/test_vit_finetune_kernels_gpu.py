"""GPU: the kernels the ViT backward adds, each against float64 on the operands it was given.

``mmf_layernorm_bwd_add_grouped`` (dx = r + LNbwd(dy)) in both backward forms with tests/test_kernel_forms_gpu.py's LayerNorm
bounds; ``mmf_vit_embed_tokens_bwd`` and ``mmf_sum_slabs_f32`` / ``FrozenBackbone._wgrad(slabs=...)`` within f32 summation noise
(``F32_TOL`` of tests/test_deberta_grad_gpu.py times the sum of the terms' magnitudes); ``mmf_attn_bwd_grouped`` in the layout of the
CLS route's last layer (``Tq = 1``, ``ldq = T * 3d``, one fused ``dqkv`` buffer) with tests/attn_ref.py's bounds as
tests/test_attention_paths_gpu.py applies them; and ``mmf_vit_cls_attn_bwd``, the f32 backward of that one query per image which
the ViT's walk uses in its place (a row of its dS sums to zero), against float64 with the bf16 outputs' 2^-8 bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vit_ref  # noqa: E402
from mmfusion import lib  # noqa: E402
from test_attention_paths_gpu import Case, bits, rec, scale_of  # noqa: E402,F401
from test_deberta_grad_gpu import E_ALIGN, E_SHAPE, E_UNSUPPORTED, F32_TOL  # noqa: E402
from test_kernel_forms_gpu import BF16_TOL, DEV, NAN, bf, f32, host, lane_id, ln_inputs, ln_ref, nan_like, rel, rnd  # noqa: E402
from test_kernel_forms_gpu import EPS as LN_EPS  # noqa: E402
from test_kernel_forms_gpu import F32_TOL as LN_F32_TOL  # noqa: E402

BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------- LayerNorm backward + residual
def _ln_run(d, rows, seed, resid, add=True, alias=False):
    """forward (for the statistics) and one backward on one problem; ``resid`` (rows, d) float64 or None -> dx, dgamma, dbeta on
    the device and the operands as the kernels saw them"""
    L = lib.load()
    (x,), (gam,), (bet,), (dy,) = ln_inputs(d, [rows], seed)
    x16, dy16, g32, b32 = bf(x), bf(dy), f32(gam), f32(bet)
    y, mean, rstd = nan_like((rows, d), BF16), nan_like((rows,)), nan_like((rows,))
    dx = nan_like((rows, d), BF16)
    r16 = None
    if add:
        r16 = bf(resid)
        if alias:
            dx.copy_(r16)
            r16 = dx
    dg0, db0 = rnd(d, seed=900).float().double(), rnd(d, seed=950).float().double()
    dg, db = f32(dg0), f32(db0)
    prob = lambda yy: [lib.LnProblem(x16.data_ptr(), yy, g32.data_ptr(), b32.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                     dy16.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows)]
    lib.layernorm_fwd_grouped(prob(y.data_ptr()), d, LN_EPS)
    ws = torch.full((L.mmf_layernorm_bwd_workspace_bytes(d) // 4,), NAN, dtype=torch.float32, device=DEV)
    r_host = None if r16 is None else host(r16)
    if add:
        lib.layernorm_bwd_add_grouped(prob(r16.data_ptr()), d, ws)
    else:
        lib.layernorm_bwd_grouped(prob(y.data_ptr()), d, ws)
    form = L.mmf_layernorm_last_form()
    torch.cuda.synchronize()
    return dict(dx=dx, dg=dg, db=db, ws=ws, x=host(x16), dy=host(dy16), gam=host(g32), bet=host(b32), r=r_host, dg0=dg0, db0=db0, form=form)


def _same_bits(a, b):
    """dx bit for bit; dgamma / dbeta bit for bit where the kernel under test leaves them: its per-workgroup column sums in the
    workspace (NaN-filled beforehand, so the workgroup count is compared too).  Behind them the finalize pass, which both
    entries share, adds each problem's partial sums with one f32 atomic per slice of workgroups, in whatever order the slices
    arrive: from two workgroups on, the last bits of the summed dgamma / dbeta differ between two runs of the SAME call, so
    those are compared bit for bit for one workgroup (rows <= 4) and within the LayerNorm cases' f32 bound otherwise"""
    assert torch.equal(bits(a["dx"]), bits(b["dx"])), "dx"
    assert torch.equal(bits(a["ws"]), bits(b["ws"])), "the workgroups' dgamma / dbeta sums"
    for k in ("dg", "db"):
        if a["dx"].shape[0] <= 4:
            assert torch.equal(bits(a[k]), bits(b[k])), k
        assert rel(a[k], host(b[k])) < LN_F32_TOL, k


@pytest.mark.parametrize("rows", [1, 37, 300])
@pytest.mark.parametrize("d", [768, 520], ids=["lane768", "chunk520"])
def test_layernorm_bwd_add_against_float64(d, rows):
    resid = rnd(rows, d, seed=77 + rows) * 0.7
    o = _ln_run(d, rows, seed=d + rows, resid=resid)
    assert o["form"] == (lane_id(d) if d == 768 else (d + 511) // 512)
    _, _, _, dxr, dgr, dbr = ln_ref(o["x"], o["gam"], o["bet"], o["dy"])
    e_dx, e_dg, e_db = rel(o["dx"], dxr + o["r"]), rel(o["dg"], dgr + o["dg0"]), rel(o["db"], dbr + o["db0"])
    print(f"layernorm_bwd_add d={d} rows={rows}: dx {e_dx:.3e} (bound {BF16_TOL:.3e}), dgamma {e_dg:.3e}, dbeta {e_db:.3e} (bound {LN_F32_TOL})")
    assert e_dx < BF16_TOL and e_dg < LN_F32_TOL and e_db < LN_F32_TOL
    # the residual aliasing dx: the same bits
    a = _ln_run(d, rows, seed=d + rows, resid=resid, alias=True)
    _same_bits(a, o)


@pytest.mark.parametrize("rows", [1, 37, 300])
@pytest.mark.parametrize("d", [768, 520], ids=["lane768", "chunk520"])
def test_layernorm_bwd_add_of_zero_is_the_plain_backward(d, rows):
    z = _ln_run(d, rows, seed=3 * d + rows, resid=torch.zeros(rows, d, dtype=torch.float64))
    p = _ln_run(d, rows, seed=3 * d + rows, resid=None, add=False)
    assert z["form"] == p["form"]
    _same_bits(z, p)


def test_layernorm_bwd_add_refusals_launch_nothing():
    L = lib.load()
    d, rows = 768, 8
    nan16 = torch.full((rows * d + 8,), NAN, dtype=BF16, device=DEV)
    nan32 = torch.full((2 * d,), NAN, device=DEV)
    x = torch.zeros(rows * d + 8, dtype=BF16, device=DEV)
    v = torch.ones(d + 4, device=DEV)
    st = torch.ones(rows, device=DEV)
    need = L.mmf_layernorm_bwd_workspace_bytes(d)
    ws = torch.full((need // 4 + 4,), NAN, device=DEV)
    s = lib.stream_ptr()

    def call(r=x.data_ptr(), dx=nan16.data_ptr(), dy=x.data_ptr(), w=ws.data_ptr(), wb=need, dd=d, n=1, nrows=rows, dg=nan32.data_ptr()):
        arr = (lib.LnProblem * 1)(lib.LnProblem(x.data_ptr(), r, v.data_ptr(), None, st.data_ptr(), st.data_ptr(), dy, dx, dg,
                                                nan32.data_ptr() + 4 * d, nrows))
        return L.mmf_layernorm_bwd_add_grouped(arr, n, dd, w, wb, s)
    cases = [(lambda: call(r=None), E_SHAPE), (lambda: call(dx=None), E_SHAPE), (lambda: call(dg=None), E_SHAPE), (lambda: call(nrows=0), E_SHAPE),
             (lambda: call(w=None), E_SHAPE), (lambda: call(wb=need - 4), E_SHAPE), (lambda: call(n=0), E_SHAPE), (lambda: call(n=9), E_SHAPE),
             (lambda: call(dd=12), E_SHAPE), (lambda: call(dd=2056), E_SHAPE),
             (lambda: call(r=x.data_ptr() + 2), E_ALIGN), (lambda: call(dx=nan16.data_ptr() + 2), E_ALIGN), (lambda: call(dy=x.data_ptr() + 4), E_ALIGN)]
    for i, (fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, (i, rc, want, L.mmf_last_error())
        assert b"mmf_layernorm_bwd_add_grouped" in L.mmf_last_error()
    assert call() == 0                                              # (the same call with nothing wrong is accepted)
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16[rows * d:]).all()) and not bool(torch.isnan(nan16[:rows * d]).any())
    nan16.fill_(NAN), nan32.fill_(NAN), ws.fill_(NAN)
    for fn, _ in cases:
        fn()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all()) and bool(torch.isnan(ws).all())


# ---------------------------------------------------------------------------------------- embedding backward
EMBED_CASES = [(1, 2, 256), (3, 17, 256), (5, 145, 768)]


def _embed_bwd(N, T, d, seed, fill):
    g = rnd(N * T, d, seed=seed).to(BF16)
    dcls = (rnd(d, seed=seed + 1) * fill).float().to(DEV)
    dpos = (rnd(T, d, seed=seed + 2) * fill).float().to(DEV)
    before = (dcls.cpu().double(), dpos.cpu().double())
    gd = g.to(DEV)
    keep = bits(gd)
    dpe = nan_like((N * (T - 1), d), BF16)
    lib.vit_embed_tokens_bwd(gd, dcls, dpos, dpe, N, T, d)
    torch.cuda.synchronize()
    assert torch.equal(bits(gd), keep), "the token gradient was written"
    return g.double().view(N, T, d), before, dcls.cpu(), dpos.cpu(), dpe.cpu()


@pytest.mark.parametrize("N,T,d", EMBED_CASES)
@pytest.mark.parametrize("fill", [0.0, 3.0], ids=["zeroed", "prefilled"])
def test_embed_tokens_bwd_against_float64(N, T, d, fill):
    g, (c0, p0), dcls, dpos, dpe = _embed_bwd(N, T, d, 40 + T, fill)
    want_pos, mag_pos = g.sum(0) + p0, g.abs().sum(0) + p0.abs()
    want_cls, mag_cls = g[:, 0].sum(0) + c0, g[:, 0].abs().sum(0) + c0.abs()
    worst_pos = float(((dpos.double() - want_pos).abs() - F32_TOL * mag_pos).max())
    worst_cls = float(((dcls.double() - want_cls).abs() - F32_TOL * mag_cls).max())
    print(f"vit_embed_tokens_bwd N={N} T={T} d={d} fill={fill}: worst (|err| - F32_TOL sum|terms|): dpos {worst_pos:.3e}, dcls {worst_cls:.3e}")
    assert worst_pos <= 0 and worst_cls <= 0
    assert torch.equal(bits(dpe), bits(g[:, 1:].reshape(N * (T - 1), d).to(BF16))), "the patch gradient is not rows 1 .. T-1"
    again = _embed_bwd(N, T, d, 40 + T, fill)
    assert torch.equal(bits(again[2]), bits(dcls)) and torch.equal(bits(again[3]), bits(dpos)) and torch.equal(bits(again[4]), bits(dpe))


def test_embed_tokens_bwd_refusals_launch_nothing():
    L = lib.load()
    s = lib.stream_ptr()
    g = torch.zeros(1 << 14, dtype=BF16, device=DEV)
    nan16 = torch.full((1 << 14,), NAN, dtype=BF16, device=DEV)
    nan32 = torch.full((1 << 14,), NAN, device=DEV)
    half = nan32.data_ptr() + 4 * (1 << 13)

    def call(gp=g.data_ptr(), c=nan32.data_ptr(), p=half, pe=nan16.data_ptr(), N=2, T=4, d=64):
        return L.mmf_vit_embed_tokens_bwd(gp, c, p, pe, N, T, d, s)
    cases = [(lambda: call(gp=None), E_SHAPE), (lambda: call(c=None), E_SHAPE), (lambda: call(p=None), E_SHAPE), (lambda: call(pe=None), E_SHAPE),
             (lambda: call(N=0), E_SHAPE), (lambda: call(T=1), E_SHAPE), (lambda: call(d=0), E_SHAPE),
             (lambda: call(d=60), E_UNSUPPORTED), (lambda: call(N=65536), E_UNSUPPORTED),
             (lambda: call(gp=g.data_ptr() + 2), E_ALIGN), (lambda: call(c=nan32.data_ptr() + 4), E_ALIGN), (lambda: call(p=half + 8), E_ALIGN),
             (lambda: call(pe=nan16.data_ptr() + 2), E_ALIGN)]
    for i, (fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, (i, rc, want, L.mmf_last_error())
        assert b"mmf_vit_embed_tokens_bwd" in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all())


# ---------------------------------------------------------------------------------------- K-slab weight gradients
@pytest.mark.parametrize("slabs,accumulate", [(1, False), (3, True), (7, False), (64, True)])
def test_sum_slabs_is_the_ordered_f32_sum(slabs, accumulate):
    n = 4 * 1237
    part = rnd(slabs, n, seed=slabs).float()
    out0 = rnd(n, seed=99).float()
    want = out0.clone() if accumulate else torch.zeros(n)
    for s_ in range(slabs):
        want = want + part[s_]                                        # f32, slab 0 first: the kernel's chain, so the bits agree
    out = out0.to(DEV)
    lib.sum_slabs(part.to(DEV), out, accumulate)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))


def test_sum_slabs_refusals_launch_nothing():
    L = lib.load()
    s = lib.stream_ptr()
    p = torch.zeros(1024, device=DEV)
    out = torch.full((256,), NAN, device=DEV)
    cases = [(lambda: L.mmf_sum_slabs_f32(None, out.data_ptr(), 64, 2, 0, s), E_SHAPE), (lambda: L.mmf_sum_slabs_f32(p.data_ptr(), None, 64, 2, 0, s), E_SHAPE),
             (lambda: L.mmf_sum_slabs_f32(p.data_ptr(), out.data_ptr(), 0, 2, 0, s), E_SHAPE), (lambda: L.mmf_sum_slabs_f32(p.data_ptr(), out.data_ptr(), 64, 0, 0, s), E_SHAPE),
             (lambda: L.mmf_sum_slabs_f32(p.data_ptr(), out.data_ptr(), 8, 65, 0, s), E_SHAPE), (lambda: L.mmf_sum_slabs_f32(p.data_ptr(), out.data_ptr(), 66, 2, 0, s), E_ALIGN),
             (lambda: L.mmf_sum_slabs_f32(p.data_ptr() + 4, out.data_ptr(), 64, 2, 0, s), E_ALIGN), (lambda: L.mmf_sum_slabs_f32(p.data_ptr(), out.data_ptr() + 8, 64, 2, 0, s), E_ALIGN)]
    for i, (fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, (i, rc, want, L.mmf_last_error())
        assert b"mmf_sum_slabs_f32" in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


_wgrad_case = {}


def _wgrad_operands():
    """rows 1000 (no slab count divides them evenly) x fc1 of the tiny ViT (1024 x 256); the float64 products, once"""
    if not _wgrad_case:
        dy, x = rnd(1000, 1024, seed=5).to(BF16), (rnd(1000, 256, seed=6) + 0.3).to(BF16)
        a, b = dy.double(), x.double()
        _wgrad_case.update(dy=dy, x=x, w=a.T @ b, wmag=a.abs().T @ b.abs(), b=a.sum(0), bmag=a.abs().sum(0))
    return _wgrad_case


@pytest.mark.parametrize("slabs", [1, 3, 7])
def test_wgrad_slabs_against_float64_and_the_arena_protocol(slabs):
    from mmfusion import arena
    from mmfusion.vit import NativeViT
    c = _wgrad_operands()
    m = NativeViT(**vit_ref.config_kwargs(vit_ref.tiny_config())).cuda()
    ar = arena.ensure(m)
    dy, x = c["dy"].to(DEV), c["x"].to(DEV)
    w, b = m.l1_fc1_w.grad, m.l1_fc1_b.grad
    assert len(m._slab_bounds(1000, slabs)) - 1 == slabs

    def check(tag, times, fill=0.0):
        torch.cuda.synchronize()
        ew = float(((w.cpu().double() - times * c["w"] - fill).abs() - F32_TOL * (times * c["wmag"] + abs(fill))).max())
        eb = float(((b.cpu().double() - times * c["b"]).abs() - F32_TOL * times * c["bmag"]).max())
        print(f"_wgrad slabs={slabs} {tag}: worst (|err| - F32_TOL sum|terms|): weight {ew:.3e}, bias {eb:.3e}")
        assert ew <= 0 and eb <= 0
    ar.zero_grad()
    m._wgrad(dy, x, "l1_fc1", slabs)
    check("onto zeros", 1)
    first = bits(w)
    m._wgrad(dy, x, "l1_fc1", slabs)
    check("a second time: accumulates", 2)
    ar.zero_grad()
    w.fill_(0.5)
    m._wgrad(dy, x, "l1_fc1", slabs)
    check("onto what the buffer holds", 1, fill=0.5)
    # lazy zeroing: the first launch of a step overwrites what the gradient holds, the next accumulates
    ar.zero_grad(lazy=True)
    w.fill_(1e3)
    m._wgrad(dy, x, "l1_fc1", slabs)
    check("first touch after zero_grad(lazy=True): overwrites", 1)
    assert torch.equal(bits(w), first), "two runs differ"
    m._wgrad(dy, x, "l1_fc1", slabs)
    ar.finalize_grads()
    check("second touch: accumulates", 2)


# ---------------------------------------------------------------------------------------- attention backward, CLS layout
class _Win:
    """a rows x d window at column ``off`` of a shared (.., ld) bf16 buffer, with ``Mat``'s surface"""

    def __init__(self, buf, rows, d, ld, off, values=None):
        self.buf, self.rows, self.d = buf, rows, d
        self.v = torch.as_strided(buf, (rows, d), (ld, 1), off)
        if values is not None:
            self.v.copy_(values.reshape(rows, d).to(BF16))
        self.off = off

    def mark(self):
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 2 * self.off

    def guards_intact(self):
        return True                                                 # (the shared buffers are checked as a whole by the test)

    def untouched(self):
        return bool(torch.equal(bits(self.buf), bits(self.before)))

    def host(self):
        return self.v.detach().cpu().double()


class ClsCase(Case):
    """``Case`` in ``NativeViT._layer_cls``'s layout: q | k | v fused in one (B T, 3d) buffer, the query row 0 of each item
    (``Tq = 1``, ``ldq = T * 3d``), and dQ | dK | dV fused the same way in one NaN-filled buffer"""

    def __init__(self, dh, B, H, T, seed):
        Case.__init__(self, dh, B, H, 1, T, seed=seed)
        d = self.d
        self.qkv = torch.full((B * T + 2, 3 * d), 777.0, dtype=BF16, device=DEV)
        self.dqkv = torch.full((B * T + 2, 3 * d), NAN, dtype=BF16, device=DEV)
        self.ldq, self.ldk, self.ldv = T * 3 * d, 3 * d, 3 * d
        self.Q, self.K, self.V = _Win(self.qkv, B, d, self.ldq, 0, self.q), _Win(self.qkv, B * T, d, 3 * d, d, self.k), _Win(self.qkv, B * T, d, 3 * d, 2 * d, self.v)
        self.dQ, self.dK, self.dV = _Win(self.dqkv, B, d, self.ldq, 0), _Win(self.dqkv, B * T, d, 3 * d, d), _Win(self.dqkv, B * T, d, 3 * d, 2 * d)
        for w in (self.Q, self.K, self.V, self.dQ, self.dK, self.dV):
            w.mark()


@pytest.mark.parametrize("T", [17, 145])
def test_attention_backward_in_the_cls_layout(rec, T):
    dh, B, H = 64, 3, 4
    c = ClsCase(dh, B, H, T, seed=T)
    d, scale = c.d, scale_of(dh)
    c.reference(scale)
    fails = []
    probs = [c.problem()]
    lib.attn_fwd_grouped(probs, dh, scale)
    torch.cuda.synchronize()
    c.check_forward(rec, fails)
    c.hand_reference_forward_to_backward()
    lib.attn_bwd_grouped(probs, dh, scale)
    torch.cuda.synchronize()
    c.check_backward(rec, fails)
    assert not fails, "\n".join(fails)
    got = c.dqkv.cpu().float()
    q_cols = got[:B * T, :d].view(B, T, d)
    assert bool(torch.isnan(q_cols[:, 1:]).all()), "dQ columns of rows other than row 0 were written"
    assert bool(torch.isnan(got[B * T:]).all()), "rows behind the buffer were written"
    assert not bool(torch.isnan(q_cols[:, 0]).any()) and not bool(torch.isnan(got[:B * T, d:]).any())


@pytest.mark.parametrize("cls", [False, True], ids=["full", "cls"])
@pytest.mark.parametrize("slabs", [1, 3])
def test_fused_qkv_wgrad_parts_share_one_slab_launch(monkeypatch, slabs, cls):
    """``NativeViT._qkv_wgrad`` on 59 images of 17 tokens (1003 rows), the slab count forced: the q | k | v row blocks of the fused
    weight as parts of one launch (the ``cls`` form: k | v over every row, q over row 0 of each image), against float64; the key
    bias stays exactly zero"""
    from mmfusion import arena
    from mmfusion.vit import NativeViT
    m = NativeViT(**vit_ref.config_kwargs(vit_ref.tiny_config())).cuda()
    ar = arena.ensure(m)
    n, T, d = 59, m.T, m.config.hidden_size
    monkeypatch.setattr(NativeViT, "_slabs_for", staticmethod(lambda rows, tiles: slabs))
    dqkv, ln = rnd(n * T, 3 * d, seed=11).to(BF16), (rnd(n * T, d, seed=12) + 0.3).to(BF16)
    a, b = dqkv.double(), ln.double()
    a0, b0 = a.view(n, T, 3 * d)[:, 0, :d], b.view(n, T, d)[:, 0]
    want_w, mag_w = a.T @ b, a.abs().T @ b.abs()
    want_b, mag_b = a.sum(0), a.abs().sum(0)
    if cls:
        want_w[:d], mag_w[:d], want_b[:d], mag_b[:d] = a0.T @ b0, a0.abs().T @ b0.abs(), a0.sum(0), a0.abs().sum(0)
    want_b[d:2 * d], mag_b[d:2 * d] = 0.0, 0.0
    g = m._grad_workspace(torch.device("cuda", torch.cuda.current_device()))
    ar.zero_grad()
    for times in (1, 2):
        m._qkv_wgrad(1, g, dqkv.to(DEV), ln.to(DEV), n, cls)
        torch.cuda.synchronize()
        w, bias = m.l1_qkv_w.grad.cpu().double(), m.l1_qkv_b.grad.cpu().double()
        ew = float(((w - times * want_w).abs() - F32_TOL * times * mag_w).max())
        eb = float(((bias - times * want_b).abs() - F32_TOL * times * mag_b).max())
        print(f"_qkv_wgrad slabs={slabs} cls={cls} x{times}: worst (|err| - F32_TOL sum|terms|): weight {ew:.3e}, bias {eb:.3e}")
        assert ew <= 0 and eb <= 0
        assert not bool(bias[d:2 * d].any()), "the key bias received a gradient"


# ---------------------------------------------------------------------------------------- the CLS query's attention backward
def _cls_attn_ref(qkv, dout, n, H, T, dh, scale):
    """float64: the backward of softmax attention of row 0 of each image over its T keys -> dq (n, d), dk, dv (n T, d)"""
    d = H * dh
    x = qkv.view(n, T, 3, H, dh)
    q, k, v = x[:, 0, 0], x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)          # (n, H, dh), (n, H, T, dh) x 2
    do = dout.view(n, H, dh)
    p = torch.softmax(torch.einsum("nhc,nhtc->nht", q, k) * scale, -1)
    dp = torch.einsum("nhc,nhtc->nht", do, v)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dq = torch.einsum("nht,nhtc->nhc", ds, k) * scale
    dk = torch.einsum("nht,nhc->nthc", ds, q) * scale
    dv = torch.einsum("nht,nhc->nthc", p, do)
    return dq.reshape(n, d), dk.reshape(n * T, d), dv.reshape(n * T, d), float(ds.sum(-1).abs().max())


@pytest.mark.parametrize("n,H,T,dh", [(3, 4, 17, 64), (3, 4, 145, 64), (2, 2, 33, 96), (2, 3, 1, 64), (1, 1, 700, 64)])
def test_cls_attn_bwd_against_float64(n, H, T, dh):
    """bf16 outputs held to 2^-8 of the tensor's scale (tests/test_kernel_forms_gpu.py's rule for them); the q columns of the rows
    other than row 0 and the rows behind the buffer keep their NaN; two runs give the same bits; the operands are not written"""
    d, scale = H * dh, float(torch.tensor(dh ** -0.5, dtype=torch.float32))
    qkv = rnd(n * T, 3 * d, seed=T + dh).to(BF16)
    qkv[:, :2 * d] *= 1.5                                             # (scores a few units apart: a softmax far from uniform)
    dout = rnd(n, d, seed=T + dh + 1).to(BF16)
    dq, dk, dv, rowsum = _cls_attn_ref(qkv.double(), dout.double(), n, H, T, dh, scale)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    before = (bits(qd), bits(dd))
    runs = []
    for _ in range(2):
        buf = torch.full((n * T + 2, 3 * d), NAN, dtype=BF16, device=DEV)
        lib.vit_cls_attn_bwd(qd, dd, buf[:n * T], n, H, T, dh, scale)
        torch.cuda.synchronize()
        runs.append(buf.cpu())
    assert torch.equal(bits(qd), before[0]) and torch.equal(bits(dd), before[1]), "an operand was written"
    got = runs[0].float()
    g_q = got[:n * T, :d].view(n, T, d)
    assert bool(torch.isnan(g_q[:, 1:]).all()) and bool(torch.isnan(got[n * T:]).all()), "written outside dq's row 0 / the buffer"
    e_q, e_k, e_v = rel(g_q[:, 0], dq), rel(got[:n * T, d:2 * d], dk), rel(got[:n * T, 2 * d:], dv)
    print(f"vit_cls_attn_bwd n={n} H={H} T={T} dh={dh}: dq {e_q:.3e}, dk {e_k:.3e}, dv {e_v:.3e} (bound {BF16_TOL:.3e}); "
          f"the reference's largest |sum_j dS_j| {rowsum:.1e}")
    assert e_q < BF16_TOL and e_k < BF16_TOL and e_v < BF16_TOL
    # the point of the kernel: a row of dS sums to zero, so the dk of one (image, head) sum to the rounding of the terms (bf16: at most 2^-8 of each)
    sum_dk = got[:n * T, d:2 * d].double().view(n, T, d).sum(1)
    noise = 2.0 ** -8 * got[:n * T, d:2 * d].double().abs().view(n, T, d).sum(1) + 1e-30
    assert bool((sum_dk.abs() <= noise).all()), float((sum_dk.abs() / noise).max())
    assert torch.equal(bits(runs[0]), bits(runs[1])), "two runs differ"


def test_cls_attn_bwd_refusals_launch_nothing():
    L = lib.load()
    s = lib.stream_ptr()
    a = torch.zeros(1 << 14, dtype=BF16, device=DEV)
    nan16 = torch.full((1 << 14,), NAN, dtype=BF16, device=DEV)
    p = lambda t, off=0: t.data_ptr() + off

    def call(q=p(a), do=p(a), dq=p(nan16), N=2, H=2, T=4, dh=64):
        return L.mmf_vit_cls_attn_bwd(q, do, dq, N, H, T, dh, 0.125, s)
    cases = [(lambda: call(q=None), E_SHAPE), (lambda: call(do=None), E_SHAPE), (lambda: call(dq=None), E_SHAPE), (lambda: call(N=0), E_SHAPE),
             (lambda: call(H=0), E_SHAPE), (lambda: call(T=0), E_SHAPE), (lambda: call(dh=32), E_UNSUPPORTED), (lambda: call(dh=128), E_UNSUPPORTED),
             (lambda: call(T=4097), E_UNSUPPORTED), (lambda: call(N=65536), E_UNSUPPORTED),
             (lambda: call(q=p(a, 2)), E_ALIGN), (lambda: call(do=p(a, 8)), E_ALIGN), (lambda: call(dq=p(nan16, 4)), E_ALIGN)]
    for i, (fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, (i, rc, want, L.mmf_last_error())
        assert b"mmf_vit_cls_attn_bwd" in L.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all())
