"""GPU: fine-tuning the native DeBERTa's top layers.  ``mmf_deberta_attn_bwd_pos`` (the attention backward that also returns the
gradient of the position tables) against the float64 closed form tests/deberta_wgrad_ref.py, then the weight gradients of
``NativeDeberta.set_trainable_layers(k)`` against float64 autograd through the restatement tests/deberta_ref.py, the arena's
accumulation protocol, the optimiser step through ``TextEncoder``, and graph capture.

Bounds.  Kernel: tests/test_deberta_grad_gpu.py's, ||got - want|| <= BOUND_A ||want|| + ||N|| with N the f32-noise term of
``table_gradients(f32_tol=F32_TOL)`` (T = 1 has a one-hot softmax: the true gradient is 0 and the kernel returns that noise); the
operands are that file's: the reference's O rounded to bf16 and its lse in f32.  Module: rule (b) per parameter tensor in
absolute form, ||got - exact|| <= 2 ||stored - exact||, ``exact`` / ``stored`` the autograd gradients of
``deberta_ref.deberta_forward`` without / with ``bf16_storage`` on the state dict's tensors as leaves; both sides are computed
here and printed per tensor."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_ref  # noqa: E402
import deberta_wgrad_ref as WG  # noqa: E402
from helpers import BOUND_A, _lib, l2_rel  # noqa: E402
from test_deberta_gpu import _inputs, _model  # noqa: E402
from test_deberta_grad_gpu import ATTN_CASES, E_ALIGN, E_SHAPE, E_UNSUPPORTED, F32_TOL, SCALE, _attn_bwd_case, _attn_bwd_run, _bits, _heads  # noqa: E402

BF16 = torch.bfloat16
POS_CASES = ATTN_CASES + [(1, 2, 33, 256, 512, None)]          # ... and a table of 512 rows of which 65 are reached
_want = {}


def _pos_want(n, H, T, S, max_pos, pad):
    """the float64 dposq | dposk as one (2S, 2 H 64) tensor and the norms of the two noise terms, once per case"""
    key = (n, H, T, S, max_pos, pad)
    if key not in _want:
        c = _attn_bwd_case(*key)
        d = H * 64
        q, k, v = (_heads(c["qkv"].double()[:, i * d:(i + 1) * d], n, T, H) for i in range(3))
        pq, pk = (t.double().reshape(2 * S, H, 64).transpose(0, 1) for t in (c["posq"], c["posk"]))
        dq, dk, nq, nk = WG.table_gradients(q, k, v, pq, pk, c["idx"], c["mask"], SCALE, _heads(c["dout"].double(), n, T, H),
                                            O=_heads(c["o16"].double(), n, T, H), lse=c["lse32"].double(), f32_tol=F32_TOL)
        flat = lambda t: t.transpose(0, 1).reshape(2 * S, d)
        _want[key] = (torch.cat([flat(dq), flat(dk)], dim=1), float(nq.norm()), float(nk.norm()))
    return _want[key]


def _pos_run(c, n, H, T, S, mask_dtype=torch.float32, fill=None):
    """-> (dqkv, dpos (2S, 2 H 64) = dposq | dposk) on the CPU; ``fill``: what dpos holds before the call (None: zeros)"""
    lib = _lib()
    d = H * 64
    dev = {k: c[k].cuda() for k in ("qkv", "posq", "posk", "idx", "dout", "o16", "lse32")}
    m = None if c["mask"] is None else c["mask"].to(mask_dtype).cuda()
    before = {k: _bits(dev[k]) for k in ("qkv", "posq", "posk", "o16", "lse32", "dout")}
    dqkv = torch.full((n * T, 3 * d), float("nan"), dtype=BF16, device="cuda")
    delta = torch.empty(n * H * T, device="cuda")
    dpos = torch.zeros(2 * S, 2 * d, device="cuda") if fill is None else fill.cuda().clone()
    nbytes = lib.deberta_attn_bwd_pos_workspace_bytes(n, H, T, S)
    assert nbytes == 2 * n * ((T + 63) // 64) * H * 2 * S * 64 * 4
    ws = torch.full((nbytes // 4,), float("nan"), device="cuda")                       # it need not be initialised
    lib.deberta_attn_bwd_pos(dev["qkv"], dev["posq"], dev["posk"], dev["idx"], m, dev["o16"], dev["lse32"].reshape(-1), dev["dout"], delta,
                             dqkv, dpos[:, :d], dpos[:, d:], ws, n, H, T, S, SCALE)
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(_bits(dev[k]), b), f"{k} was written"
    return dqkv.cpu(), dpos.cpu()


def _check_pos(n, H, T, S, max_pos, pad, mask_dtype=torch.float32):
    c = _attn_bwd_case(n, H, T, S, max_pos, pad)
    want, nq, nk = _pos_want(n, H, T, S, max_pos, pad)
    d = H * 64
    dqkv, dpos = _pos_run(c, n, H, T, S, mask_dtype)
    dqkv2, dpos2 = _pos_run(c, n, H, T, S, mask_dtype)
    plain = _attn_bwd_run(c, n, H, T, S, mask_dtype)
    # 1. dqkv is mmf_deberta_attn_bwd's, bit for bit
    assert not torch.isnan(dqkv.float()).any() and torch.equal(_bits(dqkv), _bits(plain)), "dqkv differs from mmf_deberta_attn_bwd's"
    # 4. two runs give the same bits
    assert torch.equal(_bits(dpos), _bits(dpos2)) and torch.equal(_bits(dqkv), _bits(dqkv2)), "two runs differ"
    # 2. against float64
    assert bool(torch.isfinite(dpos).all())
    for name, got, w, nz in (("dposQ", dpos[:, :d].double(), want[:, :d], nq), ("dposK", dpos[:, d:].double(), want[:, d:], nk)):
        err, bound = float((got - w).norm()), BOUND_A * float(w.norm()) + nz
        print(f"deberta table gradient {name} n={n} H={H} T={T} S={S} max_pos={max_pos} pad={pad} ({mask_dtype}): error / bound "
              f"{err / bound:.3e}; rel L2 {l2_rel(got, w):.3e}; f32 noise term / BOUND_A ||want|| {nz / max(BOUND_A * float(w.norm()), 1e-300):.1e}")
        assert err <= bound, (name, err, bound)
    # 3. rows no (i, j) pair maps to hold exactly 0
    rest = torch.ones(2 * S, dtype=torch.bool)
    rest[WG.reached_rows(c["idx"])] = False
    assert bool((dpos[rest] == 0).all()) and bool((want[rest] == 0).all())
    return c, dpos, want


@pytest.mark.parametrize("n,H,T,S,max_pos,pad", [c for c in POS_CASES if c[5] is None])
def test_table_gradients_against_float64(n, H, T, S, max_pos, pad):
    _check_pos(n, H, T, S, max_pos, pad)


@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.uint8, torch.bool])
def test_table_gradients_with_a_padded_item(mask_dtype):
    _check_pos(*ATTN_CASES[2], mask_dtype=mask_dtype)


@pytest.mark.parametrize("n,H,T,S,max_pos,pad", [POS_CASES[2], POS_CASES[3], POS_CASES[5]])
def test_table_gradients_are_added_to_what_the_buffers_hold(n, H, T, S, max_pos, pad):
    c = _attn_bwd_case(n, H, T, S, max_pos, pad)
    want, _, _ = _pos_want(n, H, T, S, max_pos, pad)
    g = torch.Generator().manual_seed(T + S)
    fill = torch.randn(2 * S, 2 * H * 64, generator=g) * float(want.abs().max())
    _, zero = _pos_run(c, n, H, T, S)
    _, got = _pos_run(c, n, H, T, S, fill=fill)
    tol = F32_TOL * torch.maximum(fill.abs().double(), want.abs())
    worst = float((((got - fill).double() - zero.double()).abs() - tol).max())
    print(f"accumulating table gradients n={n} H={H} T={T} S={S}: worst (|(got - c) - from zero| - F32_TOL max(|c|, |want|)) = {worst:.3e}")
    assert worst <= 0
    rest = torch.ones(2 * S, dtype=torch.bool)
    rest[WG.reached_rows(c["idx"])] = False
    assert torch.equal(got[rest], fill[rest])                                          # nothing is added to an unreached row


def test_pos_refusals_return_the_documented_codes_and_launch_nothing():
    lib = _lib()
    L = lib.load()
    s = lib.stream_ptr()
    nan16 = torch.full((1 << 16,), float("nan"), dtype=BF16, device="cuda")
    nan32 = torch.full((1 << 16,), float("nan"), device="cuda")
    f = torch.zeros(1 << 14, device="cuda")
    b = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    idx = torch.zeros(4096, dtype=torch.int32, device="cuda")
    need = lib.deberta_attn_bwd_pos_workspace_bytes(1, 2, 16, 8)
    ws = torch.full((need // 4,), float("nan"), device="cuda")
    p = lambda t, off=0: t.data_ptr() + off
    half = p(nan32, 4 * (1 << 15))

    def call(dq=p(nan32), dk=half, ld=128, w=p(ws), wb=need, lse=p(f), n=1, H=2, T=16, S=8, hd=64, dqkv=p(nan16)):
        return L.mmf_deberta_attn_bwd_pos(p(b), p(b), p(b), 128, p(idx), None, 0, p(b), lse, p(b), p(f), dqkv, n, H, T, S, hd, SCALE,
                                          dq, dk, ld, w, wb, s)
    cases = [
        (lambda: call(dq=None), E_SHAPE), (lambda: call(dk=None), E_SHAPE), (lambda: call(w=None), E_SHAPE),
        (lambda: call(wb=need - 4), E_SHAPE), (lambda: call(wb=0), E_SHAPE), (lambda: call(ld=64), E_SHAPE),
        (lambda: call(lse=None), E_SHAPE), (lambda: call(T=0), E_SHAPE),
        (lambda: call(dq=p(nan32, 4)), E_ALIGN), (lambda: call(dk=half + 8), E_ALIGN), (lambda: call(w=p(ws, 4), wb=need), E_ALIGN),
        (lambda: call(ld=130), E_ALIGN), (lambda: call(dqkv=p(nan16, 2)), E_ALIGN),
        (lambda: call(hd=96), E_UNSUPPORTED), (lambda: call(T=1025, wb=1 << 40), E_UNSUPPORTED), (lambda: call(S=257, wb=1 << 40), E_UNSUPPORTED),
    ]
    for i, (fn, want) in enumerate(cases):
        rc = fn()
        assert rc == want, (i, rc, want, L.mmf_last_error())
        assert b"mmf_deberta_attn_bwd_pos" in L.mmf_last_error()
    assert lib.deberta_attn_bwd_pos_workspace_bytes(0, 2, 16, 8) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan16).all()) and bool(torch.isnan(nan32).all()) and bool(torch.isnan(ws).all())      # nothing was launched


# ---- NativeDeberta: the weight gradients of the trainable top layers ---------------------------------------------------
def _layer_keys(cfg, k):
    L = cfg.num_hidden_layers
    return [key for key in deberta_ref.hf_keys(cfg) if any(key.startswith(f"encoder.layer.{i}.") for i in range(L - k, L))]


def _ref_wgrads(sd, x, mask, cfg, dout, dtype, bf16_storage, keys):
    """autograd through the restatement with the state dict's tensors as leaves of ``dtype`` (so its ``.to(dtype)`` is the
    identity) -> {key: gradient}"""
    leaves = {key: v.to(dtype).clone().requires_grad_(key in keys) for key, v in sd.items()}
    out = deberta_ref.deberta_forward(leaves, x if x.dtype == torch.int64 else x.to(dtype), mask, cfg, bf16_storage=bf16_storage, dtype=dtype)
    return dict(zip(keys, torch.autograd.grad(out, [leaves[key] for key in keys], dout.to(dtype))))


def _hf_grads(m, keys):
    out = {}
    for key in keys:
        name, rows, swapped = m._hf[key]
        g = getattr(m, name).grad
        assert g is not None and g.dtype == torch.float32 and not swapped, key
        out[key] = (g if rows is None else g[rows[0]:rows[1]]).detach().cpu().clone()
    return out


def _native_wgrads(m, x, mask, dout, keys, zero=True):
    """one forward + backward -> ({key: gradient}, the output); ``x``: ids, or embeddings (a leaf when they require a gradient)"""
    from mmfusion import arena
    ar = arena.ensure(m)
    if zero:
        ar.zero_grad()
    kw = dict(input_ids=x) if x.dtype == torch.int64 else dict(inputs_embeds=x)
    out = m(attention_mask=mask.cuda(), **kw).last_hidden_state
    assert out.requires_grad and out.dtype == torch.float32
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    return _hf_grads(m, keys), out.detach()


def _rule_b(what, got, exact, stored):
    worst = 0.0
    for key in exact:
        err, model = float((got[key].double() - exact[key].double()).norm()), float((stored[key].double() - exact[key].double()).norm())
        print(f"{what} {key}: ||got - exact|| {err:.3e} (bound (b) 2 x {model:.3e}), ||exact|| {float(exact[key].norm()):.3e}, "
              f"vs the bf16-storage gradient {float((got[key].double() - stored[key].double()).norm()):.3e}")
        assert bool(torch.isfinite(got[key]).all()) and got[key].shape == exact[key].shape
        worst = max(worst, err / max(2 * model, 1e-300))
    print(f"{what}: worst error / bound {worst:.3f}")
    for key in exact:
        err, model = float((got[key].double() - exact[key].double()).norm()), float((stored[key].double() - exact[key].double()).norm())
        assert err <= 2 * model, (key, err, 2 * model)


def _frozen_grads_are_empty(m):
    for name, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None or not bool(p.grad.any()), name


def _douts(cfg, n, T, seed):
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(n, T, cfg.hidden_size, generator=g)
    cls = torch.zeros_like(dout)
    cls[:, 0] = dout[:, 0]
    return dout, cls


@pytest.mark.parametrize("k", [1, 2])
def test_weight_gradients_against_float64_autograd_tiny(k):
    """2 layers, d 256, 4 heads, S 8; 2 items of 80 ids, the last padded from token 60; a random gradient of the result and one
    that is non-zero on row 0 of each item only"""
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 2, 80, 50, pad_from=60)
    m = _model(cfg, sd)
    with torch.no_grad():
        plain = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state.clone()
    m.set_trainable_layers(k)
    assert m.trainable_layers == k
    keys = _layer_keys(cfg, k)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted({m._hf[key][0] for key in keys})
    for tag, dout in zip(("random", "CLS-row"), _douts(cfg, 2, 80, 51)):
        exact = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float64, False, keys)
        stored = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float64, True, keys)
        got, out = _native_wgrads(m, ids.cuda(), mask, dout, keys)
        assert torch.equal(_bits(out), _bits(plain)), "the differentiable forward's bits are not the inference call's"
        _rule_b(f"NativeDeberta tiny 2 x 80, k={k}, {tag} dO,", got, exact, stored)
        _frozen_grads_are_empty(m)


def test_weight_gradients_against_autograd_base_sizes():
    """deberta-v3-base sizes (12 layers, d 768, 12 heads, S 256: the real GEMM shapes and the LayerNorm lane form), one item of 64
    ids padded from token 50, the top layer trainable, float32 references.

    The tightest tensors are the q / k biases, whose exact gradients are small (norms 4.2 and 3.9 beside 151 for db_v):
    ``query_proj.bias`` is 0.4946 from the exact gradient against a bound of 0.5138 (0.96 of it), ``key_proj.bias`` 0.3517
    against 0.4977 (0.71); ``query_proj.weight`` / ``key_proj.weight`` 12.44 / 12.90 against 19.75 / 20.08; the other twelve
    tensors sit at 0.50 to 0.54 of their bounds.  db_k is the case that pins the backward's choice to add NO column sum of dposK
    (it is identically zero in exact arithmetic): with it added, db_k carries the residue of the bf16 delta twice and measures
    0.5044, 1.014 of the bound."""
    cfg = deberta_ref.base_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 1, 64, 52, pad_from=50)
    dout, _ = _douts(cfg, 1, 64, 53)
    m = _model(cfg, sd)
    m.set_trainable_layers(1)
    keys = _layer_keys(cfg, 1)
    exact = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float32, False, keys)
    stored = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float32, True, keys)
    got, _ = _native_wgrads(m, ids.cuda(), mask, dout, keys)
    _rule_b("NativeDeberta base 1 x 64, k=1,", got, exact, stored)
    _frozen_grads_are_empty(m)


def test_prompt_route_keeps_its_input_gradient_and_gains_the_weight_gradients():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(54)
    emb = torch.randn(2, 80, cfg.hidden_size, generator=g)
    _, mask = _inputs(cfg, 2, 80, 55, pad_from=60)
    dout, _ = _douts(cfg, 2, 80, 56)
    keys = _layer_keys(cfg, 1)
    m0, m1 = _model(cfg, sd), _model(cfg, sd)
    m1.set_trainable_layers(1)
    leaf0, leaf1 = emb.cuda().requires_grad_(True), emb.cuda().requires_grad_(True)
    m0(inputs_embeds=leaf0, attention_mask=mask.cuda()).last_hidden_state.backward(dout.cuda())
    got, _ = _native_wgrads(m1, leaf1, mask, dout, keys)
    assert leaf1.grad is not None and torch.equal(_bits(leaf1.grad), _bits(leaf0.grad)), "d inputs_embeds changed with k = 1"
    exact = _ref_wgrads(sd, emb, mask, cfg, dout, torch.float64, False, keys)
    stored = _ref_wgrads(sd, emb, mask, cfg, dout, torch.float64, True, keys)
    _rule_b("NativeDeberta tiny prompt route, k=1,", got, exact, stored)
    # torch.autograd.grad for the embeddings alone: the same input gradient
    leaf2 = emb.cuda().requires_grad_(True)
    (g2,) = torch.autograd.grad(m1(inputs_embeds=leaf2, attention_mask=mask.cuda()).last_hidden_state, leaf2, dout.cuda())
    assert torch.equal(_bits(g2), _bits(leaf0.grad))


def test_chunking_changes_only_the_summation_order():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 5, 70, 57, pad_from=40)
    dout, _ = _douts(cfg, 5, 70, 58)
    keys = _layer_keys(cfg, 2)
    exact = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float64, False, keys)
    stored = _ref_wgrads(sd, ids, mask, cfg, dout, torch.float64, True, keys)
    got = {}
    for chunk in (2, 5):
        m = _model(cfg, sd, chunk=chunk)
        m.set_trainable_layers(2)
        got[chunk], _ = _native_wgrads(m, ids.cuda(), mask, dout, keys)
        _rule_b(f"NativeDeberta tiny 5 x 70, k=2, chunk {chunk},", got[chunk], exact, stored)
    for key in keys:
        e = l2_rel(got[2][key], got[5][key])
        through_pos = "query_proj" in key or "key_proj" in key          # the one bf16 rounding of dpos can flip between the two
        print(f"chunk 2 vs chunk 5, {key}: rel L2 {e:.3e}" + (" (through the position path: not asserted)" if through_pos else f" (bound {F32_TOL})"))
        assert through_pos or e <= F32_TOL, key


def test_gradients_accumulate_and_honour_the_lazy_zero_protocol():
    from mmfusion import arena
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 3, 70, 59, pad_from=50)
    dout, _ = _douts(cfg, 3, 70, 60)
    keys = _layer_keys(cfg, 2)
    m = _model(cfg, sd, chunk=2)
    m.set_trainable_layers(2)
    once, _ = _native_wgrads(m, ids.cuda(), mask, dout, keys)
    twice, _ = _native_wgrads(m, ids.cuda(), mask, dout, keys, zero=False)
    for key in keys:
        e = l2_rel(twice[key], 2 * once[key])
        print(f"two backwards vs 2 x one, {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    ar = arena.ensure(m)
    ar.zero_grad(lazy=True)
    again, _ = _native_wgrads(m, ids.cuda(), mask, dout, keys, zero=False)
    ar.finalize_grads()
    torch.cuda.synchronize()
    again = _hf_grads(m, keys)
    for key in keys:
        e = l2_rel(again[key], once[key])
        print(f"after zero_grad(lazy=True), {key}: rel L2 {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    _frozen_grads_are_empty(m)


def test_text_encoder_steps_the_trainable_layer_and_serves_the_new_weights():
    import config as cfgmod
    from mmfusion import arena
    from mmfusion.train import finetune_optimizer
    from models.encoders import TextEncoder
    tcfg = deberta_ref.tiny_config()
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.text_hidden_size = 256, 0.0, 256
    cfg.text_backbone = "native"
    cfg.text_backbone_kwargs = {k: v for k, v in deberta_ref.config_kwargs(tcfg).items() if k != "hidden_size"}
    cfg.text_backbone_trainable_layers = 1
    torch.manual_seed(3)
    enc = TextEncoder(cfg)
    assert enc.model.trainable_layers == 1
    enc.model.load_state_dict(deberta_ref.seeded_weights(tcfg, seed=31))
    enc = enc.cuda().train()
    ids, mask = _inputs(tcfg, 2, 70, 61, pad_from=50)
    ids, mask = ids.cuda(), mask.cuda()
    ar = arena.ensure(enc)
    opt = finetune_optimizer(enc, ar, lr=1e-2, weight_decay=0.01)
    with torch.no_grad():
        first = enc.model(input_ids=ids, attention_mask=mask).last_hidden_state.clone()
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    for _ in range(2):
        ar.zero_grad()
        feats = enc(ids, mask)["features"]
        assert feats.requires_grad
        feats.sum().backward()
        opt.advance()
        opt.launch()
    torch.cuda.synchronize()
    for n, p in enc.named_parameters():
        same = torch.equal(_bits(p.detach()), _bits(before[n]))
        if p.requires_grad and n.startswith(("model.", "projection.")):             # (what the forward does not use has no gradient)
            assert not same, f"{n} did not move"
        if not p.requires_grad:
            assert same, f"the frozen {n} moved"
    assert sorted(n for n, p in enc.model.named_parameters() if p.requires_grad) == sorted(enc.model._layer_params(tcfg.num_hidden_layers - 1))
    # what the kernels read now (shadows, the trainable layer's position tables) is the stepped weights
    sd = {k: v.detach().cpu().clone() for k, v in enc.model.state_dict().items()}
    assert list(sd) == list(deberta_ref.hf_keys(tcfg))
    with torch.no_grad():
        got = enc.model(input_ids=ids, attention_mask=mask).last_hidden_state
    want = deberta_ref.deberta_forward(sd, ids.cpu(), mask.cpu(), tcfg, bf16_storage=True)
    err, moved = l2_rel(got, want), l2_rel(got, first)
    print(f"TextEncoder, 2 AdamW steps on the top layer: no_grad forward vs the restatement on the new state_dict {err:.3e} (bound {BOUND_A}); "
          f"the output moved by {moved:.3e}")
    assert err <= BOUND_A and moved > 3 * BOUND_A


def test_forward_and_weight_backward_replay_from_a_captured_graph():
    from mmfusion import arena
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 3, 70, 62, pad_from=50)
    dout, _ = _douts(cfg, 3, 70, 63)
    keys = _layer_keys(cfg, 1)
    m = _model(cfg, sd, chunk=2)
    m.set_trainable_layers(1)
    eager, _ = _native_wgrads(m, ids.cuda(), mask, dout, keys)
    ar = arena.ensure(m)
    static, k, dO = ids.cuda().clone(), mask.cuda(), dout.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        m(input_ids=static, attention_mask=k).last_hidden_state.backward(dO)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m(input_ids=static, attention_mask=k).last_hidden_state.backward(dO)
    with torch.no_grad():
        static.copy_(torch.randint(1, cfg.vocab_size, static.shape, device="cuda"))
    ar.zero_grad()
    graph.replay()
    torch.cuda.synchronize()
    other = _hf_grads(m, keys)
    with torch.no_grad():
        static.copy_(ids.cuda())
    ar.zero_grad()
    graph.replay()
    torch.cuda.synchronize()
    got = _hf_grads(m, keys)
    for key in keys:
        e = l2_rel(got[key], eager[key])
        print(f"captured forward + backward, {key}: rel L2 vs eager {e:.3e} (bound {F32_TOL})")
        assert e <= F32_TOL, key
    assert any(l2_rel(other[key], eager[key]) > 1e-2 for key in keys)


def test_refusals_and_the_frozen_default():
    cfg = deberta_ref.tiny_config()
    sd = deberta_ref.seeded_weights(cfg, seed=21)
    ids, mask = _inputs(cfg, 2, 40, 64)
    m = _model(cfg, sd)
    for bad in (-1, cfg.num_hidden_layers + 1):
        with pytest.raises(ValueError):
            m.set_trainable_layers(bad)
    assert m.trainable_layers == 0 and not any(p.requires_grad for p in m.parameters())
    out = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state         # grad mode on, nothing trainable
    assert not out.requires_grad
    m.set_trainable_layers(2)
    assert m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state.requires_grad
    with torch.no_grad():
        assert not m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state.requires_grad
    m.set_trainable_layers(0)
    again = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    assert not again.requires_grad and torch.equal(again, out) and not any(p.requires_grad for p in m.parameters())
