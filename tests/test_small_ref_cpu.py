"""CPU: tests/small_ref.py, the float64 restatement the GPU tests of csrc/small.hip and csrc/optim.hip compare against,
pinned against torch autograd / torch.optim in float64 to 1e-12 — what makes that reference trustworthy independently of
the kernels."""
import pytest
import torch
import torch.nn.functional as F

import small_ref as R

F64 = torch.float64
TOL = 1e-12


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F64) * scale


def close(a, b, what=""):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
    assert err <= TOL, (what, err)


@pytest.mark.parametrize("B,H,C", [(1, 1, 8), (5, 4, 136), (2, 8, 24), (3, 2, 40)])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("grads", ["dy", "dpool", "both"])
def test_gat3_matches_dense_gat_autograd(B, H, C, relu, grads):
    h = rnd(B, 3, H, C, seed=1).requires_grad_(True)
    ps = [rnd(H, C, seed=2, scale=0.3).requires_grad_(True), rnd(H, C, seed=3, scale=0.3).requires_grad_(True),
          rnd(C, seed=4, scale=0.3).requires_grad_(True)]
    # the dense formulation of tests/test_kernels_gpu.py::test_gat3_dense_matches_torch_dense_gat
    s_src, s_dst = (h * ps[0]).sum(-1), (h * ps[1]).sum(-1)
    e = F.leaky_relu(s_dst.unsqueeze(2) + s_src.unsqueeze(1), 0.2)
    ex = torch.exp(e - e.max(dim=2, keepdim=True).values)
    alpha = ex / (ex.sum(dim=2, keepdim=True) + 1e-16)
    out = torch.einsum("bijh,bjhc->bihc", alpha, h).mean(dim=2) + ps[2]
    if relu:
        out = torch.relu(out)
    dy = rnd(B, 3, C, seed=5) if grads != "dpool" else None
    dp = rnd(B, C, seed=6) if grads != "dy" else None
    torch.autograd.backward([t for t, g in ((out, dy), (out.mean(1), dp)) if g is not None], [g for g in (dy, dp) if g is not None])
    with torch.no_grad():
        o, pooled, al, sd = R.gat3_fwd(h, ps[0], ps[1], ps[2], 0.2, relu)
        close(o, out, "out"), close(pooled, out.mean(1), "pooled"), close(al, alpha, "alpha")
        close(sd[:, 0], s_src, "s_src"), close(sd[:, 1], s_dst, "s_dst")
        live = (o > 0).double() if relu else torch.ones_like(o)
        got = R.gat3_bwd(h, ps[0], ps[1], al, sd, live, dy, dp, 0.2)
    for a, b, w in zip(got, (h.grad, ps[0].grad, ps[1].grad, ps[2].grad), ("dh", "datt_src", "datt_dst", "dbias")):
        close(a, b, w)


@pytest.mark.parametrize("B,D", [(1, 4), (2, 12), (5, 36), (16, 64)])
@pytest.mark.parametrize("temp", [0.07, 1.0])
@pytest.mark.parametrize("mode", ["all", "normalise_only", "one_null_loss", "two_null_losses", "dn_null"])
def test_infonce_matches_normalize_cross_entropy_autograd(B, D, temp, mode):
    zs = [rnd(B, D, seed=10 + m).requires_grad_(True) for m in range(3)]
    ns = [F.normalize(z, dim=-1, eps=1e-12) for z in zs]
    lab = torch.arange(B)

    def nce(a, b):
        sim = a @ b.t() / temp
        return (F.cross_entropy(sim, lab) + F.cross_entropy(sim.t(), lab)) / 2
    ls = [nce(ns[a], ns[b]) for a, b in R.PAIRS]
    dloss = {"all": [0.3, 1.1, 0.7], "dn_null": [0.3, 1.1, 0.7], "normalise_only": [None] * 3, "one_null_loss": [0.3, None, 0.7],
             "two_null_losses": [None, 1.1, None]}[mode]
    dn = None if mode == "dn_null" else [rnd(B, D, seed=20 + m, scale=0.01) for m in range(3)]
    total = sum(w * l for w, l in zip(dloss, ls) if w is not None)
    if dn is not None:
        total = total + sum((n * g).sum() for n, g in zip(ns, dn))
    total.backward()
    with torch.no_grad():
        n2, inv, l2, lse, sims = R.infonce_fwd(zs, temp)
        for m in range(3):
            close(n2[m], ns[m], "n"), close(inv[m], 1 / zs[m].norm(dim=1), "inv_norm")
        close(l2, torch.stack(ls), "losses")
        close(lse[0, 0], torch.logsumexp(sims[0], 1), "lse row"), close(lse[2, 1], torch.logsumexp(sims[2], 0), "lse col")
        dz = R.infonce_bwd(zs, temp, dn, dloss)
    for m in range(3):
        close(dz[m], zs[m].grad, f"dz{m}")


def test_infonce_zero_row_is_what_autograd_gives():
    """a zero row is clamped: n = 0, and normalize's backward passes dn / 1e-12 (the clamp has no gradient)"""
    zs = [rnd(4, 8, seed=30 + m) for m in range(3)]
    zs[1][2] = 0
    zs = [z.requires_grad_(True) for z in zs]
    dn = [rnd(4, 8, seed=40 + m) for m in range(3)]
    sum((F.normalize(z, dim=-1, eps=1e-12) * g).sum() for z, g in zip(zs, dn)).backward()
    with torch.no_grad():
        dz = R.infonce_bwd(zs, 0.07, dn, None)
    for m in range(3):
        close(dz[m], zs[m].grad, f"dz{m}")
    assert float(zs[1].grad[2].abs().max()) > 1e9


@pytest.mark.parametrize("B,d", [(1, 4), (16, 200), (3, 256)])
@pytest.mark.parametrize("which", ["both", "dweighted_null", "daw_null"])
def test_adaptive_matches_softmax_linear_autograd(B, d, which):
    hp, att = rnd(B, d, seed=1).requires_grad_(True), rnd(B, 3, d, seed=2).requires_grad_(True)
    W2, b2 = rnd(3, d, seed=3, scale=0.3).requires_grad_(True), rnd(3, seed=4, scale=0.3).requires_grad_(True)
    aw = F.softmax(F.linear(hp, W2, b2), dim=-1)
    wt = (att * aw.unsqueeze(-1)).sum(dim=1)
    gw = rnd(B, d, seed=5) if which != "dweighted_null" else None
    ga = rnd(B, 3, seed=6) if which != "daw_null" else None
    torch.autograd.backward([t for t, g in ((wt, gw), (aw, ga)) if g is not None], [g for g in (gw, ga) if g is not None])
    with torch.no_grad():
        aw2, wt2 = R.adaptive_fwd(hp, W2, b2, att)
        close(aw2, aw, "aw"), close(wt2, wt, "weighted")
        got = R.adaptive_bwd(hp, W2, att, aw2, gw, ga)
    want = (att.grad if att.grad is not None else torch.zeros_like(att), hp.grad, W2.grad, b2.grad)
    for a, b, w in zip(got, want, ("dattended", "dhp", "dW2", "db2")):
        close(a, b, w)


@pytest.mark.parametrize("B,T,H,dh", [(2, 1, 1, 8), (2, 7, 4, 16), (1, 3, 12, 8)])
def test_attn_weights_mean_matches_multihead_attention(B, T, H, dh):
    d = H * dh
    qkv = rnd(B * T, 3 * d, seed=7)
    mha = torch.nn.MultiheadAttention(d, H, batch_first=True, bias=False, dtype=F64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(d, dtype=F64).repeat(3, 1))
        q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(B, T, d) for i in range(3))
        w = mha(q, k, v, need_weights=True, average_attn_weights=True)[1]
    close(R.attn_weights_mean(qkv, B, T, H, dh), w, "w")
    close(R.attn_weights_mean(qkv, B, T, H, dh).sum(-1), torch.ones(B, T, dtype=F64), "rows sum to 1")


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (16, 7, 200), (5, 16, 257)])
def test_narrow_stack3_rowmask_match_autograd(M, N, K):
    x, W, b = (t.requires_grad_(True) for t in (rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3)))
    y = F.linear(x, W, b)
    dy = rnd(M, N, seed=4)
    y.backward(dy)
    with torch.no_grad():
        close(R.narrow_fwd(x, W, b), y, "y"), close(R.narrow_fwd(x, W), F.linear(x, W), "y no bias")
        for a, r, w in zip(R.narrow_bwd(x, W, dy), (x.grad, W.grad, b.grad), ("dx", "dW", "db")):
            close(a, r, w)
    fs = [rnd(M, K, seed=10 + i).requires_grad_(True) for i in range(3)]
    emb = rnd(3, K, seed=13).requires_grad_(True)
    xs = torch.stack(fs, dim=1) + emb
    g = rnd(M, 3, K, seed=14)
    xs.backward(g)
    with torch.no_grad():
        close(R.stack3_fwd(*fs, emb), xs, "stack3"), close(R.stack3_fwd(*fs), torch.stack(fs, 1), "stack3 no emb")
        for a, r, w in zip(R.stack3_bwd(g), (fs[0].grad, fs[1].grad, fs[2].grad, emb.grad), ("d0", "d1", "d2", "demb")):
            close(a, r, w)
        mask = (rnd(M, seed=15) > 0).double()
        close(R.rowmask(x, mask), x * mask[:, None], "rowmask")


@pytest.mark.parametrize("max_norm", [1.0, 1e6, 0.0])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adamw_matches_torch_adamw_and_clip_grad_norm(max_norm, wd):
    """four steps (step 1 has zero moments) of clip_grad_norm_ + torch.optim.AdamW on float64 parameters"""
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    p = torch.nn.Parameter(rnd(1027, seed=1))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    pr, m, v = p.detach().clone(), torch.zeros(1027, dtype=F64), torch.zeros(1027, dtype=F64)
    for t in range(1, 5):
        g = rnd(1027, seed=100 + t, scale=3.0 if t % 2 else 0.01)
        p.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        hp = [lr, b1, b2, eps, wd, 1 - b1 ** t, 1 - b2 ** t, max_norm, 1.0]
        pr, m, v = R.adamw(pr, g, m, v, hp, float((g * g).sum()))
        st = opt.state[p]
        close(pr, p.detach(), f"p step {t}"), close(m, st["exp_avg"], "m"), close(v, st["exp_avg_sq"], "v")


def test_adamw_grad_scale_is_a_scaled_gradient():
    """grad_scale s (negative included) = the step on the gradient s g, whose norm is |s| ||g||; no gnorm_sq = no clipping"""
    p, g, m, v = rnd(50, seed=1), rnd(50, seed=2, scale=4.0), rnd(50, seed=3, scale=0.1), rnd(50, seed=4).abs() * 0.01
    for s in (0.125, -0.5):
        hp = [1e-2, 0.9, 0.999, 1e-8, 1e-2, 0.19, 0.002, 1.0, s]
        hp1 = hp[:8] + [1.0]
        for a, b in zip(R.adamw(p, g, m, v, hp, float((g * g).sum())), R.adamw(p, g * s, m, v, hp1, float((g * g).sum()) * s * s)):
            close(a, b, f"scale {s}")
        assert abs(R.clip_coef(hp, None)) == abs(s) and abs(R.clip_coef(hp, float((g * g).sum()))) < abs(s)


@pytest.mark.parametrize("total,pct", [(50, 0.1), (20, 0.3), (7, 0.5)])
@pytest.mark.parametrize("cycle", [True, False])
def test_advance_matches_onecycle_lr(total, pct, cycle):
    max_lr, b2 = 3e-3, 0.999
    p = torch.nn.Parameter(torch.zeros(1, dtype=F64))
    opt = torch.optim.AdamW([p], lr=max_lr, betas=(0.9, b2))
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total, pct_start=pct, anneal_strategy="cos",
                                              cycle_momentum=cycle, div_factor=25.0, final_div_factor=1e4)
    sched = [1.0, max_lr, float(total), pct, 25.0, 1e4, float(cycle), 0.85, 0.95]
    hp, step = [0.0, 0.9, b2, 1e-8, 0.0, 0.0, 0.0, 1.0, 1.0], 0
    for t in range(1, total + 1):
        step, hp = R.adamw_advance(step, hp, sched)
        lr_t, b1_t = opt.param_groups[0]["lr"], opt.param_groups[0]["betas"][0]
        assert step == t
        assert abs(hp[0] - lr_t) <= TOL * max_lr and abs(hp[1] - b1_t) <= TOL, (t, hp[0], lr_t, hp[1], b1_t)
        assert abs(hp[5] - (1 - b1_t ** t)) <= TOL and abs(hp[6] - (1 - b2 ** t)) <= TOL
        p.grad = torch.ones_like(p)
        opt.step()
        if t < total:
            sch.step()
    last = hp[0]
    for t in range(total + 1, total + 3):          # past the end: held at the final value, the corrections keep moving
        step, hp = R.adamw_advance(step, hp, sched)
        assert step == t and hp[0] == last and hp[6] == 1 - b2 ** t
    step, hp = R.adamw_advance(4, [7e-4, 0.9, b2, 1e-8, 0.0, 0.0, 0.0, 1.0, 1.0], [0.0] * 9)    # constant mode
    assert step == 5 and hp[0] == 7e-4 and hp[1] == 0.9 and hp[5] == 1 - 0.9 ** 5 and hp[6] == 1 - b2 ** 5
