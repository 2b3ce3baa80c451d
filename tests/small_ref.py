"""float64 restatements of the small fused branch kernels (csrc/small.hip) and the optimiser tail (csrc/optim.hip) — a
test helper.

Every function takes CPU tensors that already hold the values the kernel reads (bf16 or f32 operands widened to float64)
and returns unrounded float64 results; backward passes are written out by hand from the forward equations, not taken from
autograd (tests/test_small_ref_cpu.py pins both against torch autograd in float64).  Layouts are the kernels':

  GAT      h (B, 3, H, C), att_src / att_dst (H, C), bias (C); alpha (B, 3 dst i, 3 src j, H);
           sdots (B, 2, 3, H) = [s_src | s_dst][node][head]
  InfoNCE  three (B, D) projections, pairs (0, 1) (0, 2) (1, 2); lse (3, 2, B) = per pair [row | column] log-sum-exp
  AdamW    hp = [lr, beta1, beta2, eps, weight_decay, 1 - beta1^t, 1 - beta2^t, max_grad_norm, grad_scale]
  schedule sched = [mode, max_lr, total_steps, pct_start, div_factor, final_div_factor, cycle_momentum, base_m, max_m]"""
import math

import torch

F64 = torch.float64
PAIRS = ((0, 1), (0, 2), (1, 2))


# ---------------------------------------------------------------------------------------------- dense 3-node GAT
def gat3_fwd(h, att_src, att_dst, bias, slope=0.2, relu=True):
    """PyG GATConv(heads=H, concat=False) on the 3-clique with self loops.  Returns (out, pooled, alpha, sdots): out
    (B, 3, C) after the optional ReLU, pooled = mean over the nodes."""
    s_src, s_dst = (h * att_src).sum(-1), (h * att_dst).sum(-1)                 # (B, 3, H)
    z = s_dst.unsqueeze(2) + s_src.unsqueeze(1)                                  # (B, i, j, H)
    e = torch.where(z > 0, z, z * slope)
    ex = torch.exp(e - e.max(dim=2, keepdim=True).values)
    alpha = ex / (ex.sum(dim=2, keepdim=True) + 1e-16)
    out = torch.einsum("bijh,bjhc->bic", alpha, h) / h.shape[2] + bias
    if relu:
        out = out.clamp_min(0)
    return out, out.mean(1), alpha, torch.stack([s_src, s_dst], 1)


def gat3_bwd(h, att_src, att_dst, alpha, sdots, live, dy, dpool, slope=0.2):
    """live (B, 3, C): 1 where the gradient passes the ReLU (all ones without one); dy (B, 3, C) or None; dpool (B, C) or
    None.  Returns (dh, datt_src, datt_dst, dbias)."""
    B, _, H, C = h.shape
    g = torch.zeros(B, 3, C, dtype=F64)
    if dy is not None:
        g = g + dy
    if dpool is not None:
        g = g + dpool.unsqueeze(1) / 3
    g = g * live
    dalpha = torch.einsum("bic,bjhc->bijh", g, h) / H
    dot = (alpha * dalpha).sum(2, keepdim=True)
    z = sdots[:, 1].unsqueeze(2) + sdots[:, 0].unsqueeze(1)
    dz = alpha * (dalpha - dot) * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    ds_src, ds_dst = dz.sum(1), dz.sum(2)                                        # (B, node, H)
    dh = (torch.einsum("bijh,bic->bjhc", alpha, g) / H + ds_src.unsqueeze(-1) * att_src + ds_dst.unsqueeze(-1) * att_dst)
    return dh, (ds_src.unsqueeze(-1) * h).sum((0, 1)), (ds_dst.unsqueeze(-1) * h).sum((0, 1)), g.sum((0, 1))


# ---------------------------------------------------------------------------------------------- normalise + InfoNCE
def normalize(z):
    """n = z / max(||z||, 1e-12) row-wise; returns (n, 1 / max(||z||, 1e-12))"""
    inv = 1.0 / z.norm(dim=1).clamp_min(1e-12)
    return z * inv.unsqueeze(1), inv


def infonce_fwd(zs, temperature):
    """returns (ns [3], inv_norms (3, B), losses (3,), lse (3, 2, B), sims [3] (B, B))"""
    B = zs[0].shape[0]
    nn_ = [normalize(z) for z in zs]
    ns, inv = [t[0] for t in nn_], torch.stack([t[1] for t in nn_])
    losses, lse, sims = torch.zeros(3, dtype=F64), torch.zeros(3, 2, B, dtype=F64), []
    for p, (a, b) in enumerate(PAIRS):
        sim = ns[a] @ ns[b].t() / temperature
        lse[p, 0], lse[p, 1] = torch.logsumexp(sim, 1), torch.logsumexp(sim, 0)
        losses[p] = ((lse[p, 0] - sim.diagonal()).sum() + (lse[p, 1] - sim.diagonal()).sum()) * (0.5 / B)
        sims.append(sim)
    return ns, inv, losses, lse, sims


def infonce_bwd(zs, temperature, dn=None, dloss=None):
    """dn: three (B, D) gradients of the normalised outputs or None each; dloss: three scalars or None each (a pair without
    one contributes nothing).  Returns dz [3].  A row whose norm is clamped gets autograd's dn / 1e-12 here; the kernel
    gives such a row a zero gradient on purpose (csrc/small.hip nce_clamped), and its test says so."""
    B = zs[0].shape[0]
    ns, inv, _, lse, sims = infonce_fwd(zs, temperature)
    g = [torch.zeros_like(z) if dn is None or dn[m] is None else dn[m].clone() for m, z in enumerate(zs)]
    for p, (a, b) in enumerate(PAIRS):
        if dloss is None or dloss[p] is None:
            continue
        ds = (torch.exp(sims[p] - lse[p, 0].unsqueeze(1)) + torch.exp(sims[p] - lse[p, 1].unsqueeze(0)) - 2 * torch.eye(B, dtype=F64))
        ds = ds * (float(dloss[p]) * 0.5 / B / temperature)
        g[a] = g[a] + ds @ ns[b]
        g[b] = g[b] + ds.t() @ ns[a]
    return [(g[m] - ns[m] * (g[m] * ns[m]).sum(1, keepdim=True)) * inv[m].unsqueeze(1) for m in range(3)]


# ---------------------------------------------------------------------------------------------- adaptive combination
def adaptive_fwd(hp, W2, b2, attended):
    """aw = softmax(hp W2^T + b2) (B, 3); weighted = sum_m attended[:, m] aw[:, m] (B, d)"""
    logit = hp @ W2.t() + b2
    ex = torch.exp(logit - logit.max(1, keepdim=True).values)
    aw = ex / ex.sum(1, keepdim=True)
    return aw, (attended * aw.unsqueeze(-1)).sum(1)


def adaptive_bwd(hp, W2, attended, aw, dweighted=None, daw=None):
    """returns (dattended, dhp, dW2, db2)"""
    g = torch.zeros_like(hp) if dweighted is None else dweighted
    da = (g.unsqueeze(1) * attended).sum(-1)
    if daw is not None:
        da = da + daw
    dl = aw * (da - (aw * da).sum(1, keepdim=True))
    return g.unsqueeze(1) * aw.unsqueeze(-1), dl @ W2, dl.t() @ hp, dl.sum(0)


def attn_weights_mean(qkv, B, T, H, dh):
    """qkv (B * T, 3 H dh) packed q | k | v; w (B, T, T) = mean over heads of softmax_j(q_i . k_j / sqrt(dh))"""
    d = H * dh
    q = qkv[:, :d].reshape(B, T, H, dh)
    k = qkv[:, d:2 * d].reshape(B, T, H, dh)
    w = torch.zeros(B, T, T, dtype=F64)
    for h in range(H):                                  # one head at a time: (B, T, T) float64 is 32 MiB at T = 2048
        s = q[:, :, h] @ k[:, :, h].transpose(1, 2) / math.sqrt(dh)
        ex = torch.exp(s - s.max(-1, keepdim=True).values)
        w += ex / ex.sum(-1, keepdim=True)
    return w / H


# ---------------------------------------------------------------------------------------------- narrow linear, stack3, rowmask
def narrow_fwd(x, W, b=None):
    y = x @ W.t()
    return y if b is None else y + b


def narrow_bwd(x, W, dy):
    """returns (dx, dW, db)"""
    return dy @ W, dy.t() @ x, dy.sum(0)


def stack3_fwd(f0, f1, f2, emb=None):
    """(B, 3, d): x[b][m] = f_m[b] + emb[m]"""
    x = torch.stack([f0, f1, f2], 1)
    return x if emb is None else x + emb


def stack3_bwd(dx):
    """dx (B, 3, d) -> (d0, d1, d2, demb)"""
    return dx[:, 0], dx[:, 1], dx[:, 2], dx.sum(0)


def rowmask(x, mask):
    return x * mask.unsqueeze(1)


# ---------------------------------------------------------------------------------------------- optimiser tail
def clip_coef(hp, gnorm_sq):
    """the factor every gradient is multiplied by: grad_scale, times torch.nn.utils.clip_grad_norm_'s coefficient
    min(1, max_norm / (norm * |grad_scale| + 1e-6)) when clipping is on (hp[7] > 0 and a squared norm is given)"""
    gs = float(hp[8])
    if float(hp[7]) > 0 and gnorm_sq is not None:
        norm = math.sqrt(float(gnorm_sq)) * abs(gs)
        gs *= min(1.0, float(hp[7]) / (norm + 1e-6))
    return gs


def adamw(p, g, m, v, hp, gnorm_sq=None):
    """one decoupled-weight-decay Adam step with the bias corrections passed in; returns (p, m, v)"""
    lr, b1, b2, eps, wd, bc1, bc2 = (float(hp[i]) for i in range(7))
    ge = g * clip_coef(hp, gnorm_sq)
    m = b1 * m + (1 - b1) * ge
    v = b2 * v + (1 - b2) * ge * ge
    p = p * (1 - lr * wd) - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adamw_advance(step, hp, sched):
    """step: the counter before the call; hp, sched: sequences of floats.  Returns (step + 1, hp') with hp'[0], [1], [5], [6]
    as the one-thread schedule kernel derives them: OneCycleLR (cos, two phases) evaluated at s = step, past its end held at
    the final value; beta1 cycled against the learning rate when sched[6]; bias corrections from the CURRENT beta1."""
    t = int(step) + 1
    hp = [float(x) for x in hp]
    b1, b2 = hp[1], hp[2]
    if float(sched[0]) == 1.0:
        max_lr, total, pct = float(sched[1]), float(sched[2]), float(sched[3])
        initial = max_lr / float(sched[4])
        minimum = initial / float(sched[5])
        up_end, down_end, s = pct * total - 1.0, total - 1.0, float(t - 1)
        up = s <= up_end or up_end >= down_end
        q = (s / up_end if up_end > 0 else 1.0) if up else min(1.0, (s - up_end) / (down_end - up_end))
        w = (math.cos(math.pi * q) + 1.0) / 2.0
        hp[0] = max_lr + (initial - max_lr) * w if up else minimum + (max_lr - minimum) * w
        if float(sched[6]) != 0.0:
            base_m, max_m = float(sched[7]), float(sched[8])
            b1 = base_m + (max_m - base_m) * w if up else max_m + (base_m - max_m) * w
            hp[1] = b1
    hp[5] = 1.0 - b1 ** t
    hp[6] = 1.0 - b2 ** t
    return t, hp
