"""Float64 restatement of FewShotModel's episode head (reference models/multimodal_model.py:286-362 and the loss of
training/advanced_trainer.py:539-551), written out by hand so that tests can check both torch autograd of the
reference's formulation (tests/test_fewshot_cpu.py) and the HIP kernels of csrc/fewshot.hip (tests/test_fewshot_gpu.py,
with a per-element f32 error bound next to every value):

  sf = t + a + v (support, class-major rows c * n_shot + s),  mean_c = mean_s sf[c * n_shot + s]
  P = W2 relu(W0 mean + b0) + b2                                  prototype_network
  qf = t + a + v (query),  dist_ij = ||qf_i - P_j||_2,  pred_i = softmax(-dist_i)
  loss = CE(pred, y) = mean_i (logsumexp(pred_i) - pred_i[y_i])   (nn.CrossEntropyLoss on probabilities)

The kernel-level functions take the kernels' own f32 outputs (query features, distances, probabilities) as exact inputs
of the next stage, so every bound covers one kernel's rounding only.  U is the f32 unit roundoff."""
import torch

F64 = torch.float64
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def _d(x):
    return x.detach().to(F64).cpu()


# ---------------------------------------------------------------------------------------------------------------------
# the whole head in float64: forward and hand-written gradients
# ---------------------------------------------------------------------------------------------------------------------
def torch_head(s3, q3, W0, b0, W2, b2, n_way, n_shot):
    """the reference's composition in torch ops (any dtype, autograd-able): -> (sf, P, qf, dist, pred)"""
    sf = s3[0] + s3[1] + s3[2]
    mean = sf.view(n_way, n_shot, -1).mean(1)
    P = torch.relu(mean @ W0.T + b0) @ W2.T + b2
    qf = q3[0] + q3[1] + q3[2]
    dist = torch.cdist(qf, P, p=2)
    return sf, P, qf, dist, torch.softmax(-dist, dim=-1)


def head_loss_and_grads(s3, q3, W0, b0, W2, b2, n_way, n_shot, y):
    """float64 forward + CE on the probabilities, and every gradient by hand: -> dict of loss, ds (the gradient of each
    support modality), dq (of each query modality), dW0, db0, dW2, db2"""
    s3, q3 = [_d(x) for x in s3], [_d(x) for x in q3]
    W0, b0, W2, b2 = _d(W0), _d(b0), _d(W2), _d(b2)
    sf = s3[0] + s3[1] + s3[2]
    mean = sf.view(n_way, n_shot, -1).mean(1)
    z = mean @ W0.T + b0
    h = torch.clamp_min(z, 0.0)
    P = h @ W2.T + b2
    qf = q3[0] + q3[1] + q3[2]
    diff = qf[:, None, :] - P[None, :, :]                      # (Nq, n_way, d)
    dist = diff.pow(2).sum(-1).sqrt()
    pred = torch.softmax(-dist, dim=-1)
    Nq = qf.shape[0]
    sm = torch.softmax(pred, dim=-1)                           # CE over the probabilities as logits
    loss = (torch.logsumexp(pred, dim=-1) - pred[torch.arange(Nq), y]).mean()
    gpred = (sm - torch.nn.functional.one_hot(y, n_way).to(F64)) / Nq
    gq, gP = dist_bwd(qf, P, dist, pred, None, gpred)
    dh = gP @ W2
    dW2, db2 = gP.T @ h, gP.sum(0)
    dz = dh * (z > 0)
    dW0, db0 = dz.T @ mean, dz.sum(0)
    dmean = dz @ W0
    ds = proto_bwd(dmean, None, n_shot)
    return {"loss": loss, "ds": ds, "dq": gq, "dW0": dW0, "db0": db0, "dW2": dW2, "db2": db2}


# ---------------------------------------------------------------------------------------------------------------------
# kernel-level pieces with f32 error bounds
# ---------------------------------------------------------------------------------------------------------------------
def proto_fwd(s3, n_way, n_shot):
    """f32 inputs -> float64 sf, mean and the bounds of the kernel's f32 values (sum in order, divide by n_shot)"""
    t, a, v = [_d(x) for x in s3]
    sf = t + a + v
    e_sf = U * (t + a).abs() + U * ((t + a).abs() + v.abs())
    S = sf.view(n_way, n_shot, -1)
    mean = S.mean(1)
    e_mean = (e_sf.view(n_way, n_shot, -1).sum(1) + gamma(n_shot) * S.abs().sum(1)) / n_shot + U * mean.abs()
    return {"sf": sf, "e_sf": e_sf, "mean": mean, "e_mean": e_mean}


def proto_bwd(dmean, dsf, n_shot):
    """ds[r] = dmean[r // n_shot] / n_shot + dsf[r] in float64"""
    ds = _d(dmean).repeat_interleave(n_shot, dim=0) / n_shot
    return ds if dsf is None else ds + _d(dsf)


def proto_bwd_bound(dmean, dsf, n_shot):
    ds = proto_bwd(dmean, dsf, n_shot)
    base = _d(dmean).abs().repeat_interleave(n_shot, dim=0) / n_shot
    return ds, U * base + U * ds.abs()


def query_features(q3):
    t, a, v = [_d(x) for x in q3]
    qf = t + a + v
    return qf, U * (t + a).abs() + U * ((t + a).abs() + v.abs())


def dist_fwd(qf, P):
    """distances and probabilities from the kernel's own f32 query features (exact inputs here), with bounds"""
    qf, P = _d(qf), _d(P)
    d = qf.shape[1]
    diff = qf[:, None, :] - P[None, :, :]
    S = diff.pow(2).sum(-1)
    dist = S.sqrt()
    e_S = gamma(d + 8) * S                                     # differences, squares and the sum: all terms are >= 0
    e_dist = torch.minimum(e_S / (2 * dist).clamp_min(1e-300), e_S.sqrt()) + U * dist
    pred = torch.softmax(-dist, dim=-1)
    return {"dist": dist, "e_dist": e_dist, "pred": pred}


def pred_bound(dist_f32, pred):
    """bound of softmax(-dist) computed in f32 (expf of max-subtracted values, a sum over n_way, one division) from the
    kernel's own f32 distances: relative u (|x - m| + 2) + gamma(n_way + 4)"""
    dist = _d(dist_f32)
    n = dist.shape[1]
    shift = (dist - dist.min(dim=1, keepdim=True).values).abs()
    rel = U * (2 * shift + 4) + gamma(n + 4)
    return _d(pred) * rel + 1e-44


def dist_bwd(qf, P, dist, pred, gdist, gpred):
    """float64 (dq, dP) of the distance / softmax tail; zero distance -> zero gradient (torch's cdist backward)"""
    qf, P, dist, pred = _d(qf), _d(P), _d(dist), _d(pred)
    g = torch.zeros_like(dist) if gdist is None else _d(gdist).clone()
    if gpred is not None:
        gp = _d(gpred)
        s = (pred * gp).sum(-1, keepdim=True)
        g = g - pred * (gp - s)
    c = torch.where(dist > 0, g / torch.where(dist > 0, dist, torch.ones_like(dist)), torch.zeros_like(dist))
    diff = qf[:, None, :] - P[None, :, :]
    dq = (c[:, :, None] * diff).sum(1)
    dP = -(c[:, :, None] * diff).sum(0)
    return dq, dP


def dist_bwd_bound(qf, P, dist, pred, gdist, gpred):
    """(dq, dP, e_dq, e_dP) for the kernel's f32 arithmetic on its own f32 saved tensors"""
    qf, P, dist, pred = _d(qf), _d(P), _d(dist), _d(pred)
    Nq, n = dist.shape
    dq, dP = dist_bwd(qf, P, dist, pred, gdist, gpred)
    gd = torch.zeros_like(dist) if gdist is None else _d(gdist)
    g, e_g = gd.clone(), torch.zeros_like(dist)
    if gpred is not None:
        gp = _d(gpred)
        s = (pred * gp).sum(-1, keepdim=True)
        e_s = gamma(n + 8) * (pred * gp).abs().sum(-1, keepdim=True)
        g = g - pred * (gp - s)
        e_g = pred * e_s + gamma(4) * (gd.abs() + pred * (gp.abs() + s.abs()))
    pos = dist > 0
    safe = torch.where(pos, dist, torch.ones_like(dist))
    c = torch.where(pos, g / safe, torch.zeros_like(dist))
    e_c = torch.where(pos, e_g / safe + U * c.abs(), torch.zeros_like(dist))
    adiff = (qf[:, None, :] - P[None, :, :]).abs()
    mag = (qf.abs()[:, None, :] + P.abs()[None, :, :])
    e_dq = gamma(n + 3) * (c.abs()[:, :, None] * mag).sum(1) + (e_c[:, :, None] * adiff).sum(1)
    e_dP = gamma(Nq + 3) * (c.abs()[:, :, None] * mag).sum(0) + (e_c[:, :, None] * adiff).sum(0)
    return dq, dP, e_dq, e_dP
