"""Float64 restatement of RobustMultimodalModel's head (reference models/multimodal_model.py:404-440) after the predictor's
hidden layer h, and of its backward, written out term by term so that the kernel tests have something independent of both
the HIP code and torch autograd to hold the kernels to.  Per sample, m in (text, audio, video):

    a     = sigmoid(W2 h + b2)            p_m = W_m f_m + b_m
    w     = a (mask None) or the 0/1 indicator of the mask bits (constants)
    wn_m  = w_m / (sum_k w_k + 1e-8)      y = sum_m wn_m p_m

  given g = dL/dy and the optional direct gradients P_m (of p_m), A (of a), N (of wn):
    dwn_m = g . p_m + N_m                 dp_m = wn_m g + P_m
    predicted: dz_m = (A_m + (dwn_m - sum_k wn_k dwn_k) / (S + 1e-8)) a_m (1 - a_m);  given: dz_m = A_m a_m (1 - a_m)
    df_m = W_m^T dp_m, dW_m = sum_b dp_m f_m^T, db_m = sum_b dp_m;  dh = W2^T dz, dW2 = sum_b dz h^T, db2 = sum_b dz

Error bounds of the f32 kernels (csrc/small.hip robust_*_kernel), u = 2^-24, worst case: a sum of n products to
(n + 2) u of the sum of their magnitudes; sigmoid through __expf to 4 u absolute plus a(1 - a) times the error of its
argument; a division or product to 1 u more.  The backward's bounds take the forward's saved f32 values (a, p_m, wn) as
exact: they bound the backward kernel's own arithmetic."""
import torch

F64 = torch.float64
U = 2.0 ** -24
EPS = 1e-8


def _d(x):
    return None if x is None else x.detach().to(F64).cpu()


def mask_weights(mask: int, B: int):
    return torch.tensor([float((mask >> i) & 1) for i in range(3)], dtype=F64).expand(B, 3)


def head_fwd(f, h, W2, b2, Wm, bm, mask=None):
    """f: 3 x (B, d), h (B, d), W2 (3, d), b2 (3), Wm: 3 x (C, d), bm: 3 x (C) -> dict of float64 outputs and bounds"""
    f, h, W2, b2 = [_d(x) for x in f], _d(h), _d(W2), _d(b2)
    Wm, bm = [_d(x) for x in Wm], [_d(x) for x in bm]
    B, d = h.shape
    z = h @ W2.T + b2
    ez = (d + 2) * U * (h.abs() @ W2.abs().T + b2.abs())
    a = torch.sigmoid(z)
    ea = a * (1 - a) * (ez + 2 * U * z.abs()) + 4 * U           # (__expf: the argument's scaling to 2 u |z|)
    p = [fm @ W.T + b for fm, W, b in zip(f, Wm, bm)]
    ep = [(d + 2) * U * (fm.abs() @ W.abs().T + b.abs()) for fm, W, b in zip(f, Wm, bm)]
    if mask is None or mask < 0:
        w, ew = a, ea
    else:
        w, ew = mask_weights(mask, B), torch.zeros(B, 3, dtype=F64)
    S = w.sum(dim=1, keepdim=True)
    den = S + EPS
    wn = w / den
    ewn = (ew + wn * (ew.sum(dim=1, keepdim=True) + 2 * U * S)) / den + 2 * U * wn.abs()
    y = sum(wn[:, m:m + 1] * p[m] for m in range(3))
    ey = sum(wn[:, m:m + 1].abs() * ep[m] + p[m].abs() * ewn[:, m:m + 1] for m in range(3)) \
        + 3 * U * sum((wn[:, m:m + 1] * p[m]).abs() for m in range(3))
    return {"a": a, "p": p, "wn": wn, "y": y, "ea": ea, "ep": ep, "ewn": ewn, "ey": ey}


def head_bwd(f, h, W2, Wm, a, p, wn, g, dP=None, dA=None, dN=None, mask=None):
    """float64 backward from the saved forward values (a, p_m, wn) -> dict with df (3), dh, dW2, db2, dWm (3), dbm (3) and
    an elementwise bound 'e_<name>' for each (the kernel's f32 arithmetic on the same saved values)"""
    f, h, W2, Wm = [_d(x) for x in f], _d(h), _d(W2), [_d(x) for x in Wm]
    a, p, wn, g = _d(a), [_d(x) for x in p], _d(wn), _d(g)
    B, C = g.shape
    dP = [None] * 3 if dP is None else [_d(x) for x in dP]
    dA, dN = _d(dA), _d(dN)
    zero3 = torch.zeros(B, 3, dtype=F64)
    dwn = torch.stack([(g * p[m]).sum(dim=1) for m in range(3)], dim=1) + (dN if dN is not None else zero3)
    edwn = (C + 2) * U * (torch.stack([(g * p[m]).abs().sum(dim=1) for m in range(3)], dim=1)
                          + (dN.abs() if dN is not None else zero3))
    dp = [wn[:, m:m + 1] * g + (dP[m] if dP[m] is not None else 0.0) for m in range(3)]
    edp = [2 * U * ((wn[:, m:m + 1] * g).abs() + (dP[m].abs() if dP[m] is not None else 0.0)) for m in range(3)]
    A = dA if dA is not None else zero3
    if mask is None or mask < 0:
        den = a.sum(dim=1, keepdim=True) + EPS
        dot = (wn * dwn).sum(dim=1, keepdim=True)
        dw = (dwn - dot) / den
        edot = (wn.abs() * edwn).sum(dim=1, keepdim=True) + 3 * U * (wn * dwn).abs().sum(dim=1, keepdim=True)
        edw = (edwn + edot + 2 * U * (dwn.abs() + dot.abs())) / den + 2 * U * dw.abs()
        dw = dw + A
    else:
        dw, edw = A, zero3
    s = a * (1 - a)
    dz = dw * s
    edz = (edw + 2 * U * dw.abs()) * s + 3 * U * dz.abs()
    out = {"df": [dp[m] @ Wm[m] for m in range(3)],
           "e_df": [edp[m] @ Wm[m].abs() + (C + 2) * U * (dp[m].abs() @ Wm[m].abs()) for m in range(3)],
           "dWm": [dp[m].T @ f[m] for m in range(3)],
           "e_dWm": [edp[m].T @ f[m].abs() + (B + 2) * U * (dp[m].abs().T @ f[m].abs()) for m in range(3)],
           "dbm": [dp[m].sum(dim=0) for m in range(3)],
           "e_dbm": [edp[m].sum(dim=0) + (B + 2) * U * dp[m].abs().sum(dim=0) for m in range(3)],
           "dh": dz @ W2, "e_dh": edz @ W2.abs() + 5 * U * (dz.abs() @ W2.abs()),
           "dW2": dz.T @ h, "e_dW2": edz.T @ h.abs() + (B + 2) * U * (dz.abs().T @ h.abs()),
           "db2": dz.sum(dim=0), "e_db2": edz.sum(dim=0) + (B + 2) * U * dz.abs().sum(dim=0)}
    return out


def torch_head(f, h, W2, b2, Wm, bm, available=None):
    """The reference's own formulation of the head (multimodal_model.py:404-440 after the hidden layer), in torch ops on
    whatever dtype and device the arguments have: (a, [p_t, p_a, p_v], weights, y).  ``available``: None or a list of
    modality names, as the reference takes it."""
    a = torch.sigmoid(h @ W2.T + b2)
    p = [fm @ W.T + b for fm, W, b in zip(f, Wm, bm)]
    if available is None:
        weights = a
    else:
        weights = torch.zeros_like(a)
        for i, name in enumerate(("text", "audio", "video")):
            if name in available:
                weights[:, i] = 1.0
    weights = weights / (torch.sum(weights, dim=1, keepdim=True) + 1e-8)
    y = weights[:, 0:1] * p[0] + weights[:, 1:2] * p[1] + weights[:, 2:3] * p[2]
    return a, p, weights, y
