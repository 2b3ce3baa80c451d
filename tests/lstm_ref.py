"""float64 restatement of the bidirectional LSTM the HIP path computes (csrc/lstm.hip, mmfusion/lstm_ops.py) — a test helper.

Written from ``torch.nn.LSTM``'s equations (gate order i, f, g, o; zero initial state; the reverse direction walks
t = T-1 ... 0), with a rounding hook at every point where the HIP path stores bf16.  With ``rnd=True``:
  forward   x and W_ih, W_hh are their bf16 values (the shadows), the biases stay f32; gx = x16 W_ih16^T is kept unrounded
            (the kernel stores it as f32); per step a = gx + b_ih + b_hh + bf16(h_{t-1}) W_hh16^T, the cell c unrounded,
            the stored output y = bf16(o tanh c), which the next step reads;
  backward  dh = dy16 + dhr, dG rounded to bf16, dhr = dG16 W_hh16, dW_ih = dG16^T x16, dW_hh = dG16^T h_prev16 (h_prev of
            the reverse direction is the NEXT time step's h), bias gradients the column sums of dG16, and
            dx = bf16(bf16(dG16_0 W_ih16_0) + dG16_1 W_ih16_1) (the two NN GEMMs of _BiLSTMLayer.backward, the first stored
            as bf16 and added as aux);
  dropout   between layers, as a given keep mask scaled by 1 / (1 - p), its output rounded to bf16.
With ``rnd=False`` every hook is the identity and this is nn.LSTM in float64 (tests/test_lstm_ref_cpu.py pins that).

Three levels: ``step_fwd`` / ``step_bwd`` take the previous state as an argument (the GPU tests feed them the kernel's own
state, so nothing compounds), ``layer_fwd`` / ``layer_bwd`` run one bidirectional layer free, ``bilstm_fwd`` /
``bilstm_bwd`` compose layers with the inter-layer dropout.  Tensors are batch-first: x (B, T, In), y (B, T, 2H)."""
import torch

F64 = torch.float64
GATES = ("i", "f", "g", "o")


def bf(x, rnd=True):
    """the value x has after a bf16 store (round to nearest even), as float64; the identity with rnd=False"""
    return x.to(torch.bfloat16).to(F64) if rnd else x.to(F64)


def step_fwd(gx, b_ih, b_hh, w_hh, h_prev, c_prev):
    """one step of one direction.  gx (B, 4H) = x_t W_ih^T, h_prev (B, H) the stored h_{t-1}, c_prev (B, H).
    Returns (a, gates, c, h): pre-activations (B, 4H), activated gates (B, 4H) in the order i, f, g, o, the cell and
    h = o tanh c (unrounded)."""
    H = w_hh.shape[1]
    a = gx + b_ih + b_hh + h_prev @ w_hh.t()
    i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
    c = f * c_prev + i * g
    return a, torch.cat([i, f, g, o], 1), c, o * torch.tanh(c)


def step_bwd(gates, c, c_prev, dh, dc):
    """the gate pre-activation gradient of one step.  gates (B, 4H) activated, c / c_prev the cell after / before the step,
    dh = dy + dhr the gradient reaching h_t, dc the cell gradient carried from the step processed before.
    Returns (dG (B, 4H) unrounded, dc for the next step processed)."""
    H = c.shape[1]
    i, f, g, o = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:3 * H], gates[:, 3 * H:]
    tc = torch.tanh(c)
    dct = dc + dh * o * (1 - tc * tc)
    dG = torch.cat([dct * g * i * (1 - i), dct * c_prev * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    return dG, dct * f


def _times(T, d):
    return range(T) if d == 0 else range(T - 1, -1, -1)


def layer_fwd(x, params, rnd=True):
    """one bidirectional layer, free-running.  params: (w_ih, w_hh, b_ih, b_hh) of direction 0, then of direction 1.
    Returns (y (B, T, 2H) as stored, cache for layer_bwd)."""
    x16 = bf(x, rnd)
    B, T, _ = x16.shape
    H = params[1].shape[1]
    ys, cache = [], {"x16": x16, "params": params, "rnd": rnd, "dirs": []}
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = params[4 * d:4 * d + 4]
        w_ih16, w_hh16 = bf(w_ih, rnd), bf(w_hh, rnd)
        gx = x16 @ w_ih16.t()                                     # (B, T, 4H), unrounded (f32 in the kernel)
        h = torch.zeros(B, H, dtype=F64)
        c = torch.zeros(B, H, dtype=F64)
        y = torch.zeros(B, T, H, dtype=F64)
        gates = torch.zeros(B, T, 4 * H, dtype=F64)
        cells = torch.zeros(B, T, H, dtype=F64)
        for t in _times(T, d):
            _, gt, c, hu = step_fwd(gx[:, t], b_ih.to(F64), b_hh.to(F64), w_hh16, h, c)
            h = bf(hu, rnd)
            y[:, t], gates[:, t], cells[:, t] = h, gt, c
        ys.append(y)
        cache["dirs"].append({"w_ih16": w_ih16, "w_hh16": w_hh16, "y": y, "gates": gates, "cells": cells})
    return torch.cat(ys, 2), cache


def layer_bwd(cache, dy):
    """BPTT of one layer.  dy (B, T, 2H) the gradient of the stored output.
    Returns (dx (B, T, In), [dW_ih, dW_hh, db_ih, db_hh] of direction 0 then 1, [dG16 (B, T, 4H)] per direction)."""
    rnd, x16 = cache["rnd"], cache["x16"]
    B, T, _ = x16.shape
    dy16 = bf(dy, rnd)
    H = dy16.shape[2] // 2
    grads, dGs = [], []
    for d in range(2):
        st = cache["dirs"][d]
        dG = torch.zeros(B, T, 4 * H, dtype=F64)
        dhr = torch.zeros(B, H, dtype=F64)
        dc = torch.zeros(B, H, dtype=F64)
        order = list(_times(T, d))
        for k in range(T - 1, -1, -1):                            # the forward's steps, last first
            t = order[k]
            c_prev = st["cells"][:, order[k - 1]] if k > 0 else torch.zeros(B, H, dtype=F64)
            g, dc = step_bwd(st["gates"][:, t], st["cells"][:, t], c_prev, dy16[:, t, d * H:(d + 1) * H] + dhr, dc)
            dG[:, t] = bf(g, rnd)
            dhr = dG[:, t] @ st["w_hh16"]
        # h_prev as the steps saw it: direction 0 the step before, direction 1 the step after (zero at the ends)
        h_prev = torch.zeros_like(st["y"])
        if d == 0:
            h_prev[:, 1:] = st["y"][:, :-1]
        else:
            h_prev[:, :-1] = st["y"][:, 1:]
        g2 = dG.reshape(B * T, 4 * H)
        grads += [g2.t() @ x16.reshape(B * T, -1), g2.t() @ h_prev.reshape(B * T, H), g2.sum(0), g2.sum(0)]
        dGs.append(dG)
    dx = bf(bf(dGs[0] @ cache["dirs"][0]["w_ih16"], rnd) + dGs[1] @ cache["dirs"][1]["w_ih16"], rnd)
    return dx, grads, dGs


def lstm_params(lstm, layer):
    """(w_ih, w_hh, b_ih, b_hh) of both directions of one layer of an nn.LSTM, as float64 CPU tensors"""
    return [getattr(lstm, f"{n}_l{layer}{s}").detach().cpu().to(F64)
            for s in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def param_names(layer):
    return [f"{n}_l{layer}{s}" for s in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def bilstm_fwd(x, layers, rnd=True, masks=None, p=0.0):
    """stacked bidirectional layers.  layers: one params list per layer (lstm_params); masks: one 0/1 keep mask
    (B, T, 2H) per layer boundary (len(layers) - 1 of them) or None for no dropout.  Returns (y, cache)."""
    caches, h = [], x
    for li, prm in enumerate(layers):
        h, c = layer_fwd(h, prm, rnd)
        caches.append(c)
        if li + 1 < len(layers) and masks is not None:
            h = bf(h * masks[li] / (1.0 - p), rnd)
    return h, {"layers": caches, "masks": masks, "p": p, "rnd": rnd}


def bilstm_bwd(cache, dy):
    """Returns (dx, {param name: grad}) with nn.LSTM's parameter names."""
    grads, g = {}, dy
    n = len(cache["layers"])
    for li in range(n - 1, -1, -1):
        if li + 1 < n and cache["masks"] is not None:
            g = bf(g * cache["masks"][li] / (1.0 - cache["p"]), cache["rnd"])
        g, gr, _ = layer_bwd(cache["layers"][li], g)
        grads.update(zip(param_names(li), gr))
    return g, grads
