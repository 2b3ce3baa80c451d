"""CPU: tests/lstm_ref.py with every rounding hook off is torch.nn.LSTM in float64 — forward output, input gradient and all
parameter gradients (autograd), 1e-10.  This anchors the restatement the GPU tests hold the BiLSTM kernels to
(tests/test_lstm_kernel_gpu.py) to the reference module's semantics, so those tests test only the kernels."""
import pytest
import torch

import lstm_ref

TOL = 1e-10


def _lstm(In, H, layers, seed):
    torch.manual_seed(seed)
    return torch.nn.LSTM(In, H, num_layers=layers, batch_first=True, bidirectional=True).double()


def _close(got, want, what):
    err = float((got - want).abs().max() / max(1.0, float(want.abs().max())))
    assert err <= TOL, f"{what}: {err:.3e}"


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("T", [1, 7])
def test_restatement_is_nn_lstm_in_float64(layers, T):
    B, In, H = 3, 10, 6
    lstm = _lstm(In, H, layers, seed=T + layers)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
    w = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    yr, _ = lstm(xr)
    (yr * w).sum().backward()

    y, cache = lstm_ref.bilstm_fwd(x, [lstm_ref.lstm_params(lstm, li) for li in range(layers)], rnd=False)
    dx, grads = lstm_ref.bilstm_bwd(cache, w)
    _close(y, yr.detach(), "output")
    # both directions are in the output: each half on its own
    _close(y[..., :H], yr.detach()[..., :H], "output, direction 0")
    _close(y[..., H:], yr.detach()[..., H:], "output, direction 1")
    _close(dx, xr.grad, "input gradient")
    names = dict(lstm.named_parameters())
    assert sorted(grads) == sorted(names) and len(grads) == 8 * layers
    for n, p in names.items():
        _close(grads[n], p.grad, n)


def test_restatement_with_a_dropout_mask_is_the_layer_composition():
    """inter-layer dropout as a given mask: layer 0, then y * mask / (1 - p), then layer 1 — two single-layer nn.LSTM in
    float64 with the same weights and the same mask"""
    B, T, In, H, p = 4, 5, 8, 6, 0.3
    lstm = _lstm(In, H, 2, seed=9)
    l0, l1 = _lstm(In, H, 1, seed=0), _lstm(2 * H, H, 1, seed=0)
    for dst, li in ((l0, 0), (l1, 1)):
        dst.load_state_dict({k.replace(f"_l{li}", "_l0"): v for k, v in lstm.state_dict().items() if f"_l{li}" in k})
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
    w = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64)
    mask = (torch.rand(B, T, 2 * H, generator=g) >= p).to(torch.float64)
    xr = x.clone().requires_grad_(True)
    yr = l1(l0(xr)[0] * mask / (1 - p))[0]
    (yr * w).sum().backward()

    y, cache = lstm_ref.bilstm_fwd(x, [lstm_ref.lstm_params(lstm, li) for li in range(2)], rnd=False, masks=[mask], p=p)
    dx, grads = lstm_ref.bilstm_bwd(cache, w)
    _close(y, yr.detach(), "output")
    _close(dx, xr.grad, "input gradient")
    for li, mod in ((0, l0), (1, l1)):
        for n, prm in mod.named_parameters():
            _close(grads[n.replace("_l0", f"_l{li}")], prm.grad, f"layer {li} {n}")


def test_rounding_hooks_round_where_the_kernels_store_bf16():
    """with the hooks on, the stored output and dG are bf16 values and dx is a bf16 value; the cell is not rounded"""
    lstm = _lstm(12, 8, 1, seed=4)
    x = torch.randn(2, 5, 12, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    y, cache = lstm_ref.layer_fwd(x, lstm_ref.lstm_params(lstm, 0), rnd=True)
    dx, _, dGs = lstm_ref.layer_bwd(cache, torch.randn(2, 5, 16, dtype=torch.float64))
    for t in [y, dx] + dGs:
        assert torch.equal(t, lstm_ref.bf(t))
    cells = cache["dirs"][0]["cells"]
    assert not torch.equal(cells, lstm_ref.bf(cells))
    y0, _ = lstm_ref.layer_fwd(x, lstm_ref.lstm_params(lstm, 0), rnd=False)
    assert 0 < float((y - y0).abs().max()) < 2e-2
