"""GPU: the BiLSTM kernels (csrc/lstm.hip) and their wiring (mmfusion/lstm_ops.py) step by step against the float64
restatement of tests/lstm_ref.py (itself pinned to torch.nn.LSTM by tests/test_lstm_ref_cpu.py).

Both persistent kernels hand state between workgroups every step through a device-scope counter barrier: h_t in the
forward, dG_t in the backward.  A stale read there moves a few elements by ~1e-2, which an fp32 nn.LSTM comparison at
bf16-compounded bounds cannot see.  So the kernel tests here are STEP-LOCAL: every step is restated from the kernel's own
state of the step before (its stored h_{t-1} and c_{t-1} in the forward, its own dG of the step processed before in the
backward), nothing compounds, and the bounds are f32-level error models, orders of magnitude below a stale fragment.

  A  forward through the C ABI, teacher-forced: gates and cell at f32 level, y within half a bf16 ulp of o tanh c;
  B  backward through the C ABI: dG within one bf16 rounding of the f64 BPTT fed by the kernel's dG; bit-determinism;
  C  _BiLSTMLayer: the wgrad / dx GEMMs on the exact dG the backward used, both input dtypes, and the ABI refusals;
  D  bilstm() end to end, two layers, free-running, with and without the inter-layer dropout, and batch chunking.

Shapes for A and B cover every (H, batch tiles) pair the kernels instantiate (H in 64 / 128 / 384, bt = ceil(B / 16) in
1..4) with T >= 2, T = 1, the reference's video head (H 384, B 16, T 30) and one long case (T 512).

Measured on MI355X, worst error / bound over all cases: gates 0.095 (the gamma_H term of the dot product is a worst
case), cell 0.66, y 0.995 and dG 0.993 (both are dominated by their own bf16 rounding, which reaches 2^-8 |x| just above a
power of two).  A stale 8-element fragment of h_{t-1} puts the gates at thousands of times their bound."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import lstm_ref  # noqa: E402
from helpers import l2_rel  # noqa: E402
from mmfusion import arena as arena_mod, lib, lstm_ops, ops  # noqa: E402

DEV = "cuda"
F64 = torch.float64
U = 2.0 ** -24                 # f32 unit roundoff
BF_U = 2.0 ** -8               # bf16 unit roundoff: |bf16(x) - x| <= 2^-8 |x|
MMF_E_SHAPE, MMF_E_ALIGN, MMF_E_UNSUPPORTED = -1, -3, -5

# (H, B, T): each H with bt = 1 (B 1, 16), 2 (B 17), 3 (B 40), 4 (B 64), T alternating 2 / 30; T = 1; the video head; T 512
STEP_CASES = [(64, 1, 30), (64, 16, 2), (64, 17, 30), (64, 40, 2), (64, 64, 30),
              (128, 1, 2), (128, 16, 30), (128, 17, 2), (128, 40, 30), (128, 64, 2),
              (384, 1, 30), (384, 16, 30), (384, 17, 2), (384, 40, 30), (384, 64, 2),
              (128, 40, 1), (384, 1, 1), (384, 64, 512)]


def _id(c):
    return "H%d-B%d-T%d" % c


def host(t):
    return t.detach().cpu().to(F64)


def _ws():
    return torch.zeros(lib.load().mmf_bilstm_workspace_bytes() // 4, dtype=torch.int32, device=DEV)


class Problem:
    """test-owned operands of one layer launch: gx f32 at the scale of the real projection (768 inputs, nn.LSTM init:
    std ~0.8), W_hh bf16 and the biases f32 at nn.LSTM's init scale, dy bf16"""

    def __init__(self, H, B, T, seed=0):
        g = torch.Generator().manual_seed(seed)
        k = 1.0 / math.sqrt(H)
        self.H, self.B, self.T = H, B, T
        self.gx = (torch.randn(T * B, 8 * H, generator=g) * 0.8).to(DEV)
        self.w_hh = [((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).to(torch.bfloat16).to(DEV) for _ in range(2)]
        self.b_ih = [((torch.rand(4 * H, generator=g) * 2 - 1) * k).to(DEV) for _ in range(2)]
        self.b_hh = [((torch.rand(4 * H, generator=g) * 2 - 1) * k).to(DEV) for _ in range(2)]
        self.dy = torch.randn(T * B, 2 * H, generator=g).to(torch.bfloat16).to(DEV)

    def fwd(self):
        """one forward launch; gates, cell and y's interior row blocks start as NaN, y's two padding blocks as zero"""
        H, B, T = self.H, self.B, self.T
        ybuf = torch.zeros(((T + 2) * B, 2 * H), dtype=torch.bfloat16, device=DEV)
        ybuf[B:(T + 1) * B] = float("nan")
        gates = torch.full((T * B, 8 * H), float("nan"), device=DEV)
        cell = torch.full((T * B, 2 * H), float("nan"), device=DEV)
        ws = _ws()
        P2 = C.c_void_p * 2
        args = lib.BiLstmArgs(self.gx.data_ptr(), P2(*[w.data_ptr() for w in self.w_hh]), P2(*[b.data_ptr() for b in self.b_ih]),
                              P2(*[b.data_ptr() for b in self.b_hh]), ybuf.data_ptr(), gates.data_ptr(), cell.data_ptr(),
                              None, None, T, B, H)
        lib.check(lib.load().mmf_bilstm_layer_fwd(C.byref(args), ws.data_ptr(), ws.numel() * 4, lib.stream_ptr()))
        torch.cuda.synchronize()
        assert int(ws[2]) == 0, "forward: a grid-barrier wait timed out"
        return ybuf, gates, cell

    def bwd(self, gates, cell):
        H, B, T = self.H, self.B, self.T
        dg = torch.full((T * B, 8 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
        ws = _ws()
        P2 = C.c_void_p * 2
        args = lib.BiLstmArgs(None, P2(*[w.data_ptr() for w in self.w_hh]), P2(None, None), P2(None, None), None,
                              gates.data_ptr(), cell.data_ptr(), self.dy.data_ptr(), dg.data_ptr(), T, B, H)
        lib.check(lib.load().mmf_bilstm_layer_bwd(C.byref(args), ws.data_ptr(), ws.numel() * 4, lib.stream_ptr()))
        torch.cuda.synchronize()
        assert int(ws[2]) == 0, "backward: a grid-barrier wait timed out"
        return dg


def act_err(a):
    """error of the kernel's __expf forms of sigmoid and tanh at argument a: the argument's rounding before the exp
    (|a| u), the exp itself and the three roundings around it, with a factor-2 margin"""
    return 4 * U * (a.abs() + 4)


def check_fwd_steps(p, ybuf, gates, cell):
    """every step of both directions restated from the kernel's own h_{t-1} (its y rows) and c_{t-1}.
    Error model, per element:  a = acc + gx + (b_ih + b_hh) with acc the K = H MFMA dot product in f32:
        e_a = (H + 3) u S + 3 u (|gx| + |b_ih| + |b_hh|),   S = sum_k |W_hh[n, k] h_{t-1}[k]|;
    a gate is off by its local derivative times e_a plus act_err(a); the cell is restated from the kernel's own gates
    (f c_{t-1} + i g: 3 u of its terms); y is bf16(o tanh c) of the kernel's o and c: 2^-8 |h| + act_err(c) + 2 u.
    Returns the worst error / bound ratio per quantity."""
    H, B, T = p.H, p.B, p.T
    yb, gk, ck = host(ybuf), host(gates), host(cell)
    assert torch.equal(yb[:B], torch.zeros(B, 2 * H, dtype=F64)) and torch.equal(yb[(T + 1) * B:], torch.zeros(B, 2 * H, dtype=F64)), \
        "y's padding row blocks were written"
    for name, t in (("y", yb[B:(T + 1) * B]), ("gates", gk), ("cell", ck)):
        assert bool(torch.isfinite(t).all()), f"{name}: elements never written (NaN)"
    gx = host(p.gx)
    worst = {}
    for d in range(2):
        sl, sg = slice(d * H, (d + 1) * H), slice(4 * d * H, 4 * (d + 1) * H)
        w = host(p.w_hh[d])
        b_ih, b_hh = host(p.b_ih[d]), host(p.b_hh[d])
        # h_{t-1} and c_{t-1} of every time step (rows time * B + b), the way this direction walks
        hp = yb[0:T * B, sl] if d == 0 else yb[2 * B:(T + 2) * B, sl]
        cp = torch.zeros(T * B, H, dtype=F64)
        if T > 1:
            if d == 0:
                cp[B:] = ck[:(T - 1) * B, sl]
            else:
                cp[:(T - 1) * B] = ck[B:, sl]
        a, g_ref, _, _ = lstm_ref.step_fwd(gx[:, sg], b_ih, b_hh, w, hp, cp)
        S = hp.abs() @ w.abs().t()
        e_a = (H + 3) * U * S + 3 * U * (gx[:, sg].abs() + b_ih.abs() + b_hh.abs())
        deriv = torch.cat([g_ref[:, :2 * H] * (1 - g_ref[:, :2 * H]), 1 - g_ref[:, 2 * H:3 * H] ** 2,
                           g_ref[:, 3 * H:] * (1 - g_ref[:, 3 * H:])], 1)
        bound_g = 1.01 * deriv * e_a + act_err(a) + 1e-30
        g = gk[:, sg]
        r = ((g - g_ref).abs() / bound_g).max()
        worst[f"gates d{d}"] = float(r)
        i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        c_ref = f * cp + i * gg
        c = ck[:, sl]
        worst[f"cell d{d}"] = float(((c - c_ref).abs() / (3 * U * ((f * cp).abs() + (i * gg).abs()) + 1e-30)).max())
        h = o * torch.tanh(c)
        y = yb[B:(T + 1) * B, sl]
        worst[f"y d{d}"] = float(((y - h).abs() / (BF_U * h.abs() + o.abs() * act_err(c) + 2 * U)).max())
    return worst


def check_bwd_steps(p, gates, cell, dg):
    """BPTT restated in float64 from the kernel's f32 gates and cell; dh of each step takes dhr from the KERNEL's dG of
    the step processed before, dc is carried in f64.  Error model, per element (u = 2^-24), carried along with dc:
        e_dh  = 4H u sum_n |W_hh[n, u] dG[n]| + u (|dy| + |dhr|)           (the K = 4H product over four waves)
        e_tc  = act_err(c), e_q = 2 |tanh c| e_tc + 2 u                     (q = 1 - tanh^2 c)
        e_dct = e_dc + e_dh |o q| + |dh o| e_q + 3 u (|dc| + |dh o q|),     e_dc' = |f| e_dct + u |dc'|
        e_i, e_f, e_g = e_dct |g i (1 - i)|, e_dct |c_{t-1} f (1 - f)|, e_dct |i (1 - g^2)|, each + 5 u |d|
        e_o   = e_dh |tanh c o (1 - o)| + e_tc |dh o (1 - o)| + 5 u |d_o|
    The kernel's dG is bf16(d_f32):  |dG - d| <= 2^-8 |d| + (1 + 2^-8) e_d + 2^-20 max|d of the step| (an f32-level floor
    for values near zero).  Returns the worst error / bound ratio."""
    H, B, T = p.H, p.B, p.T
    gk, ck, dgk, dy = host(gates), host(cell), host(dg), host(p.dy)
    assert bool(torch.isfinite(dgk).all()), "dgates: elements never written (NaN)"
    worst = 0.0
    for d in range(2):
        sl, sg = slice(d * H, (d + 1) * H), slice(4 * d * H, 4 * (d + 1) * H)
        w = host(p.w_hh[d])
        wa = w.abs()
        order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        dc = torch.zeros(B, H, dtype=F64)
        e_dc = torch.zeros(B, H, dtype=F64)
        for k in range(T - 1, -1, -1):
            t = order[k]
            rows = slice(t * B, (t + 1) * B)
            g, c = gk[rows, sg], ck[rows, sl]
            cp = ck[order[k - 1] * B:(order[k - 1] + 1) * B, sl] if k > 0 else torch.zeros(B, H, dtype=F64)
            if k < T - 1:
                prev = order[k + 1]
                dgp = dgk[prev * B:(prev + 1) * B, sg]
                dhr, e_dhr = dgp @ w, 4 * H * U * (dgp.abs() @ wa)
            else:
                dhr, e_dhr = torch.zeros(B, H, dtype=F64), torch.zeros(B, H, dtype=F64)
            dyt = dy[rows, sl]
            dh = dyt + dhr
            e_dh = e_dhr + U * (dyt.abs() + dhr.abs())
            d_ref, dc_new = lstm_ref.step_bwd(g, c, cp, dh, dc)
            i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
            tc = torch.tanh(c)
            q = 1 - tc * tc
            e_tc = act_err(c)
            e_q = 2 * tc.abs() * e_tc + 2 * U
            dct = dc + dh * o * q
            e_dct = e_dc + e_dh * (o * q).abs() + (dh * o).abs() * e_q + 3 * U * (dc.abs() + (dh * o * q).abs())
            e_d = torch.cat([e_dct * (gg * i * (1 - i)).abs(), e_dct * (cp * f * (1 - f)).abs(), e_dct * (i * (1 - gg * gg)).abs(),
                             e_dh * (tc * o * (1 - o)).abs() + e_tc * (dh * o * (1 - o)).abs()], 1) + 5 * U * d_ref.abs()
            bound = BF_U * d_ref.abs() + (1 + BF_U) * e_d + 2.0 ** -20 * float(d_ref.abs().max()) + 1e-30
            r = float(((dgk[rows, sg] - d_ref).abs() / bound).max())
            worst = max(worst, r)
            e_dc = f.abs() * e_dct + U * dc_new.abs()
            dc = dc_new
            assert r <= 1.0, f"dG direction {d}, time {t} (step {k}): error {r:.2f} x its bound"
    return worst


@pytest.mark.parametrize("case", STEP_CASES, ids=_id)
def test_forward_kernel_step_local(case):
    p = Problem(*case, seed=sum(case))
    ybuf, gates, cell = p.fwd()
    worst = check_fwd_steps(p, ybuf, gates, cell)
    print(f"fwd {_id(case)}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f"{k}: error {v:.2f} x its bound"


@pytest.mark.parametrize("case", STEP_CASES, ids=_id)
def test_backward_kernel_step_local_and_deterministic(case):
    p = Problem(*case, seed=sum(case) + 1)
    ybuf, gates, cell = p.fwd()
    dg = p.bwd(gates, cell)
    worst = check_bwd_steps(p, gates, cell, dg)
    print(f"bwd {_id(case)}: worst error / bound {worst:.3f}")
    ybuf2, gates2, cell2 = p.fwd()
    dg2 = p.bwd(gates2, cell2)
    for name, a, b in (("y", ybuf, ybuf2), ("gates", gates, gates2), ("cell", cell, cell2), ("dG", dg, dg2)):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32)), f"{name} not bit-identical"


# ---------------------------------------------------------------------------------------------- C: _BiLSTMLayer
def _module(In, H, layers, seed):
    torch.manual_seed(seed)
    m = torch.nn.LSTM(In, H, num_layers=layers, batch_first=True, bidirectional=True)
    ref = [lstm_ref.lstm_params(m, li) for li in range(layers)]
    m = m.to(DEV)
    arena = arena_mod.ensure(m)
    arena.zero_grad()
    return m, ref


def _rel(got, want):
    got, want = host(got), want.to(F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max() / max(float(want.abs().max()), 1e-30))


@pytest.mark.parametrize("B,T,In,H,x_dtype", [(24, 9, 96, 128, torch.float32), (24, 9, 96, 128, torch.bfloat16),
                                              (40, 30, 768, 384, torch.float32), (5, 6, 64, 64, torch.bfloat16)])
def test_layer_wiring_weight_and_input_gradients(B, T, In, H, x_dtype):
    """_BiLSTMLayer's GEMMs on the exact dG its backward used (mmf_bilstm_layer_bwd again on the saved state; the launch is
    deterministic, pinned above): dW_ih = dG^T x, dW_hh = dG^T h_prev with the shifted views of both directions, the bias
    sums (f32, 1e-5 of the tensor's scale; measured <= 5e-7) and dx = bf16(bf16(dG_0 W_ih_0) + dG_1 W_ih_1) (elementwise
    within the two roundings of its f32 noise interval, and <= 2^-7 of the scale; measured <= 2e-3), through swap01 in both
    input dtypes (an f32 input gets an f32 dx)."""
    m, _ = _module(In, H, 1, seed=B + T)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, In, generator=g).to(x_dtype).to(DEV).requires_grad_(True)
    dy = torch.randn(T * B, 2 * H, generator=g).to(torch.bfloat16).to(DEV)
    params = []
    for s in ("", "_reverse"):
        params += [getattr(m, f"{n}_l0{s}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    y = lstm_ops._BiLSTMLayer.apply(lstm_ops.swap01(x).view(T * B, In), T, B, *params)
    y.backward(dy, retain_graph=True)
    torch.cuda.synchronize()
    assert lstm_ops.last_status(y.grad_fn.status) == 0
    x_tb, ybuf, gates, cell = y.grad_fn.saved_tensors
    dg = torch.full((T * B, 8 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
    ws = _ws()
    P2 = C.c_void_p * 2
    args = lib.BiLstmArgs(None, P2(*[ops.shadow(w).data_ptr() for w in params[1::4]]), P2(None, None), P2(None, None), None,
                          gates.data_ptr(), cell.data_ptr(), dy.data_ptr(), dg.data_ptr(), T, B, H)
    lib.check(lib.load().mmf_bilstm_layer_bwd(C.byref(args), ws.data_ptr(), ws.numel() * 4, lib.stream_ptr()))
    torch.cuda.synchronize()
    dG = host(dg)
    xs, yb = host(x_tb), host(ybuf)
    assert torch.equal(xs.view(T, B, In), host(x).to(torch.bfloat16).to(F64).transpose(0, 1))
    h_prev = [yb[0:T * B, 0:H], yb[2 * B:(T + 2) * B, H:2 * H]]
    w_ih16 = [host(ops.shadow(w)) for w in params[0::4]]
    worst = {}
    for d in range(2):
        g_d = dG[:, 4 * H * d:4 * H * (d + 1)]
        want = {"weight_ih": g_d.t() @ xs, "weight_hh": g_d.t() @ h_prev[d], "bias_ih": g_d.sum(0), "bias_hh": g_d.sum(0)}
        for n, wv in want.items():
            name = f"{n}_l0{'_reverse' if d else ''}"
            e = _rel(getattr(m, name).grad, wv)
            worst[name] = e
            assert e <= 1e-5, f"{name}: {e:.3e}"
    # dx = bf16(bf16(A) + B), A = dG_0 W_ih_0 and B = dG_1 W_ih_1 from f32 GEMMs (K = 4H: |noise| <= 4H u sum |dG W|).  Both
    # roundings are monotone, so the kernel's dx lies between the roundings of the noise interval's ends; a rounding flip
    # of A in the tensor's top binade alone is one ulp = 2^-7 of the scale, so a scale-relative 2^-8 would not be a bound
    A, Bv = dG[:, :4 * H] @ w_ih16[0], dG[:, 4 * H:] @ w_ih16[1]
    e_A = 4 * H * U * (dG[:, :4 * H].abs() @ w_ih16[0].abs())
    e_B = 4 * H * U * (dG[:, 4 * H:].abs() @ w_ih16[1].abs())
    a_lo, a_hi = lstm_ref.bf(A - e_A), lstm_ref.bf(A + e_A)
    e_S = e_B + U * (torch.maximum(a_lo.abs(), a_hi.abs()) + Bv.abs())
    lo, hi = lstm_ref.bf(a_lo + Bv - e_S), lstm_ref.bf(a_hi + Bv + e_S)
    dx_tb = lstm_ref.bf(lstm_ref.bf(A) + Bv)
    assert x.grad.dtype == x_dtype
    dxk = host(x.grad).transpose(0, 1).reshape(T * B, In)
    assert bool(torch.isfinite(dxk).all())
    outside = int(((dxk < lo) | (dxk > hi)).sum())
    assert outside == 0, f"dx: {outside} elements outside their rounding interval, worst {_rel(dxk, dx_tb):.3e} of the scale"
    worst["dx"] = _rel(dxk, dx_tb)
    assert worst["dx"] <= 2 * BF_U
    print(f"layer B{B} T{T} H{H} {x_dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("what,T,B,H,expect", [("batch", 4, 65, 64, MMF_E_SHAPE), ("hidden", 4, 8, 96, MMF_E_UNSUPPORTED),
                                                ("steps", 0, 8, 64, MMF_E_SHAPE), ("w_hh alignment", 4, 8, 64, MMF_E_ALIGN)])
def test_layer_refusals_launch_nothing(bwd, what, T, B, H, expect):
    """the shape / alignment refusals return their codes before anything reaches the stream: the workspace (which every
    accepted call clears before its launch) keeps its fill"""
    Tb = max(T, 1)
    w = torch.zeros(4 * H * H + 8, dtype=torch.bfloat16, device=DEV)
    w_ptr = w.data_ptr() + (2 if what == "w_hh alignment" else 0)
    b = torch.zeros(4 * H, device=DEV)
    gx = torch.zeros(Tb * B, 8 * H, device=DEV)
    y = torch.zeros((Tb + 2) * B, 2 * H, dtype=torch.bfloat16, device=DEV)
    gates = torch.zeros(Tb * B, 8 * H, device=DEV)
    cell = torch.zeros(Tb * B, 2 * H, device=DEV)
    dy = torch.zeros(Tb * B, 2 * H, dtype=torch.bfloat16, device=DEV)
    dg = torch.zeros(Tb * B, 8 * H, dtype=torch.bfloat16, device=DEV)
    ws = torch.full((lib.load().mmf_bilstm_workspace_bytes() // 4,), 7, dtype=torch.int32, device=DEV)
    P2 = C.c_void_p * 2
    args = lib.BiLstmArgs(gx.data_ptr(), P2(w_ptr, w_ptr), P2(b.data_ptr(), b.data_ptr()), P2(b.data_ptr(), b.data_ptr()),
                          y.data_ptr(), gates.data_ptr(), cell.data_ptr(), dy.data_ptr(), dg.data_ptr(), T, B, H)
    fn = lib.load().mmf_bilstm_layer_bwd if bwd else lib.load().mmf_bilstm_layer_fwd
    rc = fn(C.byref(args), ws.data_ptr(), ws.numel() * 4, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (what, rc, lib.load().mmf_last_error())
    assert bool((ws == 7).all()), f"{what}: something was launched"
    assert not bool(y.any()) and not bool(dg.any())


# ---------------------------------------------------------------------------------------------- D: bilstm() end to end
OUT_MAXABS = 2.0 ** -7
GRAD_L2 = 5e-3


class _DropoutSpy:
    """records (input, output) of every ops.dropout call lstm_ops makes"""

    def __init__(self, monkeypatch):
        self.calls = []
        orig = ops.dropout

        def spy(x, p, training):
            y = orig(x, p, training)
            self.calls.append((x.detach(), y.detach(), p, training))
            return y
        monkeypatch.setattr(ops, "dropout", spy)


@pytest.mark.parametrize("dropout", [0.0, 0.3], ids=["nodrop", "drop0.3"])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,In,H", [(16, 30, 768, 384), (65, 9, 96, 128), (130, 7, 48, 64)])
def test_bilstm_end_to_end_free_running(B, T, In, H, x_dtype, dropout, monkeypatch):
    """two layers against the free-running restatement: output, input gradient and all 16 parameter gradients.  B 65 and
    130 run the batch in chunks of 64.  With dropout, the kernel's mask is read off the device (dropped elements are exact
    zeros) and fed to the restatement; it must sit between the layers only.

    Bounds (error model, then measured on MI355X).  The two sides round the same values at the same points and differ by f32
    noise (~1e-6 relative) until that noise straddles a bf16 rounding boundary: the stored h then differs by one ulp
    (<= 2^-8 for |h| < 1).  Through W_hh that moves the next step's pre-activations by ~1e-4, which flips further roundings,
    so over T steps the flips spread until the two sides round like independent bf16 stores; the forget gate (< 1) damps
    the differences, so they stay at that level instead of growing.  Output: every element within about one ulp of its
    binade, at most 2^-8 for |h| < 1: max-abs <= 2^-7 leaves a factor of two.  Gradients: one decorrelated bf16 rounding
    has a relative rms of ~2^-8 sqrt(2/3) 0.72 = 2.3e-3 over the two sides; dx carries the dG rounding and its own two
    (the bf16 aux GEMM and the final store), sqrt(3) x 2.3e-3 = 4e-3 if all three decorrelate, and the weight gradients
    average the dG rounding over T * B rows: relative L2 <= 5e-3.
    Measured on MI355X over the 12 cases: output max-abs 4.9e-4 ... 1.95e-3 (2^-9); input gradient rel L2 4.8e-4 ... 3.13e-3
    (H 384, T 30); parameter gradients 2.0e-4 ... 1.98e-3."""
    m, ref_layers = _module(In, H, 2, seed=B + T)
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(B, T, In, generator=g)
    w = torch.randn(B, T, 2 * H, generator=g)
    spy = _DropoutSpy(monkeypatch)
    x = x0.to(x_dtype).to(DEV).requires_grad_(True)
    y = lstm_ops.bilstm(m, x, dropout)
    (y.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert y.shape == (B, T, 2 * H) and y.dtype == torch.bfloat16

    chunks = [min(64, B - b0) for b0 in range(0, B, 64)]
    masks = None
    if dropout > 0:
        assert len(spy.calls) == len(chunks), "one dropout per chunk: between the two layers, nowhere else"
        parts = []
        for (xin, xout, p, training), Bc in zip(spy.calls, chunks):
            assert p == dropout and training and xin.shape == (T * Bc, 2 * H) and xin.dtype == torch.bfloat16
            assert not bool((xin == 0).any()), "an exact zero in the layer-0 output: the mask would be ambiguous"
            parts.append((xout != 0).to(F64).cpu().view(T, Bc, 2 * H).transpose(0, 1))
        mask = torch.cat(parts, 0)
        frac = 1 - float(mask.mean())
        n = mask.numel()
        assert abs(frac - dropout) <= 5 * math.sqrt(dropout * (1 - dropout) / n), f"dropped fraction {frac:.4f}"
        masks = [mask]
        assert float((y == 0).float().mean()) < 1e-3, "the last layer's output carries dropout zeros"
    else:
        assert all(not (c[2] > 0 and c[3]) for c in spy.calls)

    xr = lstm_ref.bf(x0.to(x_dtype).to(F64)) if x_dtype == torch.bfloat16 else x0.to(F64)
    yr, cache = lstm_ref.bilstm_fwd(xr, ref_layers, rnd=True, masks=masks, p=dropout)
    dxr, grads = lstm_ref.bilstm_bwd(cache, w.to(F64))
    e_out = float((host(y) - yr).abs().max())
    e_dx = l2_rel(x.grad, dxr)
    e_p = {n: l2_rel(prm.grad, grads[n]) for n, prm in m.named_parameters()}
    worst_p = max(e_p.items(), key=lambda kv: kv[1])
    print(f"bilstm B{B} T{T} H{H} {x_dtype} p={dropout}: out max-abs {e_out:.3e}, dx rel L2 {e_dx:.3e}, "
          f"worst param {worst_p[0]} {worst_p[1]:.3e}")
    assert len(e_p) == 16
    assert e_out <= OUT_MAXABS, f"output max-abs {e_out:.3e}"
    assert e_dx <= GRAD_L2, f"input gradient rel L2 {e_dx:.3e}"
    for n, e in e_p.items():
        assert e <= GRAD_L2, f"grad {n} rel L2 {e:.3e}"

    if B > 128 and dropout == 0:
        # the second chunk of 64 alone: bit-identical output and input gradient
        xs = x0[64:128].to(x_dtype).to(DEV).requires_grad_(True)
        ys = lstm_ops.bilstm(m, xs)
        (ys.float() * w[64:128].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(ys, y[64:128]), "chunk 64..127 output differs from running those samples alone"
        assert torch.equal(xs.grad, x.grad[64:128]), "chunk 64..127 input gradient differs from running those samples alone"
