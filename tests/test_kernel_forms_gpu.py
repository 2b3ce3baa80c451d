"""GPU: every instantiation the host dispatch selects from a problem's shape, pinned kernel by kernel against a float64 CPU
restatement of the same op on the same bf16-rounded (or f32) operands.

The unit tests in test_kernels_gpu.py reach the forms their small shapes select; the forms that run at production sizes
(the LayerNorm lane form above 4096 rows, the 64-column skinny dgrad strip, the fp32 parity-mode kernels, the fused loss)
are otherwise seen only through module and model parity at loose tolerances.  Each case here asserts the form it targets
(mmf_layernorm_last_form / mmf_skinny_last_strip), pre-fills every output with NaN unless it tests accumulation, and holds
bf16 outputs to 2^-8 of the tensor's scale and f32 results to 1e-5 (one documented exception: dgamma of rows around 1000)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mmfusion import lib, ops, small_ops  # noqa: E402
from mmfusion.lib import (EPI_ACCUM, EPI_ADD_AUX, EPI_BIAS, EPI_COLSUM_A, EPI_DROPOUT, EPI_MASK_AUX, EPI_RELU, GEMM_NN,
                          GEMM_NT, GEMM_TN)  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF16_TOL = 2 ** -8
F32_TOL = 1e-5


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def bf(x):
    """bf16 on the device (the kernel's operand); .double().cpu() of it is the reference's operand"""
    return x.to(torch.bfloat16).to(DEV)


def f32(x):
    return x.to(torch.float32).to(DEV)


def nan_like(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().double()


def rel(a, ref, floor=1e-12):
    """max |a - ref| relative to the reference's largest magnitude; NaN anywhere in `a` (an element never written) fails"""
    a, ref = host(a), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if not bool(torch.isfinite(a).all()):
        return math.inf
    return float((a - ref).abs().max() / max(float(ref.abs().max()), floor))


# ---------------------------------------------------------------------------------------- LayerNorm, bf16, grouped
EPS = 1e-5
LANE_D = (256, 512, 768, 1024)


def lane_id(d):
    return 100 + 10 * (d // 512) + (d // 256) % 2


def ln_expected_form(d, rows, fwd):
    """the dispatch rule of csrc/layernorm.hip: the lane form for d in LANE_D — always in the backward, in the forward only
    when the launch has more row blocks (4 rows each) than its workgroup budget (1024, or 2048 above 20000 rows)"""
    blocks, total = sum((r + 3) // 4 for r in rows), sum(rows)
    lane = d in LANE_D and (not fwd or blocks > (2048 if total > 20000 else 1024))
    return lane_id(d) if lane else (d + 511) // 512


def ln_ref(x, g, b, dy):
    """float64 nn.LayerNorm forward and backward on one problem: y, mean, rstd, dx, dgamma, dbeta"""
    mu = x.mean(1, keepdim=True)
    rstd = ((x - mu) ** 2).mean(1, keepdim=True).add(EPS).rsqrt()
    xh = (x - mu) * rstd
    gy = dy * g
    dx = rstd * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    return xh * g + b, mu[:, 0], rstd[:, 0], dx, (dy * xh).sum(0), dy.sum(0)


def run_ln(d, xs, gammas, betas, dys, share_first=False, dg_tol=None):
    """one grouped forward and one grouped backward over len(xs) problems (problem 1 reuses problem 0's gamma / beta when
    share_first), dgamma / dbeta pre-filled with non-zero values; every output checked against ln_ref"""
    n = len(xs)
    rows = [x.shape[0] for x in xs]
    L = lib.load()
    x16 = [bf(x) for x in xs]
    dy16 = [bf(v) for v in dys]
    gs = [f32(g) for g in gammas]
    bs = [f32(b) for b in betas]
    if share_first:
        gs[1], bs[1] = gs[0], bs[0]
    y = [nan_like((r, d), torch.bfloat16) for r in rows]
    dx = [nan_like((r, d), torch.bfloat16) for r in rows]
    mean, rstd = [nan_like((r,)) for r in rows], [nan_like((r,)) for r in rows]
    dg0 = [rnd(d, seed=900 + i).float().double() for i in range(n)]
    db0 = [rnd(d, seed=950 + i).float().double() for i in range(n)]
    dg, db = [f32(v) for v in dg0], [f32(v) for v in db0]
    probs = [lib.LnProblem(x16[i].data_ptr(), y[i].data_ptr(), gs[i].data_ptr(), bs[i].data_ptr(), mean[i].data_ptr(),
                           rstd[i].data_ptr(), dy16[i].data_ptr(), dx[i].data_ptr(), dg[i].data_ptr(), db[i].data_ptr(), rows[i])
             for i in range(n)]
    lib.layernorm_fwd_grouped(probs, d, EPS)
    assert L.mmf_layernorm_last_form() == ln_expected_form(d, rows, True)
    ws = torch.empty(L.mmf_layernorm_bwd_workspace_bytes(d) // 4, dtype=torch.float32, device=DEV)
    lib.layernorm_bwd_grouped(probs, d, ws)
    assert L.mmf_layernorm_last_form() == ln_expected_form(d, rows, False)
    torch.cuda.synchronize()
    for i in range(n):
        yr, mr, rr, dxr, dgr, dbr = ln_ref(host(x16[i]), host(gs[i]), host(bs[i]), host(dy16[i]))
        assert rel(y[i], yr) < BF16_TOL, ("y", i, rel(y[i], yr))
        assert rel(mean[i], mr) < F32_TOL, ("mean", i, rel(mean[i], mr))
        assert rel(rstd[i], rr) < F32_TOL, ("rstd", i, rel(rstd[i], rr))
        assert rel(dx[i], dxr) < BF16_TOL, ("dx", i, rel(dx[i], dxr))
        tol = dg_tol[i] if dg_tol else F32_TOL
        assert rel(dg[i], dgr + dg0[i]) < tol, ("dgamma", i, rel(dg[i], dgr + dg0[i]))
        assert rel(db[i], dbr + db0[i]) < F32_TOL, ("dbeta", i, rel(db[i], dbr + db0[i]))


def ln_inputs(d, rows, seed):
    xs = [rnd(r, d, seed=seed + 10 * i) * 2 + 0.5 for i, r in enumerate(rows)]
    gs = [rnd(d, seed=seed + 10 * i + 1) * 0.5 + 1 for i in range(len(rows))]
    bs = [rnd(d, seed=seed + 10 * i + 2) * 0.5 for i in range(len(rows))]
    dys = [rnd(r, d, seed=seed + 10 * i + 3) for i, r in enumerate(rows)]
    return xs, gs, bs, dys


# just above 4096 rows (1025 row blocks > 1024); MMF_LN_MAX_PROBLEMS very unequal problems (the 1-row one gets one
# workgroup); above 20000 rows (the 2048-workgroup budget)
LANE_ROWS = [[4100], [8192, 480, 3, 1, 77, 1000, 5, 64], [20000, 37]]


@pytest.mark.parametrize("rows", LANE_ROWS, ids=["4100", "8x_unequal", "20037"])
@pytest.mark.parametrize("d", LANE_D)
def test_layernorm_lane_form(d, rows):
    assert ln_expected_form(d, rows, True) == lane_id(d)
    xs, gs, bs, dys = ln_inputs(d, rows, seed=d)
    run_ln(d, xs, gs, bs, dys, share_first=len(rows) > 1)


@pytest.mark.parametrize("d,rows", [(256, [1000, 7]), (512, [4096]), (768, [333, 1, 64]), (1024, [2000, 2000]),
                                    (8, [130, 3]), (72, [513]), (520, [77, 1]), (1032, [64, 65]), (1536, [33]),
                                    (2040, [9, 70]), (2048, [5, 128])])
def test_layernorm_chunk_form(d, rows):
    """below the forward's lane threshold (the lane d values), and NCH 1-4 with a partial last chunk (8, 72, 520, 1032, 2040)"""
    assert ln_expected_form(d, rows, True) == (d + 511) // 512
    xs, gs, bs, dys = ln_inputs(d, rows, seed=7 * d)
    run_ln(d, xs, gs, bs, dys, share_first=len(rows) > 1)


@pytest.mark.parametrize("d,rows0", [(768, 4000), (768, 20000), (520, 300)], ids=["lane", "lane_budget2048", "chunk"])
def test_layernorm_hard_rows(d, rows0):
    """three problems of one launch: rows 1000 + N(0, 1) (a one-pass E[x^2] - mean^2 variance loses them), constant rows
    (rstd = 1/sqrt(eps)), and a gamma with zeros and negative entries"""
    rows = [rows0, 64, 200]
    assert (ln_expected_form(d, rows, True) > 100) == (d in LANE_D)
    xs = [rnd(rows[0], d, seed=1) + 1000, torch.full((rows[1], d), 3.0), rnd(rows[2], d, seed=2) * 3 - 1]
    gs = [rnd(d, seed=3) * 0.1 + 1, rnd(d, seed=4) * 0.1 + 1, rnd(d, seed=5)]
    gs[2][::7] = 0
    gs[2][1::5] = -gs[2][1::5].abs()
    bs = [rnd(d, seed=6 + i) for i in range(3)]
    dys = [rnd(r, d, seed=10 + i) for i, r in enumerate(rows)]
    # the offset problem: its f32 mean is rounded at ulp(1000) / 2 = 3e-5, which moves every x hat by ~4e-5 — summed over
    # the rows into dgamma that is up to ~1e-4 of its scale; the other outputs are held to the usual bounds
    run_ln(d, xs, gs, bs, dys, dg_tol=[2e-4, F32_TOL, F32_TOL])


# ---------------------------------------------------------------------------------------- skinny dgrad
def expected_strip(Ks):
    wide = sum((k + 63) // 64 for k in Ks)
    return 4 if wide >= 128 else 2 if wide >= 48 else 1


# (N = reduction, W rows; K = dx columns): K a multiple of 8 but not of 16 ct; N not a multiple of 16
STRIP_SHAPES = {1: (72, 1000), 2: (520, 3080), 4: (1000, 8200)}


@pytest.mark.parametrize("M", [1, 64])
@pytest.mark.parametrize("ct", [1, 2, 4])
def test_skinny_dgrad_strip_forms(ct, M):
    """dx = (dy W) [* (aux > 0) * alpha], f32 and bf16 output, every operand row-strided (ld > extent)"""
    N, K = STRIP_SHAPES[ct]
    assert expected_strip([K]) == ct and K % 8 == 0 and K % (16 * ct) and N % 16
    L = lib.load()
    dyb = bf(rnd(M, N + 24, seed=1))
    wb = bf(rnd(N, K + 8, seed=2, scale=N ** -0.5))
    auxb = bf(rnd(M, K + 16, seed=3))
    dy, w, aux = dyb[:, 8:8 + N], wb[:, :K], auxb[:, 16:16 + K]
    dref = host(dy) @ host(w)
    mask = (host(aux) > 0).double()
    for out_dt, tol in ((torch.float32, F32_TOL), (torch.bfloat16, BF16_TOL)):
        for flags, alpha, ref in ((0, 1.0, dref), (EPI_MASK_AUX, 1.25, dref * mask * 1.25)):
            ybuf = nan_like((M, K + 16), out_dt)
            y = ybuf[:, 8:8 + K]
            p = lib.SkinnyProblem(dy.data_ptr(), w.data_ptr(), y.data_ptr(), None, aux.data_ptr(), M, N, K, dyb.stride(0),
                                  wb.stride(0), ybuf.stride(0), auxb.stride(0))
            lib.skinny_dgrad([p], flags, alpha, out_dt == torch.float32)
            assert L.mmf_skinny_last_strip() == ct
            torch.cuda.synchronize()
            assert rel(y, ref) < tol, (out_dt, flags, rel(y, ref))
            assert torch.isnan(ybuf[:, :8]).all() and torch.isnan(ybuf[:, 8 + K:]).all()     # nothing written beside dx


def test_skinny_dgrad_wide_strip_from_many_narrow_problems():
    """ct = 4 reached by a launch of MMF_SKINNY_MAX_PROBLEMS narrow problems (6 strips each, the last one partial), dy / dx as
    column slices of two shared buffers, W row-strided, M from 1 to 64"""
    L = lib.load()
    n = lib.SKINNY_MAX_PROBLEMS
    Ns = [40 + 8 * (i % 9) for i in range(n)]
    Ms = [1 + (i * 37) % 64 for i in range(n)]
    Ms[0], Ms[1] = 1, 64
    K = 360
    assert expected_strip([K] * n) == 4
    dyb = bf(rnd(64, sum(Ns) + 8, seed=4))
    ws = [bf(rnd(Ns[i], K + 24, seed=100 + i, scale=0.2)) for i in range(n)]
    ybuf = nan_like((64, n * (K + 8)))
    probs, offs = [], []
    off = 0
    for i in range(n):
        dy = dyb[:Ms[i], off:off + Ns[i]]
        y = ybuf[:Ms[i], i * (K + 8):i * (K + 8) + K]
        probs.append(lib.SkinnyProblem(dy.data_ptr(), ws[i].data_ptr(), y.data_ptr(), None, None, Ms[i], Ns[i], K,
                                       dyb.stride(0), ws[i].stride(0), ybuf.stride(0), 0))
        offs.append(off)
        off += Ns[i]
    lib.skinny_dgrad(probs, 0, 1.0, True)
    assert L.mmf_skinny_last_strip() == 4
    torch.cuda.synchronize()
    for i in range(n):
        ref = host(dyb[:Ms[i], offs[i]:offs[i] + Ns[i]]) @ host(ws[i][:, :K])
        y = ybuf[:Ms[i], i * (K + 8):i * (K + 8) + K]
        assert rel(y, ref) < F32_TOL, (i, rel(y, ref))
        assert torch.isnan(ybuf[Ms[i]:, i * (K + 8):(i + 1) * (K + 8)]).all()
        assert torch.isnan(ybuf[:, i * (K + 8) + K:(i + 1) * (K + 8)]).all()


def drop_scale(p):
    thresh = min(int(p * 4294967296.0), 4294967295)
    return float(np.float32(1) / (np.float32(1) - np.float32(thresh) * np.float32(1 / 4294967296)))


@pytest.mark.parametrize("in_f32", [False, True])
def test_skinny_dgrad_ex_wide_strip_gate_and_dropout(in_f32):
    """mmf_skinny_linear_dgrad_ex at ct = 4: dz = dy * (gate > 0) * gate_scale * keep / (1 - p) formed while dy is loaded
    (dy and gate f32 or bf16), written out as bf16 by the first strip, and dx = dz W * (aux > 0) * alpha.  The keep mask is
    read off a forward_ex launch with the same rng state, site and problem index whose output has no zero but a dropped one"""
    M, N, K, p, site, gscale = 48, 1000, 8200, 0.25, 5, 0.5
    L = lib.load()
    ops.seed_dropout(77)
    st = ops.rng_state()
    # the mask: y = x W0^T + 100, f32 out, so an element is 0 exactly when it was dropped
    x0, w0 = bf(rnd(M, 64, seed=1, scale=0.1)), bf(rnd(N, 64, seed=2, scale=0.1))
    b0 = torch.full((N,), 100.0, device=DEV)
    y0 = nan_like((M, N))
    ex = lib.SkinnyExtra(0, 0, 1.0, p, st.data_ptr(), site, 0)
    pf = lib.SkinnyProblemEx(lib.SkinnyProblem(x0.data_ptr(), w0.data_ptr(), y0.data_ptr(), b0.data_ptr(), None, M, N, 64,
                                               64, 64, N, 0), None, None, None, 0, 0, 0, 0)
    lib.skinny_fwd_ex([pf], EPI_BIAS | EPI_DROPOUT, True, ex)
    torch.cuda.synchronize()
    keep = (host(y0) != 0).double()
    assert abs(float(keep.mean()) - (1 - p)) < 0.01
    # the dgrad
    dt = torch.float32 if in_f32 else torch.bfloat16
    dyb = rnd(M, N + 8, seed=3).to(dt).to(DEV)
    gateb = torch.relu(rnd(M, N + 16, seed=4)).to(dt).to(DEV)
    dy, gate = dyb[:, :N], gateb[:, 16:]
    w = bf(rnd(N, K, seed=5, scale=N ** -0.5))
    aux = bf(rnd(M, K, seed=6))
    dzb = nan_like((M, N + 8), torch.bfloat16)
    dx = nan_like((M, K))
    pd = lib.SkinnyProblemEx(lib.SkinnyProblem(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), None, aux.data_ptr(), M, N, K,
                                               dyb.stride(0), K, K, K),
                             None, gate.data_ptr(), dzb.data_ptr(), 0, gateb.stride(0), dzb.stride(0), 0)
    ex = lib.SkinnyExtra(int(in_f32), int(in_f32), gscale, p, st.data_ptr(), site, 0)
    lib.skinny_dgrad_ex([pd], EPI_DROPOUT | EPI_MASK_AUX, 2.0, True, ex)
    assert L.mmf_skinny_last_strip() == 4
    torch.cuda.synchronize()
    dz_ref = host(dy) * (host(gate) > 0).double() * gscale * keep * drop_scale(p)
    dz = dzb[:, :N]
    assert rel(dz, dz_ref) < BF16_TOL, rel(dz, dz_ref)
    assert torch.isnan(dzb[:, N:]).all()
    dx_ref = host(dz) @ host(w) * (host(aux) > 0).double() * 2.0          # the MFMA operand is the bf16 dz checked above
    assert rel(dx, dx_ref) < F32_TOL, rel(dx, dx_ref)


# ---------------------------------------------------------------------------------------- fp32 parity mode
def f32_gemm_ref(layout, A, Bm):
    A, Bm = host(A), host(Bm)
    return {GEMM_NT: lambda: A @ Bm.t(), GEMM_NN: lambda: A @ Bm, GEMM_TN: lambda: A.t() @ Bm}[layout]()


def col_slice(rows, cols, seed, scale=1.0, off=3, pad=5):
    """an f32 device operand that is a column slice of a wider buffer (odd offset, ld = cols + pad)"""
    buf = f32(rnd(rows, cols + pad, seed=seed, scale=scale))
    return buf[:, off:off + cols]


def f32_operands(layout, M, N, K, seed):
    a_shape = (K, M) if layout == GEMM_TN else (M, K)
    b_shape = (N, K) if layout == GEMM_NT else (K, N)
    return col_slice(*a_shape, seed=seed), col_slice(*b_shape, seed=seed + 1, scale=K ** -0.5)


@pytest.mark.parametrize("M,N,K", [(200, 136, 1), (130, 257, 31), (129, 100, 33), (300, 200, 3000), (7, 5, 64)])
@pytest.mark.parametrize("layout", [GEMM_NT, GEMM_NN, GEMM_TN], ids=["NT", "NN", "TN"])
def test_gemm_f32_layouts_and_epilogues(layout, M, N, K):
    from mmfusion import ops_f32
    A, Bm = f32_operands(layout, M, N, K, seed=M + N + K)
    ref = f32_gemm_ref(layout, A, Bm)
    bias = f32(rnd(N, seed=11))
    aux = col_slice(M, N, seed=12)
    auxh, biash = host(aux), host(bias)
    c_old = rnd(M, N, seed=13).float().double()
    cases = [(0, 1.0, ref), (EPI_BIAS, 1.0, ref + biash), (EPI_BIAS | EPI_RELU, 1.0, torch.relu(ref + biash)),
             (EPI_ADD_AUX, 1.0, ref + auxh), (EPI_MASK_AUX, 0.75, ref * (auxh > 0) * 0.75),
             (EPI_ACCUM, 1.0, ref + c_old), (EPI_ACCUM, -0.5, -0.5 * ref + c_old)]
    for epi, alpha, want in cases:
        Cbuf = nan_like((M, N + 6))
        Cm = Cbuf[:, 2:2 + N]
        if epi & EPI_ACCUM:
            Cm.copy_(c_old)
        ops_f32.gemm(layout, A, Bm, Cm, bias=bias if epi & EPI_BIAS else None,
                     aux=aux if epi & (EPI_ADD_AUX | EPI_MASK_AUX) else None, epilogue=epi, alpha=alpha)
        torch.cuda.synchronize()
        assert rel(Cm, want) < F32_TOL, (epi, alpha, rel(Cm, want))
        assert torch.isnan(Cbuf[:, :2]).all() and torch.isnan(Cbuf[:, 2 + N:]).all()
    if layout == GEMM_TN:                        # wgrad + bias gradient: bias[m] += sum_k A[k][m]
        Cm = nan_like((M, N))
        db0 = rnd(M, seed=14).float().double()
        db = f32(db0)
        ops_f32.gemm(layout, A, Bm, Cm, bias=db, epilogue=EPI_COLSUM_A)
        torch.cuda.synchronize()
        assert rel(Cm, ref) < F32_TOL
        assert rel(db, host(A).sum(0) + db0) < F32_TOL


# ---------------------------------------------------------------------------------------- gemm6: every stage form
# The one-wave-per-SIMD kernel's stage body is instantiated per role (csrc/gemm6.hip, `stage`): the lone stage of a one-step
# sweep, a sweep's first stage, the steady loop (both refills, no condition), the stages around it with the ring running dry, and
# the last.  At 32 k-columns per stage, K = 32 is the lone stage, 64 and 128 never reach the steady loop (2 and 4 steps: the ring of
# four stages is filled once and runs dry), 160 enters it exactly once and 320 runs it six times; TN's K = 72 leaves a
# zero-filled tail in its third stage.  300 x 264 (TN: 296, its m extent is the operands' contiguous one: a multiple of 8) is two
# tiles each way with a boundary tile in M and in N.
G6_CASES = [(lay, K) for lay in (GEMM_NT, GEMM_NN, GEMM_TN) for K in (32, 64, 128, 160, 320)] + [(GEMM_TN, 72)]


@pytest.mark.parametrize("layout,K", G6_CASES, ids=[f"{'NT NN TN'.split()[lay]}-K{K}" for lay, K in G6_CASES])
def test_gemm6_stage_forms(layout, K):
    """generation 6 pinned, both output types (all six kernels of gemm6.hip), every output pre-filled with NaN; TN also with the
    fused bias gradient, whose extra MFMAs ride in every stage form"""
    L = lib.load()
    M, N = (296 if layout == GEMM_TN else 300), 264
    a16 = bf(rnd(*((K, M) if layout == GEMM_TN else (M, K)), seed=600 + K))
    b16 = bf(rnd(*((N, K) if layout == GEMM_NT else (K, N)), seed=700 + K, scale=K ** -0.5))
    ref = f32_gemm_ref(layout, a16, b16)
    lib.check(L.mmf_gemm_select_impl(6))
    try:
        c32, c16 = nan_like((M, N)), nan_like((M, N), torch.bfloat16)
        ops.gemm(layout, a16, b16, c32)
        assert L.mmf_gemm_last_impl() == 6
        ops.gemm(layout, a16, b16, c16)
        assert L.mmf_gemm_last_impl() == 6
        assert rel(c32, ref) < F32_TOL, rel(c32, ref)
        assert rel(c16, ref) < BF16_TOL, rel(c16, ref)
        if layout == GEMM_TN:
            db0 = rnd(M, seed=800 + K).float().double()
            db, cw = f32(db0), nan_like((M, N))
            ops.gemm(layout, a16, b16, cw, bias=db, epilogue=EPI_COLSUM_A)
            assert L.mmf_gemm_last_impl() == 6
            assert rel(cw, ref) < F32_TOL, rel(cw, ref)
            assert rel(db, host(a16).sum(0) + db0) < F32_TOL, rel(db, host(a16).sum(0) + db0)
    finally:
        lib.check(L.mmf_gemm_select_impl(0))


def test_gemm_f32_max_problem_count():
    """MMF_GEMM_MAX_PROBLEMS problems of ragged shapes in one launch (NT, bias + ReLU)"""
    L = lib.load()
    n = lib.GEMM_MAX_PROBLEMS
    probs, refs, outs = [], [], []
    for i in range(n):
        M, N, K = 1 + (i * 53) % 200, 1 + (i * 29) % 150, 1 + (i * 71) % 300
        A, Bm = f32_operands(GEMM_NT, M, N, K, seed=200 + 2 * i)
        bias = f32(rnd(N, seed=300 + i))
        Cm = nan_like((M, N))
        probs.append(lib.GemmProblem(A.data_ptr(), Bm.data_ptr(), Cm.data_ptr(), bias.data_ptr(), None, M, N, K, A.stride(0),
                                     Bm.stride(0), N, 0))
        refs.append(torch.relu(f32_gemm_ref(GEMM_NT, A, Bm) + host(bias)))
        outs.append((Cm, A, Bm, bias))
    arr = (lib.GemmProblem * n)(*probs)
    lib.check(L.mmf_gemm_f32_grouped(arr, n, GEMM_NT, EPI_BIAS | EPI_RELU, 1.0, lib.stream_ptr()))
    torch.cuda.synchronize()
    for i in range(n):
        assert rel(outs[i][0], refs[i]) < F32_TOL, (i, rel(outs[i][0], refs[i]))


def test_gemm_f32_batched_as_explicit_attention_calls_it():
    """S = Q K^T, O = P V, dV = P^T dO over a (batch, head) grid: operands are head column groups of (B, T, H dh) buffers
    (both batch axes strided), scores a dense (B, H, Tq, Tk) buffer; alpha on S, ACCUM on dV"""
    B, H, dh, Tq, Tk = 3, 4, 48, 70, 130
    d = H * dh
    L = lib.load()
    S2 = C.c_int64 * 2
    q, k, v, do = (f32(rnd(B, T, d, seed=s)) for s, T in ((1, Tq), (2, Tk), (3, Tk), (4, Tq)))
    qh, kh, vh, doh = (host(t).view(B, -1, H, dh).transpose(1, 2) for t in (q, k, v, do))

    def batched(layout, A, sA, lda, Bm, sB, ldb, Cm, sC, ldc, M, N, K, epi=0, alpha=1.0):
        p = lib.GemmProblem(A.data_ptr(), Bm.data_ptr(), Cm.data_ptr(), None, None, M, N, K, lda, ldb, ldc, 0)
        lib.check(L.mmf_gemm_f32_batched(C.byref(p), layout, epi, alpha, B, H, S2(*sA), S2(*sB), S2(*sC), lib.stream_ptr()))

    scale = dh ** -0.5
    S = nan_like((B, H, Tq, Tk))
    batched(GEMM_NT, q, (Tq * d, dh), d, k, (Tk * d, dh), d, S, (H * Tq * Tk, Tq * Tk), Tk, Tq, Tk, dh, alpha=scale)
    torch.cuda.synchronize()
    assert rel(S, qh @ kh.transpose(-1, -2) * scale) < F32_TOL
    P = torch.softmax(S, -1)
    O = nan_like((B, Tq, d))
    batched(GEMM_NN, P, (H * Tq * Tk, Tq * Tk), Tk, v, (Tk * d, dh), d, O, (Tq * d, dh), d, Tq, dh, Tk)
    torch.cuda.synchronize()
    assert rel(O, (host(P) @ vh).transpose(1, 2).reshape(B, Tq, d)) < F32_TOL
    dv0 = rnd(B, Tk, d, seed=5).float().double()
    dV = f32(dv0)
    batched(GEMM_TN, P, (H * Tq * Tk, Tq * Tk), Tk, do, (Tq * d, dh), d, dV, (Tk * d, dh), d, Tk, dh, Tq, epi=EPI_ACCUM)
    torch.cuda.synchronize()
    assert rel(dV, (host(P).transpose(-1, -2) @ doh).transpose(1, 2).reshape(B, Tk, d) + dv0) < F32_TOL


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 1000])
def test_softmax_rows_f32_and_backward(cols):
    """rows = 37 (not a multiple of the 4 rows per workgroup), scale 1 / sqrt(96) on N(0, 1) rows, and scale 1 / 2 on rows
    whose entries spread over 80+ around +-400 (exp overflows / underflows without the max subtraction); a sentinel row after
    the last stays NaN"""
    L = lib.load()
    rows = 37
    base = rnd(rows, cols, seed=cols)
    wild = rnd(rows, cols, seed=cols + 1) * 40 + torch.where(torch.arange(rows) % 2 == 0, 400.0, -400.0)[:, None]
    for x, scale in ((base, 96 ** -0.5), (wild, 0.5)):
        buf = nan_like((rows + 1, cols))
        buf[:rows] = f32(x)
        lib.check(L.mmf_softmax_rows_f32(buf.data_ptr(), rows, cols, scale, lib.stream_ptr()))
        torch.cuda.synchronize()
        Pref = torch.softmax(x.float().double() * scale, -1)
        assert rel(buf[:rows], Pref) < F32_TOL, (scale, rel(buf[:rows], Pref))
        assert torch.isnan(buf[rows]).all()
        P = buf[:rows].clone()
        g = rnd(rows, cols, seed=cols + 2)
        dbuf = nan_like((rows + 1, cols))
        dbuf[:rows] = f32(g)
        lib.check(L.mmf_softmax_bwd_rows_f32(P.data_ptr(), dbuf.data_ptr(), rows, cols, scale, lib.stream_ptr()))
        torch.cuda.synchronize()
        Ph, gh = host(P), host(f32(g))
        dref = scale * Ph * (gh - (gh * Ph).sum(-1, keepdim=True))
        assert rel(dbuf[:rows], dref) < F32_TOL, (scale, rel(dbuf[:rows], dref))
        assert torch.isnan(dbuf[rows]).all()


@pytest.mark.parametrize("rows,d", [(1, 72), (67, 200), (130, 1000), (63, 1030)])
def test_layernorm_f32_fwd_bwd(rows, d):
    """d not a multiple of 64, rows not a multiple of the backward's 64-row blocks, dgamma / dbeta accumulated into"""
    L = lib.load()
    x = f32(rnd(rows, d, seed=1) * 2 + 0.5)
    g, b = f32(rnd(d, seed=2) * 0.5 + 1), f32(rnd(d, seed=3))
    dy = f32(rnd(rows, d, seed=4))
    y, mean, rstd, dx = nan_like((rows, d)), nan_like((rows,)), nan_like((rows,)), nan_like((rows, d))
    dg0, db0 = rnd(d, seed=5).float().double(), rnd(d, seed=6).float().double()
    dg, db = f32(dg0), f32(db0)
    s = lib.stream_ptr()
    lib.check(L.mmf_layernorm_f32_fwd(x.data_ptr(), y.data_ptr(), g.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                      rows, d, EPS, s))
    lib.check(L.mmf_layernorm_f32_bwd(x.data_ptr(), dy.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                      dg.data_ptr(), db.data_ptr(), rows, d, s))
    torch.cuda.synchronize()
    yr, mr, rr, dxr, dgr, dbr = ln_ref(host(x), host(g), host(b), host(dy))
    for name, got, want in (("y", y, yr), ("mean", mean, mr), ("rstd", rstd, rr), ("dx", dx, dxr), ("dgamma", dg, dgr + dg0),
                            ("dbeta", db, dbr + db0)):
        assert rel(got, want) < F32_TOL, (name, rel(got, want))


# ---------------------------------------------------------------------------------------- fused loss, modality dropout
LOSS_VARIANTS = [(0.0, 0, 0.0), (0.1, 3, 50.0), (0.1, 8, -50.0), (0.0, 8, 0.0)]       # (smoothing, n_extra, logit shift)


def loss_inputs(B, Cn, shift, seed):
    spread = 30.0 if shift else 3.0
    wide = rnd(B, Cn + 5, seed=seed) * spread + shift
    t = torch.randint(0, Cn, (B,), generator=torch.Generator().manual_seed(seed))
    if B == 1:
        t[0] = (0, Cn - 1)[seed % 2]
    else:
        t[0], t[-1] = 0, Cn - 1
    return wide, t


@pytest.mark.parametrize("Cn", [2, 7, 64])
@pytest.mark.parametrize("B", [1, 7, 255, 256, 257, 1000])
def test_fusion_loss_value_and_logit_gradient(B, Cn):
    """mmf_fusion_loss with the logits a column slice (ldl = C + 5) against float64 F.cross_entropy(label_smoothing) plus the
    weighted extra terms; small_ops.fusion_loss (the autograd path) must give the same value and gradient"""
    L = lib.load()
    for vi, (eps, n_extra, shift) in enumerate(LOSS_VARIANTS):
        wide_h, t = loss_inputs(B, Cn, shift, seed=B * 100 + Cn * 7 + vi)
        wide = f32(wide_h)
        logits = wide[:, 2:2 + Cn]
        tt = t.to(DEV)
        extras = [f32(rnd(1, seed=500 + j)) for j in range(n_extra)]
        ws = [0.1 * (j + 1) * (-1) ** j for j in range(n_extra)]
        loss, dlog = nan_like((1,)), nan_like((B, Cn))
        pe = (C.c_void_p * max(n_extra, 1))(*[e.data_ptr() for e in extras])
        pw = (C.c_float * max(n_extra, 1))(*ws)
        lib.check(L.mmf_fusion_loss(logits.data_ptr(), wide.stride(0), tt.data_ptr(), B, Cn, eps, pe, pw, n_extra,
                                    loss.data_ptr(), dlog.data_ptr(), lib.stream_ptr()))
        torch.cuda.synchronize()
        lr = host(logits).requires_grad_(True)
        ref = F.cross_entropy(lr, t, label_smoothing=eps)
        ref.backward()
        ref_total = float(ref.detach()) + sum(w * float(e) for w, e in zip(ws, extras))
        got = float(loss[0])
        assert abs(got - ref_total) <= F32_TOL * max(1.0, abs(ref_total)), (vi, got, ref_total)
        assert rel(dlog, lr.grad) < F32_TOL, (vi, rel(dlog, lr.grad))
        # the autograd wrapper: same launch, its gradient lands in the slice's columns of the wide leaf
        leaf = wide.clone().requires_grad_(True)
        lo = small_ops.fusion_loss(leaf[:, 2:2 + Cn], tt, eps, extras, ws)
        lo.backward()
        assert float(lo) == got
        assert torch.equal(leaf.grad[:, 2:2 + Cn], dlog)
        assert not leaf.grad[:, :2].any() and not leaf.grad[:, 2 + Cn:].any()


def test_fusion_loss_host_checks():
    logits = torch.zeros((4, 65), device=DEV)
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="C=65"):
        small_ops.fusion_loss(logits, t, 0.0, [], [])
    with pytest.raises(RuntimeError, match="label_smoothing"):
        small_ops.fusion_loss(logits[:, :64], t, 1.0, [], [])


@pytest.mark.parametrize("B,d", [(5, 4), (33, 2052)])
def test_modality_dropout_apply_and_draw(B, d):
    """draw = 0 (the backward) applies the given keep masks exactly, an all-zero mask row included; draw = 1 writes 0 / 1
    masks with at least one modality kept per sample and applies them exactly"""
    L = lib.load()
    xs = [f32(rnd(B, d, seed=i)) for i in range(3)]
    keep_h = (rnd(B, 3, seed=9) > 0).float()
    keep_h[0] = 0
    keep_h[-1] = 1
    keep = keep_h.to(DEV)
    ys = [nan_like((B, d)) for _ in range(3)]
    P3 = C.c_void_p * 3
    lib.check(L.mmf_modality_dropout(P3(*[x.data_ptr() for x in xs]), P3(*[y.data_ptr() for y in ys]), keep.data_ptr(), B, d,
                                     0.0, None, 0, 0, lib.stream_ptr()))
    torch.cuda.synchronize()
    for m in range(3):
        assert torch.equal(ys[m], xs[m] * keep[:, m:m + 1]), m
    assert torch.equal(keep.cpu(), keep_h)                       # the apply path leaves the masks alone
    ops.seed_dropout(31)
    kd = nan_like((B, 3))
    ys = [nan_like((B, d)) for _ in range(3)]
    lib.check(L.mmf_modality_dropout(P3(*[x.data_ptr() for x in xs]), P3(*[y.data_ptr() for y in ys]), kd.data_ptr(), B, d,
                                     0.6, ops.rng_state().data_ptr(), 3, 1, lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool(((kd == 0) | (kd == 1)).all()) and bool((kd.sum(1) >= 1).all())
    for m in range(3):
        assert torch.equal(ys[m], xs[m] * kd[:, m:m + 1]), m
