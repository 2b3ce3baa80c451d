"""GPU: layer 0 of the base Wav2Vec2 family (csrc/wav2vec2.hip), ``mmf_w2v_conv0_norm_gelu`` element by element and
``mmf_w2v_conv0_stats`` at the shapes tests/test_w2v_gpu.py leaves out.

``mmf_w2v_conv0_norm_gelu``: the checker of tests/test_w2v_ln_gpu.py, unchanged (one bf16 ulp of the float64 value outside the
cancelling set |y| < 2^-12 terms; inside it that file's caps on size and count), with terms = |gamma| rstd (sum|w x| + |mean|) + |beta|.
The TEST supplies the statistics, float64 values rounded to f32, so a failure names this kernel and not the statistics pass.  CASES
reaches: 16 idle threads per workgroup (C0 = 192), one frame per workgroup pass (C0 = 2048), the 16-tap instantiation (k0 = 12), the
next layer's (k1, s1) = (3, 2), (2, 2) and (1, 1), T0 = 1 and 2, and the 1024-workgroup cap above which a workgroup walks strided
frames (C0 = 2048 at L = 5200: 1039 frames, one per workgroup; C0 = 512 at L = 20600: 4119 frames, four per workgroup).  Where
(T0 - k1) % s1 != 0 there are frames past s1 (T1 - 1) + k1 - 1, which must not be stored: the NaN guard behind the output stays NaN.
tests/test_w2v_kernel_checks_cpu.py checks with the float64 reference alone that every case keeps its cancelling set within the cap.

``mmf_w2v_conv0_stats``: tests/test_w2v_gpu.py's 1e-4 rule at k0 = 12 and at T0 = 1, 2, 3; at T0 = 1 the variance is exactly 0 and the
mean is the frame; two runs are bit-equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import w2v_kernel_checks as K  # noqa: E402
import w2v_ref  # noqa: E402
from helpers import _lib  # noqa: E402
from test_w2v_ln_gpu import EPS, _affine, _check, _out  # noqa: E402

EPS32 = float(torch.tensor(EPS, dtype=torch.float32))         # the eps the kernel adds: its argument is a float
# (N, L, C0, k0, s0, k1, s1, affine): affine "spread" = gamma about 1, beta about 0; "tail" = every y in the left tail (beta = -5);
# "one" = beta about 1, for the clips of one frame, whose y IS beta (the frame is its own mean)
CASES = [
    (2, 10, 64, 10, 5, 1, 1, "one"),                      # T0 = 1 (L == k0)
    (2, 12, 8, 12, 5, 1, 1, "one"),                       # T0 = 1, the 16-tap form, one lane per frame
    (2, 15, 8, 10, 5, 2, 2, "spread"),                    # T0 = 2
    (2, 1237, 192, 10, 5, 3, 2, "spread"),                # T0 = 246: cgn = 24, 16 idle threads; frame 245 is not stored
    (2, 1242, 64, 12, 5, 2, 2, "spread"),                 # T0 = 247, the 16-tap form; frame 246 is not stored
    (3, 1237, 8, 10, 5, 1, 1, "spread"),                  # every frame stored once
    (2, 5200, 2048, 10, 5, 2, 2, "spread"),               # T0 = 1039 > 1024 workgroups of one frame; frame 1038 is not stored
    (2, 20600, 512, 10, 5, 3, 2, "spread"),               # T0 = 4119 > 1024 workgroups of four frames
    (2, 2000, 512, 10, 5, 3, 2, "tail"),                  # nothing cancels: the bare one-ulp rule throughout
]
IDS = [f"L{c[1]}-C{c[2]}-k0_{c[3]}-k1_{c[5]}-s1_{c[6]}-{c[7]}" for c in CASES]


def conv0_case(N, L, C0, k0, s0, k1, s1, affine):
    """the operands of a case and its float64 expectation (CPU only: tests/test_w2v_kernel_checks_cpu.py builds it too)"""
    g = torch.Generator().manual_seed(L + C0 + k0)
    wave = 0.5 * torch.randn(N, L, generator=g) + 0.5
    w = 0.4 * torch.randn(C0, 1, k0, generator=g)
    gamma, beta = _affine(C0, g, affine == "tail")
    if affine == "one":
        beta = beta + 1.0
    mean, var = w2v_ref.conv0_stats(w2v_ref.conv0_raw(wave.double(), w.double(), s0))
    stats = torch.cat([mean, var], dim=1).float()                                        # (N, 2, C0): what the kernel is given
    want, y, terms = K.conv0_expect(wave, w, stats[:, 0:1], stats[:, 1:2], gamma, beta, s0, k1, s1, EPS32)
    return dict(wave=wave, w=w, gamma=gamma, beta=beta, stats=stats, want=want, y=y, terms=terms)


@pytest.mark.parametrize("N,L,C0,k0,s0,k1,s1,affine", CASES, ids=IDS)
def test_conv0_norm_gelu_per_element(N, L, C0, k0, s0, k1, s1, affine):
    lib, c = _lib(), conv0_case(N, L, C0, k0, s0, k1, s1, affine)
    ins = [c[n].cuda() for n in ("wave", "w", "stats", "gamma", "beta")]
    before = [K.bits(t).clone() for t in ins]
    buf = _out(c["want"].numel())
    lib.w2v_conv0_norm_gelu(*ins, buf, k0, s0, k1, s1, EPS)
    torch.cuda.synchronize()
    assert all(torch.equal(K.bits(t), b) for t, b in zip(ins, before)), "an input was changed"
    T0 = (L - k0) // s0 + 1
    _check(f"PARITY conv0_norm_gelu N={N} L={L} (T0={T0}) C0={C0} k0={k0} k1={k1} s1={s1} {affine}", buf, c["want"], c["y"], c["terms"],
           affine == "tail")


@pytest.mark.parametrize("N,L,C0,k0", [(2, 1242, 64, 12), (2, 10, 64, 10), (2, 12, 8, 12), (2, 15, 8, 10), (2, 20, 8, 10), (2, 22, 64, 12)],
                         ids=["T0_247-k0_12", "T0_1", "T0_1-k0_12", "T0_2", "T0_3", "T0_3-k0_12"])
def test_conv0_stats_short_clips_and_sixteen_taps(N, L, C0, k0):
    lib = _lib()
    g = torch.Generator().manual_seed(L + C0)
    wave = 0.5 * torch.randn(N, L, generator=g) + 0.5
    w = 0.4 * torch.randn(C0, 1, k0, generator=g)
    raw = w2v_ref.conv0_raw(wave.double(), w.double(), 5)
    T0 = raw.shape[1]
    mean, var = w2v_ref.conv0_stats(raw)
    runs = []
    for _ in range(2):
        stats = torch.full((N * 2 * C0 + 4096,), float("nan"), device="cuda")
        partial = torch.full((N * lib.W2V_STATS_SLOTS * 2 * C0,), float("nan"), device="cuda")
        lib.w2v_conv0_stats(wave.cuda(), w.cuda(), stats, partial, k0, 5)
        torch.cuda.synchronize()
        assert bool(torch.isnan(stats[N * 2 * C0:]).all()), "the guard behind the statistics was written"
        runs.append(stats[:N * 2 * C0].view(N, 2, C0).cpu())
    assert torch.equal(K.bits(runs[0]), K.bits(runs[1])), "two runs differ"
    got = runs[0].double()
    std = var.sqrt()
    e_mean = float(((got[:, 0:1] - mean).abs() / (mean.abs() + std)).max())
    big = mean.abs() > std
    e_rel = float(((got[:, 0:1] - mean).abs() / mean.abs())[big].max()) if bool(big.any()) else 0.0
    if T0 == 1:
        assert bool((got[:, 1:2] == 0).all()), "one frame: the variance is exactly 0"
        e_var = 0.0
    else:
        e_var = float(((got[:, 1:2] - var).abs() / var).max())
    print(f"PARITY conv0_stats N={N} L={L} (T0={T0}) C0={C0} k0={k0}: mean err / (|mean| + std) {e_mean:.2e}, on the {int(big.sum())} channels "
          f"with |mean| > std relative to |mean| {e_rel:.2e}, variance rel err {e_var:.2e} (bound 1e-4)")
    assert e_mean <= 1e-4 and e_var <= 1e-4 and e_rel <= 1e-4
