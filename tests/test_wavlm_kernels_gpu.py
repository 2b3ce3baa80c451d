"""GPU: the two WavLM kernels of csrc/wavlm.hip against float64.

``mmf_wavlm_gate`` against ``wavlm_ref.gate_ref``: F32_TOL x max(|ref|, 1), and two runs bit-equal.

``mmf_attn_fwd_relbias`` against ``wavlm_ref.relbias_staged`` (tests/attn_ref.py's staged forward with the bias): a random f32 table
with no bucket structure, so that every offset j - i is distinguishable, gates drawn from [1, 3], B = 2, H = 2, Q / K / V in one
fused (rows, 3 d) buffer.  The bounds are the plain forward's (tests/test_attention_paths_gpu.py): O within BF16_TOL x max|ref| plus
the reference's own sensitivity to scores perturbed by 2^-22; LSE within F32_TOL x max(|ref|, 1).  With an all-zero table the same
bounds hold against the PLAIN attention restatement.  T: one key, a ragged block, exactly one block, one block and a key, one tile,
a tile and a key, a ragged second tile, two query chunks (129 -> 2 x 96 rows: a wave that only stages), a fourth tile (193).
Outputs are pre-filled with NaN; guard rows, guard columns and guard elements must come back bit-identical, as must the inputs."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as R  # noqa: E402
import wavlm_ref  # noqa: E402
from mmfusion import lib  # noqa: E402
from test_attention_paths_gpu import E_ALIGN, E_SHAPE, E_UNSUPPORTED, Mat, Vec, bits, scale_of  # noqa: E402
from test_kernel_forms_gpu import BF16_TOL, DEV, F32_TOL, NAN  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TS = (1, 31, 32, 33, 64, 65, 97, 129, 193)


# ---- mmf_wavlm_gate --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T,H,dh", [(2, 1, 2, 64), (2, 33, 4, 64), (1, 65, 12, 64), (1, 33, 8, 96)])
def test_gate_against_float64_and_bit_repeatable(n, T, H, dh):
    g = torch.Generator().manual_seed(1000 * T + H)
    x = R.bf16r(torch.randn(n * T, H * dh, generator=g, dtype=F64))
    w = R.f32r(0.3 * torch.randn(8, dh, generator=g, dtype=F64))
    b = R.f32r(0.5 * torch.randn(8, generator=g, dtype=F64))
    c = R.f32r(1.0 + torch.randn(H, generator=g, dtype=F64))
    X = Mat(n * T, H * dh, H * dh + 8, 8, x)
    out, again = Vec(n * H * T), Vec(n * H * T)
    dev = lambda t: t.to(F32).to(DEV)
    wd, bd, cd = dev(w), dev(b), dev(c)
    for o in (out, again):
        lib.wavlm_gate(X.v, wd, bd, cd, o.v, n, T, H, dh)
    ref = wavlm_ref.gate_ref(x.reshape(n, T, H, dh), w, b, c).reshape(-1)
    got = out.host()
    bound = F32_TOL * max(float(ref.abs().max()), 1.0)
    err = float((got - ref).abs().max()) if bool(torch.isfinite(got).all()) else math.inf
    print(f"PARITY gate n={n} T={T} H={H} dh={dh}: err / bound {err / bound:.3f}; gate range {float(ref.min()):.2f} .. {float(ref.max()):.2f}")
    assert err <= bound
    assert float(ref.max() - ref.min()) > 0.5                                  # the case exercises the gate
    assert torch.equal(bits(out.buf), bits(again.buf))
    assert out.guards_intact() and X.untouched()


# ---- mmf_attn_fwd_relbias ----------------------------------------------------------------------------------------
class Fused:
    """one self-attention problem read from a fused (B T, 3 d) buffer, with guards around everything"""

    def __init__(self, dh, B, H, T, seed, zero_table=False):
        self.dh, self.B, self.H, self.T = dh, B, H, T
        d = self.d = H * dh
        g = torch.Generator().manual_seed(seed)
        self.qkv = R.bf16r(torch.randn(B, T, 3 * d, generator=g, dtype=F64))
        self.gate = R.f32r(1.0 + 2.0 * torch.rand(B, H, T, generator=g, dtype=F64))
        self.table = R.f32r(torch.zeros(H, 2 * T - 1, dtype=F64) if zero_table else torch.randn(H, 2 * T - 1, generator=g, dtype=F64))
        self.QKV = Mat(B * T, 3 * d, 3 * d + 8, 8, self.qkv)
        self.O, self.LSE = Mat(B * T, d, d + 16, 8), Vec(B * H * T)
        self.G, self.TAB = Vec(B * H * T), Vec(H * (2 * T - 1))
        self.G.v.copy_(self.gate.reshape(-1).to(F32)), self.TAB.v.copy_(self.table.reshape(-1).to(F32))
        self.G.mark(), self.TAB.mark()

    def problem(self, **over):
        d, ld = self.d, 3 * self.d + 8
        f = dict(Q=self.QKV.ptr, K=self.QKV.ptr + 2 * d, V=self.QKV.ptr + 4 * d, O=self.O.ptr, LSE=self.LSE.ptr, B=self.B, H=self.H,
                 Tq=self.T, Tk=self.T, ldq=ld, ldk=ld, ldv=ld, ldo=d + 16)
        f.update(over)
        return lib.AttnProblem(f["Q"], f["K"], f["V"], f["O"], f["LSE"], None, None, None, None, None, f["B"], f["H"], f["Tq"], f["Tk"],
                               f["ldq"], f["ldk"], f["ldv"], f["ldo"])

    def qkv_parts(self):
        d = self.d
        return self.qkv[..., :d], self.qkv[..., d:2 * d], self.qkv[..., 2 * d:]

    def check(self, ref, noisy, tag):
        fails = []
        o, got = ref["o"].reshape(-1, self.d), self.O.host()
        bound = BF16_TOL * float(o.abs().max()) + float((ref["o"] - noisy["o"]).abs().max())
        err = float((got - o).abs().max()) if bool(torch.isfinite(got).all()) else math.inf
        print(f"PARITY {tag} O: err / bound {err / bound:.3f}")
        if not err <= bound:
            bad = (~((got - o).abs() <= bound)).nonzero()
            fails.append(f"{tag} O: err {err:.4g} > bound {bound:.4g}; {len(bad)} elements, first (row, col) {bad[0].tolist()}")
        lse, got = ref["lse"].reshape(-1), self.LSE.host()
        bound = F32_TOL * max(float(lse.abs().max()), 1.0)
        err = float((got - lse).abs().max()) if bool(torch.isfinite(got).all()) else math.inf
        print(f"PARITY {tag} LSE: err / bound {err / bound:.3f}")
        if not err <= bound:
            fails.append(f"{tag} LSE: err {err:.4g} > bound {bound:.4g}, first {int((~((got - lse).abs() <= bound)).nonzero()[0])}")
        if not (self.O.guards_intact() and self.LSE.guards_intact()):
            fails.append(f"{tag}: guards around O / LSE changed")
        if not (self.QKV.untouched() and self.G.untouched() and self.TAB.untouched()):
            fails.append(f"{tag}: an input changed")
        return fails


@pytest.mark.parametrize("dh", [64, 96])
@pytest.mark.parametrize("T", TS)
def test_relbias_forward_against_staged_float64(dh, T):
    c = Fused(dh, 2, 2, T, seed=7 * T + dh)
    scale = scale_of(dh)
    lib.attn_fwd_relbias(c.problem(), dh, scale, c.G.v, c.TAB.v)
    q, k, v = c.qkv_parts()
    ref = wavlm_ref.relbias_staged(q, k, v, c.H, scale, c.gate, c.table)
    noisy = wavlm_ref.relbias_staged(q, k, v, c.H, scale, c.gate, c.table, perturb=R.PERTURB, seed=1)
    plain = R.staged(q, k, v, torch.zeros_like(q), c.H, scale)
    if T > 1:                                                                  # the bias matters in this case
        assert float((ref["o"] - plain["o"]).abs().max()) > 10 * BF16_TOL * float(ref["o"].abs().max())
    fails = c.check(ref, noisy, f"relbias dh={dh} T={T}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dh", [64, 96])
@pytest.mark.parametrize("T", TS)
def test_relbias_forward_with_a_zero_table_is_the_plain_attention(dh, T):
    c = Fused(dh, 2, 2, T, seed=11 * T + dh, zero_table=True)
    scale = scale_of(dh)
    lib.attn_fwd_relbias(c.problem(), dh, scale, c.G.v, c.TAB.v)
    q, k, v = c.qkv_parts()
    z = torch.zeros_like(q)
    ref, noisy = R.staged(q, k, v, z, c.H, scale), R.staged(q, k, v, z, c.H, scale, perturb=R.PERTURB, seed=1)
    fails = c.check(ref, noisy, f"zero table dh={dh} T={T}")
    assert not fails, "\n".join(fails)


def test_refusals_return_the_documented_codes_and_launch_nothing():
    L = lib.load()
    s = lib.stream_ptr()
    c = Fused(64, 2, 2, 40, seed=3)
    gp, tp = c.G.ptr, c.TAB.ptr
    rel = lambda p, dh=64, gate=gp, table=tp: L.mmf_attn_fwd_relbias(p, dh, 0.125, gate, table, s)
    x = torch.zeros(80, 128, dtype=BF16, device=DEV)
    w, b, k = torch.zeros(8, 64, device=DEV), torch.zeros(8, device=DEV), torch.zeros(2, device=DEV)
    gout = Vec(2 * 2 * 40)
    P = lambda t, off=0: t.data_ptr() + off
    gate = lambda xp=P(x), ldx=128, wp=P(w), bp=P(b), kp=P(k), op=gout.ptr, dh=64: L.mmf_wavlm_gate(xp, ldx, wp, bp, kp, op, 2, 40, 2, dh, s)
    ref = lambda **over: __import__("ctypes").byref(c.problem(**over))
    cases = [
        ("mmf_attn_fwd_relbias", lambda: rel(None), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(Q=None)), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(O=None)), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(LSE=None)), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(), gate=None), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(), table=None), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(Tk=39)), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(Tq=41)), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(B=0)), E_SHAPE),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(K=c.QKV.ptr + 2 * c.d + 2)), E_ALIGN),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(ldq=3 * c.d + 4)), E_ALIGN),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(ldo=c.d - 8)), E_ALIGN),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(), gate=gp + 2), E_ALIGN),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(), table=tp + 1), E_ALIGN),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(), dh=128), E_UNSUPPORTED),
        ("mmf_attn_fwd_relbias", lambda: rel(ref(), dh=32), E_UNSUPPORTED),
        ("mmf_wavlm_gate", lambda: gate(xp=None), E_SHAPE),
        ("mmf_wavlm_gate", lambda: gate(wp=None), E_SHAPE),
        ("mmf_wavlm_gate", lambda: gate(op=None), E_SHAPE),
        ("mmf_wavlm_gate", lambda: gate(xp=P(x, 2)), E_ALIGN),
        ("mmf_wavlm_gate", lambda: gate(ldx=120), E_ALIGN),
        ("mmf_wavlm_gate", lambda: gate(ldx=132), E_ALIGN),
        ("mmf_wavlm_gate", lambda: gate(wp=P(w, 4)), E_ALIGN),
        ("mmf_wavlm_gate", lambda: gate(op=gout.ptr + 2), E_ALIGN),
        ("mmf_wavlm_gate", lambda: gate(dh=128), E_UNSUPPORTED),
    ]
    for name, call, want in cases:
        rc = call()
        assert rc == want, (name, rc, want, L.mmf_last_error())
        assert name.encode() in L.mmf_last_error()
    torch.cuda.synchronize()
    assert c.O.untouched() and c.LSE.untouched() and gout.untouched()                 # still NaN: nothing was launched
    assert bool(torch.isnan(c.O.v).all()) and bool(torch.isnan(c.LSE.v).all()) and bool(torch.isnan(gout.v).all())
