"""GPU: the uniform attention backward (lib.attn_bwd_grouped_uniform: one output-gradient row u[b] per batch row, the backward
of an attention consumed through its mean over T) against the float64 restatement of tests/attn_ref.py, with the rule and the
bounds tests/test_attention_paths_gpu.py applies to the general backward (its Case.check_backward, reused here).

Q, K and V are the column blocks of one packed (B*T, 3d) buffer, as MulT's self-attentions have them, dQ / dK / dV those of one
gradient buffer.  Every case also runs the general backward on the materialised broadcast dO and holds it to the same bounds,
so that an input the bounds do not fit shows on both paths.  B = 2, H = 2; self-attention T:
    7, 30     one ragged block, one active wave (the general dK/dV kernel's T <= 32 sweep split has no uniform counterpart)
    33        crosses a 32-key block
    64, 65    one tile, then two: the ring and its hand-over
    130, 200  two 128-row chunks per (b, h): two workgroups, a ragged last chunk
and once three problems of unequal T in one launch.  Every error / bound ratio is printed as a PARITY line (tag uni. / mat.)
before anything is asserted.  The pooled entry (mmf_attn_bwd_grouped_pooled: the launch makes u from the gradient of the pooled
output) is held, bit for bit, to the uniform entry on the rows it should have made."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as R  # noqa: E402
from mmfusion import lib  # noqa: E402
from test_attention_paths_gpu import BF16, F32, F64, GROWS, NAN, SENTINEL, Case, Mat, Vec, bits, rec, scale_of  # noqa: E402,F401
from test_kernel_forms_gpu import DEV  # noqa: E402

B, H = 2, 2
TS = (7, 30, 33, 64, 65, 130, 200)
DHS = (64, 96)


class Block(Mat):
    """column block `off` of a packed (rows + GROWS, 3d) buffer whose three blocks are all operands (or all outputs): its guards
    are the rows behind the matrix"""

    def __init__(self, buf, rows, d, off):
        self.rows, self.d, self.off, self.buf = rows, d, off, buf
        self.v = buf[:rows, off:off + d]
        self.mark()

    def guards_intact(self):
        return bool(torch.equal(bits(self.buf)[self.rows:], bits(self.before)[self.rows:]))


class Packed(Case):
    """a self-attention problem on packed (B*T, 3d) operands with dO = u[b] in every row of batch row b"""

    def __init__(self, dh, T, seed):
        self.dh, self.B, self.H, self.Tq, self.Tk = dh, B, H, T, T
        d = self.d = H * dh
        g = torch.Generator().manual_seed(seed)
        mk = lambda rows: R.bf16r(torch.randn(B, rows, d, generator=g, dtype=F64))
        self.q, self.k, self.v, self.u = mk(T), mk(T), mk(T), mk(1)
        self.do = self.u.expand(B, T, d).contiguous()
        self.ldq = self.ldk = self.ldv = 3 * d
        self.ldo = d
        qkv = torch.full((B * T + GROWS, 3 * d), SENTINEL, dtype=BF16, device=DEV)
        qkv[:B * T] = torch.cat([self.q, self.k, self.v], dim=-1).reshape(B * T, 3 * d).to(BF16)
        self.Q, self.K, self.V = (Block(qkv, B * T, d, i * d) for i in range(3))
        self.O = Mat(B * T, d, d, 0)
        self.LSE = Vec(B * H * T)
        self.U = Mat(B, d, d, 0, self.u)
        self.dO = Mat(B * T, d, d, 0, self.do)
        self.fresh_outputs()

    def fresh_outputs(self):
        d, T = self.d, self.Tq
        dqkv = torch.full((B * T + GROWS, 3 * d), SENTINEL, dtype=BF16, device=DEV)
        dqkv[:B * T] = NAN
        self.dQ, self.dK, self.dV = (Block(dqkv, B * T, d, i * d) for i in range(3))
        self.delta = Vec(B * H * T)

    def problem(self, uniform):
        p = super().problem()
        if uniform:
            p.dO = self.U.ptr
        return p


_CASES = {}


def case(dh, T):
    """the operands and the float64 reference of (dh, T): built once, shared by every test that needs them"""
    if (dh, T) not in _CASES:
        c = Packed(dh, T, seed=1000 * dh + T)
        c.reference(scale_of(dh))
        c.hand_reference_forward_to_backward()
        _CASES[(dh, T)] = c
    return _CASES[(dh, T)]


def run_both(rec, dh, cases):
    scale = scale_of(dh)
    fails = []
    tags = [""] if len(cases) == 1 else [f"p{i}." for i in range(len(cases))]
    for uniform in (True, False):
        for c in cases:
            c.fresh_outputs()
        probs = [c.problem(uniform) for c in cases]
        if uniform:
            assert lib.attn_bwd_uniform_available(dh, 0.0)
            ws = torch.full((lib.attn_bwd_uniform_workspace_bytes(probs) // 4 + 16,), SENTINEL, dtype=F32, device=DEV)
            lib.attn_bwd_grouped_uniform(probs, dh, scale, ws)
        else:
            lib.attn_bwd_grouped(probs, dh, scale)
        torch.cuda.synchronize()
        for c, t in zip(cases, tags):
            c.check_backward(rec, fails, t + ("uni." if uniform else "mat."))
            if not c.U.untouched():
                fails.append(f"{t}u: changed by the backward")
        if uniform and not bool((ws[-16:] == SENTINEL).all()):
            fails.append("workspace: written past its size")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dh", DHS)
def test_uniform_backward_against_float64(rec, dh, T):
    run_both(rec, dh, [case(dh, T)])


@pytest.mark.parametrize("dh", DHS)
def test_three_unequal_problems_in_one_launch(rec, dh):
    run_both(rec, dh, [case(dh, 200), case(dh, 30), case(dh, 65)])


@pytest.mark.parametrize("dh", DHS)
def test_pooled_entry_makes_the_rows_itself(dh):
    """mmf_attn_bwd_grouped_pooled: handed the gradient g of the pooled output as column blocks of one (B, 2d + 8) tensor, the launch
    writes u[b] = bf16(g[b] / T) (f32 product with the f32 1 / T, as mmf_meanpool_cat_bwd rounds) and gives, bit for bit, what
    the uniform entry gives for that u.  Two problems, T = 65 and 30."""
    scale, cases = scale_of(dh), [case(dh, 65), case(dh, 30)]
    d = H * dh
    gen = torch.Generator().manual_seed(dh)
    g = torch.full((B, 2 * d + 8), SENTINEL, dtype=BF16, device=DEV)
    g[:, :2 * d] = torch.randn(B, 2 * d, generator=gen).to(BF16).to(DEV)
    want_u = [(g[:, i * d:(i + 1) * d].float() * (torch.ones((), dtype=F32, device=DEV) / c.Tq)).to(BF16) for i, c in enumerate(cases)]
    outs = []
    for pooled in (True, False):
        us = [torch.full((B + GROWS, d), SENTINEL, dtype=BF16, device=DEV) for _ in cases]
        probs = []
        for i, c in enumerate(cases):
            c.fresh_outputs()
            if not pooled:
                us[i][:B] = want_u[i]
            p = c.problem(True)
            p.dO = us[i].data_ptr()
            probs.append(p)
        ws = torch.empty((lib.attn_bwd_uniform_workspace_bytes(probs) // 4,), dtype=F32, device=DEV)
        lib.attn_bwd_grouped_uniform(probs, dh, scale, ws,
                                     pooled=([g.data_ptr() + 2 * i * d for i in range(2)], g.stride(0)) if pooled else None)
        torch.cuda.synchronize()
        for i, c in enumerate(cases):
            assert torch.equal(bits(us[i][:B]), bits(want_u[i])), f"u of problem {i}"
            assert bool((us[i][B:] == SENTINEL).all()), "guard rows behind u"
        outs.append([bits(x.buf) for c in cases for x in (c.dQ, c.delta)])
    assert bool((g[:, 2 * d:] == SENTINEL).all())
    for a, b in zip(*outs):
        assert torch.equal(a, b), "the pooled entry differs from the uniform entry on the same rows"


def test_availability_and_refusals():
    assert lib.attn_bwd_uniform_available(64, 0.0) and lib.attn_bwd_uniform_available(96, 0.0)
    assert not lib.attn_bwd_uniform_available(96, 0.1) and not lib.attn_bwd_uniform_available(128, 0.0)
    c = case(64, 7)
    c.fresh_outputs()
    probs = [c.problem(True)]
    need = lib.attn_bwd_uniform_workspace_bytes(probs)
    assert need == 4 * B * H * 7
    short = torch.empty((need // 4 - 1,), dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        lib.attn_bwd_grouped_uniform(probs, 64, scale_of(64), short)
    torch.cuda.synchronize()
    assert bool(torch.isnan(c.dQ.v.float()).all()), "a refused call launched something"
