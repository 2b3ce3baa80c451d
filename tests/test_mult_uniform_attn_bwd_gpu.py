"""GPU: MultimodalTransformer on ops.attention_meanpool_group — the self-attentions and their mean over T as one node, whose
backward goes from the pooled (B, 3d) gradient to the uniform attention backward — against the same module with that op replaced,
in this test, by the two steps it stands for (ops.attention_group, then ops.meanpool_cat: `composed`).

B = 2, T = (40, 33, 7), d = 768, H = 8 (head_dim 96), training mode, on one stream and on the default two.
  * dropout 0: the op takes the uniform backward (spy).  The forward is the same launches, so the four outputs must be BIT-EQUAL;
    the backward differs by rounding, so the input gradients are held to tests/test_model_gpu.py's input-gradient bound (relative
    L2 5e-2) and every parameter's slice of the gradient arena to its parameter bounds (tests/test_parity_gpu.py's GP_L2, GP_L2_RELU
    for ReLU-fed tensors), composed as the reference.
  * dropout 0.1, and the fp32 mode: the op must take its fallback (spy: no uniform launch); outputs and input gradients must be
    BIT-EQUAL to the composed form, parameter gradients equal up to the order of their f32 atomic sums (assert_bit_equal)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import l2_rel  # noqa: E402
from mmfusion import lib, ops  # noqa: E402
from test_parity_gpu import GP_L2, GP_L2_RELU, RELU_FED  # noqa: E402

DEV = "cuda"
D, H, B, T = 768, 8, 2, (40, 33, 7)
GIN_L2 = 5e-2                      # tests/test_model_gpu.py, input gradient
KEYS = ("fused_features", "text_features", "audio_features", "video_features")


def build(dropout):
    import config as cfgmod
    from models import fusion_layers as fl
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_num_heads, cfg.fusion_dropout = D, H, dropout
    torch.manual_seed(3)
    return fl.MultimodalTransformer(cfg).to(DEV).train()


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator(device=DEV).manual_seed(sum(T))
    return [torch.randn(B, t, D, device=DEV, generator=g) for t in T]


def composed(specs, H_, dh, srcs, dropout_p=0.0):
    att = ops.attention_group(specs, H_, dh, srcs, dropout_p=dropout_p)
    return ops.meanpool_cat([o.view(s.B, s.Tq, H_ * dh) for o, s in zip(att, specs)])


class uniform_spy:
    """counts the uniform backward's launches"""

    def __enter__(self):
        self.n, self.real = 0, lib.attn_bwd_grouped_uniform

        def spy(*a, **kw):
            self.n += 1
            return self.real(*a, **kw)
        lib.attn_bwd_grouped_uniform = spy
        return self

    def __exit__(self, *exc):
        lib.attn_bwd_grouped_uniform = self.real


def run(model, xs, fp32=False):
    if not fp32:
        from mmfusion import arena as arena_mod
        arena_mod.ensure(model).zero_grad()
    else:
        model.zero_grad(set_to_none=True)
    ops.seed_dropout(77)
    ins = [x.clone().requires_grad_(True) for x in xs]
    out = model(*ins)
    sum(out[k].square().sum() for k in KEYS).backward()
    torch.cuda.synchronize()
    return ({k: out[k].detach().clone() for k in KEYS}, [x.grad.clone() for x in ins],
            {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})


def both(model, xs, streams=1, fp32=False):
    """(module run, uniform launches in it, composed run)"""
    from models import fusion_layers as fl
    saved = fl._MULT_STREAMS
    fl._MULT_STREAMS = streams
    try:
        with uniform_spy() as s:
            got = run(model, xs, fp32)
        real = ops.attention_meanpool_group
        ops.attention_meanpool_group = composed
        try:
            with uniform_spy() as s2:
                want = run(model, xs, fp32)
        finally:
            ops.attention_meanpool_group = real
        assert s2.n == 0
    finally:
        fl._MULT_STREAMS = saved
    return got, s.n, want


def params_close(got, want, tol):
    """every parameter gradient within tol(name) in relative L2, as tests/test_model_gpu.py walks them (a gradient that is zero up
    to cancellation in the reference must be (near-)zero); returns the worst (error, name)"""
    assert set(got) == set(want)
    scale = max(float(v.norm()) for v in want.values())
    worst = (0.0, "")
    for n, ref in want.items():
        a, b = got[n].float().cpu(), ref.float().cpu()
        if float(b.norm()) <= 1e-6 * scale:
            assert float(a.norm()) <= 1e-3 * scale, f"{n} should have a (near-)zero gradient"
            continue
        e = l2_rel(a, b)
        worst = max(worst, (e, n))
        assert e <= tol(n), f"gradient of {n}: rel L2 {e:.3e} > {tol(n)}"
    return worst


def assert_bit_equal(got, want):
    for k in KEYS:
        assert not bool(torch.isnan(got[0][k].float()).any()), k
        assert torch.equal(got[0][k], want[0][k]), f"{k}: the module differs from the composed form"
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        assert torch.equal(a, b), f"input gradient {i}"
    # Parameter gradients are not bit-repeatable between two runs of ONE form: bias and LayerNorm gradients are summed with f32
    # atomics in launch order.  They are held to what reordering an f32 sum can do: 2^-24 per addition, B * max(T) = 80 rows
    # per workgroup-level addend chain at most -> 80 x 2^-24 = 5e-6 of the sum of magnitudes; 1e-4 of the L2 norm leaves
    # room for cancellation and is a thousand times below the rounding of one bf16 operand.
    params_close(got[2], want[2], lambda n: 1e-4)


@pytest.mark.parametrize("streams", [1, 2], ids=["one_stream", "two_streams"])
def test_uniform_backward_in_the_module(inputs, streams):
    got, launches, want = both(build(0.0), inputs, streams)
    assert launches == (1 if streams == 1 else 2), launches
    for k in KEYS:
        assert not bool(torch.isnan(got[0][k].float()).any()), k
        assert torch.equal(got[0][k], want[0][k]), f"{k}: the forward is the same launches and must be bit-equal"
    worst = 0.0
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        e = l2_rel(a.float().cpu(), b.float().cpu())
        worst = max(worst, e)
        assert e <= GIN_L2, f"input gradient {i}: rel L2 {e:.3e}"
    pworst = params_close(got[2], want[2], lambda n: GP_L2_RELU if any(s in n for s in RELU_FED) else GP_L2)
    print(f"uniform vs composed ({streams} stream(s)): input gradients worst rel L2 {worst:.3e}; parameters worst {pworst[0]:.3e} ({pworst[1]})")


def test_dropout_takes_the_fallback(inputs):
    got, launches, want = both(build(0.1), inputs)
    assert launches == 0
    assert_bit_equal(got, want)


def test_fp32_mode_takes_the_fallback(inputs):
    model = build(0.0)
    model.precision = "fp32"
    got, launches, want = both(model, inputs, fp32=True)
    assert launches == 0
    assert_bit_equal(got, want)
