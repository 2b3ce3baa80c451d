"""GPU: MultimodalTransformer's input gradients through the chained in-projection dgrad (ops._FanoutLinear: one GEMM per
modality over the four projections' stacked K, the pass-through gradients added in its drain) against the path it replaces
(ops.fanout_group + the in-projection linear group: twelve dgrads and a seven-operand sum), on one stream.

  * the forward is the same launches: every output bit-equal between the two paths;
  * input and parameter gradients of BOTH paths are set against a float64 restatement (oracle/ref_cpu.py run in float64 on the
    bf16-rounded inputs and the bf16 weight shadows): the new path's worst error may be at most the old path's worst error on the
    same inputs plus 10 % of it — it rounds the GEMM part once instead of four times, the margin covers the reassociated
    pass-through sum;
  * where the library refuses the chain the node issues the separate launches: bit-equal to the old path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import l2_rel  # noqa: E402
from mmfusion import lib, ops  # noqa: E402

DEV = "cuda"
KEYS = ("fused_features", "text_features", "audio_features", "video_features")
SHAPES = {"d192": (2, (33, 30, 7), 192, 2), "d768": (2, (64, 40, 30), 768, 8)}
_cache = {}


def _model(d, H):
    import config as cfgmod
    from models import fusion_layers as fl
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_num_heads, cfg.fusion_dropout = d, H, 0.0
    torch.manual_seed(11)
    return fl.MultimodalTransformer(cfg).to(DEV).train()


def _loss(out):
    return sum(out[k].double().square().sum() for k in KEYS)


def _run(model, xs, chain=True, refuse=False):
    """one forward + backward on one stream -> (outputs, input gradients, parameter gradients, chained launches)"""
    from mmfusion import arena as arena_mod
    from models import fusion_layers as fl
    arena_mod.ensure(model).zero_grad()
    ins = [x.clone().requires_grad_(True) for x in xs]
    saved = (fl._MULT_STREAMS, ops.fanout_linear_ok, lib.gemm_grouped_chain, ops.gemm_chain_available)
    count = [0]

    def spy(*a):
        count[0] += 1
        return saved[2](*a)
    fl._MULT_STREAMS, lib.gemm_grouped_chain = 1, spy
    if not chain:
        ops.fanout_linear_ok = lambda *a: False
    if refuse:
        ops.gemm_chain_available = lambda *a: False
    try:
        out = model(*ins)
        _loss(out).backward()
        torch.cuda.synchronize()
    finally:
        fl._MULT_STREAMS, ops.fanout_linear_ok, lib.gemm_grouped_chain, ops.gemm_chain_available = saved
    return ({k: out[k].detach().clone() for k in KEYS}, [x.grad.clone() for x in ins],
            {n: p.grad.detach().clone() for n, p in model.named_parameters()}, count[0])


def _case(name):
    """model, inputs, the old path's run, the new path's run and the float64 restatement of one shape: computed once"""
    if name not in _cache:
        from oracle import ref_cpu
        B, T, d, H = SHAPES[name]
        model = _model(d, H)
        g = torch.Generator(device=DEV).manual_seed(sum(T) + d)
        xs = [torch.randn(B, t, d, device=DEV, generator=g) for t in T]
        old, new = _run(model, xs, chain=False), _run(model, xs, chain=True)
        # float64 on what the kernels read: bf16 rows at the module boundary, bf16 shadows of the matrices, f32 vectors
        P = {k: (v.detach().to(torch.bfloat16) if v.dim() == 2 else v.detach()).double().cpu().requires_grad_(True)
             for k, v in model.state_dict().items()}
        xr = [x.to(torch.bfloat16).double().cpu().requires_grad_(True) for x in xs]
        _loss(ref_cpu.multimodal_transformer(P, "", *xr, H)).backward()
        _cache[name] = (model, xs, old, new, [x.grad for x in xr], {k: v.grad for k, v in P.items()})
    return _cache[name]


def _worst(gin, gp, rin, rp):
    win = max(l2_rel(a, b) for a, b in zip(gin, rin))
    scale = max(float(v.norm()) for v in rp.values() if v is not None)
    wp = max(l2_rel(gp[k], v) for k, v in rp.items() if v is not None and float(v.norm()) > 1e-7 * scale)
    return win, wp


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_bit_equal_and_the_chain_runs(name):
    _, _, old, new, _, _ = _case(name)
    assert old[3] == 0 and new[3] == 1, (old[3], new[3])              # one chained launch per backward, none on the old path
    for k in KEYS:
        assert not bool(torch.isnan(new[0][k].float()).any()), k
        assert torch.equal(old[0][k], new[0][k]), f"{k}: the forward is the same launches and must be bit-equal"
    for i, (a, b) in enumerate(zip(old[1], new[1])):
        assert a.shape == b.shape and not bool(torch.isnan(b).any()), f"input gradient {i}"


@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_against_float64_no_worse_than_the_old_path(name):
    _, _, old, new, rin, rp = _case(name)
    oin, op = _worst(old[1], old[2], rin, rp)
    nin, np_ = _worst(new[1], new[2], rin, rp)
    B, T, d, H = SHAPES[name]
    print(f"input-grad chain {name} (B {B}, T {T}, d {d}, H {H}): worst rel L2 against float64: input gradients old {oin:.6e} new {nin:.6e}; "
          f"parameter gradients old {op:.6e} new {np_:.6e}")
    assert nin <= 1.1 * oin, (nin, oin)
    assert np_ <= 1.1 * op, (np_, op)


@pytest.mark.parametrize("name", list(SHAPES))
def test_refused_chain_issues_the_separate_launches(name):
    model, xs, old, _, _, _ = _case(name)
    out, gin, _, launched = _run(model, xs, chain=True, refuse=True)
    assert launched == 0
    for k in KEYS:
        assert torch.equal(old[0][k], out[k]), k
    for i, (a, b) in enumerate(zip(old[1], gin)):
        assert torch.equal(a, b), f"input gradient {i}: the node's separate launches differ from the old path"
