"""GPU: MultimodalTransformer with the two fused seams — the FFN's keep-mask as bits, norm2 fused into the three-way modality sum —
against the same module with both seams replaced, in this test, by the two-launch forms they stand for (fused_seams_ref: the FFN
whose dgrad reads h through MASK_AUX; layernorm_group then add3_group).  fused_features, the three pooled features and the three
input gradients must be BIT-EQUAL between the module run and the composed run.

Shapes: B = 2, T = (40, 33, 7), d = 768, H = 8, in training mode with dropout (the bits then carry the dropout mask too) on the
default two streams and on one.  At these rows the FFN launches of the single-stream run have 72 tiles and take the bits (on two
streams they stay on generation 2 and on MASK_AUX); the LayerNorm launches are below the lane form's budget, so the fused sum
composes by itself (mmf_layernorm2_add3_available).  A second shape, T = (1100, 33, 7), is the smallest that puts the norm2
launches above that budget, so that the fused kernel itself
runs inside the module; which seams ran is asserted per case."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fused_seams_ref as old  # noqa: E402
from mmfusion import lib, ops  # noqa: E402
from mmfusion.lib import EPI_MASK_BITS  # noqa: E402

DEV = "cuda"
D, H, B = 768, 8, 2


@pytest.fixture(scope="module")
def model():
    import config as cfgmod
    from models import fusion_layers as fl
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_num_heads, cfg.fusion_dropout = D, H, 0.1
    torch.manual_seed(3)
    return fl.MultimodalTransformer(cfg).to(DEV).train()


class spies:
    """counts the launches of the two fused forms"""

    def __enter__(self):
        self.bits, self.ln2 = 0, 0
        self.real = (ops.gemm_group, lib.layernorm2_add3_fwd_grouped)

        def gemm_group(layout, probs, epilogue, **kw):
            self.bits += bool(epilogue & EPI_MASK_BITS)
            return self.real[0](layout, probs, epilogue, **kw)

        def ln2(*a):
            self.ln2 += 1
            return self.real[1](*a)
        ops.gemm_group, lib.layernorm2_add3_fwd_grouped = gemm_group, ln2
        return self

    def __exit__(self, *exc):
        ops.gemm_group, lib.layernorm2_add3_fwd_grouped = self.real


def run(model, xs):
    from mmfusion import arena as arena_mod
    arena_mod.ensure(model).zero_grad()
    ops.seed_dropout(77)
    ins = [x.clone().requires_grad_(True) for x in xs]
    out = model(*ins)
    keys = ("fused_features", "text_features", "audio_features", "video_features")
    sum(out[k].square().sum() for k in keys).backward()
    torch.cuda.synchronize()
    return {**{k: out[k].detach().clone() for k in keys}, **{f"d_input{i}": x.grad.clone() for i, x in enumerate(ins)}}


# (T, streams) -> (the FFN launches take the bits, the fused norm2 + sum kernel runs): on two streams the small shape's FFN launches
# have 24 and 48 tiles, below the 64 from which a launch leaves generation 2
CASES = [((40, 33, 7), 1, True, False), ((40, 33, 7), 2, False, False), ((1100, 33, 7), 1, True, True), ((1100, 33, 7), 2, True, True)]


@pytest.mark.parametrize("T,streams,bits,ln2_fused", CASES, ids=["T40_one_stream", "T40_two_streams", "T1100_one_stream", "T1100_two_streams"])
def test_module_equals_composed_seams(model, T, streams, bits, ln2_fused):
    from models import fusion_layers as fl
    g = torch.Generator(device=DEV).manual_seed(sum(T))
    xs = [torch.randn(B, t, D, device=DEV, generator=g) for t in T]
    saved = fl._MULT_STREAMS
    fl._MULT_STREAMS = streams
    try:
        with spies() as s:
            got = run(model, xs)
        assert (s.bits > 0) == bits and (s.ln2 > 0) == ln2_fused, (s.bits, s.ln2)
        real = (ops.ffn_residual_group, ops.ln2_add3_group)
        ops.ffn_residual_group, ops.ln2_add3_group = old.ffn_residual_group, old.ln2_add3_group
        try:
            with spies() as s:
                want = run(model, xs)
        finally:
            ops.ffn_residual_group, ops.ln2_add3_group = real
        assert s.bits == 0 and s.ln2 == 0
    finally:
        fl._MULT_STREAMS = saved
    for k in want:
        assert not bool(torch.isnan(got[k].float()).any()), k
        assert torch.equal(got[k], want[k]), f"{k}: the module differs from the composed seams"
