"""RobustMultimodalModel without a GPU: the reference's state-dict layout, the float64 restatement of the head's backward
(tests/robust_ref.py) against torch autograd of the reference's formulation, and the optimiser's range coalescing."""
import pytest
import torch

from robust_ref import head_bwd, head_fwd, torch_head

F64 = torch.float64


def _cfg(d=256, heads=4, G=256, C=7):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.feature_inputs = True
    cfg.fusion_type = "hierarchical"
    cfg.fusion_hidden_size, cfg.fusion_num_heads, cfg.graph_hidden_size = d, heads, G
    cfg.num_emotions = C
    return cfg


@pytest.mark.parametrize("d,heads,C", [(256, 4, 7), (512, 8, 5)])
def test_state_dict_has_reference_layout(d, heads, C):
    from models.multimodal_model import MultimodalEmotionModel, RobustMultimodalModel
    cfg = _cfg(d, heads, d, C)
    torch.manual_seed(0)
    model = RobustMultimodalModel(cfg)
    sd = model.state_dict()
    base = MultimodalEmotionModel(cfg).state_dict()
    want = {f"base_model.{k}": tuple(v.shape) for k, v in base.items()}
    for m in ("text", "audio", "video"):
        want[f"{m}_only_classifier.weight"] = (C, d)
        want[f"{m}_only_classifier.bias"] = (C,)
    want.update({"modality_predictor.0.weight": (d, 3 * d), "modality_predictor.0.bias": (d,),
                 "modality_predictor.2.weight": (3, d), "modality_predictor.2.bias": (3,)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(sd)[:len(base)] == list(want)[:len(base)]          # base_model first, in the reference's order


def _case(B, d, C, seed):
    g = torch.Generator().manual_seed(seed)
    f = [torch.randn(B, d, generator=g, dtype=F64) for _ in range(3)]
    h = torch.relu(torch.randn(B, d, generator=g, dtype=F64))
    W2 = torch.randn(3, d, generator=g, dtype=F64) / d ** 0.5
    b2 = torch.randn(3, generator=g, dtype=F64)
    Wm = [torch.randn(C, d, generator=g, dtype=F64) / d ** 0.5 for _ in range(3)]
    bm = [torch.randn(C, generator=g, dtype=F64) for _ in range(3)]
    return f, h, W2, b2, Wm, bm


NAMES = ("text", "audio", "video")


@pytest.mark.parametrize("available", [None, [], ["video"], ["text", "audio"], ["text", "audio", "video"], ["nope", "audio"]],
                         ids=lambda a: "predicted" if a is None else ("none" if not a else "_".join(a)))
@pytest.mark.parametrize("direct", ["y", "all", "p_only", "a_only", "wn_only"])
def test_restated_backward_equals_float64_autograd(available, direct):
    B, d, C = 5, 12, 7
    f, h, W2, b2, Wm, bm = _case(B, d, C, 3)
    mask = None if available is None else sum(1 << i for i, n in enumerate(NAMES) if n in available)
    leaves = [x.clone().requires_grad_(True) for x in (*f, h, W2, b2, *Wm, *bm)]
    lf, lh, lW2, lb2, lWm, lbm = leaves[0:3], leaves[3], leaves[4], leaves[5], leaves[6:9], leaves[9:12]
    a, p, wn, y = torch_head(lf, lh, lW2, lb2, lWm, lbm, available)
    fw = head_fwd(f, h, W2, b2, Wm, bm, mask)
    for name, got, want in (("a", fw["a"], a), ("wn", fw["wn"], wn), ("y", fw["y"], y)):
        assert torch.allclose(got, want.detach(), rtol=1e-12, atol=1e-12), name
    for m in range(3):
        assert torch.allclose(fw["p"][m], p[m].detach(), rtol=1e-12, atol=1e-12)
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    g = rnd(B, C) if direct in ("y", "all") else torch.zeros(B, C, dtype=F64)
    dP = [rnd(B, C) for _ in range(3)] if direct in ("all", "p_only") else None
    dA = rnd(B, 3) if direct in ("all", "a_only") else None
    dN = rnd(B, 3) if direct in ("all", "wn_only") else None
    loss = (g * y).sum()
    if dP is not None:
        loss = loss + sum((dP[m] * p[m]).sum() for m in range(3))
    if dA is not None:
        loss = loss + (dA * a).sum()
    if dN is not None and wn.requires_grad:
        loss = loss + (dN * wn).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if gr is None else gr for x, gr in zip(leaves, grads)]
    bw = head_bwd(f, h, W2, Wm, fw["a"], fw["p"], fw["wn"], g, dP, dA, dN, mask)
    got = {"df": bw["df"], "dh": bw["dh"], "dW2": bw["dW2"], "db2": bw["db2"], "dWm": bw["dWm"], "dbm": bw["dbm"]}
    want = {"df": grads[0:3], "dh": grads[3], "dW2": grads[4], "db2": grads[5], "dWm": grads[6:9], "dbm": grads[9:12]}
    for k in got:
        gs, ws = (got[k], want[k]) if isinstance(got[k], list) else ([got[k]], [want[k]])
        for i, (gg, ww) in enumerate(zip(gs, ws)):
            assert torch.allclose(gg, ww, rtol=1e-10, atol=1e-12), f"{k}[{i}]: {float((gg - ww).abs().max()):.3e}"
    if mask is not None:
        # constants: exactly 1, 1/2, 1/3 or 0 after the f64 normalisation of the reference (1 / (1 + 1e-8) aside)
        n = bin(mask).count("1")
        assert torch.allclose(fw["wn"].sum(dim=1), torch.full((B,), 1.0 if n else 0.0, dtype=F64), atol=1e-7)


def test_coalesce_ranges():
    from mmfusion.train import coalesce_ranges
    # arena neighbours share a range across their alignment padding; a parameter left out splits it
    assert coalesce_ranges([]) == []
    assert coalesce_ranges([(0, 10), (64, 64), (128, 1)]) == [(0, 129)]
    assert coalesce_ranges([(128, 1), (0, 10)]) == [(0, 10), (128, 129)]
    assert coalesce_ranges([(0, 64), (64, 3), (192, 5), (256, 64)]) == [(0, 67), (192, 320)]
    assert coalesce_ranges([(0, 65), (128, 2)]) == [(0, 130)]
    assert coalesce_ranges([(0, 65), (192, 2)]) == [(0, 65), (192, 194)]


def test_robust_wrapper_signature_and_factory():
    import inspect
    from models.multimodal_model import RobustMultimodalModel, create_model
    sig = inspect.signature(RobustMultimodalModel.forward)
    assert list(sig.parameters)[1:] == ["text_input", "audio_input", "video_input", "available_modalities",
                                        "missing_modalities"]
    with pytest.raises(NotImplementedError):
        create_model(_cfg(), "robust")


def test_reached_parameters_are_encoders_and_head():
    from models.multimodal_model import RobustMultimodalModel
    from mmfusion.train import RobustTrainStep
    model = RobustMultimodalModel(_cfg())
    ids = {id(p) for p in RobustTrainStep.reached_parameters(model)}
    names = {n for n, p in model.named_parameters() if id(p) in ids}
    for n, _ in model.named_parameters():
        enc = n.split(".")[1] in ("text_encoder", "audio_encoder", "video_encoder") if n.startswith("base_model.") else True
        side = ".adapter." in n or n.endswith("prompt_embeddings")
        assert (n in names) == (enc and not side), n
    assert "base_model.video_encoder.temporal_lstm.weight_ih_l0" in names
    assert "modality_predictor.0.weight" in names and "text_only_classifier.bias" in names
    assert not any(n.startswith("base_model.fusion_layer.") or n.startswith("base_model.classifier.") for n in names)
