"""FewShotModel without a GPU: the reference's state-dict layout and forward signature, the row-count check, which
parameters the few-shot step trains, the factory's refusal, and the float64 restatement of the head's gradients
(tests/fewshot_ref.py) against torch autograd of the reference's formulation."""
import inspect
import types

import pytest
import torch
import torch.nn as nn

from fewshot_ref import head_loss_and_grads, torch_head

F64 = torch.float64


def _cfg(d=256, heads=4, G=256, C=7, feature_inputs=True):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.feature_inputs = feature_inputs
    cfg.fusion_type = "hierarchical"
    cfg.fusion_hidden_size, cfg.fusion_num_heads, cfg.graph_hidden_size = d, heads, G
    cfg.num_emotions = C
    return cfg


class _Backbone(nn.Module):
    """stands in for a pretrained backbone: only ``config.hidden_size`` and one parameter"""

    def __init__(self, hidden=768):
        super().__init__()
        self.config = types.SimpleNamespace(hidden_size=hidden, model_type="bert")
        self.embeddings = nn.Module()
        self.embeddings.word_embeddings = nn.Embedding(10, hidden)


def _model(cfg, backbones=None):
    from models.multimodal_model import FewShotModel, MultimodalEmotionModel
    return FewShotModel(MultimodalEmotionModel(cfg, backbones), cfg)


@pytest.mark.parametrize("d,heads", [(256, 4), (512, 8)])
def test_state_dict_has_reference_layout(d, heads):
    from models.multimodal_model import MultimodalEmotionModel
    cfg = _cfg(d, heads, d)
    torch.manual_seed(0)
    model = _model(cfg)
    sd = model.state_dict()
    base = MultimodalEmotionModel(cfg).state_dict()
    want = {f"base_model.{k}": tuple(v.shape) for k, v in base.items()}
    H = d // 2
    for enc in ("support_encoder", "query_encoder"):            # nn.LSTM(d, d / 2, batch_first, bidirectional)
        for sfx in ("", "_reverse"):
            want.update({f"{enc}.weight_ih_l0{sfx}": (4 * H, d), f"{enc}.weight_hh_l0{sfx}": (4 * H, H),
                         f"{enc}.bias_ih_l0{sfx}": (4 * H,), f"{enc}.bias_hh_l0{sfx}": (4 * H,)})
    want.update({"prototype_network.0.weight": (d, d), "prototype_network.0.bias": (d,),
                 "prototype_network.2.weight": (d, d), "prototype_network.2.bias": (d,)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(sd) == list(want)                                     # the reference's order
    assert isinstance(model.prototype_network[1], nn.ReLU)


def test_forward_signature_and_factory():
    from models.multimodal_model import FewShotModel, MultimodalEmotionModel, create_model
    assert list(inspect.signature(FewShotModel.__init__).parameters)[1:] == ["base_model", "config"]
    assert list(inspect.signature(FewShotModel.forward).parameters)[1:] == ["support_data", "query_data", "n_way", "n_shot"]
    assert list(inspect.signature(MultimodalEmotionModel.encode).parameters)[1:] == [
        "text_input", "audio_input", "video_input", "use_adapter", "use_prompt", "missing_modalities"]
    with pytest.raises(NotImplementedError):
        create_model(_cfg(), "few_shot")


def test_support_row_count_must_be_n_way_times_n_shot():
    model = _model(_cfg())
    data = lambda B: {"text": {"input_ids": torch.randn(B, 4, 768), "attention_mask": torch.ones(B, 4, dtype=torch.long)},
                      "audio": torch.randn(B, 5, 768), "video": torch.randn(B, 3, 768)}
    with pytest.raises(ValueError):
        model(data(7 * 5 - 1), data(4), 7, 5)
    with pytest.raises(ValueError):
        model(data(10), data(4), 3, 3)


def _names(model, params):
    ids = {id(p) for p in params}
    return {n for n, p in model.named_parameters() if id(p) in ids}


def test_reached_parameters_feature_mode():
    from mmfusion.train import FEWSHOT_TRAINABLE, FewShotTrainStep
    model = _model(_cfg())
    names = _names(model, FewShotTrainStep.reached_parameters(model))
    assert names, "nothing reached"
    for n, _ in model.named_parameters():
        by_name = any(k in n for k in FEWSHOT_TRAINABLE)
        # feature inputs bypass the prompt: torch leaves its .grad None, AdamW skips it
        assert (n in names) == (by_name and not n.endswith("prompt_embeddings")), n
    for m in ("text", "audio", "video"):
        assert f"base_model.{m}_encoder.adapter.down_project.weight" in names
        assert f"base_model.{m}_encoder.adapter.up_project.bias" in names
    assert {"prototype_network.0.weight", "prototype_network.2.bias"} <= names
    assert not any(n.startswith(("support_encoder.", "query_encoder.")) for n in names)
    assert "base_model.text_encoder.prompt_embeddings" not in names


def test_reached_parameters_backbone_mode():
    from mmfusion.train import FewShotTrainStep
    bb = {"text": _Backbone(), "audio": _Backbone(), "video": _Backbone()}
    model = _model(_cfg(feature_inputs=False), bb)
    names = _names(model, FewShotTrainStep.reached_parameters(model))
    assert "base_model.text_encoder.prompt_embeddings" in names
    assert "base_model.text_encoder.model.embeddings.word_embeddings.weight" not in names
    assert all(".adapter." in n or n.startswith("prototype_network.") or n.endswith("prompt_embeddings") for n in names)


@pytest.mark.parametrize("n_way,n_shot,Nq,d", [(7, 1, 16, 12), (7, 5, 16, 8), (3, 4, 9, 16), (5, 2, 1, 4)])
def test_restated_head_gradients_equal_float64_autograd(n_way, n_shot, Nq, d):
    g = torch.Generator().manual_seed(100 * n_way + n_shot)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    s3 = [rnd(n_way * n_shot, d).requires_grad_(True) for _ in range(3)]
    q3 = [rnd(Nq, d).requires_grad_(True) for _ in range(3)]
    params = [(rnd(d, d) / d ** 0.5).requires_grad_(True), rnd(d).requires_grad_(True),
              (rnd(d, d) / d ** 0.5).requires_grad_(True), rnd(d).requires_grad_(True)]
    y = torch.randint(0, n_way, (Nq,), generator=g)
    _, _, _, _, pred = torch_head(s3, q3, *params, n_way, n_shot)
    loss = nn.CrossEntropyLoss()(pred, y)
    loss.backward()
    ref = head_loss_and_grads(s3, q3, *params, n_way, n_shot, y)
    assert abs(float(ref["loss"]) - loss.item()) <= 1e-12
    for m in range(3):
        assert torch.allclose(ref["ds"], s3[m].grad, rtol=1e-10, atol=1e-13), f"support {m}"
        assert torch.allclose(ref["dq"], q3[m].grad, rtol=1e-10, atol=1e-13), f"query {m}"
    for k, p in zip(("dW0", "db0", "dW2", "db2"), params):
        assert torch.allclose(ref[k], p.grad, rtol=1e-10, atol=1e-13), k


def test_zero_distance_gives_zero_gradient_like_torch_cdist():
    from fewshot_ref import dist_bwd
    P = torch.randn(4, 8, dtype=F64)
    q = torch.cat([P[2:3], torch.randn(2, 8, dtype=F64)]).requires_grad_(True)
    Pl = P.clone().requires_grad_(True)
    dist = torch.cdist(q, Pl, p=2)
    gd = torch.randn(3, 4, dtype=F64)
    (gd * dist).sum().backward()
    assert float(dist[0, 2]) == 0.0
    dq, dP = dist_bwd(q, Pl, dist, torch.softmax(-dist, -1), gd, None)
    assert torch.isfinite(q.grad).all() and torch.allclose(dq, q.grad, atol=1e-13)
    assert torch.allclose(dP, Pl.grad, atol=1e-13)
