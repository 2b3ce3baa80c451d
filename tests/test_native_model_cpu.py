"""Models on the three native backbones without a GPU: which parameters the training steps select.  A native backbone registers
its frozen weights as ``nn.Parameter``s (``requires_grad = False``) under ``base_model.<kind>_encoder``, in the model's arena, and
``FusedAdamW`` applies weight decay to whatever range it is given: no frozen parameter may be in a step's selection."""
import pytest
import torch

import native_model_cases as cases


def _names(model, params):
    ids = {id(p) for p in params}
    return {n for n, p in model.named_parameters() if id(p) in ids}


def _robust(k):
    from models.multimodal_model import RobustMultimodalModel
    torch.manual_seed(3)
    return RobustMultimodalModel(cases.config(k=k))


def _fewshot(k):
    from models.multimodal_model import FewShotModel, MultimodalEmotionModel
    cfg = cases.config(k=k)
    torch.manual_seed(3)
    return FewShotModel(MultimodalEmotionModel(cfg), cfg)


@pytest.mark.parametrize("k", [0, 1, "all"])
def test_robust_step_reaches_no_frozen_parameter(k):
    from mmfusion.train import RobustTrainStep
    model = _robust(k)
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen and all(cases.is_backbone(n) for n in frozen)          # (even "all" keeps the feature-extractor convolutions)
    names = _names(model, RobustTrainStep.reached_parameters(model))
    assert not names & frozen, sorted(names & frozen)[:4]
    # ... and every trainable backbone parameter is reached: the loss goes through all three encoders
    live = {n for n, p in model.named_parameters() if p.requires_grad and cases.is_backbone(n)}
    assert live <= names and bool(live) == (k != 0)
    # the selection outside the backbones is what it is on feature inputs
    from models.multimodal_model import RobustMultimodalModel
    plain = RobustMultimodalModel(cases.config(feature_inputs=True))
    assert {n for n in names if not cases.is_backbone(n)} == _names(plain, RobustTrainStep.reached_parameters(plain))


@pytest.mark.parametrize("k", [0, 1])
def test_fewshot_step_reaches_no_frozen_parameter(k):
    from mmfusion.train import FEWSHOT_TRAINABLE, FewShotTrainStep
    model = _fewshot(k)
    names = _names(model, FewShotTrainStep.reached_parameters(model))
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen and not names & frozen
    assert not any(cases.is_backbone(n) for n in names)                  # no backbone parameter has a trainable name
    assert "base_model.text_encoder.prompt_embeddings" in names          # the native text backbone carries the prompt's gradient
    assert all(any(key in n for key in FEWSHOT_TRAINABLE) for n in names)
    # a parameter frozen from outside leaves the selection too
    model.base_model.text_encoder.prompt_embeddings.requires_grad_(False)
    assert "base_model.text_encoder.prompt_embeddings" not in _names(model, FewShotTrainStep.reached_parameters(model))


def test_twin_state_dict_is_the_whole_models_without_its_backbones():
    model = cases.base_model(cases.config(k=1))
    twin = cases.twin_of(model)
    assert list(twin.state_dict()) == list(cases.non_backbone_state(model))
    enc, bb = cases.pieces(model)
    for kind in cases.KINDS:
        assert bb[kind].trainable_layers == 1 and bb[kind] is not cases.backbones(model)[kind]
        for (n, p), (_, q) in zip(bb[kind].named_parameters(), cases.backbones(model)[kind].named_parameters()):
            assert torch.equal(p, q) and p.requires_grad == q.requires_grad and p.data_ptr() != q.data_ptr(), n


@pytest.mark.parametrize("kind", cases.KINDS)
def test_restatements_are_finite_and_well_scaled_on_the_zeroed_inputs(kind):
    """what ``missing_modalities`` feeds a backbone (ids and mask all 0, a zero waveform, zero frames) through the float64
    restatement the GPU test compares with, without and with bf16 storage: finite, of unit scale per element (every one ends in a
    LayerNorm) and the two a storage error apart, so the relative bound ``BOUND_A`` is meaningful there"""
    import deberta_ref
    import vit_ref
    import w2v_ref
    from helpers import BOUND_A, l2_rel
    model = cases.base_model(cases.config(k=1))
    sd = cases.seed_backbones(model)[kind]
    cfg = cases.backbones(model)[kind].config
    text, wave, frames, _ = cases.inputs()
    if kind == "text":
        ids, mask = torch.zeros_like(text["input_ids"]), torch.zeros_like(text["attention_mask"])
        run = lambda stored: deberta_ref.deberta_forward(sd, ids, mask, cfg, bf16_storage=stored)
    elif kind == "audio":
        run = lambda stored: w2v_ref.w2v_forward(sd, torch.zeros_like(wave).double(), cfg, bf16_storage=stored)
    else:
        run = lambda stored: vit_ref.vit_forward(sd, torch.zeros(6, 3, 64, 64, dtype=torch.float64), cfg, bf16_storage=stored, cls_last_only=True)
    exact, stored = run(False), run(True)
    assert bool(torch.isfinite(exact).all()) and bool(torch.isfinite(stored).all())
    rms = float(exact.square().mean().sqrt())
    assert 0.3 < rms < 3.0, rms
    assert 0.0 < l2_rel(stored, exact) < BOUND_A


def test_restated_attention_is_uniform_for_a_masked_query_row():
    """the rule ``NativeDeberta``'s docstring states, in the restatement: under an all-zero mask every query row is masked and
    every key too, and each row's result is the plain mean of all T values"""
    import deberta_ref
    g = torch.Generator().manual_seed(5)
    n, H, T, dh, S = 2, 3, 12, 64, 8
    q, k, v = (torch.randn(n, H, T, dh, generator=g, dtype=torch.float64) for _ in range(3))
    posq, posk = (torch.randn(H, 2 * S, dh, generator=g, dtype=torch.float64) for _ in range(2))
    idx = deberta_ref.bucket_index(T, S, 32)
    mask = torch.ones(n, T, dtype=torch.long)
    mask[1] = 0
    out = deberta_ref.disentangled_attention(q, k, v, posq, posk, idx, mask, (3.0 * dh) ** 0.5)
    assert torch.allclose(out[1], v[1].mean(dim=-2, keepdim=True).expand_as(out[1]), rtol=0, atol=1e-12)
    assert not torch.allclose(out[0], v[0].mean(dim=-2, keepdim=True).expand_as(out[0]), atol=1e-3)
