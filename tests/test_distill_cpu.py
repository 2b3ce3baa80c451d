"""Knowledge distillation without a GPU: the wrapper's construction, attributes, freezing, modes and state_dict layout
(reference models/multimodal_model.py:222-262, :465-468), its refusals, the ABI declaration of the two KD entry points, and
the float64 restatement of tests/distill_ref.py against torch's own formulation."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from distill_ref import kd_value_grad

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(d=64, heads=2, **kw):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.feature_inputs = True
    cfg.fusion_hidden_size, cfg.fusion_num_heads = d, heads
    cfg.graph_hidden_size, cfg.graph_num_layers = d, 2
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_create_model_distillation_state_dict_layout():
    from models.multimodal_model import KnowledgeDistillationModel, MultimodalEmotionModel, create_model
    torch.manual_seed(0)
    kd = create_model(_cfg(), "distillation")
    assert isinstance(kd, KnowledgeDistillationModel)
    assert isinstance(kd.teacher, MultimodalEmotionModel) and isinstance(kd.student, MultimodalEmotionModel)
    assert kd.temperature == 4.0 and kd.alpha == 0.7
    want = {"teacher." + k for k in kd.teacher.state_dict()} | {"student." + k for k in kd.student.state_dict()}
    assert set(kd.state_dict()) == want
    assert len(kd.state_dict()) == len(kd.teacher.state_dict()) + len(kd.student.state_dict())


def test_teacher_frozen_and_modes_follow_nn_module():
    from models.multimodal_model import KnowledgeDistillationModel, MultimodalEmotionModel
    torch.manual_seed(0)
    teacher = MultimodalEmotionModel(_cfg(128, 4))
    kd = KnowledgeDistillationModel(teacher, _cfg(64, 2))
    assert all(not p.requires_grad for p in kd.teacher.parameters())
    assert all(p.requires_grad for p in kd.student.parameters())
    assert kd.teacher.training is False
    kd.train()                        # the reference trainer's model.train() reaches the teacher (advanced_trainer.py:118)
    assert kd.teacher.training is True and kd.student.training is True
    kd.eval()
    assert kd.teacher.training is False and kd.student.training is False


def test_wrapper_is_not_an_arena_root():
    from models.fusion_layers import _FusionBase
    from models.multimodal_model import KnowledgeDistillationModel
    assert not issubclass(KnowledgeDistillationModel, _FusionBase)


def test_mismatched_teacher_and_student_refused():
    from models.multimodal_model import KnowledgeDistillationModel, MultimodalEmotionModel
    teacher = MultimodalEmotionModel(_cfg())
    with pytest.raises(ValueError):
        KnowledgeDistillationModel(teacher, _cfg(num_emotions=5))
    with pytest.raises(ValueError):
        KnowledgeDistillationModel(teacher, _cfg(feature_inputs=False))


def test_other_research_wrappers_still_out_of_scope():
    from models.multimodal_model import create_model
    for kind in ("few_shot", "robust"):
        with pytest.raises(NotImplementedError):
            create_model(_cfg(), kind)
    with pytest.raises(ValueError):
        create_model(_cfg(), "nope")


def test_wrapper_state_round_trip_and_reference_format_student(tmp_path):
    """The wrapper's model state loads into a fresh wrapper; the student saved alone is a reference-format checkpoint that
    ``load_pretrained_model`` reads as a teacher of the next run."""
    from mmfusion.train import save_checkpoint
    from models.multimodal_model import KnowledgeDistillationModel, MultimodalEmotionModel, load_checkpoint_file, \
        load_pretrained_model
    torch.manual_seed(1)
    cfg = _cfg()
    kd = KnowledgeDistillationModel(MultimodalEmotionModel(cfg), cfg)
    torch.manual_seed(2)
    kd2 = KnowledgeDistillationModel(MultimodalEmotionModel(cfg), cfg)
    kd2.load_state_dict(kd.state_dict())
    for k, v in kd.state_dict().items():
        assert torch.equal(v, kd2.state_dict()[k]), k
    path = str(tmp_path / "student.pt")
    save_checkpoint(path, kd.student, None, epoch=3)
    ck = load_checkpoint_file(path)
    assert ck["epoch"] == 3 and set(ck["model_state_dict"]) == set(kd.student.state_dict())
    m = load_pretrained_model(path, cfg)
    for k, v in kd.student.state_dict().items():
        assert torch.equal(v, m.state_dict()[k]), k
    KnowledgeDistillationModel(m, cfg)          # a loaded model serves as the teacher


def test_header_and_loader_declare_kd_entry_points():
    from mmfusion import lib
    hdr = open(os.path.join(REPO, "include", "mmfusion.h")).read()
    for sym in ("mmf_distill_kl", "mmf_fusion_loss_kd"):
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
        assert sym in lib.SYMBOLS, sym


@pytest.mark.parametrize("T", [0.5, 1.0, 4.0])
@pytest.mark.parametrize("B,C", [(1, 2), (16, 7), (33, 64)])
def test_distill_ref_matches_torch_kl_div(B, C, T):
    g = torch.Generator().manual_seed(B * 100 + C)
    s = (torch.randn(B, C, generator=g, dtype=torch.float64) * 5).requires_grad_(True)
    t = torch.randn(B, C, generator=g, dtype=torch.float64) * 5
    want = F.kl_div(F.log_softmax(s / T, dim=-1), F.softmax(t / T, dim=-1), reduction="batchmean") * T ** 2
    want.backward()
    loss, grad = kd_value_grad(s, t, T)
    want = want.detach()
    assert abs(float(loss) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert float((grad - s.grad).abs().max()) <= 1e-12
    loss0, grad0 = kd_value_grad(s, s, T)           # teacher == student
    assert abs(float(loss0)) <= 1e-12 and float(grad0.abs().max()) <= 1e-12
