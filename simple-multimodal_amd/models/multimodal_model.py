"""``MultimodalEmotionModel`` — drop-in for the reference's ``models/multimodal_model.py:12-219``.

Kept verbatim: constructor ``(config)``, ``forward(text_input, audio_input, video_input,
use_adapter, use_prompt, compute_contrastive_loss, missing_modalities) -> Dict`` and its output
keys (reference :159-181), ``fusion_type`` dispatch incl. the ``ValueError`` (:29-46),
``EmotionClassifier`` (:186-219), ``create_model`` / ``load_pretrained_model`` (:453-485) and all
``state_dict`` names.  The fusion layer, the encoder tails and the heads are the MI355X HIP path: the
classifier's d -> d/2 layer on the skinny MFMA kernel, the 7-class / 1-unit output layers (classifier, valence,
arousal, uncertainty) on the narrow-linear kernel (f32 masters); the softmaxes over 7 logits are torch glue.

``KnowledgeDistillationModel`` (reference :222-262, ``create_model(config, "distillation")``): a frozen teacher and a
student ``MultimodalEmotionModel``, each in its own parameter arena, the distillation loss on the fused KD kernel
(``csrc/loss.hip``); the teacher's dropout draws from a state of its own (see the class).

``RobustMultimodalModel`` (reference :365-450): the base model, three modality-only classifiers and an availability
predictor in ONE arena; the head after the predictor's hidden layer is one HIP launch each way (``small_ops.robust_head``).
``create_model(config, "robust")`` still raises ``NotImplementedError``: construct ``RobustMultimodalModel(config)``.

``FewShotModel`` (reference :265-362): the base model, the (unused) support / query LSTMs and the prototype network in ONE
arena; the features come from ``MultimodalEmotionModel.encode`` (no fusion layer, no heads), the class means and the
distance / softmax tail are one HIP launch each way (``small_ops.fewshot_prototypes`` / ``fewshot_scores``).
``create_model(config, "few_shot")`` still raises ``NotImplementedError``: construct ``FewShotModel(base_model, config)``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from mmfusion import ops
from mmfusion import small_ops as sops
from mmfusion.ops import W

from .encoders import AudioEncoder, ModalityDropout, TextEncoder, VideoEncoder
from .fusion_layers import (AdaptiveFusion, ContrastiveFusion, EarlyFusion, GraphFusion,
                            HierarchicalFusion, LateFusion, MultimodalTransformer, _FusionBase)

_FUSIONS = {"early": EarlyFusion, "late": LateFusion, "mult": MultimodalTransformer, "graph": GraphFusion,
            "contrastive": ContrastiveFusion, "adaptive": AdaptiveFusion, "hierarchical": HierarchicalFusion}


class EmotionClassifier(nn.Module):
    """d -> d/2 -> num_emotions main head; the three hierarchical heads exist for state_dict
    compatibility (the reference computes and discards them, :204-219)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        d = config.fusion_hidden_size
        self.classifier = nn.Sequential(nn.Linear(d, d // 2), nn.ReLU(), nn.Dropout(config.fusion_dropout),
                                        nn.Linear(d // 2, config.num_emotions))
        self.sentiment_classifier = nn.Linear(d, 3)
        self.positive_classifier = nn.Linear(d, 2)
        self.negative_classifier = nn.Linear(d, 4)

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        """d -> d/2 (ReLU, dropout) on the skinny MFMA kernel, d/2 -> num_emotions on the narrow-linear kernel."""
        if not features.is_cuda:
            raise RuntimeError("mmfusion: the classifier head runs on the GPU only (no CPU fallback)")
        from mmfusion import arena as _arena_mod
        if getattr(self.classifier[0].weight, "_mmf_arena", None) is None:
            _arena_mod.ensure(self)                # stand-alone use; inside MultimodalEmotionModel the root did it
        p = float(self.config.fusion_dropout) if self.training else 0.0
        x = features.float().contiguous()                  # f32 rows: narrowed by the linear itself (mmfusion.ops._RowLinear)
        if ops.fp32_mode():
            x = ops.to_bf16(x)
        l0 = self.classifier[0]
        h = ops.linear(x, W(l0.weight), W(l0.bias), relu=True, out_f32=True, dropout_p=p)
        return sops.narrow_linear(h, self.classifier[3])


class MultimodalEmotionModel(_FusionBase):
    def __init__(self, config, backbones: Optional[Dict[str, nn.Module]] = None):
        super().__init__()
        self.config = config
        bb = backbones or {}
        self.text_encoder = TextEncoder(config, bb.get("text"))
        self.audio_encoder = AudioEncoder(config, bb.get("audio"))
        self.video_encoder = VideoEncoder(config, bb.get("video"))
        self.modality_dropout = ModalityDropout(dropout_rate=0.1)
        self.fusion_type = getattr(config, "fusion_type", "hierarchical")
        if self.fusion_type not in _FUSIONS:
            raise ValueError(f"Unknown fusion type: {self.fusion_type}")
        self.fusion_layer = _FUSIONS[self.fusion_type](config)
        self.classifier = None if self.fusion_type == "late" else EmotionClassifier(config)
        d = config.fusion_hidden_size
        self.valence_regressor = nn.Linear(d, 1)
        self.arousal_regressor = nn.Linear(d, 1)
        self.uncertainty_head = nn.Linear(d, config.num_emotions)

    def encode(self, text_input: Dict[str, torch.Tensor], audio_input: torch.Tensor, video_input: torch.Tensor,
               use_adapter: bool = False, use_prompt: bool = False,
               missing_modalities: Optional[List[str]] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The three encoders and, in training mode, ``ModalityDropout``: -> (text, audio, video) features, exactly the
        ``*_features`` outputs of ``forward``, without the fusion layer and the heads (``FewShotModel`` needs only these)."""
        if missing_modalities:                                                   # reference :77-86
            if "text" in missing_modalities:
                text_input = {"input_ids": torch.zeros_like(text_input["input_ids"]),
                              "attention_mask": torch.zeros_like(text_input["attention_mask"])}
            if "audio" in missing_modalities:
                audio_input = torch.zeros_like(audio_input)
            if "video" in missing_modalities:
                video_input = torch.zeros_like(video_input)
        tf = self.text_encoder(text_input["input_ids"], text_input["attention_mask"],
                               use_adapter=use_adapter, use_prompt=use_prompt)["features"]
        af = self.audio_encoder(audio_input, use_adapter=use_adapter)["features"]
        vf = self.video_encoder(video_input, use_adapter=use_adapter)["features"]
        if self.training:                                                        # reference :104-107
            tf, af, vf = self.modality_dropout(tf, af, vf, training=True)
        return tf, af, vf

    def forward(self, text_input: Dict[str, torch.Tensor], audio_input: torch.Tensor, video_input: torch.Tensor,
                use_adapter: bool = False, use_prompt: bool = False, compute_contrastive_loss: bool = False,
                missing_modalities: Optional[List[str]] = None) -> Dict[str, torch.Tensor]:
        tf, af, vf = self.encode(text_input, audio_input, video_input, use_adapter, use_prompt, missing_modalities)

        individual_logits = fusion_weights = None
        if self.fusion_type == "late":
            fo = self.fusion_layer(tf, af, vf)
            emotion_logits = fo["fused_logits"]
            individual_logits = {"text": fo["text_logits"], "audio": fo["audio_logits"], "video": fo["video_logits"]}
            fusion_weights = fo["fusion_weights"]
            head_in = (tf + af + vf) / 3                                         # reference :153
        else:
            if self.fusion_type in ("contrastive", "hierarchical"):
                fo = self.fusion_layer(tf, af, vf, compute_contrastive_loss=compute_contrastive_loss)
            else:
                fo = self.fusion_layer(tf, af, vf)
            head_in = fo["fused_features"] if isinstance(fo, dict) else fo
            emotion_logits = self.classifier(head_in)
        out = {"emotion_logits": emotion_logits, "emotion_probs": F.softmax(emotion_logits, dim=-1),
               "valence": sops.narrow_linear(head_in, self.valence_regressor),
               "arousal": sops.narrow_linear(head_in, self.arousal_regressor),
               "uncertainty": F.softmax(sops.narrow_linear(head_in, self.uncertainty_head), dim=-1),
               "text_features": tf, "audio_features": af, "video_features": vf}
        if self.fusion_type == "late":
            out.update({"individual_logits": individual_logits, "fusion_weights": fusion_weights})
        if isinstance(fo, dict):                                                 # reference :177-181
            for k, v in fo.items():
                if k != "fused_features":
                    out[k] = v
        return out


class KnowledgeDistillationModel(nn.Module):
    """Reference :222-262: ``teacher`` (frozen: ``requires_grad=False``, ``eval()``) and ``student =
    MultimodalEmotionModel(student_config)``; ``forward`` returns the student's outputs plus ``distillation_loss`` =
    T^2 * KL(softmax(t / T) || softmax(s / T)) (batchmean, ``small_ops.distill_kl``) and ``teacher_logits``.  ``alpha`` is
    stored and unused, as in the reference (its trainer weights the term 0.5).

    Not an arena root: teacher and student each become the root of their own arena at their first forward, so an
    optimiser over ``student``'s arena never sees a teacher weight.  Modes follow ``nn.Module``: ``kd.train()`` reaches the
    teacher too (the reference trainer does that, advanced_trainer.py:118), and the teacher then runs its dropout.  Its
    forward runs between the student's forward and the student's backward, whose dropout sites regenerate their masks
    from the LIVE device state (mmfusion.ops: dropout section), so the teacher draws from a state tensor of its own
    (``ops.dropout_state``) and leaves the student's state and site numbering where the student's forward left them."""

    def __init__(self, teacher_model: "MultimodalEmotionModel", student_config,
                 backbones: Optional[Dict[str, nn.Module]] = None):
        super().__init__()
        tcfg = getattr(teacher_model, "config", None)
        if tcfg is not None:
            if int(tcfg.num_emotions) != int(student_config.num_emotions):
                raise ValueError(f"KnowledgeDistillationModel: teacher has {tcfg.num_emotions} emotions, "
                                 f"the student config {student_config.num_emotions}")
            if bool(getattr(tcfg, "feature_inputs", False)) != bool(getattr(student_config, "feature_inputs", False)):
                raise ValueError("KnowledgeDistillationModel: teacher and student disagree on feature_inputs "
                                 "(both must take the same inputs)")
        self.teacher = teacher_model
        self.student = MultimodalEmotionModel(student_config, backbones=backbones)
        self.temperature = student_config.distill_temperature
        self.alpha = student_config.distill_alpha
        for param in self.teacher.parameters():
            param.requires_grad = False
        self.teacher.eval()
        self._teacher_rng: Optional[torch.Tensor] = None

    def teacher_rng_state(self) -> torch.Tensor:
        """The teacher's dropout state (device int64 [1]): the student's state at first use with the high word flipped, so
        the two never draw the same masks.  Created outside any capture by the first call (a training step's warm-up)."""
        st = ops.rng_state()
        if self._teacher_rng is None or self._teacher_rng.device != st.device:
            self._teacher_rng = st.clone() ^ (0x7EAC4E12 << 32)
        return self._teacher_rng

    def teacher_forward(self, *args, **kwargs) -> Dict[str, torch.Tensor]:
        """The teacher's forward without gradients, its dropout isolated from the student's (see the class)."""
        with torch.no_grad(), ops.dropout_state(self.teacher_rng_state()):
            return self.teacher(*args, **kwargs)

    def forward(self, *args, **kwargs) -> Dict[str, torch.Tensor]:
        student_output = self.student(*args, **kwargs)
        teacher_output = self.teacher_forward(*args, **kwargs)
        student_logits = student_output["emotion_logits"]
        teacher_logits = teacher_output["emotion_logits"]
        student_output["distillation_loss"] = sops.distill_kl(student_logits, teacher_logits, self.temperature)
        student_output["teacher_logits"] = teacher_logits
        return student_output


class FewShotModel(_FusionBase):
    """Reference :265-362: ``base_model`` (a ``MultimodalEmotionModel``), ``support_encoder`` / ``query_encoder``
    (``nn.LSTM(d, d / 2, bidirectional)``: constructed, never run, as in the reference; they keep its state_dict keys) and
    ``prototype_network`` (Linear(d, d), ReLU, Linear(d, d)).  ``forward(support_data, query_data, n_way, n_shot)`` takes
    the reference's dicts (``text`` {input_ids, attention_mask}, ``audio``, ``video``) and returns ``predictions`` =
    softmax(-distances), ``distances`` = cdist(query_features, prototypes), ``prototypes`` = prototype_network(class means
    of the support features), ``support_features`` and ``query_features`` (text + audio + video features of the base
    model with adapters and prompt, after ``ModalityDropout`` in training mode).  Support rows are class-major: row
    c * n_shot + s is shot s of class c; any other row count than n_way * n_shot raises ``ValueError``.

    Deliberate deviation in cost only: the features come from ``base_model.encode`` (encoders + ModalityDropout); the
    reference also runs the fusion layer and the heads and throws their outputs away (no gradient reaches them).

    An arena root (``_FusionBase``): the base model and the head share one parameter arena (a ``base_model`` that had an
    arena of its own moves into this one).  The class means, the sums of the three modalities and the distance / softmax
    tail are HIP launches (``small_ops.fewshot_prototypes`` / ``fewshot_scores``); the prototype MLP runs on the row linear."""

    def __init__(self, base_model: MultimodalEmotionModel, config):
        super().__init__()
        self.base_model = base_model
        self.config = config
        d = config.fusion_hidden_size
        self.support_encoder = nn.LSTM(d, d // 2, batch_first=True, bidirectional=True)
        self.query_encoder = nn.LSTM(d, d // 2, batch_first=True, bidirectional=True)
        self.prototype_network = nn.Sequential(nn.Linear(d, d), nn.ReLU(), nn.Linear(d, d))

    def _encode(self, data: Dict[str, torch.Tensor]):
        return self.base_model.encode(data["text"], data["audio"], data["video"], use_adapter=True, use_prompt=True)

    def head(self, support: Tuple[torch.Tensor, ...], query: Tuple[torch.Tensor, ...], n_way: int, n_shot: int):
        """(text, audio, video) support and query features -> (support_features, prototypes, query_features, distances,
        predictions)"""
        if not support[0].is_cuda:
            raise RuntimeError("mmfusion: the few-shot head runs on the GPU only (no CPU fallback)")
        sf, mean = sops.fewshot_prototypes(*support, n_way, n_shot)
        l0, l2 = self.prototype_network[0], self.prototype_network[2]
        h = ops.linear(mean, W(l0.weight), W(l0.bias), relu=True, out_f32=True)
        prototypes = ops.linear(h, W(l2.weight), W(l2.bias), out_f32=True)
        qf, distances, predictions = sops.fewshot_scores(*query, prototypes)
        return sf, prototypes, qf, distances, predictions

    @staticmethod
    def _check_rows(support_data: Dict[str, torch.Tensor], n_way: int, n_shot: int) -> None:
        rows = support_data["audio"].shape[0]
        if rows != int(n_way) * int(n_shot):
            raise ValueError(f"FewShotModel: {rows} support rows, n_way * n_shot = {n_way} * {n_shot} (class-major)")

    def __call__(self, support_data, query_data, n_way, n_shot):
        self._check_rows(support_data, n_way, n_shot)            # before the arena is touched (the reference's view fails)
        return super().__call__(support_data, query_data, n_way, n_shot)

    def forward(self, support_data: Dict[str, torch.Tensor], query_data: Dict[str, torch.Tensor], n_way: int,
                n_shot: int) -> Dict[str, torch.Tensor]:
        n_way, n_shot = int(n_way), int(n_shot)
        self._check_rows(support_data, n_way, n_shot)
        support = self._encode(support_data)
        query = self._encode(query_data)
        sf, prototypes, qf, distances, predictions = self.head(support, query, n_way, n_shot)
        return {"predictions": predictions, "distances": distances, "prototypes": prototypes,
                "support_features": sf, "query_features": qf}


class RobustMultimodalModel(_FusionBase):
    """Reference :365-450: ``base_model = MultimodalEmotionModel(config)``, ``{text,audio,video}_only_classifier``
    (d -> C) and ``modality_predictor`` (Linear(3d, d), ReLU, Linear(d, 3), Sigmoid); state_dict keys and shapes are the
    reference's.  ``forward`` returns the base model's outputs plus ``robust_prediction``, ``modality_availability``,
    ``individual_predictions`` {text, audio, video} and ``modality_weights``, computed from the base model's returned
    features (after ``ModalityDropout`` in training mode).  The weights are the predicted availability, or with
    ``available_modalities`` the constant indicator of the named modalities (unknown names ignored), normalised by their
    sum + 1e-8.

    Deliberate deviation: ``missing_modalities`` is accepted and passed to ``base_model`` (which zeroes those inputs).  The
    reference trainer calls the wrapper that way (advanced_trainer.py:583-588) and the reference class rejects it with a
    TypeError.  It does not select the weights: those still come from
    ``available_modalities`` or the predictor.

    An arena root (``_FusionBase``): the base model and the head share one parameter arena, hence one optimiser.  The
    predictor's hidden layer runs on the row linear (``ops.linear``, ReLU epilogue) over the concatenated features; the
    rest of the head is ``small_ops.robust_head``."""

    def __init__(self, config, backbones: Optional[Dict[str, nn.Module]] = None):
        super().__init__()
        self.base_model = MultimodalEmotionModel(config, backbones)
        self.config = config
        d, C = config.fusion_hidden_size, config.num_emotions
        self.text_only_classifier = nn.Linear(d, C)
        self.audio_only_classifier = nn.Linear(d, C)
        self.video_only_classifier = nn.Linear(d, C)
        self.modality_predictor = nn.Sequential(nn.Linear(d * 3, d), nn.ReLU(), nn.Linear(d, 3), nn.Sigmoid())

    def head(self, text_features: torch.Tensor, audio_features: torch.Tensor, video_features: torch.Tensor,
             available_modalities: Optional[List[str]] = None):
        """-> (modality_availability, text_pred, audio_pred, video_pred, modality_weights, robust_prediction)"""
        if not text_features.is_cuda:
            raise RuntimeError("mmfusion: the robust head runs on the GPU only (no CPU fallback)")
        cat = torch.cat([text_features.float(), audio_features.float(), video_features.float()], dim=-1)
        l0 = self.modality_predictor[0]
        h = ops.linear(cat, W(l0.weight), W(l0.bias), relu=True, out_f32=True)
        return sops.robust_head(text_features, audio_features, video_features, h, self, available_modalities)

    def forward(self, text_input: Dict[str, torch.Tensor], audio_input: torch.Tensor, video_input: torch.Tensor,
                available_modalities: Optional[List[str]] = None,
                missing_modalities: Optional[List[str]] = None) -> Dict[str, torch.Tensor]:
        output = self.base_model(text_input=text_input, audio_input=audio_input, video_input=video_input,
                                 missing_modalities=missing_modalities)
        a, pt, pa, pv, wn, y = self.head(output["text_features"], output["audio_features"], output["video_features"],
                                         available_modalities)
        output.update({"robust_prediction": y, "modality_availability": a,
                       "individual_predictions": {"text": pt, "audio": pa, "video": pv}, "modality_weights": wn})
        return output


def create_model(config, model_type: str = "standard") -> nn.Module:
    if model_type == "standard":
        return MultimodalEmotionModel(config)
    if model_type == "distillation":
        # reference :465-468: teacher and student from the same config (train_advanced.py:247-250 builds a half-size student
        # itself and calls KnowledgeDistillationModel directly); the teacher is expected to be loaded afterwards
        return KnowledgeDistillationModel(MultimodalEmotionModel(config), config)
    if model_type == "robust":
        # the reference factory returns RobustMultimodalModel(config) here; this factory keeps refusing as before (callers
        # and tests rely on it), the class itself is constructed directly
        raise NotImplementedError("model_type 'robust': construct RobustMultimodalModel(config) directly")
    if model_type == "few_shot":
        # the reference factory returns FewShotModel(MultimodalEmotionModel(config), config); this one keeps refusing as
        # before (callers and tests rely on it): construct the class directly
        raise NotImplementedError(f"model_type '{model_type}': construct FewShotModel(base_model, config) directly")
    raise ValueError(f"Unknown model type: {model_type}")


def load_checkpoint_file(checkpoint_path: str) -> Dict:
    """Read a reference-format checkpoint (advanced_trainer.py:396-411: epoch, model_state_dict,
    optimizer_state_dict, scheduler_state_dict, metrics, config) without executing anything from the file:
    ``weights_only=True``, with this package's own ``config`` dataclasses as the only extra classes the unpickler
    may construct — the reference pickles its ``ExperimentConfig`` instance under the same module path
    (``config.ExperimentConfig``), which is why a bare ``weights_only=True`` refuses its files.
    The reference's ``metrics`` entry holds sklearn results (advanced_trainer.py:245-261: ``f1_score`` /
    ``accuracy_score`` return ``numpy.float64``), which pickle as ``numpy._core.multiarray.scalar`` + ``numpy.dtype``:
    those reconstructors (data only, no code) and the float / int dtype classes are allowed too.
    A file that needs any other class is refused with torch's error."""
    import config as _cfg
    import numpy as _np
    allow = [getattr(_cfg, n) for n in ("ModelConfig", "DataConfig", "ExperimentConfig") if hasattr(_cfg, n)]
    allow.append(_np.dtype)
    for modname in ("numpy._core.multiarray", "numpy.core.multiarray"):      # numpy >= 2 / numpy 1.x pickles
        try:
            mod = __import__(modname, fromlist=["scalar"])
            # torch matches allowed globals by the (module, name) the pickle names: register under both spellings
            allow.append((mod.scalar, f"{modname}.scalar"))
        except (ImportError, AttributeError):
            pass
    for tname in ("float64", "float32", "int64", "int32", "bool_"):
        allow.append(type(_np.dtype(getattr(_np, tname))))
    with torch.serialization.safe_globals(allow):
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    return ckpt if isinstance(ckpt, dict) and "model_state_dict" in ckpt else {"model_state_dict": ckpt}


def load_pretrained_model(checkpoint_path: str, config) -> MultimodalEmotionModel:
    """Reference ``load_pretrained_model`` (multimodal_model.py:472-485): {'model_state_dict': ...} or a bare
    state_dict, loaded through ``load_checkpoint_file`` (nothing in the file is executed)."""
    model = MultimodalEmotionModel(config)
    model.load_state_dict(load_checkpoint_file(checkpoint_path)["model_state_dict"])
    return model
