"""Per-modality encoder projection tails — drop-in names for the reference's ``models/encoders.py``.

In scope: everything *after* the pretrained backbone —
pool -> optional ``AdapterLayer`` -> ``projection`` Linear(hidden -> fusion_hidden_size) -> dropout
(reference encoders.py:86-98, :151-161, :232-245), plus ``AdapterLayer`` (:254-277) and
``ModalityDropout`` (:280-321).  The projections, the adapter GEMMs and the temporal / facial
self-attention heads run on the HIP kernels (``mmfusion.ops``).

The HuggingFace backbones themselves (DeBERTa-v3 / Wav2Vec2 / ViT, reference :20,116,179) are third-party pretrained
models fetched by name.  All three have native forms on the HIP kernels that need no network (below), frozen by default.  The
text backbone has the gradient with respect to its input embeddings, which is what prompt tuning needs; all three can train their top
layers (``config.text_backbone_trainable_layers`` / ``config.video_backbone_trainable_layers`` /
``config.audio_backbone_trainable_layers``).  The encoders take a ``backbone`` argument:
  * ``backbone=None`` (default) reproduces the reference: ``from_pretrained(config.*_model_name)``;
  * any ``nn.Module`` returning an object with ``.last_hidden_state`` is used as is;
  * ``config.video_backbone = "native"`` (dynamic attribute, ``VideoEncoder`` only) builds ``mmfusion.vit.NativeViT``: the
    ViT on the HIP kernels, which takes HuggingFace ``state_dict``s and needs no network.  Frozen unless
    ``config.video_backbone_trainable_layers`` (dynamic attribute; default 0) is ``k`` > 0: the top ``k`` layers and the final
    LayerNorm then train, as the reference's optimiser trains ``video_encoder.vit``; ``"all"``: every layer and the embeddings;
  * ``config.audio_backbone = "native"`` (dynamic attribute, ``AudioEncoder`` only) builds ``mmfusion.wav2vec2.NativeWav2Vec2``
    the same way: the base-family Wav2Vec2 (feature-extractor convolutions, positional convolution, post-LN layers) or, with
    ``config.audio_backbone_kwargs = mmfusion.wav2vec2.FAMILIES["large-lv60"]``'s three switches, the layer-norm family (at widths
    512 / 768 here: the temporal attention's 8 heads have no form for the head_dim 128 of a 1024-wide backbone yet).  Frozen
    unless ``config.audio_backbone_trainable_layers`` (dynamic attribute; default 0) is ``k`` > 0: the top ``k`` layers then
    train; ``"all"``: every layer and the front end above the feature-extractor convolutions (feature projection, positional
    convolution, encoder LayerNorm), which stay frozen as under HuggingFace's ``freeze_feature_encoder()``; ``"full"``: the
    feature-extractor convolutions and layer 0's GroupNorm as well, every parameter the reference's optimiser trains.
    ``config.audio_backbone_regularisation`` (dynamic attribute; default 0: off) switches HuggingFace's training-mode regularisers
    on: ``True`` for wav2vec2-base-960h's dropouts, LayerDrop and SpecAugment time mask, which is what the reference trains under, or
    a dict of ``NativeWav2Vec2.set_regularisation``'s names; they act in ``train()`` while the backbone has something to train;
  * ``config.audio_backbone = "native-wavlm"`` builds ``mmfusion.wavlm.NativeWavLM`` the same way (sizes and
    ``audio_backbone_kwargs`` as for ``"native"``): WavLM-base / base-plus, whose attention adds a gated relative position bias, on
    a fused HIP kernel.  A frozen forward: ``audio_backbone_trainable_layers`` > 0 or ``audio_backbone_regularisation`` on raise
    that class's refusal at construction;
  * ``config.audio_backbone = "native-whisper"`` builds ``mmfusion.whisper.NativeWhisperEncoder`` (``d_model`` =
    ``audio_hidden_size``, the rest from ``audio_backbone_kwargs`` in ``WhisperConfig``'s names): Whisper's encoder, which takes the
    same 16 kHz waveform and makes its log-mel features on the device.  Widths 512 (base) and 768 (small): the temporal attention's
    8 heads have no form for the other families' head_dim.  Frozen, as ``"native-wavlm"`` is, with the same refusals;
  * ``config.text_backbone = "native"`` (dynamic attribute, ``TextEncoder`` only) builds ``mmfusion.deberta.NativeDeberta`` the
    same way: the DeBERTa-v3 family (disentangled relative-position attention with a padding mask), from raw token ids or,
    on the prompt route, from input embeddings.  On that route, with grad mode on and ``prompt_embeddings.requires_grad``, the
    backbone is called differentiably and ``prompt_embeddings`` trains through the frozen layers, as it does through
    HuggingFace's model in the reference (:49-71).  Frozen unless ``config.text_backbone_trainable_layers`` (dynamic attribute;
    default 0) is ``k`` > 0: the top ``k`` layers then train; ``"all"``: every layer and the embedding side (word embeddings,
    embedding LayerNorm, relative embeddings, encoder LayerNorm), which is every parameter the reference's optimiser steps; on
    the prompt route the word embeddings then train through ``word_embeddings(input_ids)`` as well.
    ``config.text_backbone_dropout`` (dynamic attribute; default 0: off) switches the backbone's training-mode dropout on:
    ``True`` for HuggingFace's 0.1 / 0.1, which is what the reference trains under, or a pair (hidden, attention); it acts while
    the encoder is in ``train()`` and the backbone has something to train, never under ``eval()``;
  * ``config.text_backbone = "native-bert"`` / ``"native-roberta"`` builds ``mmfusion.bert.NativeBert`` / ``NativeRoberta`` the same
    way (sizes and ``text_backbone_kwargs`` as for ``"native"``): the BERT family with absolute positions, whose attention honours
    the key padding mask on a fused HIP kernel; ``model_type`` contains "bert", so the CLS row is pooled as in the reference (:87).
    A frozen forward: ``text_backbone_trainable_layers`` > 0, ``text_backbone_dropout`` on, or prompt embeddings that require a
    gradient in grad mode raise that class's refusal;
  * ``config.feature_inputs = True`` (dynamic attribute) builds no backbone at all: the ``forward``
    inputs are then precomputed backbone features ``(B, T, hidden)`` — the synthetic-feature route
    of BASELINE.json's configs.
``VideoEncoder.forward`` also takes decoded frames, uint8 ``(B, frames, Hs, Ws, 3)`` of any size, with an optional
``video_aug`` (``mmfusion.prep.VideoAug``): the native ViT resizes them straight into its patch matrix, any other backbone
receives ``mmfusion.prep.prepare_video``'s f32 tensor at ``config.video_frame_size``, read as (height, width).
The video BiLSTM (reference :183-190,233) runs on the HIP path too (``mmfusion.lstm_ops``: grouped MFMA GEMMs for the
input projections, one persistent launch per layer for the 30 sequential steps of both directions); the
``torch.nn.LSTM`` module is only the parameter container (state_dict keys ``temporal_lstm.weight_ih_l0`` ...).
The audio / video heads return the head-averaged ``attention_weights`` (B, T, T) like the reference
(:152-154,236-238; no gradient); ``config.encoder_attention_weights = False`` (dynamic attribute) skips that kernel.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from mmfusion import ops, prep
from mmfusion.bert import NativeBert, NativeRoberta
from mmfusion.deberta import NativeDeberta
from mmfusion.ops import AttnSpec, W
from mmfusion.vit import NativeViT
from mmfusion.wav2vec2 import NativeWav2Vec2
from mmfusion.wavlm import NativeWavLM
from mmfusion.whisper import NativeWhisperEncoder
from .fusion_layers import _FusionBase, _MHAParams, _as_rows, _p, _wb


def _feature_mode(config) -> bool:
    return bool(getattr(config, "feature_inputs", False))


def _load_backbone(kind: str, name: str):
    """Reference behaviour (encoders.py:20,116,179).  Needs the HF weights on disk or a network."""
    from transformers import AutoModel, ViTModel, Wav2Vec2Model
    cls = {"text": AutoModel, "audio": Wav2Vec2Model, "video": ViTModel}[kind]
    return cls.from_pretrained(name)


def _square(size) -> int:
    if not isinstance(size, int) and len(set(size)) != 1:
        raise ValueError(f"the native ViT backbone takes square frames, not {tuple(size)}")
    return size if isinstance(size, int) else size[0]


# kind -> (its native class, the sizes it takes from the config).  ``config.<kind>_backbone = "native"`` builds the class with its
# family's base sizes otherwise (``config.<kind>_backbone_kwargs``, a dict, overrides any of them); weights come from
# ``load_state_dict`` / a checkpoint, nothing is fetched.
_NATIVE = {
    "text": (NativeDeberta, lambda c: dict(hidden_size=c.text_hidden_size)),
    "audio": (NativeWav2Vec2, lambda c: dict(hidden_size=c.audio_hidden_size)),
    "video": (NativeViT, lambda c: dict(hidden_size=c.video_hidden_size, image_size=_square(c.video_frame_size))),
}
# (kind, ``config.<kind>_backbone``) -> the same pair for a kind's further native models, handled as "native" is
_NATIVE_OTHER = {
    ("audio", "native-wavlm"): (NativeWavLM, lambda c: dict(hidden_size=c.audio_hidden_size)),
    ("audio", "native-whisper"): (NativeWhisperEncoder, lambda c: dict(d_model=c.audio_hidden_size)),
    ("text", "native-bert"): (NativeBert, lambda c: dict(hidden_size=c.text_hidden_size)),
    ("text", "native-roberta"): (NativeRoberta, lambda c: dict(hidden_size=c.text_hidden_size)),
}


def _backbone(config, kind: str, given: Optional[nn.Module]):
    """-> (module | None, hidden_size, native).  ``feature_inputs`` beats everything (no backbone); an explicit ``backbone=`` beats
    the config switch and is never ``native``; then ``config.<kind>_backbone == "native"``; else the reference's ``from_pretrained``."""
    if _feature_mode(config):
        return None, getattr(config, kind + "_hidden_size"), False
    choice = getattr(config, kind + "_backbone", None)
    native = given is None and (choice == "native" or (kind, choice) in _NATIVE_OTHER)
    if native:
        cls, sizes = _NATIVE[kind] if choice == "native" else _NATIVE_OTHER[(kind, choice)]
        given = cls(**{**sizes(config), **(getattr(config, kind + "_backbone_kwargs", None) or {})})
    elif given is None:
        given = _load_backbone(kind, getattr(config, kind + "_model_name"))
    return given, given.config.hidden_size, native


def _backbone_dropout(value) -> Tuple[float, float]:
    """``config.text_backbone_dropout`` (dynamic attribute) -> (hidden, attention) probabilities of the native backbone's
    training-mode dropout: absent, 0 or False: off; True: HuggingFace's 0.1 / 0.1 for deberta-v3-base, what the reference trains
    with; a pair: those values (``NativeDeberta.set_dropout`` checks them)"""
    if value is True:
        return 0.1, 0.1
    if value is False or value is None or (isinstance(value, (int, float)) and value == 0):
        return 0.0, 0.0
    if isinstance(value, (tuple, list)) and len(value) == 2:
        return value[0], value[1]
    raise ValueError(f"text_backbone_dropout={value!r}: 0 (off), True (0.1 / 0.1) or a pair (hidden, attention)")


def _audio_regularisation(value) -> dict:
    """``config.audio_backbone_regularisation`` (dynamic attribute) -> the settings of ``NativeWav2Vec2.set_regularisation``: absent,
    0 or False: all off; True: wav2vec2-base-960h's training regime (``mmfusion.wav2vec2.REG_960H``: the four dropouts and layerdrop
    0.1, mask_time_prob 0.05 / length 10 / min 2), what the reference trains with; a dict of those names: its values over all-off
    (``set_regularisation`` checks them)"""
    from mmfusion.wav2vec2 import REG_960H, REG_NAMES
    off = {**{n: 0.0 for n in REG_NAMES}, "mask_time_length": 10, "mask_time_min_masks": 2}
    if value is True:
        return dict(REG_960H)
    if value is None or value is False or (isinstance(value, (int, float)) and value == 0):
        return off
    if isinstance(value, dict) and value and all(isinstance(k, str) for k in value):
        return {**off, **value}
    raise ValueError(f"audio_backbone_regularisation={value!r}: 0 (off), True (wav2vec2-base-960h's values) or a dict of "
                     f"{', '.join(REG_NAMES)}")


def _run_backbone(fn, native: bool, *args, input_grad: bool = False, **kw):
    """``fn(*args, **kw)``, under ``no_grad`` iff the backbone is the native one: that one is frozen.  ``input_grad``: the caller
    wants a gradient through it (``NativeDeberta`` with ``inputs_embeds``: the prompt route; or any native backbone with trainable
    top layers), so a native backbone is called in the caller's grad mode too"""
    with torch.no_grad() if native and not input_grad else contextlib.nullcontext():
        return fn(*args, **kw)


class AdapterLayer(_FusionBase):
    """x + up(relu(down(x)))  (reference :254-277; N(0, 0.02) weights, zero biases).
    Both GEMMs run on the MFMA kernel; the residual add is the up-projection's epilogue."""

    def __init__(self, hidden_size: int, adapter_size: int):
        super().__init__()
        self.down_project = nn.Linear(hidden_size, adapter_size)
        self.up_project = nn.Linear(adapter_size, hidden_size)
        self.activation = nn.ReLU()
        self.dropout = nn.Dropout(0.1)
        nn.init.normal_(self.down_project.weight, std=0.02)
        nn.init.normal_(self.up_project.weight, std=0.02)
        nn.init.zeros_(self.down_project.bias)
        nn.init.zeros_(self.up_project.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        rows = _as_rows(x)
        h = ops.dropout(ops.linear(rows, *_wb(self.down_project), relu=True), _p(self, self.dropout.p), True)
        y = ops.linear(h, *_wb(self.up_project), residual=rows)
        return ops.to_f32(y).reshape(x.shape)


def _mha_mean_project(mha: _MHAParams, projection: nn.Linear, seq: torch.Tensor, p: float = 0.0,
                      want_weights: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """self-MHA over T -> mean(T) -> Linear  (reference :152-160 / :236-244).
    Returns (projected (B, d_fusion) fp32, attended (B, T, hidden) fp32, head-averaged weights (B, T, T) fp32 | None)."""
    B, T, hdim = seq.shape
    rows = _as_rows(seq)
    qkv = ops.linear(rows, mha.qkv_spec().w, mha.qkv_spec().b)
    weights = None
    if want_weights and ops.fp32_mode():
        # fp32 parity mode: qkv holds f32 rows, which the bf16 kernel below must not read — the head-averaged
        # softmax(q k^T / sqrt(dh)) as f32 torch arithmetic on the GPU (no gradient, like the kernel)
        with torch.no_grad():
            H, dh = mha.num_heads, mha.head_dim
            q = qkv[:, :hdim].reshape(B, T, H, dh).transpose(1, 2)
            k = qkv[:, hdim:2 * hdim].reshape(B, T, H, dh).transpose(1, 2)
            weights = torch.softmax((q * (dh ** -0.5)) @ k.transpose(-1, -2), dim=-1).mean(dim=1)
    elif want_weights and T <= 2048 and mha.head_dim % 8 == 0:
        from mmfusion import lib as _lib
        weights = torch.empty((B, T, T), dtype=torch.float32, device=qkv.device)
        _lib.check(_lib.load().mmf_attn_weights_mean(qkv.data_ptr(), weights.data_ptr(), B, T, mha.num_heads, mha.head_dim,
                                                     _lib.stream_ptr()))
    att = ops.attention_group([AttnSpec(B, T, T, q=(0, 0), k=(0, hdim), v=(0, 2 * hdim))],
                              mha.num_heads, mha.head_dim, [qkv], dropout_p=p)[0]
    attended = ops.linear(att, *_wb(mha.out_proj))
    pooled = ops.meanpool_cat([attended.view(B, T, hdim)])
    projected = ops.linear(pooled, *_wb(projection), out_f32=True, dropout_p=p)              # reference :161 / :245
    return projected, ops.to_f32(attended).view(B, T, hdim), weights


class TextEncoder(_FusionBase):
    def __init__(self, config, backbone: Optional[nn.Module] = None):
        super().__init__()
        self.config = config
        self.model, self.hidden_size, self._native = _backbone(config, "text", backbone)
        if self._native:      # fine-tune the native backbone (NativeDeberta.set_trainable_layers): the top k layers, "all": every
            k = getattr(config, "text_backbone_trainable_layers", 0)           # layer and the embeddings; 0: frozen
            if k == "all":
                self.model.set_trainable_layers(self.model.config.num_hidden_layers, embeddings=True)
            else:
                self.model.set_trainable_layers(int(k))
            self.model.set_dropout(*_backbone_dropout(getattr(config, "text_backbone_dropout", 0)))
        self.adapter = AdapterLayer(self.hidden_size, config.adapter_size) if hasattr(config, "adapter_size") else None
        self.prompt_embeddings = nn.Parameter(torch.randn(config.prompt_length, self.hidden_size)) \
            if hasattr(config, "prompt_length") else None
        self.projection = nn.Linear(self.hidden_size, config.fusion_hidden_size)
        self.dropout = nn.Dropout(config.fusion_dropout)

    def forward(self, input_ids, attention_mask, use_adapter: bool = False, use_prompt: bool = False
                ) -> Dict[str, torch.Tensor]:
        cls_pool = True
        if self.model is None:                       # feature mode: input_ids holds (B, T, hidden)
            sequence_output = input_ids
        else:
            B = input_ids.size(0)
            prompt_grad = False
            if use_prompt and self.prompt_embeddings is not None:        # reference :49-71
                prompt_grad = torch.is_grad_enabled() and self.prompt_embeddings.requires_grad
                pe = self.prompt_embeddings.unsqueeze(0).expand(B, -1, -1)
                emb = self.model.embeddings.word_embeddings(input_ids)
                pm = torch.ones(B, self.config.prompt_length, device=attention_mask.device, dtype=attention_mask.dtype)
                attention_mask = torch.cat([pm, attention_mask], dim=1)
                kw = dict(inputs_embeds=torch.cat([pe, emb], dim=1), attention_mask=attention_mask)
            else:
                kw = dict(input_ids=input_ids, attention_mask=attention_mask)
            tuned = self._native and self.model.trainable_layers > 0          # the backbone's own parameters train
            sequence_output = _run_backbone(self.model, self._native, input_grad=prompt_grad or tuned, **kw).last_hidden_state
            cls_pool = "bert" in getattr(self.model.config, "model_type", "")     # reference :87
        if use_adapter and self.adapter is not None:
            sequence_output = self.adapter(sequence_output)
        if cls_pool:
            pooled = sequence_output[:, 0]
        else:                                                              # reference :90-94
            m = attention_mask.unsqueeze(-1).to(sequence_output.dtype)
            pooled = (sequence_output * m).sum(1) / m.sum(1).clamp_min(1e-9)
        projected = ops.linear(_as_rows(pooled), *_wb(self.projection), out_f32=True,
                               dropout_p=_p(self, self.config.fusion_dropout))               # reference :97-98
        return {"features": projected, "sequence_output": sequence_output, "attention_mask": attention_mask}


class AudioEncoder(_FusionBase):
    def __init__(self, config, backbone: Optional[nn.Module] = None):
        super().__init__()
        self.config = config
        self.model, self.hidden_size, self._native = _backbone(config, "audio", backbone)
        if self._native:      # fine-tune the native backbone (NativeWav2Vec2.set_trainable_layers): the top k layers, "all": every
            k = getattr(config, "audio_backbone_trainable_layers", 0)          # layer and the front end; "full": the feature
            if k in ("all", "full"):                                           # extractor as well; 0: frozen
                self.model.set_trainable_layers(self.model.config.num_hidden_layers, front=True, feature_encoder=k == "full")
            else:
                self.model.set_trainable_layers(k)
            self.model.set_regularisation(**_audio_regularisation(getattr(config, "audio_backbone_regularisation", 0)))
        self.adapter = AdapterLayer(self.hidden_size, config.adapter_size) if hasattr(config, "adapter_size") else None
        self.temporal_attention = _MHAParams(self.hidden_size, 8)
        self.projection = nn.Linear(self.hidden_size, config.fusion_hidden_size)
        self.dropout = nn.Dropout(config.fusion_dropout)

    def forward(self, waveform, use_adapter: bool = False) -> Dict[str, torch.Tensor]:
        if self.model is None:                       # feature mode: waveform holds (B, T, hidden)
            seq = waveform
        else:
            tuned = self._native and self.model.trainable_layers > 0          # the backbone's own parameters train
            seq = _run_backbone(self.model, self._native, waveform, input_grad=tuned).last_hidden_state
        if use_adapter and self.adapter is not None:
            seq = self.adapter(seq)
        projected, attended, weights = _mha_mean_project(self.temporal_attention, self.projection, seq,
                                                         _p(self, self.config.fusion_dropout),
                                                         getattr(self.config, "encoder_attention_weights", True))
        return {"features": projected, "sequence_output": attended, "attention_weights": weights}


class VideoEncoder(_FusionBase):
    def __init__(self, config, backbone: Optional[nn.Module] = None):
        super().__init__()
        self.config = config
        self.vit, self.hidden_size, native = _backbone(config, "video", backbone)
        # the frozen route that runs the last layer for the CLS rows only.  Deliberately also for a NativeViT handed in as
        # ``backbone=`` (it always was): the one case where a given backbone is treated like the native one
        self._cls_route = native or isinstance(self.vit, NativeViT)
        if native:            # fine-tune the native backbone (NativeViT.set_trainable_layers): the top k layers, "all": every layer
            k = getattr(config, "video_backbone_trainable_layers", 0)          # and the embeddings; 0: frozen
            if k == "all":
                self.vit.set_trainable_layers(self.vit.config.num_hidden_layers, embeddings=True)
            else:
                self.vit.set_trainable_layers(k)
        self.temporal_lstm = nn.LSTM(self.hidden_size, self.hidden_size // 2, num_layers=2, batch_first=True,
                                     bidirectional=True, dropout=config.fusion_dropout)
        self.facial_attention = _MHAParams(self.hidden_size, 8)
        self.adapter = AdapterLayer(self.hidden_size, config.adapter_size) if hasattr(config, "adapter_size") else None
        self.projection = nn.Linear(self.hidden_size, config.fusion_hidden_size)
        self.dropout = nn.Dropout(config.fusion_dropout)

    def forward(self, video_frames, use_adapter: bool = False, video_aug=None) -> Dict[str, torch.Tensor]:
        if self.vit is None:                         # feature mode: (B, frames, hidden) CLS features
            frame_features = video_frames
        elif video_frames.dtype == torch.uint8:      # decoded frames (B, frames, Hs, Ws, 3): prepared on the device (mmfusion/prep.py)
            B, n, hs, wsrc, c = video_frames.shape
            flat, aug = video_frames.reshape(-1, hs, wsrc, c), video_aug if video_aug is not None else prep.VideoAug()
            if self._cls_route:                      # straight into the ViT's patch matrix
                cls = _run_backbone(self.vit.cls_features, True, flat, aug=aug, input_grad=self.vit.trainable_layers > 0)
            else:
                pixels = prep.prepare_video(flat, self.config.video_frame_size, bgr=aug.bgr, live=aug.live,
                                            brightness=aug.brightness, flip=aug.flip)
                cls = self.vit(pixel_values=pixels).last_hidden_state[:, 0]
            frame_features = cls.view(B, n, -1)
        else:
            if video_aug is not None:
                raise ValueError("VideoEncoder: video_aug goes with uint8 (B, frames, Hs, Ws, 3) frames")
            B, n, c, h, w = video_frames.shape
            if self._cls_route:
                cls = _run_backbone(self.vit.cls_features, True, video_frames.reshape(-1, c, h, w), input_grad=self.vit.trainable_layers > 0)
            else:
                cls = self.vit(pixel_values=video_frames.view(-1, c, h, w)).last_hidden_state[:, 0]
            frame_features = cls.view(B, n, -1)
        if use_adapter and self.adapter is not None:
            frame_features = self.adapter(frame_features)
        from mmfusion import lstm_ops
        lstm_out = lstm_ops.bilstm(self.temporal_lstm, frame_features, _p(self, self.config.fusion_dropout))   # :233
        projected, attended, weights = _mha_mean_project(self.facial_attention, self.projection, lstm_out,
                                                         _p(self, self.config.fusion_dropout),
                                                         getattr(self.config, "encoder_attention_weights", True))
        return {"features": projected, "sequence_output": attended, "attention_weights": weights}


class ModalityDropout(nn.Module):
    """Per-sample Bernoulli keep-masks, p = dropout_rate, **no** 1/(1-p) rescale, at least one
    modality kept (reference :289-321).  On the GPU (2-D features) the masks come from the build's counter-based RNG and are
    drawn and applied by one kernel; the torch formulation serves CPU tensors, 3-D features and the fp32 parity mode."""

    def __init__(self, dropout_rate: float = 0.1):
        super().__init__()
        self.dropout_rate = dropout_rate

    def forward(self, text_features, audio_features, video_features, training: bool = True):
        if not training:
            return text_features, audio_features, video_features
        B, dev = text_features.size(0), text_features.device
        if (text_features.is_cuda and text_features.dim() == 2 and text_features.shape[1] % 4 == 0
                and text_features.shape == audio_features.shape == video_features.shape and not ops.fp32_mode()):
            # masks drawn and applied by ONE kernel from the build's counter-based RNG (csrc/loss.hip modality_dropout_kernel:
            # Bernoulli(1 - p) per (sample, modality), a sample with nothing left gets one modality back) — the torch formulation
            # below is ~16 launches forward and 6 backward for 3 x B numbers
            from mmfusion import small_ops as sops
            t, a, v, _ = sops.modality_dropout(text_features, audio_features, video_features, self.dropout_rate)
            return t, a, v
        keep = torch.rand(B, 3, device=dev) > self.dropout_rate
        # samples that lost all three modalities get one back at random (:308-314) — written without the
        # reference's data-dependent branch so that nothing synchronises with the host (hipGraph-capturable)
        choice = torch.nn.functional.one_hot(torch.randint(0, 3, (B,), device=dev), 3).bool()
        keep = torch.where(keep.any(dim=1, keepdim=True), keep, choice)
        k = keep.float()
        return text_features * k[:, 0:1], audio_features * k[:, 1:2], video_features * k[:, 2:3]
