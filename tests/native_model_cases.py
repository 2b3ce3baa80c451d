"""The shared configurations of tests/test_native_model_gpu.py and tests/test_native_model_cpu.py: a ``MultimodalEmotionModel`` on
the three native backbones at the smallest shapes the encoder tests use, its inputs, and the pieces a whole model is compared with
(the stand-alone backbones and encoders, the ``feature_inputs`` twin).  Nothing here needs a GPU to import or to construct.

Shapes.  B = 2, ``fusion_hidden_size`` 256, the three hidden sizes 768; backbones of 2 layers with the ``*_backbone_kwargs`` of
``test_audio_encoder_steps_the_trainable_parameters``, ``test_video_encoder_steps_the_trainable_layer_and_serves_the_new_weights``
and ``test_text_encoder_steps_the_trainable_layer_and_serves_the_new_weights``.  That last test runs ``deberta_ref.tiny_config()``
at its own hidden size of 256 in 4 heads; at 768 the disentangled attention's one head width (64) needs 12 heads, so
``num_attention_heads`` is 12 here and every other entry is the tiny configuration's.  Weights are the seeded ones of
``deberta_ref`` / ``w2v_ref`` / ``vit_ref``; inputs a 3000-sample waveform (149 frames), 3 frames of 64 x 64 (17 tokens) and 12
tokens with the second item padded from token 8."""
import copy

import torch

import deberta_ref
import vit_ref
import w2v_ref

B, D, HIDDEN, LAYERS = 2, 256, 768, 2
TEXT_KW = {**{k: v for k, v in deberta_ref.config_kwargs(deberta_ref.tiny_config()).items() if k != "hidden_size"}, "num_attention_heads": 12}
AUDIO_KW = dict(num_hidden_layers=2, intermediate_size=512, conv_dim=(256, 256, 256), conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2),
                num_conv_pos_embeddings=16)
VIDEO_KW = dict(num_hidden_layers=2, intermediate_size=1024)
# the audio regularisers of a training call, span masking included; LayerDrop stays off: its skip pattern is drawn on the host
# from a generator of the module's own, so two models would not share it, and a graph capture refuses it
AUDIO_REG = dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, feat_proj_dropout=0.1, mask_time_prob=0.05,
                 mask_time_length=10, mask_time_min_masks=2)
BACKBONE_PREFIXES = ("text_encoder.model.", "audio_encoder.model.", "video_encoder.vit.")
KINDS = ("text", "audio", "video")


def config(fusion="hierarchical", k=1, dropout=0.0, backbone_dropout=False, feature_inputs=False):
    """``k``: the three ``*_backbone_trainable_layers`` (0, 1, ... or "all"); ``dropout``: ``fusion_dropout`` / ``graph_dropout``;
    ``backbone_dropout``: the text backbone's 0.1 / 0.1 and ``AUDIO_REG``"""
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.fusion_type = fusion
    cfg.fusion_hidden_size, cfg.fusion_num_heads = D, 4
    cfg.graph_hidden_size, cfg.graph_num_layers = D, 3
    cfg.fusion_dropout = cfg.graph_dropout = dropout
    cfg.text_hidden_size = cfg.audio_hidden_size = cfg.video_hidden_size = HIDDEN
    cfg.video_frame_size = (64, 64)
    cfg.encoder_attention_weights = False
    if feature_inputs:
        cfg.feature_inputs = True
        return cfg
    cfg.text_backbone = cfg.audio_backbone = cfg.video_backbone = "native"
    cfg.text_backbone_kwargs, cfg.audio_backbone_kwargs, cfg.video_backbone_kwargs = dict(TEXT_KW), dict(AUDIO_KW), dict(VIDEO_KW)
    cfg.text_backbone_trainable_layers = cfg.audio_backbone_trainable_layers = cfg.video_backbone_trainable_layers = k
    if backbone_dropout:
        cfg.text_backbone_dropout = True
        cfg.audio_backbone_regularisation = dict(AUDIO_REG)
    return cfg


def backbones(model):
    """{kind: the native backbone} of a ``MultimodalEmotionModel``"""
    return {"text": model.text_encoder.model, "audio": model.audio_encoder.model, "video": model.video_encoder.vit}


def encoders(model):
    return {"text": model.text_encoder, "audio": model.audio_encoder, "video": model.video_encoder}


def seed_backbones(model, seed=31):
    """the restatements' seeded weights into the three backbones -> {kind: that state dict}"""
    bb = backbones(model)
    sds = {"text": deberta_ref.seeded_weights(bb["text"].config, seed=seed), "audio": w2v_ref.seeded_weights(bb["audio"].config, seed=seed),
           "video": vit_ref.seeded_weights(bb["video"].config, seed=seed)}
    for kind in KINDS:
        bb[kind].load_state_dict(sds[kind])
    return sds


def base_model(cfg, seed=3):
    """a ``MultimodalEmotionModel`` of ``cfg`` on the CPU with seeded backbone weights; ``modality_dropout`` off (its rate is a
    constant of the constructor, and a seam test wants every item of every modality)"""
    from models.multimodal_model import MultimodalEmotionModel
    torch.manual_seed(seed)
    model = MultimodalEmotionModel(cfg)
    if not getattr(cfg, "feature_inputs", False):
        seed_backbones(model)
    model.modality_dropout.dropout_rate = 0.0
    return model


def pieces(model):
    """copies, made on the CPU before the model has an arena, of what the whole model is compared with ->
    ({kind: stand-alone encoder}, {kind: stand-alone backbone})"""
    enc = {kind: copy.deepcopy(e) for kind, e in encoders(model).items()}
    return enc, {kind: copy.deepcopy(b) for kind, b in backbones(model).items()}


def non_backbone_state(model, prefix=""):
    """the ``state_dict`` entries a ``feature_inputs`` twin has: everything outside the three backbones"""
    skip = tuple(prefix + p for p in BACKBONE_PREFIXES)
    return {k: v.detach().clone() for k, v in model.state_dict().items() if not k.startswith(skip)}


def twin_of(model, fusion="hierarchical", dropout=0.0):
    """the ``feature_inputs`` model with the whole model's non-backbone weights (on the CPU)"""
    from models.multimodal_model import MultimodalEmotionModel
    twin = MultimodalEmotionModel(config(fusion, dropout=dropout, feature_inputs=True))
    twin.load_state_dict(non_backbone_state(model))
    twin.modality_dropout.dropout_rate = 0.0
    return twin


def inputs(seed=32, n=B):
    """-> ({"input_ids", "attention_mask"}, waveform (n, 3000), frames (n, 3, 3, 64, 64), labels (n,)) on the CPU: 12 tokens with
    the last item padded from token 8"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, TEXT_KW["vocab_size"], (n, 12), generator=g)
    mask = torch.ones(n, 12, dtype=torch.long)
    mask[-1, 8:] = 0
    ids[-1, 8:] = 0
    wave = 0.5 * torch.randn(n, 3000, generator=g)
    frames = torch.rand(n, 3, 3, 64, 64, generator=g)
    labels = torch.randint(0, 7, (n,), generator=g)
    return {"input_ids": ids, "attention_mask": mask}, wave, frames, labels


def is_backbone(name: str) -> bool:
    """whether ``name`` (of ``named_parameters()``, under any wrapper prefix) is a native backbone's parameter"""
    return any(p in name for p in BACKBONE_PREFIXES)
