"""CPU: a forward pass of a frozen backbone (mmfusion/backbone.py) leaves nothing on the module.  What its launches need
beyond the workspace travels as arguments.  Held twice: a ``forward`` that is refused (CPU tensors, which every one of them
refuses before it launches anything) leaves ``vars(model)`` as it was, and so does a whole forward on CPU tensors with every
launch replaced by a stub, except for the two places a forward may write: the workspace and the ``_derived`` cache."""
import contextlib

import pytest
import torch

import deberta_ref
import vit_ref
import w2v_ref


def _tensors(m):
    return {k for k, v in vars(m).items() if isinstance(v, torch.Tensor)}


def _cases():
    from mmfusion.deberta import NativeDeberta
    from mmfusion.vit import NativeViT
    from mmfusion.wav2vec2 import NativeWav2Vec2
    v, w, t = vit_ref.tiny_config(), w2v_ref.tiny_config(), deberta_ref.tiny_config()
    ids = torch.ones(2, 8, dtype=torch.int64)
    return [
        (NativeViT(**vit_ref.config_kwargs(v)), [lambda m: m(torch.zeros(2, v.num_channels, v.image_size, v.image_size)),
                                                 lambda m: m.cls_features(torch.zeros(2, v.num_channels, v.image_size, v.image_size))]),
        (NativeWav2Vec2(**w2v_ref.config_kwargs(w)), [lambda m: m(torch.zeros(2, 4000))]),
        (NativeDeberta(**deberta_ref.config_kwargs(t)), [lambda m: m(input_ids=ids, attention_mask=torch.ones(2, 8)),
                                                         lambda m: m(inputs_embeds=torch.zeros(2, 8, t.hidden_size), attention_mask=torch.ones(2, 8))]),
    ]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["vit", "wav2vec2", "deberta"])
def test_a_refused_forward_leaves_no_state_on_the_module(which):
    model, calls = _cases()[which]
    keys, tensors = set(vars(model)), _tensors(model)
    assert not hasattr(model, "_call")
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU only"):
            call(model)
        assert set(vars(model)) == keys and _tensors(model) == tensors
        assert model._ws is None and not model._cache                  # nor anything in the two places a forward may write


def _stub_launches(monkeypatch):
    """every launch the backbones make becomes a no-op, and the GPU-only refusal is lifted: the Python of a forward runs whole"""
    from mmfusion import arena, backbone, lib, ops
    nothing = lambda *a, **k: None
    for name in ("layernorm_fwd_grouped", "attn_fwd_grouped", "bias_gelu", "vit_patchify", "vit_embed_tokens", "w2v_conv0_stats",
                 "w2v_conv0_norm_gelu", "w2v_gelu_window", "w2v_posconv", "deberta_embed", "deberta_attn_fwd"):
        monkeypatch.setattr(lib, name, nothing)
    monkeypatch.setattr(lib, "_Timed", lambda *a, **k: contextlib.nullcontext())
    for name in ("gemm", "gemm_group"):
        monkeypatch.setattr(ops, name, nothing)
    monkeypatch.setattr(ops, "shadow", lambda p: p.detach())
    monkeypatch.setattr(arena, "ensure", nothing)
    monkeypatch.setattr(backbone.FrozenBackbone, "_check_input", nothing)
    monkeypatch.setattr(backbone.FrozenBackbone, "_widen", staticmethod(nothing))


@pytest.mark.parametrize("which", [0, 1, 2], ids=["vit", "wav2vec2", "deberta"])
def test_a_whole_forward_writes_only_the_workspace_and_the_derived_cache(which, monkeypatch):
    _stub_launches(monkeypatch)
    model, calls = _cases()[which]
    before = dict(vars(model))
    for call in calls:
        call(model)
        after = vars(model)
        assert set(after) == set(before) and _tensors(model) == set()
        changed = {k for k in before if after[k] is not before[k]}
        assert changed == {"_ws"} and model._ws["chunk"] == model.chunk          # (_cache and DeBERTa's index table are filled in place)
        assert set(model._cache) <= {"pos", "pos_w16"}
