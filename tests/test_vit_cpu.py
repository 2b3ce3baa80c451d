"""CPU: the ViT restatement (tests/vit_ref.py) is pinned to HuggingFace's ``ViTModel`` — live where transformers is
installed, and through a captured vector (tests/golden/vit_tiny.npz, tools/capture_vit_golden.py) everywhere; and
``mmfusion.vit.NativeViT`` speaks HuggingFace's ``state_dict`` of both key generations (CPU tensors, no kernel runs)."""
import os

import numpy as np
import pytest
import torch

import vit_ref
from helpers import rel_err

TOL = 2e-5          # tests/test_oracle_golden.py's bound for restatement vs reference
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_tiny.npz")


def _hf_model(cfg, sd):
    transformers = pytest.importorskip("transformers")
    m = transformers.ViTModel(transformers.ViTConfig(**vit_ref.config_kwargs(cfg))).eval()
    m.load_state_dict(sd)
    return m


@pytest.mark.parametrize("which,n_images", [("tiny", 3), ("base", 2)])
def test_restatement_matches_huggingface(which, n_images):
    cfg = vit_ref.tiny_config() if which == "tiny" else vit_ref.base_config()
    sd = vit_ref.seeded_weights(cfg, seed=3)
    model = _hf_model(cfg, sd)
    x = torch.rand(n_images, cfg.num_channels, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        want = model(pixel_values=x).last_hidden_state
    got = vit_ref.vit_forward(sd, x, cfg, dtype=torch.float64)
    err = rel_err(got, want)
    print(f"vit_ref (fp64) vs HuggingFace fp32, {which}: {err:.3e}")
    assert err <= TOL
    cls = vit_ref.vit_forward(sd, x, cfg, dtype=torch.float64, cls_last_only=True)
    assert rel_err(cls, want[:, 0]) <= TOL


def _load_golden():
    z = np.load(GOLDEN)
    sd = {}
    for k in z.files:
        if k.startswith("q:"):
            sd[k[2:]] = torch.from_numpy(z[k].astype(np.float32)) * float(z["s:" + k[2:]])
        elif k.startswith("f:"):
            sd[k[2:]] = torch.from_numpy(z[k])
    return sd, torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["last_hidden_state"])


def test_restatement_matches_captured_huggingface_vector():
    cfg = vit_ref.tiny_config()
    sd, x, want = _load_golden()
    assert {k: tuple(v.shape) for k, v in sd.items()} == vit_ref.hf_keys(cfg)
    assert os.path.getsize(GOLDEN) <= 746560                      # no larger than the largest fixture beside it
    got, probs = vit_ref.vit_forward(sd, x, cfg, dtype=torch.float64, return_probs=True)
    assert rel_err(got, want) <= TOL
    # the captured weights make the softmax matter: some attention row is far from uniform (a broken softmax would not pass)
    T = probs.shape[-1]
    assert float(probs.max()) >= 5.0 / T, float(probs.max())
    uniform = vit_ref.vit_forward(sd, x, cfg, dtype=torch.float64)       # sanity of the claim: zeroed q gives a different result
    sd0 = dict(sd)
    for i in range(cfg.num_hidden_layers):
        sd0[f"layers.{i}.attention.q_proj.weight"] = torch.zeros_like(sd[f"layers.{i}.attention.q_proj.weight"])
        sd0[f"layers.{i}.attention.q_proj.bias"] = torch.zeros_like(sd[f"layers.{i}.attention.q_proj.bias"])
    assert rel_err(vit_ref.vit_forward(sd0, x, cfg, dtype=torch.float64), uniform) > 100 * TOL


def test_bf16_storage_switch_rounds_and_stays_close():
    cfg = vit_ref.tiny_config()
    sd = vit_ref.seeded_weights(cfg, seed=5)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(6))
    exact = vit_ref.vit_forward(sd, x, cfg, dtype=torch.float64)
    stored = vit_ref.vit_forward(sd, x, cfg, bf16_storage=True, dtype=torch.float64)
    assert torch.equal(stored, stored.to(torch.bfloat16).to(torch.float64))          # the result itself is a stored value
    err = float((stored - exact).norm() / exact.norm())
    assert 1e-4 < err < 2e-2, err


def _native(cfg):
    from mmfusion.vit import NativeViT
    return NativeViT(**vit_ref.config_kwargs(cfg))


def test_native_vit_state_dict_is_huggingface_5x_surface():
    cfg = vit_ref.tiny_config()
    m = _native(cfg)
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(mine.items()) == list(vit_ref.hf_keys(cfg).items())                   # names, shapes and order
    assert all(not p.requires_grad for p in m.parameters())
    assert m.config.hidden_size == cfg.hidden_size
    transformers = pytest.importorskip("transformers")
    hf = transformers.ViTModel(transformers.ViTConfig(**vit_ref.config_kwargs(cfg)))
    assert list(mine.items()) == [(k, tuple(v.shape)) for k, v in hf.state_dict().items()]
    assert len(_native(vit_ref.base_config()).state_dict()) == 200


@pytest.mark.parametrize("generation", [5, 4])
def test_native_vit_state_dict_round_trip(generation):
    from mmfusion.vit import hf_key_to_v4, hf_key_to_v5
    cfg = vit_ref.tiny_config()
    sd = vit_ref.seeded_weights(cfg, seed=7)
    src = sd if generation == 5 else {hf_key_to_v4(k): v for k, v in sd.items()}
    if generation == 4:
        assert "encoder.layer.1.attention.attention.query.weight" in src and "encoder.layer.0.attention.output.dense.bias" in src
        assert "encoder.layer.0.intermediate.dense.weight" in src and "encoder.layer.1.output.dense.weight" in src
        assert "encoder.layer.0.layernorm_before.weight" in src and not any(k.startswith("layers.") for k in src)
        assert {hf_key_to_v5(k) for k in src} == set(sd)
    m = _native(cfg)
    res = m.load_state_dict(src)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.hf_state_dict(generation)
    assert list(back) == list(src)
    for k, v in src.items():
        assert torch.equal(back[k], v), k
    # q / k / v are fused for the kernel
    d = cfg.hidden_size
    assert m.l0_qkv_w.shape == (3 * d, d) and torch.equal(m.l0_qkv_w[d:2 * d], sd["layers.0.attention.k_proj.weight"])
    # strict loading still reports what does not fit
    bad = dict(src)
    bad["nonsense.weight"] = torch.zeros(1)
    del bad["layernorm.bias"]
    with pytest.raises(RuntimeError, match="nonsense.weight"):
        _native(cfg).load_state_dict(bad)
    bad = dict(src)
    bad["layernorm.weight"] = torch.zeros(3)
    with pytest.raises(RuntimeError, match="size mismatch"):
        _native(cfg).load_state_dict(bad)


@pytest.mark.parametrize("generation", [5, 4])
def test_checkpoint_keys_under_video_encoder_prefix_load(generation, tmp_path):
    """``video_encoder.vit.*`` of a reference checkpoint, either key generation, through ``mmfusion.train.load_checkpoint``"""
    from mmfusion.train import load_checkpoint
    from mmfusion.vit import hf_key_to_v4
    cfg = vit_ref.tiny_config()
    sd = vit_ref.seeded_weights(cfg, seed=8)

    class _Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.vit = _native(cfg)
            self.projection = torch.nn.Linear(4, 4)

    class _Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.video_encoder = _Enc()

    model = _Model()
    state = {"video_encoder.vit." + (k if generation == 5 else hf_key_to_v4(k)): v for k, v in sd.items()}
    state.update({"video_encoder.projection." + k: v.detach().clone() + 1 for k, v in model.video_encoder.projection.state_dict().items()})
    path = str(tmp_path / "ckpt.pth")
    torch.save({"epoch": 3, "model_state_dict": state, "optimizer_state_dict": {}, "scheduler_state_dict": {}, "metrics": {},
                "config": None}, path)
    ckpt = load_checkpoint(path, model)
    assert ckpt["epoch"] == 3
    got = model.video_encoder.vit.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v), k


def test_native_vit_refuses_unsupported_sizes():
    from mmfusion.vit import NativeViT
    with pytest.raises(ValueError, match="head_dim"):
        NativeViT(hidden_size=256, num_attention_heads=8)
    with pytest.raises(ValueError, match="LayerNorm"):
        NativeViT(hidden_size=384, num_attention_heads=6)
    with pytest.raises(ValueError, match="patch_size"):
        NativeViT(image_size=224, patch_size=14)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native(vit_ref.tiny_config())(torch.zeros(1, 3, 64, 64))
