"""GPU: decoded uint8 frames through ``NativeViT`` and ``VideoEncoder``.  The uint8 route writes the ViT's patch matrix straight
from the frames (``mmf_video_prepare_patches``); it must give the bits of the f32 route fed with ``prepare_video``'s tensor,
and the f32 route must be what it was."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import vit_ref  # noqa: E402


def _tiny_vit():
    from mmfusion.vit import NativeViT
    cfg = vit_ref.tiny_config()
    m = NativeViT(**vit_ref.config_kwargs(cfg))
    m.load_state_dict(vit_ref.seeded_weights(cfg, seed=51))
    return cfg, m.cuda().eval()


def _frames(*shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).cuda()


def _aug(n):
    from mmfusion.prep import VideoAug
    return VideoAug(bgr=True, live=(torch.arange(n) != 2).to(torch.uint8).cuda(),
                    brightness=torch.tensor([0.8, 1.2, 1.0])[torch.arange(n) % 3].cuda(),
                    flip=(torch.arange(n) % 2).to(torch.uint8).cuda())


@pytest.mark.parametrize("chunk", [160, 2])
def test_native_vit_uint8_frames_equal_prepared_f32(chunk):
    """also across chunks: the per-frame arrays are cut with the frames"""
    from mmfusion import prep
    cfg, m = _tiny_vit()
    m.chunk = chunk
    fr, aug = _frames(5, 37, 53, 3, seed=1), _aug(5)
    pixels = prep.prepare_video(fr, cfg.image_size, bgr=aug.bgr, live=aug.live, brightness=aug.brightness, flip=aug.flip)
    assert torch.equal(m.cls_features(fr, aug=aug), m.cls_features(pixels))
    assert torch.equal(m(fr, aug=aug).last_hidden_state, m(pixels).last_hidden_state)
    plain = prep.prepare_video(fr, cfg.image_size)
    assert torch.equal(m.cls_features(fr), m.cls_features(plain))                      # no aug: plain RGB frames
    assert not torch.equal(m.cls_features(fr), m.cls_features(fr, aug=aug))


def test_native_vit_f32_route_and_its_messages_are_unchanged():
    from helpers import BOUND_A, l2_rel
    cfg, m = _tiny_vit()
    x = torch.rand(3, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(4))
    want = vit_ref.vit_forward(vit_ref.seeded_weights(cfg, seed=51), x, cfg, bf16_storage=True, dtype=torch.float64)
    assert l2_rel(m(x.cuda()).last_hidden_state, want) <= BOUND_A
    with pytest.raises(ValueError, match=r"is not \(N, 3, 64, 64\) \(position embeddings are not interpolated\)"):
        m(torch.rand(2, 3, 32, 64, device="cuda"))
    with pytest.raises(TypeError, match="pixel_values must be float32, got torch.float16"):
        m(x.cuda().half())
    with pytest.raises(RuntimeError, match="GPU only"):
        m(x)
    with pytest.raises(ValueError, match="aug goes with uint8"):
        m(x.cuda(), aug=_aug(3))
    with pytest.raises(ValueError, match=r"is not \(N, Hs, Ws, 3\) decoded frames"):
        m.cls_features(_frames(2, 3, 37, 53, seed=5))
    with pytest.raises(RuntimeError, match="GPU only"):
        m.cls_features(_frames(2, 37, 53, 3, seed=5).cpu())


def test_video_encoder_uint8_frames_equal_prepared_f32():
    import config as cfgmod
    from mmfusion import prep
    from models.encoders import VideoEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout = 256, 0.0
    cfg.video_hidden_size, cfg.video_frame_size = 768, (32, 32)
    cfg.video_backbone = "native"
    cfg.video_backbone_kwargs = dict(num_hidden_layers=2, intermediate_size=1024)
    torch.manual_seed(4)
    enc = VideoEncoder(cfg)
    enc.vit.load_state_dict(vit_ref.seeded_weights(enc.vit.config, seed=52))
    enc = enc.cuda().eval()
    fr = _frames(2, 3, 37, 53, 3, seed=2)
    pixels = prep.prepare_video(fr.view(-1, 37, 53, 3), 32).view(2, 3, 3, 32, 32)
    with torch.no_grad():
        got, want = enc(fr), enc(pixels)
        assert torch.equal(got["features"], want["features"]) and got["features"].shape == (2, 256)
        aug = _aug(6)
        auged = prep.prepare_video(fr.view(-1, 37, 53, 3), 32, bgr=True, live=aug.live, brightness=aug.brightness, flip=aug.flip)
        assert torch.equal(enc(fr, video_aug=aug)["features"], enc(auged.view(2, 3, 3, 32, 32))["features"])
        # missing-modality zeroing (MultimodalEmotionModel.forward): zero frames prepare to zero pixels
        assert torch.equal(enc(torch.zeros_like(fr))["features"], enc(torch.zeros_like(pixels))["features"])
        with pytest.raises(ValueError, match="video_aug goes with uint8"):
            enc(pixels, video_aug=aug)
        with pytest.raises(ValueError, match="position embeddings are not interpolated"):
            enc(torch.rand(2, 3, 3, 48, 48, device="cuda"))


class _StubBackbone(torch.nn.Module):
    """a non-native backbone: records what it is given"""

    def __init__(self, hidden):
        super().__init__()
        self.config, self.seen = types.SimpleNamespace(hidden_size=hidden), None

    def forward(self, pixel_values):
        self.seen = pixel_values
        g = torch.Generator().manual_seed(3)
        return types.SimpleNamespace(last_hidden_state=torch.randn(pixel_values.shape[0], 2, self.config.hidden_size, generator=g).cuda())


def test_other_backbone_receives_the_prepared_f32_tensor():
    import config as cfgmod
    from mmfusion import prep
    from models.encoders import VideoEncoder
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_dropout, cfg.video_frame_size = 256, 0.0, (32, 40)
    stub = _StubBackbone(768)
    enc = VideoEncoder(cfg, backbone=stub).cuda().eval()
    fr, aug = _frames(2, 3, 37, 53, 3, seed=3), _aug(6)
    with torch.no_grad():
        out = enc(fr, video_aug=aug)
    want = prep.prepare_video(fr.view(-1, 37, 53, 3), (32, 40), bgr=True, live=aug.live, brightness=aug.brightness, flip=aug.flip)
    assert stub.seen.dtype == torch.float32 and stub.seen.shape == (6, 3, 32, 40) and torch.equal(stub.seen, want)
    assert out["features"].shape == (2, 256)
    with torch.no_grad():
        enc(want.view(2, 3, 3, 32, 40))
    assert stub.seen.shape == (6, 3, 32, 40) and torch.equal(stub.seen, want)          # f32 input goes through as before
