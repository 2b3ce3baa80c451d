"""GPU: the input-preparation kernels (csrc/prep.hip) against their float64 restatement tests/prep_ref.py.

Bounds.  Video, 2e-6 absolute: outputs lie in [0, 1], the source coordinates are exact integers and the value is five f32
operations on numbers of at most 255 (three fused multiply-adds and two multiplies: a few 2^-24 relative each).  Resampling,
2e-5 absolute for |x| <= 1: at most 2 width (20 .. 38) live taps accumulated in f32 against an f32-rounded table.
Augmentation, 2e-5 absolute: one f32 interpolation of values of order 1 plus 0.01 times a Box-Muller draw whose f32 logarithm,
square root and cosine are good to about 1e-6.  The patch form is compared bit for bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import prep_ref  # noqa: E402
from helpers import _lib  # noqa: E402

BF16 = torch.bfloat16
VIDEO_TOL, RESAMPLE_TOL, AUGMENT_TOL = 2e-6, 2e-5, 2e-5
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -3, -5


def _frames(N, Hs, Ws, seed):
    """random bytes with both extremes present, so brightness 1.2 clamps and 0 stays 0"""
    fr = torch.randint(0, 256, (N, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    if Hs * Ws > 1:
        fr[:, 0, 0, :] = 255
        fr[:, -1, -1, :] = 0
    return fr


def _options(N):
    """N = 5: a dead frame in the middle, brightness on both sides of 1, some frames flipped; N = 1: every array absent"""
    if N == 1:
        return {}
    assert N == 5
    return dict(live=torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8), brightness=torch.tensor([0.8, 1.2, 1.2, 1.0, 1.2]),
                flip=torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8))


def _cuda(opts):
    return {k: v.cuda() for k, v in opts.items()}


# ---- video ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("dst", [32, 224])
@pytest.mark.parametrize("src", [(37, 53), (1, 1), (224, 224), (270, 480)])
def test_video_f32_form_against_float64(src, dst, N, bgr):
    from mmfusion import prep
    fr, opts = _frames(N, *src, seed=src[0] + dst + N), _options(N)
    got = prep.prepare_video(fr.cuda(), dst, bgr=bgr, **_cuda(opts)).cpu().double().numpy()
    want = prep_ref.video_prepare(fr.numpy(), dst, dst, bgr=bgr, **{k: v.numpy() for k, v in opts.items()})
    err = float(np.abs(got - want).max())
    print(f"video {src} -> {dst} N={N} bgr={bgr}: max abs err {err:.3e} (tol {VIDEO_TOL})")
    assert got.shape == (N, 3, dst, dst) and err <= VIDEO_TOL
    assert got.min() >= 0.0 and got.max() <= 1.0
    if N == 5:
        assert not got[2].any()                                                       # the dead frame
        assert src == (1, 1) or ((want[1] == 1.0).any() and got[1].max() == 1.0)      # the clamp acted
    if src == (dst, dst) and N == 1:
        ch = fr.numpy()[..., ::-1] if bgr else fr.numpy()
        assert np.abs(got - ch.transpose(0, 3, 1, 2) / 255.0).max() <= VIDEO_TOL      # same size: the bytes over 255


@pytest.mark.parametrize("size", [(12, 40), (20, 260), (8200, 260)])
def test_video_rectangular_output_and_tuple_size(size):
    """a last row band of 4 of the kernel's 8 rows; 260 columns: a second column tile, 4 wide; 8200 rows: 1025 x 2 = 2050 tiles,
    two more than the grid's 2048 workgroups, so the grid-stride loop takes a second turn"""
    from mmfusion import prep
    fr, flip = _frames(2, 19, 7, seed=9), torch.tensor([0, 1], dtype=torch.uint8)
    got = prep.prepare_video(fr.cuda(), size, flip=flip.cuda()).cpu().double().numpy()
    assert np.abs(got - prep_ref.video_prepare(fr.numpy(), *size, flip=flip.numpy())).max() <= VIDEO_TOL


@pytest.mark.parametrize("dst", [32, 224, 272])
def test_video_patch_form_is_bit_equal_to_patchify_of_the_f32_form(dst):
    """272: more than one of the kernel's 256-column tiles"""
    lib = _lib()
    from mmfusion import prep
    N, P = 5, 16
    fr, opts = _frames(N, 37, 53, seed=dst).cuda(), _cuda(_options(N))
    pixels = prep.prepare_video(fr, dst, bgr=True, **opts)
    want = torch.full((N * (dst // P) ** 2, 3 * P * P), float("nan"), dtype=BF16, device="cuda")
    lib.vit_patchify(pixels, want, N, 3, dst, dst, P)
    got = torch.full_like(want, float("nan"))
    lib.video_prepare(fr, got, dst, dst, P, True, opts["live"], opts["brightness"], opts["flip"])
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert bool(got.float().abs().max() > 0)


# ---- resampling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("rates,Ls", [((3, 2), 50), ((441, 160), 1767), ((1, 2), 50), ((1, 1), 50), ((1001, 1000), 2504)])
def test_audio_resample_against_float64(rates, Ls, C):
    """(1001, 1000): 1000 phases of 14 taps do not fit a workgroup's LDS, so the kernel's direct form runs; the other unequal pairs
    take the tile form, here with ONE tile per clip (test_audio_resample_across_tiles has more).  One batch with a clip shorter
    than the filter (5 samples), a length that is no multiple of ``orig`` and whose resampled length needs padding, and two
    clips whose resampled length exceeds ``out_len``"""
    from mmfusion import prep
    rs = prep.Resampler(*rates)
    lens = [5, Ls // 2 + 1, Ls, Ls - 2]
    assert rs.orig == 1 or lens[1] % rs.orig
    L = rs.out_len(lens[1]) + 3
    assert rs.out_len(lens[0]) < rs.out_len(lens[1]) < L < rs.out_len(lens[3])
    x = torch.rand(len(lens), C, Ls, generator=torch.Generator().manual_seed(Ls + C)) * 2 - 1
    got = prep.prepare_audio(x.cuda(), torch.tensor(lens), rs, L).cpu()
    want = prep_ref.resample(x.numpy(), lens, rates[0], rates[1], L)
    err = float(np.abs(got.double().numpy() - want).max())
    print(f"resample {rates} C={C}: max abs err {err:.3e} (tol {RESAMPLE_TOL}), width {rs.width}")
    assert got.shape == (len(lens), L) and got.dtype == torch.float32 and err <= RESAMPLE_TOL
    for b, n in enumerate(lens):
        assert not got[b, rs.out_len(n):].any()                                        # exactly 0 past the clip's end
        assert got[b, :min(L, rs.out_len(n))].abs().max() > 0


@pytest.mark.parametrize("rates,Ls,L,lens", [((441, 160), 9800, 3500, [9800, 4000, 5, 7000]), ((3, 2), 5000, 3200, [5000, 2000, 5, 3500])])
def test_audio_resample_across_tiles(rates, Ls, L, lens):
    """The tile form as the product runs it: a workgroup owns ceil(1024 / new) input blocks, 1120 outputs for 441 -> 160 and 1024
    for 3 -> 2, so ``L`` is three whole tiles and a part of a fourth.  Clip 0 fills every tile and is truncated; clip 1 ends
    inside tile 1, so tiles 2 and 3 lie wholly past its end (the zero-fill tiles); clip 2 ends inside tile 0; clip 3 ends inside
    tile 2.  Windows straddle every tile boundary."""
    from mmfusion import prep
    rs = prep.Resampler(*rates)
    tile = -(-1024 // rs.new) * rs.new
    ends = [min(L, rs.out_len(n)) for n in lens]
    assert L > 3 * tile and ends[0] == L and tile < ends[1] < 2 * tile and ends[2] < tile and 2 * tile < ends[3] < 3 * tile
    x = torch.rand(len(lens), 2, Ls, generator=torch.Generator().manual_seed(Ls)) * 2 - 1
    got = prep.prepare_audio(x.cuda(), torch.tensor(lens), rs, L).cpu()
    want = prep_ref.resample(x.numpy(), lens, rates[0], rates[1], L)
    err = np.abs(got.double().numpy() - want)
    print(f"resample {rates} over {-(-L // tile)} tiles: max abs err {err.max():.3e} (tol {RESAMPLE_TOL}); per tile "
          + ", ".join(f"{err[:, t:t + tile].max():.1e}" for t in range(0, L, tile)))
    assert err.max() <= RESAMPLE_TOL
    for b, end in enumerate(ends):
        assert not got[b, end:].any() and got[b, :end].abs().max() > 0
        for t in range(0, end, tile):                                                  # every live tile carries signal
            assert got[b, t:min(end, t + tile)].abs().max() > 0


def test_audio_resample_without_lengths_and_2d_input():
    from mmfusion import prep
    rs = prep.Resampler(48000, 16000)
    x = torch.rand(3, 100, generator=torch.Generator().manual_seed(7)) * 2 - 1
    got = prep.prepare_audio(x.cuda(), None, rs, 40).cpu().double().numpy()
    assert np.abs(got - prep_ref.resample(x.numpy()[:, None], None, 3, 1, 40)).max() <= RESAMPLE_TOL


# ---- augmentation -----------------------------------------------------------------------------------------------------
@pytest.fixture
def rng_state():
    """the device-resident dropout state, put back afterwards"""
    from mmfusion import ops
    saved = ops.rng_state().clone()
    yield ops.rng_state()
    ops.rng_state().copy_(saved)


def _augment(x, noise_on, stretch_len, site):
    lib = _lib()
    from mmfusion import ops
    out = torch.full_like(x, float("nan"))
    lib.audio_augment(x, out, noise_on, stretch_len, ops.rng_state().data_ptr(), site)
    return out


def test_audio_augment_against_float64(rng_state):
    from mmfusion import ops
    ops.seed_dropout(1234)
    L, site = 1000, 3
    stretch, noise = [800, 1000, 1200, 800, 1000, 1200], [1, 1, 1, 0, 0, 0]
    x = torch.rand(6, L, generator=torch.Generator().manual_seed(11)) * 2 - 1
    xd = x.cuda()
    nd, sd = torch.tensor(noise, dtype=torch.uint8).cuda(), torch.tensor(stretch, dtype=torch.int32).cuda()
    got = _augment(xd, nd, sd, site)
    want = prep_ref.augment(x.numpy(), noise, stretch, int(rng_state.item()), site)
    err = float(np.abs(got.cpu().double().numpy() - want).max())
    print(f"augment L={L}: max abs err {err:.3e} (tol {AUGMENT_TOL})")
    assert err <= AUGMENT_TOL
    assert not got[0, 800:].any() and not got[3, 800:].any()                          # everything past the stretched length
    assert torch.equal(got[4], xd[4])                                                  # no noise, no stretch: the input
    assert float((got[1] - xd[1]).abs().max()) > 1e-3                                  # noise alone is there
    assert torch.equal(_augment(xd, nd, sd, site), got)                                # same state, same site: same bits
    assert not torch.equal(_augment(xd, nd, sd, site + 1)[:3], got[:3])                # another site
    assert torch.equal(_augment(xd, None, sd, site)[3:], got[3:])                      # absent arrays are "off"
    assert torch.equal(_augment(xd, nd, None, site)[1], got[1])
    ops.seed_dropout(4321)
    other = _augment(xd, nd, sd, site)
    assert not torch.equal(other[:3], got[:3]) and torch.equal(other[3:], got[3:])


def test_audio_augment_noise_is_standard_normal(rng_state):
    from mmfusion import ops
    ops.seed_dropout(99)
    n = 1 << 16
    clean = (torch.rand(1, n, generator=torch.Generator().manual_seed(12)) * 0.2 - 0.1).cuda()
    out = _augment(clean, torch.ones(1, dtype=torch.uint8, device="cuda"), None, 1)
    z = ((out.double() - clean.double()) / 0.01).cpu().numpy()[0]
    print(f"noise over {n} samples: mean {z.mean():+.4f}, variance {z.var():.4f}")
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1) <= 5 * math.sqrt(2 / n)
    want = prep_ref.normal(prep_ref.rng_key(int(rng_state.item()), 1, 0), np.arange(n))
    assert np.abs(z - want).max() <= 1e-3                                              # z itself, through the f32 sum clean + 0.01 z


def test_prepare_audio_with_augmentation_is_two_launches_on_the_live_state(rng_state):
    """``prepare_audio`` with augmentation arrays = its own resampled output put through ``mmf_audio_augment`` at the next site"""
    from mmfusion import ops, prep
    ops.seed_dropout(5)
    rs = prep.Resampler(3, 2)
    x = (torch.rand(2, 2, 90, generator=torch.Generator().manual_seed(13)) * 2 - 1).cuda()
    lens = torch.tensor([90, 47])
    nd, sd = torch.tensor([1, 0], dtype=torch.uint8).cuda(), torch.tensor([50, 70], dtype=torch.int32).cuda()
    plain = prep.prepare_audio(x, lens, rs, 60)
    site = ops._site + 1
    got = prep.prepare_audio(x, lens, rs, 60, noise_on=nd, stretch_len=sd)
    assert ops._site == site
    want = prep_ref.augment(plain.cpu().double().numpy(), [1, 0], [50, 70], int(rng_state.item()), site)
    assert np.abs(got.cpu().double().numpy() - want).max() <= AUGMENT_TOL
    assert torch.equal(got, _augment(plain, nd, sd, site))


# ---- error paths ------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_launch_nothing():
    lib = _lib()
    from mmfusion import prep
    L, s = lib.load(), lib.stream_ptr()
    fr = _frames(1, 9, 9, seed=1).cuda()
    out = torch.full((3 * 16 * 16 + 8,), 7.0, device="cuda")
    outb = torch.full((3 * 16 * 16 + 8,), 7.0, dtype=BF16, device="cuda")
    video = lambda o, H, W: L.mmf_video_prepare(fr.data_ptr(), None, None, None, o, 1, 9, 9, H, W, 0, s)
    patches = lambda o, H, W, P: L.mmf_video_prepare_patches(fr.data_ptr(), None, None, None, o, 1, 9, 9, H, W, P, 0, s)
    assert video(out.data_ptr(), 16, 14) == E_UNSUPPORTED and b"mmf_video_prepare" in L.mmf_last_error()      # W % 4
    assert video(out.data_ptr() + 4, 16, 16) == E_ALIGN
    assert patches(outb.data_ptr() + 2, 16, 16, 16) == E_ALIGN
    for H, W, P in ((16, 16, 12), (16, 24, 16), (24, 16, 16)):
        assert patches(outb.data_ptr(), H, W, P) == E_UNSUPPORTED
    assert video(None, 16, 16) == E_SHAPE and video(out.data_ptr(), 0, 16) == E_SHAPE
    rs = prep.Resampler(3, 2)
    tab = rs.table("cuda")
    x, y = torch.ones(1, 1, 30, device="cuda"), torch.full((20,), 7.0, device="cuda")
    res = lambda t, elems, orig, new, width: L.mmf_audio_resample(x.data_ptr(), None, t, elems, y.data_ptr(), 1, 1, 30, 20, orig, new,
                                                                  width, s)
    assert res(tab.data_ptr(), tab.numel() - 1, 3, 2, rs.width) == E_SHAPE                                     # wrong table size
    assert res(tab.data_ptr(), tab.numel(), 3, 2, rs.width - 1) == E_SHAPE                                     # not this filter's width
    assert res(None, 0, 3, 2, rs.width) == E_SHAPE and res(tab.data_ptr(), tab.numel(), 2, 2, rs.width) == E_SHAPE
    assert L.mmf_audio_augment(y.data_ptr(), y.data_ptr(), None, None, None, 0, 1, 20, s) == E_UNSUPPORTED     # in place
    noise = torch.ones(1, dtype=torch.uint8, device="cuda")
    assert L.mmf_audio_augment(x.data_ptr(), y.data_ptr(), noise.data_ptr(), None, None, 0, 1, 20, s) == E_SHAPE   # noise without a state
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((outb == 7.0).all()) and bool((y == 7.0).all())
    with pytest.raises(ValueError, match="uint8"):
        prep.prepare_video(fr.float(), 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        prep.prepare_video(fr.cpu(), 16)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        prep.prepare_video(fr, (16, 14))
