"""CPU: tests/prep_ref.py (the float64 restatement the GPU tests of csrc/prep.hip compare against) pinned against torch's own
interpolation, the ``Resampler`` bank of mmfusion/prep.py pinned against the restatement's direct sum, and ``draw_augment``'s
policy against the reference's probabilities."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prep_ref
from mmfusion import prep


@pytest.mark.parametrize("src,dst", [((37, 53), (32, 32)), ((7, 5), (16, 16)), ((270, 480), (224, 224)), ((1, 1), (8, 8)),
                                     ((32, 32), (32, 32)), ((9, 64), (33, 7))])
def test_bilinear_ref_matches_torch_interpolate(src, dst):
    x = torch.rand(2, 3, *src, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    want = F.interpolate(x, size=dst, mode="bilinear", align_corners=False).numpy()
    got = prep_ref.bilinear(x.numpy(), *dst)
    assert np.abs(got - want).max() <= 1e-12


def test_video_ref_order_of_options():
    """bgr picks byte 2 - c; brightness clamps before the flip mirrors; a dead frame is zeros"""
    rng = np.random.default_rng(1)
    fr = rng.integers(0, 256, (3, 6, 8, 3), dtype=np.uint8)
    plain = prep_ref.video_prepare(fr, 6, 8)
    assert np.array_equal(plain, fr.transpose(0, 3, 1, 2) / 255.0)                  # same size: the identity
    got = prep_ref.video_prepare(fr, 6, 8, bgr=True, live=[1, 0, 1], brightness=[1.2, 1.2, 0.8], flip=[0, 1, 1])
    assert np.array_equal(got[0], np.clip(plain[0][::-1] * 1.2, 0, 1)) and got[0].max() == 1.0
    assert not got[1].any()
    assert np.array_equal(got[2], (plain[2][::-1] * 0.8)[..., ::-1])


@pytest.mark.parametrize("L,n", [(1000, 800), (1000, 1200), (1000, 1000), (37, 5), (5, 37)])
def test_stretch_ref_matches_torch_interpolate(L, n):
    x = torch.randn(2, L, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    want = F.interpolate(x[:, None], size=n, mode="linear", align_corners=False)[:, 0].numpy()
    got = prep_ref.augment(x.numpy(), None, [n, n], 0, 0)
    keep = min(n, L)
    assert np.abs(got[:, :keep] - want[:, :keep]).max() <= 1e-12
    assert not got[:, keep:].any()


def test_noise_ref_is_standard_normal_and_keyed():
    z = prep_ref.normal(prep_ref.rng_key(123 << 20, 1, 0), np.arange(1 << 16))
    n = z.size
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1) <= 5 * math.sqrt(2 / n)
    assert np.array_equal(z, prep_ref.normal(prep_ref.rng_key(123 << 20, 1, 0), np.arange(n)))
    for other in (prep_ref.rng_key(124 << 20, 1, 0), prep_ref.rng_key(123 << 20, 2, 0), prep_ref.rng_key(123 << 20, 1, 1)):
        assert not np.array_equal(z, prep_ref.normal(other, np.arange(n)))


def _polyphase(rs: prep.Resampler, x: np.ndarray, L: int) -> np.ndarray:
    """the bank applied as the kernel applies it: out[i new + j] = sum_k x[i orig + k - width] bank[j][k]"""
    bank = rs.bank.numpy()
    out = np.zeros(L)
    for m in range(min(L, rs.out_len(x.size))):
        i, j = divmod(m, rs.new)
        for k in range(bank.shape[1]):
            n = i * rs.orig + k - rs.width
            if 0 <= n < x.size:
                out[m] += x[n] * bank[j, k]
    return out


@pytest.mark.parametrize("rates", [(3, 2), (44100, 16000), (1, 2), (48000, 16000), (8000, 16000)])
def test_resampler_bank_reproduces_direct_sum(rates):
    rs = prep.Resampler(*rates)
    g = math.gcd(*rates)
    assert (rs.orig, rs.new) == (rates[0] // g, rates[1] // g)
    assert rs.width == math.ceil(6 * rs.orig / (min(rs.orig, rs.new) * 0.99))
    assert tuple(rs.bank.shape) == (rs.new, 2 * rs.width + rs.orig) and rs.bank.dtype == torch.float64
    assert rs.table("cpu").dtype == torch.float32 and rs.table("cpu") is rs.table("cpu")
    n_in = 3 * rs.orig + 7
    x = np.random.default_rng(3).standard_normal(n_in)
    L = rs.out_len(n_in) + 5
    want = prep_ref.resample(x[None, None], None, rates[0], rates[1], L)[0]
    assert np.abs(_polyphase(rs, x, L) - want).max() <= 1e-12
    assert not want[rs.out_len(n_in):].any()


def test_equal_rates_are_the_identity():
    rs = prep.Resampler(16000, 16000)
    assert (rs.orig, rs.new) == (1, 1) and rs.bank is None and rs.table("cpu") is None
    x = np.random.default_rng(4).standard_normal((2, 2, 50))
    got = prep_ref.resample(x, [50, 20], 16000, 16000, 60)
    assert np.array_equal(got[0, :50], x[0].mean(0)) and not got[0, 50:].any()
    assert np.array_equal(got[1, :20], x[1, :, :20].mean(0)) and not got[1, 20:].any()


@pytest.mark.parametrize("rates", [(3, 2), (441, 160), (1, 2)])
def test_constant_stays_constant_within_the_banks_dc_ripple(rates):
    """away from the ends every phase sees its whole filter, so a constant input comes out as that phase's DC gain: the
    ripple is read from the bank, not chosen"""
    rs = prep.Resampler(*rates)
    gain = rs.bank.sum(dim=1).numpy()
    ripple = np.abs(gain - 1).max()
    assert ripple < 0.02                                       # a low-pass at 0.99 of Nyquist with 6 zero crossings
    n_in = 8 * rs.orig + 4 * rs.width
    out = prep_ref.resample(np.ones((1, 1, n_in)), None, rates[0], rates[1], rs.out_len(n_in))[0]
    margin = -(-2 * rs.width * rs.new // rs.orig) + rs.new
    interior = out[margin:-margin]
    assert interior.size >= rs.new
    assert np.abs(interior - 1).max() <= ripple + 1e-12
    m = np.arange(margin, out.size - margin)
    assert np.abs(interior - gain[m % rs.new]).max() <= 1e-12


def test_draw_augment_policy():
    n, frames, L = 20000, 3, 160000
    a = prep.draw_augment(n, frames, L, device="cpu", generator=torch.Generator().manual_seed(5))
    assert a.noise_on.dtype == torch.uint8 and a.stretch_len.dtype == torch.int32 and a.flip.dtype == torch.uint8
    assert a.brightness.dtype == torch.float32 and a.stretch_factor.dtype == torch.float64
    assert a.noise_on.shape == a.stretch_len.shape == (n,) and a.brightness.shape == a.flip.shape == (n * frames,)
    # per-clip draws, one value per frame
    bright, flip = a.brightness.view(n, frames), a.flip.view(n, frames)
    assert bool((bright == bright[:, :1]).all()) and bool((flip == flip[:, :1]).all())
    stretch_on, bright_on = a.stretch_factor != 1.0, bright[:, 0] != 1.0
    for rate, p, five_sigma in ((a.noise_on.float().mean(), 0.3, 0.0162), (stretch_on.float().mean(), 0.3, 0.0162),
                                (bright_on.float().mean(), 0.3, 0.0162), (flip[:, 0].float().mean(), 0.5, 0.0177)):
        assert abs(float(rate) - p) <= five_sigma
    for f in (a.stretch_factor[stretch_on], bright[:, 0][bright_on].double()):
        assert float(f.min()) >= 0.8 and float(f.max()) < 1.2
        assert float(f.min()) < 0.81 and float(f.max()) > 1.19                     # the whole interval is used
    assert a.stretch_len.tolist() == [int(L * f) for f in a.stretch_factor.tolist()]
    assert bool((a.stretch_len[~stretch_on] == L).all()) and bool((bright[:, 0][~bright_on] == 1.0).all())
    assert set(a.noise_on.tolist()) == {0, 1} and set(a.flip.tolist()) == {0, 1}
    # the draws are independent of each other
    both = (a.noise_on.bool() & stretch_on).float().mean()
    assert abs(float(both) - 0.09) <= 5 * math.sqrt(0.09 * 0.91 / n)
    v = a.video(bgr=True)
    assert v.bgr and v.live is None and v.brightness is a.brightness and v.flip is a.flip
    assert v.rows(3, 6).flip.tolist() == a.flip[3:6].tolist()


def test_draw_augment_keeps_the_length_where_the_stretch_would_be_empty():
    a = prep.draw_augment(4000, 1, 1, device="cpu", generator=torch.Generator().manual_seed(6))
    on = a.stretch_factor != 1.0
    assert bool((a.stretch_factor[on] < 1.0).any())                                # int(1 * 0.9) == 0: stays 1
    assert bool((a.stretch_len == 1).all())
