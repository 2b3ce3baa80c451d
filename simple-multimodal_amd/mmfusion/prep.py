"""Input preparation on the GPU: what a decoder emits -> what the backbones read (csrc/prep.hip).

The reference prepares every sample on the host (data/dataset_loaders.py): ``cv2.resize`` + ``/255`` + HWC -> CHW per frame
(:137-193), ``torchaudio`` resampling + mono mix + pad / truncate per clip (:95-131), and the train-time augmentations
(:195-261).  Here the decoder's output goes to the device as it is, uint8 ``(N, Hs, Ws, 3)`` frames and f32 PCM at the source
rate with per-clip lengths, and three kernels do the rest:

    prepare_video   mmf_video_prepare          frames -> (N, 3, H, W) f32 in [0, 1]  (bilinear, BGR -> RGB, brightness, flip)
                    mmf_video_prepare_patches  the same values as the native ViT's bf16 patch matrix (``NativeViT`` calls it
                                               for uint8 input: the f32 pixels are never written)
    prepare_audio   mmf_audio_resample         (B, C, Ls) -> (B, L): mono mean, windowed-sinc resampling, pad / truncate
                    mmf_audio_augment          additive noise, then the time stretch of the noisy signal

``draw_augment`` draws the reference's augmentation policy for a batch as device arrays, without a host round trip.  DESIGN.md
section 11 has the definitions (geometry, filter, RNG keying) and what is left on the host.  No CPU fallback: the kernels are
the product; only ``Resampler``'s filter bank and ``draw_augment`` are plain tensor code and run anywhere.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, NamedTuple, Optional, Tuple, Union

import torch

from . import lib, ops

LOWPASS_WIDTH, ROLLOFF = 6, 0.99             # torchaudio.transforms.Resample's documented defaults (Hann-windowed sinc)
NOISE_P, STRETCH_P, BRIGHTNESS_P, FLIP_P = 0.3, 0.3, 0.3, 0.5          # reference dataset_loaders.py:200,205,253,258
FACTOR_LO, FACTOR_SPAN = 0.8, 0.4                                       # :206,254


@dataclasses.dataclass
class VideoAug:
    """What ``mmf_video_prepare`` takes beside the frames: ``bgr`` (the decoder emits BGR, as cv2 does) and three optional
    per-frame device arrays, ``live`` uint8 (0: the frame is padding and prepares to zeros), ``brightness`` f32, ``flip`` uint8."""
    bgr: bool = False
    live: Optional[torch.Tensor] = None
    brightness: Optional[torch.Tensor] = None
    flip: Optional[torch.Tensor] = None

    def rows(self, n0: int, n1: int) -> "VideoAug":
        cut = lambda t: None if t is None else t[n0:n1]
        return VideoAug(self.bgr, cut(self.live), cut(self.brightness), cut(self.flip))


class Augment(NamedTuple):
    """One batch's draws: per clip ``noise_on`` uint8 (B,), ``stretch_len`` int32 (B,) (L: off) and the ``stretch_factor``
    float64 (B,) it came from (1.0: off); per frame ``brightness`` f32 and ``flip`` uint8 (B * frames_per_clip,)."""
    noise_on: torch.Tensor
    stretch_len: torch.Tensor
    stretch_factor: torch.Tensor
    brightness: torch.Tensor
    flip: torch.Tensor

    def video(self, bgr: bool = False, live: Optional[torch.Tensor] = None) -> VideoAug:
        return VideoAug(bgr, live, self.brightness, self.flip)


def _hw(size: Union[int, Tuple[int, int]]) -> Tuple[int, int]:
    """an output size as (H, W).  A tuple is read as (height, width), as ``torch.zeros(frames, 3, *size)`` reads the reference's
    ``config.video_frame_size``; ``cv2.resize`` reads the same tuple as (width, height), so the reference itself is only
    consistent for square sizes"""
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


def prepare_video(frames_u8: torch.Tensor, size: Union[int, Tuple[int, int]], *, bgr: bool = False, live=None, brightness=None,
                  flip=None) -> torch.Tensor:
    """uint8 ``(N, Hs, Ws, 3)`` frames on the GPU -> ``(N, 3, H, W)`` f32 in [0, 1], ``size`` = H or (H, W) (height first): the reference's
    frame tensor (dataset_loaders.py:161-169 with the exact bilinear value instead of cv2's fixed-point one, and :248-261)."""
    H, W = _hw(size)
    frames_u8 = frames_u8.contiguous()
    out = torch.empty((frames_u8.shape[0], 3, H, W), dtype=torch.float32, device=frames_u8.device)
    lib.video_prepare(frames_u8, out, H, W, None, bgr, live, brightness, flip)
    return out


def filter_geometry(orig_rate: int, new_rate: int) -> Tuple[int, int, int, float]:
    """-> (orig, new, width, base): the rates over their gcd, the filter's half width in input samples and its cutoff"""
    if orig_rate < 1 or new_rate < 1:
        raise ValueError(f"Resampler: rates must be positive, got {orig_rate} -> {new_rate}")
    g = math.gcd(int(orig_rate), int(new_rate))
    orig, new = int(orig_rate) // g, int(new_rate) // g
    base = min(orig, new) * ROLLOFF
    return orig, new, int(math.ceil(LOWPASS_WIDTH * orig / base)), base


class Resampler:
    """The polyphase bank of a rate pair.  ``bank``: float64 ``(new, 2 width + orig)``, ``bank[j][k] = g(((k - width) / orig -
    j / new) base)`` with ``g(t) = cos^2(pi t / (2 lpw)) sinc(pi t) base / orig`` inside ``|t| < lpw``;
    None when the rates are equal.  ``table(device)``: the bank in f32 on that device, made once per device."""

    def __init__(self, orig_rate: int, new_rate: int):
        self.orig, self.new, self.width, self.base = filter_geometry(orig_rate, new_rate)
        self._tables: Dict[torch.device, torch.Tensor] = {}
        self.bank: Optional[torch.Tensor] = None
        if self.orig == self.new:
            return
        o, n, w = self.orig, self.new, self.width
        k = torch.arange(2 * w + o, dtype=torch.float64)[None, :]
        j = torch.arange(n, dtype=torch.float64)[:, None]
        t = ((k - w) / o - j / n) * self.base
        g = torch.cos(t * (math.pi / (2 * LOWPASS_WIDTH))) ** 2 * torch.special.sinc(t) * (self.base / o)
        self.bank = torch.where(t.abs() < LOWPASS_WIDTH, g, torch.zeros_like(g))
        # the kernel reads k in (orig j / new, orig j / new + 2 width] of row j only: nothing else may be set
        lo = (torch.arange(n) * o // n)[:, None]
        kk = torch.arange(2 * w + o)[None, :]
        assert not bool((self.bank != 0)[(kk <= lo) | (kk > lo + 2 * w)].any()), "filter support outside the kernel's taps"

    def table(self, device) -> Optional[torch.Tensor]:
        if self.bank is None:
            return None
        device = torch.device(device)
        if device not in self._tables:
            self._tables[device] = self.bank.to(torch.float32).to(device).contiguous()
        return self._tables[device]

    def out_len(self, in_len: int) -> int:
        return -(-self.new * int(in_len) // self.orig)


def prepare_audio(wave: torch.Tensor, lengths: Optional[torch.Tensor], resampler: Resampler, out_len: int, *, noise_on=None,
                  stretch_len=None) -> torch.Tensor:
    """f32 PCM ``(B, C, Ls)`` (or ``(B, Ls)``) at the source rate on the GPU, valid up to ``lengths[b]`` (None: all of it) ->
    ``(B, out_len)`` f32 mono at the target rate, zero padded / truncated (dataset_loaders.py:109-125).  With ``noise_on`` uint8
    (B,) / ``stretch_len`` int32 (B,) a second launch applies the reference's ``_augment_audio`` (:195-246) with the noise drawn
    from the device-resident RNG state (``ops.rng_state()``, one site per call)."""
    if wave.dim() == 2:
        wave = wave[:, None, :]
    wave = wave.contiguous()
    if lengths is not None:
        lengths = lengths.to(device=wave.device, dtype=torch.int32).contiguous()
    out = torch.empty((wave.shape[0], int(out_len)), dtype=torch.float32, device=wave.device)
    lib.audio_resample(wave, lengths, resampler.table(wave.device), out, resampler.orig, resampler.new, resampler.width)
    if noise_on is None and stretch_len is None:
        return out
    aug = torch.empty_like(out)
    lib.audio_augment(out, aug, noise_on, stretch_len, ops.rng_state().data_ptr() if noise_on is not None else None,
                      ops.next_site() if noise_on is not None else 0)
    return aug


def draw_augment(B: int, frames_per_clip: int, L: int, *, device, generator: Optional[torch.Generator] = None) -> Augment:
    """The reference's augmentation policy (dataset_loaders.py:195-261) for ``B`` clips, drawn with ``torch.rand`` on ``device``
    and never read back: noise with p 0.3; stretch with p 0.3 to ``int(L * factor)`` samples, factor uniform on [0.8, 1.2)
    (``L`` when off or when it would be 0); brightness with p 0.3 by such a factor (1.0 when off); flip with p 0.5.  The
    video draws are per clip, expanded to one value per frame."""
    u = torch.rand((6, B), device=device, generator=generator)
    factor = lambda r: FACTOR_LO + u[r].double() * FACTOR_SPAN            # the reference's Python-float arithmetic on an f32 draw
    noise_on = (u[0] < NOISE_P).to(torch.uint8)
    stretch_on = u[1] < STRETCH_P
    stretch_factor = torch.where(stretch_on, factor(2), torch.ones((), dtype=torch.float64, device=device))
    n = (L * stretch_factor).long()
    stretch_len = torch.where(n > 0, n, torch.full_like(n, L)).to(torch.int32)
    brightness = torch.where(u[3] < BRIGHTNESS_P, factor(4), torch.ones((), dtype=torch.float64, device=device)).float()
    flip = (u[5] < FLIP_P).to(torch.uint8)
    per_frame = lambda t: t.repeat_interleave(frames_per_clip).contiguous()
    return Augment(noise_on, stretch_len, stretch_factor, per_frame(brightness), per_frame(flip))
