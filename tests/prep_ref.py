"""The three input-preparation kernels (csrc/prep.hip) restated in float64 numpy from their definitions,
as direct sums and gathers: no polyphase table, no import of the code under test.  The counter hash, its key and the
integer-to-unit conversion of the Box-Muller draw are restated with exact integers, so the noise is the kernel's noise up to the
rounding of its f32 logarithm, square root and cosine."""
import math

import numpy as np

LPW, ROLLOFF = 6, 0.99
M32 = 0xFFFFFFFF


# ---- geometry ---------------------------------------------------------------------------------------------------------
def linear_taps(dst: int, src: int):
    """half-sample centres, resized ``src`` -> ``dst``: s = (o + 0.5) src / dst - 0.5 clamped below at 0 -> (i0, i1, w) with
    i1 = min(i0 + 1, src - 1); integer arithmetic: numerator (2 o + 1) src - dst over 2 dst"""
    i0, i1, w = np.empty(dst, np.int64), np.empty(dst, np.int64), np.empty(dst, np.float64)
    for o in range(dst):
        num, den = max((2 * o + 1) * src - dst, 0), 2 * dst
        i0[o] = num // den
        i1[o] = min(i0[o] + 1, src - 1)
        w[o] = (num % den) / den
    return i0, i1, w


def bilinear(img, H: int, W: int):
    """img (..., Hs, Ws) float64 -> (..., H, W): bilinear, half-pixel centres, no antialiasing, edge replication"""
    y0, y1, wy = linear_taps(H, img.shape[-2])
    x0, x1, wx = linear_taps(W, img.shape[-1])
    rows0, rows1 = img[..., y0, :], img[..., y1, :]
    top = rows0[..., x0] * (1 - wx) + rows0[..., x1] * wx
    bot = rows1[..., x0] * (1 - wx) + rows1[..., x1] * wx
    return top * (1 - wy)[:, None] + bot * wy[:, None]


def video_prepare(frames, H: int, W: int, bgr=False, live=None, brightness=None, flip=None):
    """frames (N, Hs, Ws, 3) uint8 -> (N, 3, H, W) float64: channel c reads byte 2 - c under ``bgr``; /255; brightness then
    clamp to [0, 1]; flip (column x takes column W - 1 - x); a frame with live == 0 is zeros"""
    x = np.asarray(frames).astype(np.float64).transpose(0, 3, 1, 2)
    if bgr:
        x = x[:, ::-1]
    out = bilinear(x, H, W) / 255.0
    if brightness is not None:
        out = np.clip(out * np.asarray(brightness, np.float64)[:, None, None, None], 0.0, 1.0)
    if flip is not None:
        f = np.asarray(flip).astype(bool)
        out[f] = out[f][..., ::-1]
    if live is not None:
        out[~np.asarray(live).astype(bool)] = 0.0
    return out


# ---- resampling -------------------------------------------------------------------------------------------------------
def filter_g(t, base: float, orig: int):
    t = np.asarray(t, np.float64)
    safe = np.where(t == 0, 1.0, t)
    sinc = np.where(t == 0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
    return np.where(np.abs(t) >= LPW, 0.0, np.cos(np.pi * t / (2 * LPW)) ** 2 * sinc * base / orig)


def resample(wave, lengths, orig_rate: int, new_rate: int, L: int):
    """wave (B, C, Ls) -> (B, L) float64: mono mean, out[m] = sum_n x[n] g((n / orig - m / new) base) over the clip's
    ``lengths[b]`` samples (None: all), 0 from m = ceil(new len / orig) on; equal rates copy.  The sum runs over the n where g
    can be non-zero (it is evaluated with its cutoff there, so the window only has to contain the support)"""
    wave = np.asarray(wave, np.float64)
    B, C, Ls = wave.shape
    g = math.gcd(orig_rate, new_rate)
    orig, new = orig_rate // g, new_rate // g
    base = min(orig, new) * ROLLOFF
    out = np.zeros((B, L), np.float64)
    for b in range(B):
        n_in = Ls if lengths is None else int(lengths[b])
        x = wave[b, :, :n_in].mean(axis=0) if n_in else np.zeros(0)
        n_out = min(L, -(-new * n_in // orig))
        if orig == new:
            out[b, :n_out] = x[:n_out]
            continue
        reach = LPW * orig / base                                  # g is 0 from |n - m orig / new| = reach on
        for m in range(n_out):
            centre = m * orig / new
            lo, hi = max(0, int(centre - reach) - 1), min(n_in, int(centre + reach) + 3)      # a superset of the support
            n = np.arange(lo, hi, dtype=np.float64)
            out[b, m] = np.dot(x[lo:hi], filter_g((n / orig - m / new) * base, base, orig))
    return out


# ---- noise and stretch -------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def rng_key(seed: int, site: int, sub: int) -> int:
    return int(mix32((seed & M32) ^ ((site * 0x9E3779B9) & M32))) ^ ((seed >> 32) & M32) ^ ((sub * 0x85EBCA6B) & M32)


def normal(key: int, j):
    """z(key, j): Box-Muller from draws 2 j and 2 j + 1; the top 24 bits of a draw give (0, 1] under the logarithm and [0, 1)
    in the angle (both exact in f32, so exact here)"""
    j = np.asarray(j, np.uint64)
    u1 = mix32((key + ((2 * j) & M32) * 0x9E3779B9) & M32)
    u2 = mix32((key + ((2 * j + 1) & M32) * 0x9E3779B9) & M32)
    f1 = ((u1 >> 8) + 1).astype(np.float64) * 2.0 ** -24
    f2 = (u2 >> 8).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(f1)) * np.cos(2.0 * np.pi * f2)


def augment(x, noise_on, stretch_len, seed: int, site: int):
    """x (B, L) -> (B, L) float64: xn = x + 0.01 z where noise_on, then xn resized L -> stretch_len by linear interpolation in
    the first min(stretch_len, L) outputs and 0 behind them"""
    x = np.asarray(x, np.float64)
    B, L = x.shape
    out = np.zeros_like(x)
    for b in range(B):
        xn = x[b] + (0.01 * normal(rng_key(seed, site, b), np.arange(L)) if noise_on is not None and noise_on[b] else 0.0)
        n = L if stretch_len is None else int(stretch_len[b])
        i0, i1, w = linear_taps(n, L)
        r = xn[i0] * (1 - w) + xn[i1] * w
        out[b, :min(n, L)] = r[:L]
    return out
