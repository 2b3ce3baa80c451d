#!/usr/bin/env python3
"""Cost of the device-side input preparation (mmfusion/prep.py, csrc/prep.hip) at the bench batch, each against the same result
composed from stock torch operations on the GPU (what the project could do before it had these kernels):

  * video: 480 decoded 360 x 640 uint8 frames -> the ViT's (480 * 196, 768) bf16 patch matrix.  Fused: one
    ``mmf_video_prepare_patches``.  Composition: ``permute / float / div``, ``F.interpolate(bilinear)``, ``contiguous``, ``mmf_vit_patchify``.
  * audio: 16 clips x 2 channels x 441000 samples at 44.1 kHz -> (16, 160000) at 16 kHz.  Fused: one ``mmf_audio_resample``.
    Composition: ``mean``, ``F.pad``, ``F.conv1d`` with the same filter bank (stride ``orig``), reshape, truncate.

Per route: microseconds per call (HIP events around ``--steps`` calls after ``--warmup``), the HBM bytes the result needs (inputs
read once + outputs written once) as TB/s over that time, and the ratio composition / fused.  Successive calls read different
copies of the input, 512 MB of them in turn, twice the 256 MB last-level cache, so an input is not served from the cache a
previous call left warm and the rate is an HBM rate.  Both routes allocate their result per call.  The conditions (``ok``):
fused is not slower than the composition, with a 5 % margin for run-to-run noise, and the two results agree (``max_abs_diff``
within ``agree_within``: one bf16 ulp below 1 for the patches, where torch interpolates with float coordinates; the kernel
test's 2e-5 for the waveform).

    python tools/prep_bench.py [--steps 20] [--warmup 3] [--frames 480] [--clips 16]
Prints one JSON line."""
import argparse
import json

from backbone_bench import time_eager  # (first: it sets the import path)
import torch
import torch.nn.functional as F

MARGIN = 1.05
ROTATE_BYTES = 512 << 20
VIDEO_AGREE, AUDIO_AGREE = 2.0 ** -8, 2e-5


def _copies(x: torch.Tensor) -> list:
    """``x`` and enough copies of it to hold ROTATE_BYTES"""
    n = -(-ROTATE_BYTES // (x.numel() * x.element_size()))
    return [x] + [x.clone() for _ in range(n - 1)]


class _Turn:
    """the next copy on every call"""

    def __init__(self, copies: list):
        self.copies, self.i = copies, 0

    def __call__(self) -> torch.Tensor:
        self.i = (self.i + 1) % len(self.copies)
        return self.copies[self.i]


def _row(ms: float, nbytes: int) -> dict:
    return {"us": round(ms * 1e3, 1), "tb_per_s": round(nbytes / ms / 1e9, 3)}


def video(args) -> dict:
    from mmfusion import lib
    N, Hs, Ws, S, P = args.frames, 360, 640, 224, 16
    fr = torch.randint(0, 256, (N, Hs, Ws, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    nxt = _Turn(_copies(fr))
    fused = torch.empty((N * (S // P) ** 2, 3 * P * P), dtype=torch.bfloat16, device="cuda")
    stock = torch.empty_like(fused)

    def run_fused():
        lib.video_prepare(nxt(), fused, S, S, P)

    def run_stock():
        x = nxt().permute(0, 3, 1, 2).float().div(255.0)
        x = F.interpolate(x, size=(S, S), mode="bilinear", align_corners=False).contiguous()      # (it comes back channels-last)
        lib.vit_patchify(x, stock, N, 3, S, S, P)

    nbytes = fr.numel() + fused.numel() * 2
    a, b = time_eager(run_fused, args.steps, args.warmup), time_eager(run_stock, args.steps, args.warmup)
    a2 = time_eager(run_fused, args.steps, args.warmup)                         # again behind the other: the spread of the fused figure
    fa = 0.5 * (a + a2)
    diff = float((fused.float() - stock.float()).abs().max())
    return {"shape": [N, Hs, Ws, 3], "bytes": nbytes, "fused": _row(fa, nbytes), "fused_repeat_us": [round(a * 1e3, 1), round(a2 * 1e3, 1)],
            "torch_composition": _row(b, nbytes), "ratio": round(b / fa, 2), "max_abs_diff": diff, "agree_within": VIDEO_AGREE,
            "input_copies": len(nxt.copies), "ok": fa <= MARGIN * b and diff <= VIDEO_AGREE}


def audio(args) -> dict:
    from mmfusion import prep
    B, C, Ls, L = args.clips, 2, 441000, 160000
    rs = prep.Resampler(44100, 16000)
    x = (torch.rand(B, C, Ls, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    bank = rs.table("cuda")[:, None, :]
    nxt = _Turn(_copies(x))
    out = {}

    def run_fused():
        out["fused"] = prep.prepare_audio(nxt(), None, rs, L)

    def run_stock():
        mono = F.pad(nxt().mean(dim=1, keepdim=True), (rs.width, rs.width + rs.orig))
        y = F.conv1d(mono, bank, stride=rs.orig).transpose(1, 2).reshape(B, -1)[:, :min(L, rs.out_len(Ls))]
        out["stock"] = F.pad(y, (0, L - y.shape[1]))

    nbytes = x.numel() * 4 + B * L * 4
    a, b = time_eager(run_fused, args.steps, args.warmup), time_eager(run_stock, args.steps, args.warmup)
    a2 = time_eager(run_fused, args.steps, args.warmup)
    fa = 0.5 * (a + a2)
    diff = float((out["fused"] - out["stock"]).abs().max())
    return {"shape": [B, C, Ls], "rates": [rs.orig, rs.new], "taps": 2 * rs.width, "bytes": nbytes, "fused": _row(fa, nbytes),
            "fused_repeat_us": [round(a * 1e3, 1), round(a2 * 1e3, 1)], "torch_composition": _row(b, nbytes),
            "ratio": round(b / fa, 2), "max_abs_diff": diff, "agree_within": AUDIO_AGREE, "input_copies": len(nxt.copies),
            "ok": fa <= MARGIN * b and diff <= AUDIO_AGREE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--clips", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prep_bench needs a GPU"
    print(json.dumps({"video": video(args), "audio": audio(args)}))


if __name__ == "__main__":
    main()
