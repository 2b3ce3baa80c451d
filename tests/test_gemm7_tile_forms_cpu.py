"""CPU: generation 7's 256 x 192 tile form (csrc/gemm7.hip, TN = 3).  Its n-operand tiles use the shared LDS image at width 192
([192][32] row-read tiles for NT, [32][192] transposed-read tiles for NN): both reads must stay on their conflict-free floor and
the LDS-DMA pieces must cover the tile exactly once.  The host's width choice (mmf_gemm7_tile_n) on 256 workgroups must pick 192
for the fusion step's launches whose makespan it shortens and keep 256 where it ties or loses."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import lds_image_check as chk  # noqa: E402
from gemm7_step_launches import STEP_LAUNCHES  # noqa: E402
from mmfusion import lib  # noqa: E402


def test_width_192_image_reads_and_piece_maps():
    assert chk.gemm6_row_read_cycles(32, rows=192) == 4              # NT: n-operand [192][32], row reads
    ok, cyc = chk.gemm6_tr_read_ok(2, W=192)                          # NN: n-operand [32][192], transposed reads (BK = 32: G = 0, 1)
    assert ok and cyc == 2
    assert chk.gemm6_piece_map_ok(False, 32, 192) and chk.gemm6_piece_map_ok(True, 32, 192)
    # the 256-wide forms the kernels keep using are unchanged by the width parameter
    assert chk.gemm6_tr_read_ok(2) == chk.gemm6_tr_read_ok(2, W=256) == (True, 2)
    assert chk.gemm6_piece_map_ok(True, 32) and chk.gemm6_piece_map_ok(False, 32)


def _problems(shapes):
    arr = (lib.GemmProblem * len(shapes))()
    for p, (M, N, K) in zip(arr, shapes):
        p.M, p.N, p.K = M, N, K
    return arr


def _tile_n(shapes, workgroups=256):
    L = lib.load()
    r = L.mmf_gemm7_tile_n(_problems(shapes), len(shapes), workgroups)
    lib.check(r if r < 0 else 0)
    return r


def test_automatic_width_on_the_step_launches():
    for name, _layout, _epi, shapes, want in STEP_LAUNCHES:
        assert _tile_n(shapes) == want, name


def test_automatic_width_rule():
    assert _tile_n([(4096, 4096, 4096)]) == 256                       # one full round of 256 tiles; at 192: 352 tiles, two rounds
    assert _tile_n([(256, 768, 768)], workgroups=1) == 256            # one workgroup does the same work either way: a tie keeps 256
    assert _tile_n([(256, 768, 768)]) == 192                          # one round either way (3 or 4 tiles): the narrower tile is shorter
    assert _tile_n([(8192, 3072, 768)]) == 192                        # 384 tiles (2 rounds of width 256) vs 512 (2 rounds of 192)
    assert _tile_n([(8192, 3072, 768)], workgroups=128) == 256        # 3 rounds of 256 vs 4 rounds of 192: a tie
