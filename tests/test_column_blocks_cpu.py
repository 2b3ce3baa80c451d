"""``ops._column_blocks``: whether some 2-D tensors are, in order, the adjacent column blocks of one contiguous 2-D
tensor.  It reads tensor metadata only, so it is pinned here on CPU tensors, together with the two of its three call
sites that are plain torch (``small_ops.cat3``, ``small_ops._Split3``); the third, ``ops._GroupedLinear.backward``, is
pinned on the GPU by tests/test_kernels_gpu.py::test_linear_group_on_split3_returns_one_gradient_buffer."""
import pytest
import torch

from mmfusion import small_ops as sops
from mmfusion.ops import _column_blocks, _column_views


def cols(t, *bounds):
    return [t[:, a:b] for a, b in zip(bounds, bounds[1:])]


def test_blocks_that_tile_their_base_give_the_base():
    for base, bounds in ((torch.randn(4, 12), (0, 4, 8, 12)),
                         (torch.randn(4, 32).to(torch.bfloat16), (0, 8, 24, 32)),        # widths 8, 16, 8
                         (torch.randn(1, 12), (0, 4, 8, 12))):                           # one row
        assert _column_blocks(cols(base, *bounds)) is base
        assert _column_blocks(_column_views(base, [b - a for a, b in zip(bounds, bounds[1:])])) is base


REFUSED = {
    "wrong order": lambda b: [b[:, 4:8], b[:, 0:4], b[:, 8:12]],
    "columns left over": lambda b: cols(b, 0, 4, 8),
    "a column skipped": lambda b: [b[:, 0:4], b[:, 5:8], b[:, 8:12]],
    "overlap": lambda b: [b[:, 0:5], b[:, 4:8], b[:, 8:12]],
    "base is the left column slice of something wider": lambda b: cols(torch.randn(4, 24)[:, :12], 0, 4, 8, 12),
    "base is the right column slice of something wider": lambda b: cols(torch.randn(4, 24)[:, 12:], 0, 4, 8, 12),
    "two bases with equal contents": lambda b: [b[:, 0:4], *cols(b.clone(), 4, 8, 12)],
    "row slice: not from the base's first element": lambda b: cols(b[1:], 0, 4, 8, 12),
    "row slice from the first element: rows left over": lambda b: cols(b[:3], 0, 4, 8, 12),
    "3-D base": lambda b: cols(torch.randn(2, 4, 12)[0], 0, 4, 8, 12),
    "fresh tensors": lambda b: [torch.randn(4, 4) for _ in range(3)],
    "first block copied": lambda b: [b[:, 0:4].contiguous(), b[:, 4:8], b[:, 8:12]],
    "strided columns": lambda b: [b[:, 0:12:2], b[:, 6:12]],
    "another dtype through the same storage": lambda b: [b[:, 0:4], b.view(torch.int32)[:, 4:8], b[:, 8:12]],
    "nothing": lambda b: [],
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_anything_else_gives_none(case):
    assert _column_blocks(REFUSED[case](torch.randn(4, 12))) is None


def test_cat3_returns_the_base_only_for_equal_float32_thirds():
    base = torch.randn(4, 12)
    assert sops.cat3(*cols(base, 0, 4, 8, 12)) is base
    b16 = torch.randn(4, 12).to(torch.bfloat16)                    # bf16 thirds: a fresh f32 concatenation
    y = sops.cat3(*cols(b16, 0, 4, 8, 12))
    assert y is not b16 and y.dtype == torch.float32 and y._base is None and torch.equal(y, b16.float())
    wide = torch.randn(4, 32)                                      # unequal widths: tiles its base, but not in thirds
    y = sops.cat3(*cols(wide, 0, 8, 24, 32))
    assert y is not wide and y._base is None and torch.equal(y, wide)


def test_split3_backward_concatenates_separate_gradients():
    c = torch.randn(4, 12, requires_grad=True)
    gs = [torch.randn(4, 4) for _ in range(3)]
    hits = sops.split3_nocopy_hits
    torch.autograd.backward(sops.split3(c), gs)
    assert sops.split3_nocopy_hits == hits
    assert torch.equal(c.grad, torch.cat(gs, dim=1))


def test_split3_backward_returns_a_gradient_buffer_given_in_thirds():
    leaf = torch.randn(4, 12, requires_grad=True)
    c, seen = leaf * 1.0, []
    c.register_hook(seen.append)                                   # what _Split3.backward returned, as it returned it
    buf = torch.randn(4, 12)
    hits = sops.split3_nocopy_hits
    torch.autograd.backward(sops.split3(c), cols(buf, 0, 4, 8, 12))
    assert sops.split3_nocopy_hits == hits + 1
    assert len(seen) == 1 and seen[0].data_ptr() == buf.data_ptr() and seen[0].shape == buf.shape and seen[0].is_contiguous()
    assert torch.equal(leaf.grad, buf)
