"""GPU: norm2 of two cross-modal blocks fused with the three-way modality sum (mmf_layernorm2_add3_fwd_grouped, csrc/layernorm.hip)
against the two launches it replaces: mmf_layernorm_fwd_grouped over (pre_a, pre_b) of every sum, then mmf_add3_grouped on
(x, y_a, y_b).  e and the four statistics must be BIT-EQUAL: the kernel normalises through the routine the lane-form forward uses,
rounds each normalised value to bf16 where the tensor was stored, and sums as add3 does.

The separate forward has two forms that reduce a row in different orders (lane form for launches above its workgroup budget, chunk
form below), so the fused launch can only equal the lane form: mmf_layernorm2_add3_available says whether the separate forward over
the same rows would take it, and ``ops.ln2_add3_group`` composes the two launches where it would not (small launches, other
widths).  Cases: d = 768 / 512 / 256; rows 5, 60 and 4099 (more rows than workgroups x 4: waves walk several rows) as three unequal
problems of one launch and each alone.  A launch of 5 or 60 rows alone is below the budget: the op takes the composed path there
(checked against the composition all the same), and the kernel itself, launched alone on those rows, is held to what it wrote for
the same rows inside the three-problem launch (a row's result does not depend on the launch around it).  d = 520: composed path.

Through autograd the gradients of x, pre_a and pre_b are bit-equal to the two-op composition; gamma / beta gradients end in float
atomics (ln_bwd_finalize_kernel) and are held to F32_TOL, the bound of tests/test_kernel_forms_gpu.py for them."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import fused_seams_ref as old  # noqa: E402
from mmfusion import lib, ops  # noqa: E402
from test_kernel_forms_gpu import F32_TOL, rel  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
EPS = 1e-5
ROWS = (5, 60, 4099)
LANE_D = (768, 512, 256)


def nan_like(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def inputs(d):
    """per row count: x, pre_a, pre_b (bf16) and the two norms' gamma / beta (f32); made once per width and never written"""
    g = torch.Generator(device=DEV).manual_seed(d)
    out = {}
    for r in ROWS:
        x = torch.randn(r, d, device=DEV, generator=g).to(BF16)
        pa = (torch.randn(r, d, device=DEV, generator=g) * 2 + 0.5).to(BF16)
        pb = (torch.randn(r, d, device=DEV, generator=g) * 0.7 - 1).to(BF16)
        par = [torch.randn(d, device=DEV, generator=g) * s + o for s, o in ((0.5, 1), (0.5, 0), (0.3, 1), (0.3, 0))]
        out[r] = (x, pa, pb, *par)
    return out


def composed(d, rows):
    """the two launches: (e, mean_a, rstd_a, mean_b, rstd_b) per problem"""
    inp = inputs(d)
    ln, add, outs = [], [], []
    for r in rows:
        x, pa, pb, ga, ba, gb, bb = inp[r]
        ya, yb, e = nan_like((r, d), BF16), nan_like((r, d), BF16), nan_like((r, d), BF16)
        st = nan_like((4, r))
        ln.append(lib.LnProblem(pa.data_ptr(), ya.data_ptr(), ga.data_ptr(), ba.data_ptr(), st[0].data_ptr(), st[1].data_ptr(),
                                None, None, None, None, r))
        ln.append(lib.LnProblem(pb.data_ptr(), yb.data_ptr(), gb.data_ptr(), bb.data_ptr(), st[2].data_ptr(), st[3].data_ptr(),
                                None, None, None, None, r))
        add.append(lib.Add3Problem(x.data_ptr(), ya.data_ptr(), yb.data_ptr(), e.data_ptr(), r * d))
        outs.append((e, st, ya, yb))
    lib.layernorm_fwd_grouped(ln, d, EPS)
    form = lib.load().mmf_layernorm_last_form()
    lib.check(lib.load().mmf_add3_grouped((lib.Add3Problem * len(add))(*add), len(add), lib.stream_ptr()))
    torch.cuda.synchronize()
    return [(e, st) for e, st, _, _ in outs], form


def fused(d, rows):
    inp = inputs(d)
    probs, outs = [], []
    for r in rows:
        x, pa, pb, ga, ba, gb, bb = inp[r]
        e, st = nan_like((r, d), BF16), nan_like((4, r))
        probs.append(lib.Ln2Add3Problem(x.data_ptr(), pa.data_ptr(), ga.data_ptr(), ba.data_ptr(), pb.data_ptr(), gb.data_ptr(),
                                        bb.data_ptr(), e.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
                                        st[3].data_ptr(), r))
        outs.append((e, st))
    lib.layernorm2_add3_fwd_grouped(probs, d, EPS)
    torch.cuda.synchronize()
    return outs


def assert_same(got, want, what):
    for i, ((e, st), (e0, st0)) in enumerate(zip(got, want)):
        assert not bool(torch.isnan(e.float()).any()) and not bool(torch.isnan(st).any()), f"{what}: problem {i} left unwritten"
        assert torch.equal(e, e0), f"{what}: e of problem {i} differs"
        for k, name in enumerate(("mean_a", "rstd_a", "mean_b", "rstd_b")):
            assert torch.equal(st[k], st0[k]), f"{what}: {name} of problem {i} differs"


@pytest.mark.parametrize("rows", [ROWS, (4099,)], ids=["three_unequal", "4099_alone"])
@pytest.mark.parametrize("d", LANE_D)
def test_fused_launch_equals_the_two_launches(d, rows):
    assert lib.layernorm2_add3_available(rows, d)
    want, form = composed(d, rows)
    assert form > 100                                           # the separate forward took its lane form, as the query said
    assert_same(fused(d, rows), want, f"d={d} rows={rows}")


@pytest.mark.parametrize("r", [5, 60])
@pytest.mark.parametrize("d", LANE_D)
def test_small_launch_alone(d, r):
    """below the separate forward's budget: the op composes (and equals the composition); the kernel alone on these rows writes what
    it wrote for them inside the three-problem launch, which test_fused_launch_equals_the_two_launches holds to the composition"""
    assert not lib.layernorm2_add3_available((r,), d)
    x, pa, pb, ga, ba, gb, bb = inputs(d)[r]
    na, nb = _norm(ga, ba), _norm(gb, bb)
    e = ops.ln2_add3_group([(x, pa, na, pb, nb)], EPS)[0]
    torch.cuda.synchronize()
    want, form = composed(d, (r,))
    assert form < 100 and torch.equal(e, want[0][0])
    assert_same(fused(d, (r,)), [fused(d, ROWS)[ROWS.index(r)]], f"d={d} rows={r} alone against the same rows in the launch of three")


def _norm(gamma, beta):
    m = torch.nn.LayerNorm(gamma.numel(), eps=EPS).to(DEV)
    with torch.no_grad():
        m.weight.copy_(gamma), m.bias.copy_(beta)
    m.weight.grad, m.bias.grad = torch.zeros_like(m.weight), torch.zeros_like(m.bias)
    return m


def _autograd(group_fn, tensors, dys):
    """tensors: per sum (x, pre_a, pre_b, gamma_a, beta_a, gamma_b, beta_b) -> e, input gradients, parameter gradients"""
    items, leaves, norms = [], [], []
    for x, pa, pb, ga, ba, gb, bb in tensors:
        xs = [t.clone().requires_grad_(True) for t in (x, pa, pb)]
        na, nb = _norm(ga, ba), _norm(gb, bb)
        items.append((xs[0], xs[1], na, xs[2], nb))
        leaves += xs
        norms += [na, nb]
    es = group_fn(items, EPS)
    torch.autograd.backward(es, dys)
    torch.cuda.synchronize()
    return [e.detach() for e in es], [t.grad for t in leaves], [q.grad for n in norms for q in (n.weight, n.bias)]


@pytest.mark.parametrize("d,rows,is_fused", [(768, ROWS, True), (512, ROWS, True), (256, ROWS, True), (768, (60,), False),
                                             (520, (60, 4099), False)],
                         ids=["768", "512", "256", "768_small_composed", "520_composed"])
def test_autograd_equals_the_two_op_composition(d, rows, is_fused):
    assert lib.layernorm2_add3_available(rows, d) == is_fused
    g = torch.Generator(device=DEV).manual_seed(1000 + d)
    if d in LANE_D:
        tensors = [inputs(d)[r] for r in rows]
    else:                                                       # d = 520: no lane width, the composed path
        tensors = [((torch.randn(r, d, device=DEV, generator=g)).to(BF16), (torch.randn(r, d, device=DEV, generator=g) * 2).to(BF16),
                    (torch.randn(r, d, device=DEV, generator=g) - 1).to(BF16), *[torch.randn(d, device=DEV, generator=g) for _ in range(4)])
                   for r in rows]
    dys = [torch.randn(r, d, device=DEV, generator=g).to(BF16) for r in rows]
    calls = []
    real = lib.layernorm2_add3_fwd_grouped
    lib.layernorm2_add3_fwd_grouped = lambda *a: (calls.append(1), real(*a))[1]
    try:
        got = _autograd(ops.ln2_add3_group, tensors, dys)
    finally:
        lib.layernorm2_add3_fwd_grouped = real
    assert bool(calls) == is_fused
    want = _autograd(old.ln2_add3_group, tensors, dys)
    for name, a, b in zip(("e", "input gradient"), got[:2], want[:2]):
        for i, (u, v) in enumerate(zip(a, b)):
            assert not bool(torch.isnan(u.float()).any()) and torch.equal(u, v), f"{name} {i} differs from the composition"
    for i, (u, v) in enumerate(zip(got[2], want[2])):           # dgamma / dbeta: float atomics in the finalize pass
        assert rel(u, v.double().cpu()) < F32_TOL, ("parameter gradient", i, rel(u, v.double().cpu()))
