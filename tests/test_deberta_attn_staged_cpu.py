"""CPU: the staged restatement of the DeBERTa attention kernels (tests/deberta_attn_staged_ref.py) against the float64
definitions it stands on, its window arithmetic and index tables, and the proof that the element-wise bounds of
tests/test_deberta_attention_paths_gpu.py have teeth: every mutant of the reference (one window's chunk not formed, table rows
added twice or never, a key counted twice, a clamp off by one) is at least 2 x outside the bound computed from the unmutated
reference, where the whole-tensor relative L2 the kernels were held to before (BOUND_A = 2e-2) lets it pass.  Each mutant's line
prints both figures; the old bar is printed, not asserted."""
import pytest
import torch

import deberta_attn_staged_ref as R
import deberta_dropout_ref as D
import deberta_grad_ref as G
import deberta_wgrad_ref as WG
from helpers import BOUND_A, l2_rel

_refs = {}


def _ref(name, mask_kind=None, backward_too=True):
    key = (name, mask_kind, backward_too)
    if key not in _refs:
        p = R.problem(name, mask_kind)
        _refs[key] = (p, R.reference(*p.args, p.dO, backward_too=backward_too))
    return _refs[key]


def _definition(p):
    """the unstaged float64 definition: O, lse, then the closed-form backward on its own exact O and lse"""
    O, lse = G.attention_stats(*p.args)
    ones = torch.ones(p.n, p.H, p.T, p.T, dtype=torch.float64)
    (dq, dk, dv, dposq, dposk), _ = D.attention_backward(*p.args, p.dO, ones, O, lse, R.F32_TOL)
    return dict(o=O, lse=lse, dq=dq, dk=dk, dv=dv, dposq=dposq, dposk=dposk)


@pytest.mark.parametrize("name,mask_kind", [(n, None) for n in R.CASES] + [("c", m) for m in R.MASKS])
def test_staged_agrees_with_the_definition_to_within_the_staging(name, mask_kind):
    p, ref = _ref(name, mask_kind)
    want = _definition(p)
    on = ref["on"][:, None, :].expand(p.n, p.H, p.T)
    for key in ("o", "dq", "dk", "dv", "dposq", "dposk"):
        if p.T == 1 and key in ("dq", "dk", "dposq", "dposk"):          # one-hot softmax: the true gradient is 0, no relative scale
            assert float(ref[key].abs().max()) <= 1e-6
            continue
        if key in ("dposq", "dposk") and float(want[key].norm()) <= 1e-9 * float(ref["s" + key[1:]].norm()):
            # the bucket sums cancel (a constant table: A_ir = sum_j dS_ij = 0): the true gradient is 0 and what is left is the
            # rounding of the per-tile sums, which the element's own bound holds
            assert bool((ref[key].abs() <= ref["bound"][key]).all())
            continue
        e = l2_rel(ref[key], want[key])
        print(f"staged vs definition {name} {mask_kind} {key}: rel L2 {e:.3e} (bound {BOUND_A / 4})")
        assert e <= BOUND_A / 4, (key, e)
    # lse: only the f32 rounding of 1 / scale separates the two (a relative 2^-24 of every score); a quarter of the GPU bound
    assert bool(((ref["lse"] - want["lse"]).abs() <= R.F32_TOL / 4 * want["lse"].abs().clamp_min(1.0))[on].all())
    # with the rounding functions replaced by the identity the staged form IS the definition (float64 summation order aside)
    O, lse = R.forward(*p.args, rnd=R.IDENTITY)
    back = R.backward(*p.args, p.dO, want["o"], want["lse"], rnd=R.IDENTITY)
    for key, got in dict(back, o=O).items():
        if key in want:
            scale = max(float(want[key].abs().max()), 1e-30)
            assert float((got - want[key]).abs().max()) <= 1e-11 * max(scale, 1.0), key
    assert float((lse - want["lse"])[on].abs().max()) <= 1e-11


def test_staged_table_gradients_are_autograd_of_the_definition():
    p = R.problem("b")
    q, k, v, posq, posk, idx, mask, scale = p.args
    leaves = [t.clone().requires_grad_(True) for t in (posq, posk)]
    out, lse = G.attention_stats(q, k, v, *leaves, idx, mask, scale)
    want = torch.autograd.grad(out, leaves, p.dO)
    exact = R.backward(*p.args, p.dO, out.detach(), lse.detach(), rnd=R.IDENTITY)
    staged = _ref("b")[1]
    for name, w, key in (("posQ", want[0], "dposq"), ("posK", want[1], "dposk")):
        assert float((exact[key] - w).abs().max()) <= 1e-12
        e = l2_rel(staged[key], w)
        print(f"staged d{name} against autograd: rel L2 {e:.3e}")
        assert e <= BOUND_A / 4


def test_case_list_reaches_every_chunk_count_in_both_passes():
    """the kernels' formula (db_chunks of the two lo / hi pairs), enumerated over every (block, tile, wave) of the GPU cases"""
    seen = {"fwd": (set(), set(), set()), "kpass": (set(), set(), set())}
    each = {}
    for name, (n, H, T, S, _) in R.CASES.items():
        each[name] = R.forms_summary(R.window_forms(T, S, R.case_index(name)))
        for pas, sets in each[name].items():
            for have, new in zip(seen[pas], sets):
                have |= new
        print(f"WINDOWS {name} T={T} S={S}: " + "; ".join(f"{pas} C2P {sorted(s[0])} P2C {sorted(s[1])}" for pas, s in each[name].items()))
    for pas in ("fwd", "kpass"):
        assert seen[pas][0] == {1, 2, 3} and seen[pas][1] == {1, 2, 3, 4, 5, 6}, (pas, seen[pas])
        assert each["e"][pas][:2] == ({1, 2, 3}, {2, 3, 5, 6})
        assert each["d"][pas][:2] == ({1, 2, 3}, {1, 2, 3})
        assert each["f"][pas][:2] == ({1, 2, 3}, {1, 2, 3, 4, 5, 6})
        assert each["g_linear"][pas][0] == {3} and each["g_constant"][pas][:2] == ({1}, {1})
        assert {15, 16, 31, 32, 46} <= each["g_steps"][pas][2]          # hi - lo on either side of db_chunks' divisions, and the most
    assert R.window_forms(200, 256, 512)["fwd"] == R.window_forms(200, 256, R.case_index("e"))["fwd"]


def test_every_index_table_satisfies_the_contract():
    for name, (n, H, T, S, _) in R.CASES.items():
        idx = R.case_index(name)
        assert idx.shape == (2 * T - 1,) and R.contract_ok(idx, S), name
    assert not R.contract_ok(torch.tensor([3, 5, 6], dtype=torch.int32), 8)          # a skipped row
    assert not R.contract_ok(torch.tensor([3, 2, 2], dtype=torch.int32), 8)          # decreasing
    assert not R.contract_ok(torch.tensor([14, 15, 16], dtype=torch.int32), 8)       # past the table
    lin = R.case_index("h")
    assert int(lin[0]) == 0 and int(lin[-1]) == 255 and int((lin == 0).sum()) > 1 and int((lin == 255).sum()) > 1


MUTANTS = [
    # (label, case, output, how)
    ("c2p chunk 2 of block 1 tile 1 wave 0 not formed", "t512", "o", lambda p: R.mut_drop_chunk(p.T, p.idx, p.S, "c2p", 1, 1, 0, 2)),
    ("c2p chunk 2 of block 1 tile 1 wave 0 not formed", "f", "o", lambda p: R.mut_drop_chunk(p.T, p.idx, p.S, "c2p", 1, 1, 0, 2)),
    ("p2c chunk 5 of block 1 tile 1 not formed", "t512", "o", lambda p: R.mut_drop_chunk(p.T, p.idx, p.S, "p2c", 1, 1, 0, 5)),
    ("last 16 queries count key T - 1 twice", "e", "o", lambda p: R.mut_double_last_key(p.T)),
    ("the end rows' pairs read the neighbouring row", "h", "o", lambda p: R.mut_shift_extreme_rows(p.T, p.idx, p.S)),
    ("the two end rows of dposK added twice", "e", "dposk", 2.0),
    ("the two end rows of dposK added twice", "t512", "dposk", 2.0),
    ("the two end rows of dposQ never written", "e", "dposq", 0.0),
]
T512 = (1, 1, 512, 256, 512)             # CPU only: the case the first measurements of these mutants were taken on


@pytest.mark.parametrize("label,name,key,how", MUTANTS, ids=[f"{m[1]}-{m[2]}-{i}" for i, m in enumerate(MUTANTS)])
def test_the_bounds_see_every_mutant(label, name, key, how):
    p, ref = _ref(T512 if name == "t512" else name, None, backward_too=key != "o")
    if key == "o":
        mut = how(p)
        pairs = sum(int(v.sum()) for kk, v in mut.items() if kk.startswith("drop_"))
        got, _ = R.forward(*p.args, mut=mut)
        label += f" ({pairs} pairs)" if pairs else ""
    else:
        reached = WG.reached_rows(p.idx)
        got = R.mut_table_rows(ref[key], [reached[0], reached[-1]], how)
    ratio = float(((got - ref[key]).abs() / ref["bound"][key].clamp_min(1e-300)).max())
    print(f"MUTANT {name} n,H,T,S={p.n},{p.H},{p.T},{p.S} {key}: {label}: whole-tensor rel L2 {l2_rel(got, ref[key]):.2e} (the old bar: "
          f"{BOUND_A}); worst |mutant - staged| / bound {ratio:.1f} (must be >= 2)")
    assert ratio >= 2.0
