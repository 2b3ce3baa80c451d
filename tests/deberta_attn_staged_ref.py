"""The disentangled attention of csrc/deberta.hip, forward and backward, restated in float64 with the kernels' rounding points
and only those (the DeBERTa counterpart of ``attn_ref.staged``), on top of the float64 definitions tests/deberta_ref.py,
deberta_grad_ref.py, deberta_wgrad_ref.py and deberta_dropout_ref.py; the element-wise bounds the GPU tests hold the kernels to;
the host restatement of the kernels' window arithmetic; index tables that satisfy the contract; and mutants of the reference
that tests/test_deberta_attn_staged_cpu.py uses to show that the bounds would see a fault confined to one window.

Operands are float64 tensors of bf16-representable values: q, k, v, dO (n, H, T, 64); posq, posk (H, 2S, 64); idx int (2T - 1,);
mask (n, T) or None; ``w`` (n, H, T, T) = keep * c or None (``deberta_dropout_ref.probs_keep``, ``attn_ref.inv_keep_of``).

Staging points, read off csrc/deberta.hip (line numbers of that file).  Everything between two of them is f32 arithmetic on the
device and float64 here.

forward, deberta_attn_fwd_kernel (204-343)
  F1  s = (S + c2p + p2c) * inv_scale (db_score, 179), inv_scale the f32 ``1.0f / scale`` of the entry (959); the three products are
      f32 MFMA accumulators and the two parked position products stay f32 in LDS (163, 214-215): not rounded.
  F2  a masked pair scores -FLT_MAX (299); a key past T has probability 0 (300).
  F3  per 32-key tile the row maximum is raised (304-307) and p = exp(s - m_tile) (313) is rounded to bf16 as the B operand of
      P V (324-329) RELATIVE TO THE RUNNING MAXIMUM OF THAT TILE, the accumulator rescaled by exp(m_old - m_new) (329); l takes
      the unrounded p (314-316).  DROP: keep ? p c : 0 is what is rounded (322), l and lse run over the undropped p (318).
  F4  O = acc / l rounded to bf16 (339); lse = m + log l stored as f32 (341).  ``forward`` returns O BEFORE that rounding (the
      kernel is then half a bf16 ulp plus accumulation noise away, where two roundings could differ by a whole ulp on a flip) and
      ``o16`` / ``lse32`` are the rounded values a backward is handed.
delta pre-pass, deberta_attn_delta_kernel (543-561)
  D1  delta = sum_d dO O over the bf16 O it is given, accumulated and stored in f32 (558-560).
backward passes, deberta_attn_bwd_kernel (607-867); "own" = the 64 tokens of the workgroup, "other" = the 32 of the tile
  B1  s as F1 (771, the same db_score); P = exp(s - lse) with the f32 lse it is given, 1 / T (the f32 quotient, 647) on a masked
      query row, 0 where only the key is masked (775): f32, NOT rounded for dS.
  B2  dP = dO . V is an f32 MFMA accumulator (759): not rounded.  DROP: dP w (779).
  B3  dS = P (dP - delta) inv_scale on unmasked pairs, else 0 (779 / 782): f32; it is parked in LDS as f32 (789) for the bucket
      sums and rounded to bf16 (792) only as the B operand of the content products dQ += dS K, dK += dS^T Q (797).
  B4  P (DROP: P w) rounded to bf16 as the B operand of dV += P^T dO (800-805); a masked query row contributes 1 / T to every key.
  B5  the bucket sums: per own token, per 32-token tile and per table row the f32 sum of the f32 dS over the run of the tile's
      tokens that gather that row (809-820), THEN rounded to bf16 (821); those bf16 sums are the B operand of the position term of
      dQ / dK (826) and, through LDS (832), the A operand of the table gradients (843-844).  So the sums are rounded once per
      (own token, tile, row), not once per row.
  B6  the transposed position window sT holds the table's bf16 rows as they are (723-732): exact, no rounding.  Likewise own^T (673).
  B7  dQ, dK, dV accumulate in f32 over the tiles and are rounded to bf16 once (863-864): as F4, returned before that rounding.
      The table gradients are f32: a workgroup's partial table (851), then deberta_pos_reduce_kernel's sum over blocks and items
      in a fixed order (886-895), ADDED to what dposq / dposk held.

Bounds (``bounds``), all from the reference and the project's two constants BF16_TOL = 2^-8 and F32_TOL = 1e-5:
  O, dQ, dK, dV   BF16_TOL max|ref| over the (item, head) slice + N.  N = max|staged - perturbed| of that case and output, the
                  reference's own sensitivity to f32-sized errors in the scores (every score multiplied by 1 + 2^-22 u: flipped
                  roundings at F3 / B3 / B4 / B5); for dQ and dK plus, per element, the f32 summation noise of dP - delta carried
                  through dS (``deberta_dropout_ref.attention_backward``'s noise, each sum held to F32_TOL x its terms'
                  magnitudes): where the softmax is one-hot (T = 1, one unmasked token) dP - delta cancels to 0 exactly and a
                  kernel returns that noise.
  lse             F32_TOL max(|ref|, 1) per element, on unmasked query rows.
  delta           per row F32_TOL sum|O dO| of the operands given.
  dposQ, dposK    per element BF16_TOL sum|bucket sum| |own vector element| over that element's own contraction (every
                  (item, own token, tile) term of B5) + the f32-noise term of that element.  The scale is local to the table row.
"""
import math
import types

import numpy as np
import torch

import attn_ref
import deberta_dropout_ref as D
import deberta_grad_ref as G

F64 = torch.float64
BF16_TOL = 2.0 ** -8                 # tests/test_kernel_forms_gpu.py's (the GPU file asserts they are the same)
F32_TOL = 1e-5
PERTURB = attn_ref.PERTURB           # 2^-22
FLT_MAX = float(np.finfo(np.float32).max)
BQ, BK, NIDX, CROWS, PROWS = 64, 32, 95, 48, 96          # DB_BQ, DB_BK, DB_NIDX, DB_CROWS, DB_PROWS

ROUND = types.SimpleNamespace(bf16=attn_ref.bf16r, f32=attn_ref.f32r, inv=lambda x: float(np.float32(1.0) / np.float32(x)))
IDENTITY = types.SimpleNamespace(bf16=lambda x: x, f32=lambda x: x, inv=lambda x: 1.0 / x)


# ---- scores -------------------------------------------------------------------------------------------------------------
def pair_index(idx, T):
    """(T, T): idx(i - j)"""
    ar = torch.arange(T)
    return idx.long()[(ar[:, None] - ar[None, :]) + T - 1]


def staged_scores(q, k, posq, posk, idx, scale, rnd=ROUND, perturb=0.0, seed=1, mut=None):
    """F1 -> (s (n, H, T, T) before masking, ix (T, T)).  Unmutated, the raw sum is ``deberta_grad_ref.scores`` at scale 1.
    ``mut``: dict(ix= a (T, T) index to gather with, drop_c2p= / drop_p2c= (T, T) bool pairs that lose that term)."""
    n, H, T, _ = q.shape
    mut = mut or {}
    if not mut:
        raw, ix = G.scores(q, k, posq, posk, idx, 1.0)
    else:
        ix = mut.get("ix", pair_index(idx, T))
        c2p = torch.gather(q @ posk.transpose(-1, -2), -1, ix.expand(n, H, T, T))
        p2c = torch.gather(k @ posq.transpose(-1, -2), -1, ix.t().expand(n, H, T, T)).transpose(-1, -2)
        if "drop_c2p" in mut:
            c2p = c2p.masked_fill(mut["drop_c2p"], 0.0)
        if "drop_p2c" in mut:
            p2c = p2c.masked_fill(mut["drop_p2c"], 0.0)
        raw = q @ k.transpose(-1, -2) + c2p + p2c
    s = raw * rnd.inv(scale)
    if perturb:
        g = torch.Generator().manual_seed(seed)
        s = s * (1.0 + perturb * (2.0 * torch.rand(s.shape, generator=g, dtype=F64) - 1.0))
    return s, ix


def _masks(mask, n, H, T):
    m = torch.ones(n, T, dtype=torch.bool) if mask is None else mask != 0
    keep = (m[:, :, None] & m[:, None, :])[:, None].expand(n, H, T, T)
    return m, keep, m[:, None, :, None].expand(n, H, T, T)


# ---- forward ------------------------------------------------------------------------------------------------------------
def forward(q, k, v, posq, posk, idx, mask, scale, w=None, rnd=ROUND, perturb=0.0, mut=None):
    """F1 - F4 -> (O (n, H, T, 64) before its rounding, lse (n, H, T)).  ``mut`` as ``staged_scores`` plus dup= (T, T) weights a
    pair's probability is counted with (1 everywhere in the kernel)."""
    n, H, T, dh = q.shape
    s, _ = staged_scores(q, k, posq, posk, idx, scale, rnd, perturb, mut=mut)
    _, keep, _ = _masks(mask, n, H, T)
    s = torch.where(keep, s, torch.full((), -FLT_MAX, dtype=F64))                                     # F2
    dup = (mut or {}).get("dup")
    m_run = torch.full((n, H, T), -math.inf, dtype=F64)
    l = torch.zeros(n, H, T, dtype=F64)
    o = torch.zeros(n, H, T, dh, dtype=F64)
    for j0 in range(0, T, BK):                                                                        # F3
        sl = slice(j0, min(j0 + BK, T))
        m_new = torch.maximum(m_run, s[..., sl].max(-1).values)
        alpha = torch.exp(m_run - m_new)
        p = torch.exp(s[..., sl] - m_new[..., None])
        if dup is not None:
            p = p * dup[:, sl]
        l = l * alpha + p.sum(-1)
        pd = p if w is None else p * w[..., sl]
        o = o * alpha[..., None] + rnd.bf16(pd) @ v[:, :, sl]
        m_run = m_new
    return o / l[..., None], m_run + torch.log(l)


# ---- backward -----------------------------------------------------------------------------------------------------------
def backward(q, k, v, posq, posk, idx, mask, scale, dO, o16, lse32, w=None, rnd=ROUND, perturb=0.0, mut=None):
    """D1, B1 - B7 on the bf16 ``o16`` and f32 ``lse32`` the kernels are handed -> dict(dq, dk, dv (n, H, T, 64) before their
    rounding, dposq, dposk (H, 2S, 64), delta (n, H, T), sposq, sposk: sum|bucket sum| |own vector element| of every element
    of dposq / dposk)"""
    n, H, T, dh = q.shape
    R = posq.shape[1]
    s, ix = staged_scores(q, k, posq, posk, idx, scale, rnd, perturb, mut=mut)
    m, keep, q_on = _masks(mask, n, H, T)
    zero = torch.zeros((), dtype=F64)
    lse_safe = torch.where(m[:, None, :], lse32, zero)
    P = torch.where(keep, torch.exp(s - lse_safe[..., None]), zero)                                   # B1
    P = torch.where(q_on, P, torch.full((), rnd.inv(float(T)), dtype=F64))
    delta = rnd.f32((dO * o16).sum(-1))                                                               # D1
    dP = dO @ v.transpose(-1, -2)                                                                     # B2
    if w is not None:
        dP = dP * w
    dS = torch.where(keep, P * (dP - delta[..., None]), zero) * rnd.inv(scale)                        # B3
    dv = rnd.bf16(P if w is None else P * w).transpose(-1, -2) @ dO                                   # B4
    ds16 = rnd.bf16(dS)
    dq, dk = ds16 @ k, ds16.transpose(-1, -2) @ q
    out = dict(delta=delta, dv=dv, dposq=torch.zeros(H, R, dh, dtype=F64), dposk=torch.zeros(H, R, dh, dtype=F64),
               sposq=torch.zeros(H, R, dh, dtype=F64), sposk=torch.zeros(H, R, dh, dtype=F64))
    dSt = dS.transpose(-1, -2)
    for o0 in range(0, T, BK):                                                                        # B5: one tile of others
        sl = slice(o0, min(o0 + BK, T))
        nt = sl.stop - sl.start
        A = rnd.bf16(torch.zeros(n, H, T, R, dtype=F64).scatter_add_(-1, ix[:, sl].expand(n, H, T, nt), dS[..., sl]))          # [i, r]
        B = rnd.bf16(torch.zeros(n, H, T, R, dtype=F64).scatter_add_(-1, ix[sl, :].t().expand(n, H, T, nt), dSt[..., sl]))     # [j, r]
        dq, dk = dq + A @ posk, dk + B @ posq
        out["dposk"] += torch.einsum("nhir,nhid->hrd", A, q)
        out["dposq"] += torch.einsum("nhjr,nhjd->hrd", B, k)
        out["sposk"] += torch.einsum("nhir,nhid->hrd", A.abs(), q.abs())
        out["sposq"] += torch.einsum("nhjr,nhjd->hrd", B.abs(), k.abs())
    out.update(dq=dq, dk=dk)
    return out


def perturbed(q, k, v, posq, posk, idx, mask, scale, dO, o16, lse32, w=None, backward_too=True):
    """the staged outputs with every score perturbed by a seeded relative 2^-22 (o, lse, and the backward's on the SAME o16 /
    lse32), and per element the f32-noise terms ndq, ndk, ndposq, ndposk of ``deberta_dropout_ref.attention_backward``"""
    o, lse = forward(q, k, v, posq, posk, idx, mask, scale, w, perturb=PERTURB)
    out = dict(o=o, lse=lse)
    if backward_too:
        out.update(backward(q, k, v, posq, posk, idx, mask, scale, dO, o16, lse32, w, perturb=PERTURB))
        ones = torch.ones(q.shape[0], q.shape[1], q.shape[2], q.shape[2], dtype=F64) if w is None else w
        _, (ndq, ndk, _, ndposq, ndposk) = D.attention_backward(q, k, v, posq, posk, idx, mask, scale, dO, ones, o16, lse32, F32_TOL)
        out.update(ndq=ndq, ndk=ndk, ndposq=ndposq, ndposk=ndposk)
    return out


def reference(q, k, v, posq, posk, idx, mask, scale, dO, w=None, backward_too=True):
    """everything a test needs of one problem: the staged outputs, o16 / lse32, the perturbed twin and ``bound`` per output"""
    n, H, T, _ = q.shape
    o, lse = forward(q, k, v, posq, posk, idx, mask, scale, w)
    ref = dict(o=o, lse=lse, o16=attn_ref.bf16r(o), lse32=attn_ref.f32r(lse))
    if backward_too:
        ref.update(backward(q, k, v, posq, posk, idx, mask, scale, dO, ref["o16"], ref["lse32"], w))
    twin = perturbed(q, k, v, posq, posk, idx, mask, scale, dO, ref["o16"], ref["lse32"], w, backward_too)
    ref["twin"] = twin
    ref["bound"] = bounds(ref, twin, dO, backward_too)
    ref["on"] = torch.ones(n, T, dtype=torch.bool) if mask is None else mask != 0
    return ref


def bounds(ref, twin, dO, backward_too=True):
    slice_max = lambda t: t.abs().amax(dim=(-1, -2), keepdim=True)
    N = lambda key: float((ref[key] - twin[key]).abs().max())
    b = dict(o=BF16_TOL * slice_max(ref["o"]) + N("o") + torch.zeros_like(ref["o"]),
             lse=F32_TOL * ref["lse"].abs().clamp_min(1.0))
    if backward_too:
        b["dq"] = BF16_TOL * slice_max(ref["dq"]) + N("dq") + twin["ndq"]
        b["dk"] = BF16_TOL * slice_max(ref["dk"]) + N("dk") + twin["ndk"]
        b["dv"] = BF16_TOL * slice_max(ref["dv"]) + N("dv") + torch.zeros_like(ref["dv"])
        b["delta"] = F32_TOL * (dO * ref["o16"]).abs().sum(-1)
        b["dposq"] = BF16_TOL * ref["sposq"] + twin["ndposq"]
        b["dposk"] = BF16_TOL * ref["sposk"] + twin["ndposk"]
    return b


# ---- the kernels' window arithmetic ---------------------------------------------------------------------------------------
def db_idx(idx, delta, T, S2):
    return min(max(int(idx[min(max(delta, -(T - 1)), T - 1) + T - 1]), 0), S2 - 1)


def db_chunks(rows, lo, hi):
    return min(max((hi - lo) // 16 + 1, 1), rows // 16)


def tile_window(idx, T, S2, block, tile, kpass=False):
    """the 95 sIdx values of (own block, other tile): slot t belongs to the pairs with own - other + 31 = t (db_fill_idx)"""
    sgn = -1 if kpass else 1
    d0 = sgn * (block * BQ - tile * BK - (BK - 1))
    return [db_idx(idx, d0 + sgn * t, T, S2) for t in range(NIDX)]


def window_forms(T, S, idx_or_max_position):
    """for every (pass, block, tile, wave) whose wave owns a token below T: the wave window's (lo_c, hi_c) at slots 16 w and
    16 w + 46 and its C2P chunk count (1 - 3), the block window's (lo_p, hi_p) at slots 0 and 94 and its P2C chunk count (1 - 6).
    -> dict(fwd=[...], kpass=[...]) of namespaces; the dK/dV pass has the delta negated (and the two tables swapped)."""
    import deberta_ref
    idx = deberta_ref.bucket_index(T, S, idx_or_max_position) if isinstance(idx_or_max_position, int) else idx_or_max_position
    idx, S2, out = idx.tolist(), 2 * S, {}
    for name, kpass in (("fwd", False), ("kpass", True)):
        rows = out[name] = []
        for b in range((T + BQ - 1) // BQ):
            for t in range((T + BK - 1) // BK):
                sidx = tile_window(idx, T, S2, b, t, kpass)
                lo_p, hi_p = sorted((sidx[0], sidx[NIDX - 1]))
                for wv in range(4):
                    if b * BQ + 16 * wv >= T:
                        continue
                    lo_c, hi_c = sorted((sidx[16 * wv], sidx[16 * wv + 46]))
                    rows.append(types.SimpleNamespace(block=b, tile=t, wave=wv, lo_c=lo_c, hi_c=hi_c, lo_p=lo_p, hi_p=hi_p,
                                                      ncc=db_chunks(CROWS, lo_c, hi_c), npc=db_chunks(PROWS, lo_p, hi_p)))
    return out


def forms_summary(forms):
    """-> per pass: (set of C2P counts, set of P2C counts, set of wave-window widths hi_c - lo_c)"""
    return {name: ({r.ncc for r in rows}, {r.npc for r in rows}, {r.hi_c - r.lo_c for r in rows}) for name, rows in forms.items()}


# ---- index tables that satisfy the contract ---------------------------------------------------------------------------------
def contract_ok(idx, S):
    """what mmfusion/deberta.py checks of the table it builds (``NativeDeberta._index``): non-decreasing in delta with steps of at
    most 1; and the rows exist (include/mmfusion.h)"""
    step = idx[1:] - idx[:-1]
    return bool(idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) <= 2 * S - 1
                and (idx.numel() == 1 or (int(step.min()) >= 0 and int(step.max()) <= 1)))


def linear(T, S):
    """clamp(delta + S, 0, 2S - 1): a new row at every delta, the widest window everywhere"""
    return torch.clamp(torch.arange(-(T - 1), T) + S, 0, 2 * S - 1).to(torch.int32)


def constant(T, S, r):
    return torch.full((2 * T - 1,), r, dtype=torch.int32)


STEP_WINDOWS = ((-111, 15), (-63, 16), (-15, 31), (33, 32), (81, 46))


def steps_at(T, S, windows=STEP_WINDOWS):
    """flat but for ``windows`` = ((D, k), ...): the first k of the 46 transitions D -> D + 46 step by one.  A wave window is the 47
    deltas from 64 b - 32 t - 31 + 16 w (= 1 mod 16; the dK/dV pass's are the same sets), so with D = 1 mod 16 inside the deltas
    of a real (block, tile, wave) the window's hi - lo is exactly k: 15 | 16 and 31 | 32 are the two sides of db_chunks'
    divisions, 46 the most a wave window can span."""
    step = torch.zeros(2 * T - 2, dtype=torch.int64)
    for D0, kk in windows:
        assert D0 % 16 == 1 and -(T - 1) <= D0 and D0 + 46 <= T - 1 and 0 <= kk <= 46
        step[D0 + T - 1:D0 + T - 1 + kk] += 1
    assert int(step.max()) <= 1
    idx = torch.cat([torch.zeros(1, dtype=torch.int64), step.cumsum(0)])
    idx = idx + (S - int(idx[T - 1]))                       # delta 0 reads row S
    assert int(idx.min()) >= 0 and int(idx.max()) <= 2 * S - 1
    return idx.to(torch.int32)


# ---- mutants: the reference with one localized fault ----------------------------------------------------------------------------
def chunk_pairs(T, idx, S, term, block, tile, wave, chunk):
    """(T, T) bool: the forward's (query, key) pairs of (block, tile[, wave]) whose ``term`` ("c2p": the wave's window; "p2c":
    the block's) is gathered from row chunk ``chunk`` of the window"""
    S2 = 2 * S
    sidx = tile_window(idx.tolist(), T, S2, block, tile)
    lo = min(sidx[16 * wave], sidx[16 * wave + 46]) if term == "c2p" else min(sidx[0], sidx[NIDX - 1])
    ix = pair_index(idx, T)
    sel = torch.zeros(T, T, dtype=torch.bool)
    i0 = block * BQ + (16 * wave if term == "c2p" else 0)
    i1 = min(i0 + (16 if term == "c2p" else BQ), T)
    j0, j1 = tile * BK, min(tile * BK + BK, T)
    off = ix[i0:i1, j0:j1] - lo
    sel[i0:i1, j0:j1] = (off >= 16 * chunk) & (off < 16 * chunk + 16)
    return sel


def mut_drop_chunk(T, idx, S, term, block, tile, wave, chunk):
    """that window forms no chunk ``chunk``: its pairs lose the term"""
    return {("drop_" + term): chunk_pairs(T, idx, S, term, block, tile, wave, chunk)}


def mut_double_last_key(T, rows=16):
    """the last ``rows`` queries count key T - 1 twice (a ragged tail read twice)"""
    dup = torch.ones(T, T, dtype=F64)
    dup[T - rows:, T - 1] = 2.0
    return dict(dup=dup)


def mut_shift_extreme_rows(T, idx, S):
    """the pairs that gather the table's two end rows read the neighbouring row instead (a clamp off by one)"""
    ix = pair_index(idx, T)
    ix = torch.where(ix == 2 * S - 1, torch.full_like(ix, 2 * S - 2), torch.where(ix == 0, torch.ones_like(ix), ix))
    return dict(ix=ix)


def mut_table_rows(dpos, rows, factor):
    """a table gradient (H, 2S, 64) with ``rows`` multiplied by ``factor`` (2: added twice; 0: never written)"""
    out = dpos.clone()
    out[:, rows] *= factor
    return out


# ---- the problems the two test files share --------------------------------------------------------------------------------
SCALE = math.sqrt(3.0 * 64)
CASES = {                                   # name -> (n, H, T, S, max_position | the name of a synthetic table)
    "a": (1, 3, 1, 8, 32),                  # T = 1
    "b": (1, 2, 33, 8, 32),                 # one key past a tile
    "c": (2, 2, 70, 8, 32),                 # both clamps; ragged second query block
    "d": (1, 2, 130, 32, 128),              # small table, every C2P count
    "e": (2, 2, 200, 256, 512),             # real geometry, linear and log region
    "f": (1, 1, 530, 256, 512),             # T > max_position; all nine chunk counts
    "g_linear": (1, 2, 160, 256, "linear"),         # full-width windows
    "g_constant": (1, 2, 160, 256, "constant"),     # one-row windows
    "g_steps": (1, 2, 160, 256, "steps_at"),        # the chunk-division edges
    "h": (1, 1, 200, 128, "linear"),        # deltas -199 .. 199 on 256 rows: both far-end clamps bind, neighbouring rows differ
}
MASKS = ("tail", "left", "hole", "one", "empty_item")          # on case c's geometry


def case_index(name):
    """``name``: a key of CASES, or such a tuple itself"""
    import deberta_ref
    n, H, T, S, table = CASES[name] if isinstance(name, str) else name
    if isinstance(table, int):
        return deberta_ref.bucket_index(T, S, table)
    return {"linear": lambda: linear(T, S), "constant": lambda: constant(T, S, S + 3), "steps_at": lambda: steps_at(T, S)}[table]()


def case_mask(name, kind):
    """(n, T) f32 of ones and zeros on item n - 1 (the other items stay whole)"""
    n, _, T = (CASES[name] if isinstance(name, str) else name)[:3]
    m = torch.ones(n, T)
    if kind == "tail":
        m[n - 1, 50:] = 0
    elif kind == "left":                    # the first 32-key tile fully masked, the second partly
        m[n - 1, :40] = 0
    elif kind == "hole":
        m[n - 1, 20:46] = 0
    elif kind == "one":
        m[n - 1] = 0
        m[n - 1, 37] = 1
    elif kind == "empty_item":              # a missing modality: ids and mask all 0, next to a normal item
        m[n - 1] = 0
    else:
        raise KeyError(kind)
    return m


def problem(name, mask_kind=None, n=None, H=None):
    """the operands of a case as the kernels take them (bf16 rows) and as the reference does (float64 heads)"""
    from test_deberta_gpu import _attn_case
    n0, H0, T, S, table = CASES[name] if isinstance(name, str) else name
    n, H = n or n0, H or H0
    qkv, posq, posk, _, _ = _attn_case(n, H, T, S, table if isinstance(table, int) else 512)
    idx = case_index(name)
    assert contract_ok(idx, S)
    d = H * 64
    dout = torch.randn(n * T, d, generator=torch.Generator().manual_seed(7 * T + S)).to(torch.bfloat16)
    hd = lambda t: t.double().reshape(n, T, H, 64).transpose(1, 2)
    q, k, v = (hd(qkv[:, i * d:(i + 1) * d]) for i in range(3))
    pq, pk = (t.double().reshape(2 * S, H, 64).transpose(0, 1) for t in (posq, posk))
    mask = None if mask_kind is None else case_mask(name, mask_kind)
    return types.SimpleNamespace(name=name, n=n, H=H, T=T, S=S, d=d, qkv=qkv, posq=posq, posk=posk, idx=idx, mask=mask, dout=dout,
                                 args=(q, k, v, pq, pk, idx, mask, SCALE), dO=hd(dout))


def rows_of(t):
    """(n, H, T, 64) -> (n T, H 64)"""
    n, H, T, dh = t.shape
    return t.transpose(1, 2).reshape(n * T, H * dh)


def table_of(t):
    """(H, 2S, 64) -> (2S, H 64)"""
    H, R, dh = t.shape
    return t.transpose(0, 1).reshape(R, H * dh)
