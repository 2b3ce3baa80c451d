"""CPU: properties of the keyed-dropout restatement (tests/keyed_dropout_ref.py) that tests/test_keyed_masks_gpu.py holds the
kernels to — so that the GPU tests compare against something that has itself been checked: keep rates, independence of the
masks of different problems / sites / states / neighbouring rows and columns (two independent Bernoulli(0.75) masks agree on
0.75^2 + 0.25^2 = 0.625 of their elements), the modality fallback, and literal hash values (computed once by a C transcription of
csrc/mmf_internal.h's three functions in uint32 arithmetic) that a later edit of the helper cannot move."""
import math

import numpy as np
import torch

import keyed_dropout_ref as K

STATE = (0x1234567 << 32) | 0x89ABCDEF
SITE, P = 5, 0.25
THRESH = K.mmf_drop_thresh(P)
M, N = 300, 264


def within(frac, q, n):
    return abs(frac - q) <= 4.0 * math.sqrt(q * (1.0 - q) / n)


def agree(a, b):
    return float((a == b).mean())


def test_threshold_and_scale():
    assert THRESH == 1 << 30 and K.inv_keep_of(THRESH) == float(np.float32(1) / np.float32(0.75))
    assert K.mmf_drop_thresh(0.0) == 0 and K.inv_keep_of(0) == 1.0
    assert K.mmf_drop_thresh(0.5) == 1 << 31 and K.mmf_drop_thresh(0.99999999) == 4294967295


def test_gemm_keep_rate_and_independence():
    k = K.gemm_keep(STATE, SITE, 0, M, N, THRESH)
    assert k.shape == (M, N) and k.dtype == np.bool_
    assert within(float(k.mean()), 1 - P, M * N), float(k.mean())
    q = (1 - P) ** 2 + P ** 2
    others = {"problem": K.gemm_keep(STATE, SITE, 1, M, N, THRESH), "site": K.gemm_keep(STATE, SITE + 1, 0, M, N, THRESH),
              "state": K.gemm_keep(STATE + 1, SITE, 0, M, N, THRESH), "high word": K.gemm_keep(STATE + (1 << 32), SITE, 0, M, N, THRESH)}
    for what, o in others.items():
        assert within(float(o.mean()), 1 - P, M * N), (what, float(o.mean()))
        assert within(agree(k, o), q, M * N), (what, agree(k, o))
    assert within(agree(k[:-1], k[1:]), q, (M - 1) * N), agree(k[:-1], k[1:])              # adjacent rows: not idx = n
    assert within(agree(k[:, :-1], k[:, 1:]), q, M * (N - 1)), agree(k[:, :-1], k[:, 1:])  # adjacent columns
    # the index is m * N + n with THIS N: the same stream read at another width is the same sequence re-wrapped
    assert np.array_equal(k.reshape(-1), K.gemm_keep(STATE, SITE, 0, 1, M * N, THRESH).reshape(-1))
    assert np.array_equal(K.gemm_keep(STATE, SITE, 0, 1, 5000, THRESH)[0], K.elementwise_keep(STATE, SITE, 5000, THRESH))   # sub 0 = mmf_dropout's stream


def test_gat3_keep_layout():
    B, H = 5, 4
    k = K.gat3_keep(STATE, SITE, B, H, K.mmf_drop_thresh(0.5))
    assert k.shape == (B, 3, 3, H)
    for b in (0, 4):
        key = K.mmf_rng_key(STATE, SITE, b)
        for (i, j, h) in ((0, 0, 0), (1, 2, 3), (2, 1, 0), (2, 2, 3)):
            assert bool(k[b, i, j, h]) == bool(K.mmf_keep(key, (3 * i + j) * H + h, K.mmf_drop_thresh(0.5)))
    big = K.gat3_keep(STATE, SITE, 400, 8, K.mmf_drop_thresh(0.5))
    assert within(float(big.mean()), 0.5, big.size)
    assert within(agree(big[:-1], big[1:]), 0.5, big[1:].size)                               # per-sample streams
    upper = np.stack([big[:, i, j] for i, j in ((0, 1), (0, 2), (1, 2))])
    lower = np.stack([big[:, j, i] for i, j in ((0, 1), (0, 2), (1, 2))])
    assert within(agree(upper, lower), 0.5, upper.size)                                       # (i, j) is not (j, i)


def test_modality_keep_fallback():
    for p, rows, least in ((0.8, 125, (39, 43, 43)), (0.5, 29, (6, 10, 13))):
        keep, fell = K.modality_keep(STATE, 9, 257, K.mmf_drop_thresh(p))
        assert keep.shape == (257, 3) and fell.shape == (257,)
        assert bool(keep.any(axis=1).all())
        assert int(fell.sum()) == rows
        assert bool((keep[fell].sum(axis=1) == 1).all())
        picks = np.bincount(keep[fell].argmax(axis=1), minlength=3)
        assert tuple(int(c) for c in picks) == least, picks
        raw = K.mmf_keep(K.mmf_rng_key(STATE, 9, 0), np.arange(3 * 257, dtype=np.uint64), K.mmf_drop_thresh(p)).reshape(257, 3)
        assert np.array_equal(keep[~fell], raw[~fell]) and not bool(raw[fell].any())
    keep, fell = K.modality_keep(STATE, 9, 257, K.mmf_drop_thresh(0.8))
    assert int(fell.sum()) >= 60 and min(np.bincount(keep[fell].argmax(axis=1), minlength=3)) >= 15


def test_ops_state():
    assert K.ops_state(0x7654321, 2) == 0x0000765432100002
    assert K.ops_state(-1, 0) == 0x7FFFFFFF << 20 and K.ops_state(1 << 31, 5) == 5
    assert K.ops_state(0x7654321, 2) >> 32 != 0
    assert int(K.state_tensor(0xFFFFFFFFFFFFFFFF, "cpu")) == -1 and int(K.state_tensor(STATE, "cpu")) == STATE


# (state, site, sub, idx, mmf_rng_key, mmf_mix32(key + idx * 0x9E3779B9)): uint32 arithmetic of csrc/mmf_internal.h
FIXED = [
    (0x0123456789ABCDEF, 0x5, 0x0, 0x0, 0x60C3B8AB, 0xDB25F24A),
    (0x0123456789ABCDEF, 0x1, 0x3, 0x1355F, 0x036ADFB3, 0xCF97D542),
    (0x0123456789ABCDEF, 0xFFFFFFFF, 0x1001, 0x0, 0x7C84D7B5, 0x383DD916),
    (0x0123456789ABCDEF, 0x0, 0xFFFFFFFF, 0x1355F, 0x2065B382, 0x07101BD3),
    (0xFFFFFFFFFFFFFFFF, 0x5, 0x3, 0x1, 0xFE1FE161, 0xCDA935FB),
    (0xFFFFFFFFFFFFFFFF, 0x1, 0x1001, 0xFFFFFFFF, 0x888C6635, 0x679C3A86),
    (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x1, 0x211C4306, 0xD88C5A95),
    (0xFFFFFFFFFFFFFFFF, 0x0, 0x0, 0xFFFFFFFF, 0x98977DB5, 0x4B0B86D9),
    (0x0000765432100002, 0x5, 0x1001, 0x1355F, 0x74A80B3B, 0x87429F56),
    (0x0000765432100002, 0x1, 0xFFFFFFFF, 0x0, 0x2F347BBC, 0x41A1DE4B),
    (0x0000765432100002, 0xFFFFFFFF, 0x0, 0x1355F, 0x23A77374, 0x76914ACE),
    (0x0000765432100002, 0x0, 0x3, 0x0, 0xC23F55F8, 0xE1566D44),
    (0x0000000000000000, 0x5, 0xFFFFFFFF, 0xFFFFFFFF, 0x7F6B826C, 0xB09BF751),
    (0x0000000000000000, 0x1, 0x0, 0x1, 0x01FCE552, 0xA0117BE9),
    (0x0000000000000000, 0xFFFFFFFF, 0x3, 0xFFFFFFFF, 0xEF172610, 0x71A7CCDA),
    (0x0000000000000000, 0x0, 0x1001, 0x1, 0x42927A6B, 0x6774FB84),
]


def test_fixed_points():
    for state, site, sub, idx, key, h in FIXED:
        assert int(K.mmf_rng_key(state, site, sub)) == key, (hex(state), site, sub)
        assert bool(K.mmf_keep(key, idx, h)) and (h == 0xFFFFFFFF or not bool(K.mmf_keep(key, idx, h + 1))), (hex(key), idx)   # the hash value is exactly h
    # index 0x1355F is the last element (299, 263) of a 300 x 264 problem: gemm_keep reads the same hash there
    assert 0x1355F == 299 * 264 + 263
    k = K.gemm_keep(0x0123456789ABCDEF, 1, 3, 300, 264, 0xCF97D542)
    assert bool(k[299, 263]) and not bool(K.gemm_keep(0x0123456789ABCDEF, 1, 3, 300, 264, 0xCF97D543)[299, 263])
    # the modality fallback's pick for rows 7 and 2^32 - 1 under the key of (state, site 9, sub 0)
    key = K.mmf_rng_key(0x0123456789ABCDEF, 9, 0)
    pick = [int(K.mmf_mix32(key ^ np.uint64((K.FALLBACK_SALT + b) & 0xFFFFFFFF)) % np.uint64(3)) for b in (7, 0xFFFFFFFF)]
    assert pick == [0, 2]


def test_epilogue_order():
    """each stage against a scalar worked by hand: acc 1.5, bias -0.5 -> 1; relu; kept x 4/3; aux > 0; x 2; + aux; + C_old"""
    one = lambda v: torch.tensor([[v]], dtype=torch.float64)     # noqa: E731
    kw = dict(bias=torch.tensor([-0.5], dtype=torch.float64), relu=True, keep=np.array([[True]]), inv_keep=4.0 / 3.0, alpha=2.0)
    assert float(K.epilogue(one(1.5), **kw)) == 1.0 * (4.0 / 3.0) * 2.0
    assert float(K.epilogue(one(1.5), add_aux=one(-7.0), c_old=one(0.25), **kw)) == 1.0 * (4.0 / 3.0) * 2.0 - 7.0 + 0.25   # the residual and old C: neither dropped nor scaled
    kw["keep"] = np.array([[False]])
    assert float(K.epilogue(one(1.5), add_aux=one(-7.0), c_old=one(0.25), **kw)) == -6.75
    assert float(K.epilogue(one(1.5), mask_aux=one(0.0), alpha=2.0)) == 0.0 and float(K.epilogue(one(1.5), mask_aux=one(-1.0))) == 0.0
    assert float(K.epilogue(one(1.5), mask_aux=one(0.5), alpha=2.0)) == 3.0
    assert float(K.epilogue(one(0.25), bias=torch.tensor([-0.5], dtype=torch.float64), relu=True, keep=np.array([[True]]), inv_keep=2.0)) == 0.0   # bias before relu
    b = K.epilogue_bound(one(3.0), one(2.0), 8, True, keep=np.array([[True]]), inv_keep=2.0, alpha=0.5)
    assert float(b) == 8 * 2.0 ** -24 * 2.0 + 2.0 ** -8 * 3.0
    assert float(K.epilogue_bound(one(0.0), one(2.0), 8, True, keep=np.array([[False]]), inv_keep=2.0)) == 0.0
