"""CPU: the host side of the grouped-attention entry points of include/mmfusion.h (mmf_attn_fwd_grouped[_ex|_keyed],
mmf_attn_bwd_grouped[_ex|_delta|_delta_keyed|_uniform|_pooled], mmf_attn_delta_f32[_keyed]) and of the pure functions beside them
(mmf_attn_bwd_grouped_uniform_available, _uniform_workspace_bytes, mmf_attn_select_impl).  Validation launches nothing, so it runs
without a GPU on made-up (aligned) addresses.  Only refused calls and pure functions are here: every call below is answered by the
entry point's validation, or by the launch function's 2 GiB descriptor rule, BEFORE a kernel is enqueued — a case that got past them
would launch on addresses nobody owns.  The answers (code, the entry's own name in the message, the order of the checks) are the
ones the library gave before the entries shared their validation and the launches their dispatch (profiles/attention_shared_parts.txt)."""
import ctypes as C

from mmfusion import lib

E_SHAPE, E_ALIGN, E_LAUNCH, E_UNSUPPORTED = -1, -3, -4, -5
BASE = 0x7F0000000000                       # addresses are only looked at (null, alignment), never followed
RNG, WS, DY = BASE + 0x70000000, BASE + 0x71000000, BASE + 0x72000000
SCALE = 0.125
OPERANDS = ("Q", "K", "V", "O", "LSE", "dO", "delta", "dQ", "dK", "dV")


def _problem(B=1, H=2, Tq=8, Tk=8, ld=128, **kw):
    p = lib.AttnProblem()
    for i, name in enumerate(OPERANDS):
        setattr(p, name, BASE + 0x01000000 * (i + 1))
    p.B, p.H, p.Tq, p.Tk = B, H, Tq, Tk
    p.ldq = p.ldk = p.ldv = p.ldo = ld
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Entry:
    """one entry point: ``who`` is the name its operand validation prints, ``own`` the name its own further checks print (dropout rule,
    workspace, pooled gradient), ``ranges`` the name the 2 GiB rule prints (None: the entry has no descriptor behind it)"""

    def __init__(self, name, who, own, ranges, bwd, drop=None, delta=False):
        self.name, self.who, self.own, self.ranges, self.bwd, self.drop, self.delta = name, who, own, ranges, bwd, drop, delta

    def __call__(self, problems, head_dim=64, n=None, p=0.0, rng=None, base=0, ws=WS, ws_bytes=1 << 40, dys="aligned", lddy=1536):
        L = lib.load()
        arr = (lib.AttnProblem * max(1, len(problems)))(*problems) if problems is not None else None
        n = len(problems) if n is None else n
        f = getattr(L, self.name)
        if self.drop == "ex":
            rc = f(arr, n, head_dim, SCALE, p, rng, 3, None)
        elif self.drop == "keyed":
            rc = f(arr, n, head_dim, SCALE, p, rng, 3, base, None)
        elif self.name == "mmf_attn_bwd_grouped_uniform":
            rc = f(arr, n, head_dim, SCALE, ws, ws_bytes, None)
        elif self.name == "mmf_attn_bwd_grouped_pooled":
            if dys == "aligned":
                dys = [DY + 0x10000 * i for i in range(max(1, n))]
            rc = f(arr, n, head_dim, SCALE, (C.c_void_p * len(dys))(*dys) if dys is not None else None, lddy, ws, ws_bytes, None)
        else:
            rc = f(arr, n, head_dim, SCALE, None)
        assert rc not in (0, E_LAUNCH), "a case of this file reached a launch"
        return rc, L.mmf_last_error().decode()


ENTRIES = [
    Entry("mmf_attn_fwd_grouped", "mmf_attn_fwd_grouped", None, "mmf_attn_fwd_grouped", False),
    Entry("mmf_attn_fwd_grouped_ex", "mmf_attn_fwd_grouped", "mmf_attn_fwd_grouped_ex", "mmf_attn_fwd_grouped", False, "ex"),
    Entry("mmf_attn_fwd_grouped_keyed", "mmf_attn_fwd_grouped_keyed", "mmf_attn_fwd_grouped_keyed", "mmf_attn_fwd_grouped", False, "keyed"),
    Entry("mmf_attn_bwd_grouped", "mmf_attn_bwd_grouped", None, "mmf_attn_bwd_grouped", True),
    Entry("mmf_attn_bwd_grouped_ex", "mmf_attn_bwd_grouped", "mmf_attn_bwd_grouped_ex", "mmf_attn_bwd_grouped", True, "ex"),
    Entry("mmf_attn_bwd_grouped_delta", "mmf_attn_bwd_grouped_delta", None, "mmf_attn_bwd_grouped", True),
    Entry("mmf_attn_bwd_grouped_delta_keyed", "mmf_attn_bwd_grouped_delta_keyed", "mmf_attn_bwd_grouped_delta_keyed", "mmf_attn_bwd_grouped",
          True, "keyed"),
    Entry("mmf_attn_bwd_grouped_uniform", "mmf_attn_bwd_grouped_uniform", "mmf_attn_bwd_grouped_uniform", "mmf_attn_bwd_grouped_uniform", True),
    Entry("mmf_attn_bwd_grouped_pooled", "mmf_attn_bwd_grouped_pooled", "mmf_attn_bwd_grouped_pooled", "mmf_attn_bwd_grouped_uniform", True),
    Entry("mmf_attn_delta_f32", "mmf_attn_delta_f32", None, None, False, delta=True),
    Entry("mmf_attn_delta_f32_keyed", "mmf_attn_delta_f32_keyed", "mmf_attn_delta_f32_keyed", None, False, "keyed", delta=True),
]
DROPPING = [e for e in ENTRIES if e.drop]
KEYED = [e for e in ENTRIES if e.drop == "keyed"]
WORKSPACE = [e for e in ENTRIES if e.name in ("mmf_attn_bwd_grouped_uniform", "mmf_attn_bwd_grouped_pooled")]
POOLED = ENTRIES[8]


def test_every_grouped_entry_is_here():
    grouped = {s for s in lib.SYMBOLS if s.startswith("mmf_attn_") and ("grouped" in s or "delta_f32" in s)}
    assert grouped == {e.name for e in ENTRIES} | {"mmf_attn_bwd_grouped_uniform_available", "mmf_attn_bwd_grouped_uniform_workspace_bytes"}


def test_problem_count_and_head_dim():
    for e in ENTRIES:
        for n in (0, -1, lib.ATTN_MAX_PROBLEMS + 1):
            rc, msg = e([_problem()] * max(n, 1), n=n)
            assert rc == E_SHAPE and msg == "%s: num_problems=%d out of range" % (e.who, n), (e.name, msg)
        rc, msg = e(None, n=1)
        assert rc == E_SHAPE and msg == "%s: num_problems=1 out of range" % e.who, (e.name, msg)
        for hd in (32, 128):
            rc, msg = e([_problem(ld=2 * hd)], head_dim=hd)
            assert rc == E_UNSUPPORTED and msg == "%s: head_dim=%d (supported: 64, 96)" % (e.who, hd), (e.name, msg)
        # the count is looked at before head_dim, head_dim before the problems
        rc, msg = e([_problem()], head_dim=32, n=0)
        assert rc == E_SHAPE and "num_problems=0" in msg, (e.name, msg)
        rc, msg = e([_problem(Q=BASE + 8, ldq=4)], head_dim=128)
        assert rc == E_UNSUPPORTED and "head_dim=128" in msg, (e.name, msg)


def test_each_problem_is_validated():
    strides = "row strides must be >= H*head_dim and multiples of 8"
    for e in ENTRIES:
        cases = [(dict(B=0), E_SHAPE, "B=0 H=2 Tq=8 Tk=8"), (dict(H=0), E_SHAPE, "B=1 H=0"), (dict(Tq=-8), E_SHAPE, "Tq=-8"), (dict(Tk=0), E_SHAPE, "Tk=0")]
        for ld in ("ldq", "ldk", "ldv", "ldo"):
            cases += [({ld: 120}, E_ALIGN, strides), ({ld: 132}, E_ALIGN, strides)]
        cases += [({"ld": 184}, E_ALIGN, strides)]                                       # below H * 96 at head_dim 96 (hd below)
        cases += [({x: None}, E_SHAPE, "null operand") for x in ("Q", "K", "V", "O", "LSE")]
        cases += [({x: getattr(_problem(), x) + 8}, E_ALIGN, "Q/K/V/O must be 16-byte aligned") for x in ("Q", "K", "V", "O")]
        if e.bwd:
            cases += [({x: None}, E_SHAPE, "null gradient operand") for x in ("dO", "delta", "dQ", "dK", "dV")]
            cases += [({x: getattr(_problem(), x) + 8}, E_ALIGN, "gradient pointers must be 16-byte aligned") for x in ("dO", "dQ", "dK", "dV")]
        if e.delta:
            cases += [({x: None}, E_SHAPE, "null gradient operand") for x in ("dO", "delta")]
            cases += [(dict(dO=_problem().dO + 2), E_ALIGN, "gradient pointers must be 16-byte aligned")]
            cases += [(dict(B=65536), E_UNSUPPORTED, "B and H at most 65535"), (dict(H=65536, ld=65536 * 64), E_UNSUPPORTED, "B and H at most 65535")]
        for kw, code, want in cases:
            hd = 96 if kw.get("ld") == 184 else 64
            rc, msg = e([_problem(**kw)], head_dim=hd)
            assert rc == code and msg.startswith(e.who + "[0]: ") and want in msg, (e.name, kw, rc, msg)
            good = _problem(ld=192 if hd == 96 else 128)
            rc, msg = e([good, good, _problem(**kw)], head_dim=hd)                       # the message names the caller's problem
            assert rc == code and msg.startswith(e.who + "[2]: ") and want in msg, (e.name, kw, rc, msg)
        # one problem's checks in their order: sizes, strides, null, alignment, then the gradients
        rc, msg = e([_problem(Tk=0, ldq=4, Q=None)])
        assert rc == E_SHAPE and "Tk=0" in msg, (e.name, msg)
        rc, msg = e([_problem(ldk=4, K=None, V=BASE + 8)])
        assert rc == E_ALIGN and strides in msg, (e.name, msg)
        rc, msg = e([_problem(LSE=None, V=BASE + 8, dO=None)])
        assert rc == E_SHAPE and "null operand" in msg, (e.name, msg)
        rc, msg = e([_problem(O=BASE + 4, dO=None)])
        assert rc == E_ALIGN and "Q/K/V/O" in msg, (e.name, msg)
        if e.bwd:
            rc, msg = e([_problem(dV=None, dO=BASE + 8)])
            assert rc == E_SHAPE and "null gradient operand" in msg, (e.name, msg)


def test_dropout_probability_and_state():
    want = ": dropout needs 0 <= p < 1 and an rng_state"
    for e in DROPPING:
        for p, rng in ((-0.1, RNG), (1.0, RNG), (1.5, RNG), (float("nan"), RNG), (0.1, None)):
            rc, msg = e([_problem()], p=p, rng=rng)
            assert rc == E_SHAPE and msg == e.own + want, (e.name, p, msg)
        # the operands are validated before the dropout arguments, under the name that check prints
        rc, msg = e([_problem(ldq=132)], p=-0.1, rng=RNG)
        assert rc == E_ALIGN and msg.startswith(e.who + "[0]: "), (e.name, msg)


def test_dropout_stream_ids():
    for e in (e for e in DROPPING if e.drop == "ex"):
        rc, msg = e([_problem(B=4097, H=1)], p=0.1, rng=RNG)
        assert rc == E_SHAPE and msg == e.own + "[0]: dropout needs B*H <= 4096 (B=4097 H=1)", (e.name, msg)
        rc, msg = e([_problem(), _problem(B=2049, H=2)], p=0.1, rng=RNG)
        assert rc == E_SHAPE and msg == e.own + "[1]: dropout needs B*H <= 4096 (B=2049 H=2)", (e.name, msg)
        rc, msg = e([_problem(B=4097, H=1)], p=1.0, rng=RNG)                             # the probability first
        assert rc == E_SHAPE and "0 <= p < 1" in msg, (e.name, msg)
    tail = " leaves the problem's stream ids (4096 per problem of a group, 2^32 alone)"
    for e in KEYED:
        rc, msg = e([_problem(), _problem()], p=0.1, rng=RNG, base=4095)                 # 4095 + 2 within a group of two
        assert rc == E_SHAPE and msg == e.own + "[0]: stream_base=4095 + B*H=2" + tail, (e.name, msg)
        rc, msg = e([_problem(), _problem(B=2, H=2)], p=0.1, rng=RNG, base=4093)         # the first fits (4095), the second does not
        assert rc == E_SHAPE and msg == e.own + "[1]: stream_base=4093 + B*H=4" + tail, (e.name, msg)
        rc, msg = e([_problem()], p=0.1, rng=RNG, base=0xFFFFFFFF)                       # alone: the ids must not wrap
        assert rc == E_SHAPE and msg == e.own + "[0]: stream_base=4294967295 + B*H=2" + tail, (e.name, msg)
        for p in (0.1, 0.0):                                                             # the state's alignment is looked at whatever p
            rc, msg = e([_problem()], p=p, rng=RNG + 4)
            assert rc == E_ALIGN and msg == e.own + ": rng_state must be 8-byte aligned", (e.name, msg)
        rc, msg = e([_problem()], p=1.0, rng=RNG + 4)                                    # the probability, the alignment, then the ids
        assert rc == E_SHAPE and "0 <= p < 1" in msg, (e.name, msg)
        rc, msg = e([_problem(), _problem()], p=0.1, rng=RNG + 4, base=4095)
        assert rc == E_ALIGN and "8-byte aligned" in msg, (e.name, msg)


def test_operands_behind_buffer_descriptors_stay_below_2_gib():
    big = 1 << 20                                                                        # 2^20 x 1536 x 2 bytes = 3 GiB
    for e in ENTRIES:
        if e.ranges is None:
            continue
        for kw in (dict(Tq=big, ldq=1536), dict(Tq=big, ldo=1536), dict(Tk=big, ldk=1536), dict(Tk=big, ldv=1536)):
            for problems in ([_problem(**kw)], [_problem(), _problem(**kw)]):
                rc, msg = e(problems)
                assert rc == E_SHAPE and msg == e.ranges + ": T*ld exceeds the 2 GiB buffer-descriptor range", (e.name, kw, msg)
    for e in WORKSPACE:                                                                  # ... and the statistics launch's grid
        rc, msg = e([_problem(B=1 << 28)])
        assert rc == E_SHAPE and msg == "mmf_attn_bwd_grouped_uniform[0]: B*Tk*H*head_dim exceeds the statistics launch", (e.name, msg)


def test_uniform_workspace_and_pooled_gradient():
    for e in WORKSPACE:
        two = [_problem(), _problem(B=3, Tk=16)]                                         # 64 + 384 bytes
        for problems, need, kw in [([_problem()], 64, dict(ws=None)), ([_problem()], 64, dict(ws=WS + 2)), ([_problem()], 64, dict(ws_bytes=63)),
                                   ([_problem()], 64, dict(ws_bytes=0)), (two, 448, dict(ws_bytes=447)), (two, 448, dict(ws=WS + 1))]:
            rc, msg = e(problems, **kw)
            assert rc == E_SHAPE and msg == "%s: workspace of %d bytes (4-byte aligned) required" % (e.own, need), (e.name, kw, msg)
        rc, msg = e([_problem(dQ=None)], ws=None)                                        # the operands first
        assert rc == E_SHAPE and "null gradient operand" in msg, (e.name, msg)
        rc, msg = e([_problem(Tq=1 << 20, ldq=1536)], ws_bytes=63)                       # the 2 GiB rule last
        assert rc == E_SHAPE and "workspace of 64 bytes" in msg, (e.name, msg)
    e, who = POOLED, "mmf_attn_bwd_grouped_pooled"
    for kw in (dict(lddy=132), dict(lddy=4), dict(dys=None)):
        rc, msg = e([_problem()], **kw)
        assert rc == E_ALIGN and msg == "%s: lddy=%d (a multiple of 8) and the gradient pointers are required" % (who, kw.get("lddy", 1536)), (kw, msg)
    want = ": the pooled gradient must be 16-byte aligned with lddy >= H*head_dim"
    for at, dys, lddy in ((0, [None], 1536), (0, [DY + 8], 1536), (0, [DY], 120), (1, [DY, None], 1536), (1, [DY, DY + 4], 1536)):
        rc, msg = e([_problem()] * len(dys), dys=dys, lddy=lddy)
        assert rc == E_ALIGN and msg == "%s[%d]" % (who, at) + want, (dys, lddy, msg)
    rc, msg = e([_problem(), _problem(H=4, ld=256)], dys=[DY, DY + 0x10000], lddy=128)   # lddy against each problem's own H
    assert rc == E_ALIGN and msg == who + "[1]" + want, msg
    rc, msg = e([_problem()], ws=None, dys=None)                                         # the workspace before the gradient
    assert rc == E_SHAPE and "workspace of 64 bytes" in msg, msg


def test_uniform_available_and_workspace_bytes():
    L = lib.load()
    assert L.mmf_attn_bwd_grouped_uniform_available(64, 0.0) == 1 and L.mmf_attn_bwd_grouped_uniform_available(96, 0.0) == 1
    assert L.mmf_attn_bwd_grouped_uniform_available(32, 0.0) == 0 and L.mmf_attn_bwd_grouped_uniform_available(128, 0.0) == 0
    assert L.mmf_attn_bwd_grouped_uniform_available(64, 0.1) == 0 and L.mmf_attn_bwd_grouped_uniform_available(96, 0.1) == 0
    assert lib.attn_bwd_uniform_available(96, 0.0) is True and lib.attn_bwd_uniform_available(96, 0.5) is False
    problems = [_problem(), _problem(B=3, H=4, Tq=30, Tk=50), _problem(B=2, H=2, Tk=1)]
    arr = (lib.AttnProblem * 3)(*problems)
    assert L.mmf_attn_bwd_grouped_uniform_workspace_bytes(arr, 1) == 1 * 2 * 8 * 4
    assert L.mmf_attn_bwd_grouped_uniform_workspace_bytes(arr, 3) == (16 + 600 + 4) * 4
    assert lib.attn_bwd_uniform_workspace_bytes(problems) == (16 + 600 + 4) * 4
    assert L.mmf_attn_bwd_grouped_uniform_workspace_bytes(arr, 0) == 0
    assert L.mmf_attn_bwd_grouped_uniform_workspace_bytes(None, 3) == 0
    assert L.mmf_attn_bwd_grouped_uniform_workspace_bytes((lib.AttnProblem * 2)(_problem(B=0), _problem()), 2) == 64    # an empty problem counts 0


def test_select_impl():
    L = lib.load()
    assert L.mmf_attn_select_impl(0) == 0 and L.mmf_attn_select_impl(2) == 0
    for impl in (1, 3, 4, -1):
        assert L.mmf_attn_select_impl(impl) == E_UNSUPPORTED
        assert L.mmf_last_error().decode() == "mmf_attn_select_impl: impl=%d (only generation 2 is built: 0 or 2)" % impl
