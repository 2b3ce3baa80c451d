"""Instruments for the multi-stream schedules (test infrastructure, used by tests/test_stream_schedules_gpu.py and pinned on
the CPU by tests/test_stream_sched_cpu.py).

The default eager configuration issues one step over up to four streams (the current stream, ``ops.branch_stream(0)`` for
HierarchicalFusion's small branches, ``ops.branch_stream(1)`` for root MulT's audio + video chains, the early wgrad stream);
every ordering edge between them is a hand-written ``wait_stream`` / ``record_stream``.  Three context managers make a missing
edge deterministic without touching the product:

  * ``serial_replay()``    the REFERENCE schedule: the same host code, the same library launches with the same grouping,
                           arguments and dropout sites, all of them on the current stream;
  * ``launch_census()``    the stream of every library launch of a step in host order, and from it the launches at which the
                           schedule changes stream or phase (``boundaries``);
  * ``delayed_launch()``   a bounded on-device sleep on the stream of the k-th launch, immediately in front of it.

The census and the delay wrap ``mmfusion.lib.stream_ptr``, the one place every launch asks for its stream.  Every caller
reaches it through the module attribute (``lib.stream_ptr()`` / ``_lib.stream_ptr()``, and as a module global inside lib.py
itself), so replacing the attribute reaches them all; nothing binds the name at import time.  A caller that asks once for
several consecutive launches (``L, st = lib.load(), lib.stream_ptr()``: the fan-out sums, the LayerNorm backward pair) is one
entry of the census: those launches share a stream and nothing can be issued between them.

All three restore what they patched on any exit."""
import contextlib
import re


def _lib(lib_mod):
    if lib_mod is None:
        from mmfusion import lib as lib_mod
    return lib_mod


def _ops(ops_mod):
    if ops_mod is None:
        from mmfusion import ops as ops_mod
    return ops_mod


@contextlib.contextmanager
def serial_replay(ops_mod=None, current_stream=None):
    """Within: ``ops.branch_stream(i)`` is the current stream, ``ops._wgrad_stream`` is preset to the current stream (so
    ``issue_wgrad(side=True)`` stays on it) and ``ops._branch_streams`` is empty.  ``fl._MULT_STREAMS``, ``fl._BRANCH_STREAM``
    and ``ops._WGRAD_EARLY`` are NOT touched: the host takes the concurrent code path — 4 + 2 cross blocks, the interleaved
    thunks, the early wgrad launch — and every fork and join becomes a stream waiting for itself."""
    ops_mod = _ops(ops_mod)
    if current_stream is None:
        import torch
        current_stream = torch.cuda.current_stream
    saved = (ops_mod.branch_stream, ops_mod._branch_streams, ops_mod._wgrad_stream)
    ops_mod.branch_stream = lambda i=0: current_stream()
    ops_mod._branch_streams = []
    ops_mod._wgrad_stream = current_stream()
    try:
        yield
    finally:
        ops_mod.branch_stream, ops_mod._branch_streams, ops_mod._wgrad_stream = saved


def boundaries(streams, phase_starts=()):
    """Indices k of a launch sequence (``streams[k]`` = the stream of launch k) at which the schedule has an edge: the stream
    of launch k differs from launch k-1's or from launch k+1's, or k is the first launch of a phase (``phase_starts``: the
    first launch of backward, of the wgrad flush).  Sorted, without repeats."""
    n = len(streams)
    out = set(k for k in phase_starts if 0 <= k < n)
    for k in range(n):
        if (k > 0 and streams[k] != streams[k - 1]) or (k + 1 < n and streams[k] != streams[k + 1]):
            out.add(k)
    return sorted(out)


class Census:
    """``streams[k]``: the stream launch k went to; ``marks``: (label, index of the first launch after the mark) in host order."""

    def __init__(self):
        self.streams, self.marks = [], []

    def mark(self, label):
        self.marks.append((label, len(self.streams)))

    def starts(self, *patterns):
        """launch indices at which a phase whose label matches one of the regular expressions begins"""
        return [k for label, k in self.marks if any(re.fullmatch(p, label) for p in patterns)]

    def phase(self, k):
        """label of the last mark at or before launch k (None in front of the first)"""
        label = None
        for name, k0 in self.marks:
            if k0 <= k:
                label = name
        return label

    def counts(self):
        out = {}
        for s in self.streams:
            out[s] = out.get(s, 0) + 1
        return out


@contextlib.contextmanager
def _wrapped(obj, name, make):
    orig = getattr(obj, name)
    setattr(obj, name, make(orig))
    try:
        yield
    finally:
        setattr(obj, name, orig)


@contextlib.contextmanager
def launch_census(lib_mod=None, ops_mod=None, flush_label="flush"):
    """Within: every ``lib.stream_ptr()`` call is recorded; yields the ``Census``.  ``ops._flush_wgrad`` (the end-of-backward
    callback, looked up as a module global when it is queued) is wrapped to mark the first launch of the wgrad flush; the
    caller marks the other phases (``census.mark("backward")`` in front of ``backward()``)."""
    lib_mod, ops_mod = _lib(lib_mod), _ops(ops_mod)
    census = Census()

    def counting(orig):
        def stream_ptr():
            s = orig()
            census.streams.append(s)
            return s
        return stream_ptr

    def marking(orig):
        def _flush_wgrad():
            census.mark(flush_label)
            return orig()
        return _flush_wgrad
    with _wrapped(lib_mod, "stream_ptr", counting), _wrapped(ops_mod, "_flush_wgrad", marking):
        yield census


@contextlib.contextmanager
def delayed_launch(k, sleep, lib_mod=None):
    """Within: immediately before the k-th ``lib.stream_ptr()`` call returns (0-based, the census numbering), ``sleep(stream)``
    is called once with the stream that launch goes to — the caller's ``sleep`` enqueues its delay on the CURRENT stream, which
    is that stream.  Yields a list that holds the stream once the delay has fired."""
    lib_mod = _lib(lib_mod)
    fired, count = [], [0]

    def delaying(orig):
        def stream_ptr():
            s = orig()
            if count[0] == k:
                fired.append(s)
                sleep(s)
            count[0] += 1
            return s
        return stream_ptr
    with _wrapped(lib_mod, "stream_ptr", delaying):
        yield fired


# ---- the on-device delay --------------------------------------------------------------------------------------------------
SLEEP_CAP_MS = 50.0
_sleeper = None


class Sleeper:
    """A bounded delay on the current stream: ``torch.cuda._sleep(cycles)`` with the cycle rate measured once per session by two
    events around a sleep, or — if that does not sleep for what it was asked — a chain of stock 1024^3 matmuls timed the same
    way.  ``enqueue(ms)`` never asks for more than SLEEP_CAP_MS."""

    def __init__(self):
        import torch
        self.torch = torch
        self.kind, self.rate, self.check = "_sleep", 0.0, 0.0
        want = 5.0
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)                                 # (loads the kernel: not part of the measurement)
            probe = 1_000_000
            t = self._time(lambda: torch.cuda._sleep(probe))
            if t > 0 and 1e4 <= probe / t <= 1e7:                   # 10 MHz ... 10 GHz: a counter a GPU can have
                self.rate = probe / t                               # cycles per ms
                self.check = self._time(lambda: self.enqueue(want))
        if not 0.5 * want <= self.check <= 2.0 * want:
            self.kind = "matmul"
            self.a = torch.randn(1024, 1024, device="cuda")
            self.b = torch.empty_like(self.a)
            chain = lambda n: [torch.mm(self.a, self.a, out=self.b) for _ in range(n)]
            chain(20)                                               # (the library picks its kernel: not part of the measurement)
            self.rate = 200 / self._time(lambda: chain(200))        # matmuls per ms
            self.check = self._time(lambda: self.enqueue(want))
        # an instrument that does not delay would make every D_k a repeat of C
        assert 0.5 * want <= self.check <= 2.0 * want, f"the {self.kind} delay ran {self.check:.2f} ms when asked for {want} ms"

    def _time(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return float(e0.elapsed_time(e1))

    def enqueue(self, ms):
        ms = min(float(ms), SLEEP_CAP_MS)
        if self.kind == "_sleep":
            self.torch.cuda._sleep(int(ms * self.rate))
        else:
            # operands of the chain belong to the stream the Sleeper was built on; the chain only reads a and rewrites b
            for _ in range(max(1, int(ms * self.rate))):
                self.torch.mm(self.a, self.a, out=self.b)


def sleeper():
    global _sleeper
    if _sleeper is None:
        _sleeper = Sleeper()
    return _sleeper
