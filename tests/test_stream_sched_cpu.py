"""The instruments of tests/stream_sched.py on fakes: a fake ``stream_ptr``, fake stream objects, a recording ``sleep``.  What the
GPU file (tests/test_stream_schedules_gpu.py) relies on — the boundary derivation, the k-th-call trigger, the serial replay's
patching, and that everything is restored after an exception — is checked here without a GPU."""
from types import SimpleNamespace

import pytest

import stream_sched as ss

MAIN, SIDE0, SIDE1, WG = 100, 200, 300, 400


def _fake_lib(sequence):
    it = iter(sequence)
    return SimpleNamespace(stream_ptr=lambda: next(it))


def _fake_ops():
    ns = SimpleNamespace(_branch_streams=["s0", "s1"], _wgrad_stream="wg", flushed=[])
    ns.branch_stream = lambda i=0: ns._branch_streams[i]
    ns._flush_wgrad = lambda: ns.flushed.append(True)
    return ns


def test_boundaries_of_a_hand_written_sequence():
    #         0     1     2      3      4     5     6     7      8     9   10  11
    seq = [MAIN, MAIN, SIDE1, SIDE1, SIDE1, MAIN, MAIN, MAIN, SIDE1, MAIN, WG, WG]
    # stream changes: 1|2, 4|5, 7|8, 8|9, 9|10 -> both neighbours of every change
    assert ss.boundaries(seq) == [1, 2, 4, 5, 7, 8, 9, 10]
    # the first launch of backward (6) and of the wgrad flush (11) are boundaries although their stream does not change
    assert ss.boundaries(seq, phase_starts=[6, 11]) == [1, 2, 4, 5, 6, 7, 8, 9, 10, 11]
    assert ss.boundaries(seq, phase_starts=[2, 2, 12, -1]) == [1, 2, 4, 5, 7, 8, 9, 10]     # repeats and out-of-range starts
    assert ss.boundaries([MAIN] * 5) == [] and ss.boundaries([]) == [] and ss.boundaries([MAIN]) == []
    assert ss.boundaries([MAIN, SIDE0]) == [0, 1]
    assert ss.boundaries([MAIN] * 3, phase_starts=[0]) == [0]


def test_census_records_streams_marks_and_the_flush():
    seq = [MAIN, SIDE0, SIDE0, MAIN, MAIN, WG, MAIN]
    lib, ops = _fake_lib(seq), _fake_ops()
    orig_ptr, orig_flush = lib.stream_ptr, ops._flush_wgrad
    with ss.launch_census(lib, ops) as census:
        assert lib.stream_ptr is not orig_ptr and ops._flush_wgrad is not orig_flush
        census.mark("forward")
        got = [lib.stream_ptr() for _ in range(3)]
        census.mark("backward")
        got += [lib.stream_ptr() for _ in range(2)]
        ops._flush_wgrad()                                     # what the autograd engine calls at the end of backward
        got += [lib.stream_ptr() for _ in range(2)]
    assert got == seq and census.streams == seq                # the wrapper hands the stream through unchanged
    assert ops.flushed == [True]                               # ... and the flush itself still ran
    assert census.marks == [("forward", 0), ("backward", 3), ("flush", 5)]
    assert census.starts("backward", "flush") == [3, 5] and census.starts("f.*") == [0, 5]
    assert [census.phase(k) for k in range(7)] == ["forward"] * 3 + ["backward"] * 2 + ["flush"] * 2
    assert census.counts() == {MAIN: 4, SIDE0: 2, WG: 1}
    assert ss.boundaries(census.streams, census.starts("backward", "flush")) == [0, 1, 2, 3, 4, 5, 6]
    assert lib.stream_ptr is orig_ptr and ops._flush_wgrad is orig_flush


@pytest.mark.parametrize("k", [0, 3, 6])
def test_delay_fires_once_before_the_kth_launch_on_its_stream(k):
    seq = [MAIN, SIDE0, SIDE0, SIDE1, MAIN, WG, MAIN]
    lib = _fake_lib(seq)
    orig = lib.stream_ptr
    log = []
    with ss.delayed_launch(k, lambda s: log.append(("sleep", s)), lib) as fired:
        for _ in seq:
            log.append(("launch", lib.stream_ptr()))
    assert fired == [seq[k]]
    assert [e for e in log if e[0] == "launch"] == [("launch", s) for s in seq]
    assert log.count(("sleep", seq[k])) == 1 and sum(e[0] == "sleep" for e in log) == 1
    assert log.index(("sleep", seq[k])) == k                   # k launches in front of it, launch k right behind it
    assert log[k + 1] == ("launch", seq[k])
    assert lib.stream_ptr is orig


def test_delay_past_the_last_launch_never_fires_and_census_nests_inside_it():
    seq = [MAIN, SIDE0, MAIN]
    lib, ops = _fake_lib(seq), _fake_ops()
    orig = lib.stream_ptr
    slept = []
    with ss.delayed_launch(3, slept.append, lib) as fired, ss.launch_census(lib, ops) as census:
        for _ in seq:
            lib.stream_ptr()
    assert fired == [] and slept == [] and census.streams == seq
    assert lib.stream_ptr is orig


def test_serial_replay_patches_and_restores():
    ops = _fake_ops()
    saved = (ops.branch_stream, ops._branch_streams, ops._wgrad_stream)
    cur = ["main"]
    with ss.serial_replay(ops, lambda: cur[0]):
        assert ops._branch_streams == [] and ops._wgrad_stream == "main"
        assert ops.branch_stream() == "main" and ops.branch_stream(1) == "main"
        cur[0] = "other"                                       # (a backward thread whose current stream differs)
        assert ops.branch_stream(0) == "other"
    assert (ops.branch_stream, ops._branch_streams, ops._wgrad_stream) == saved
    assert ops._branch_streams == ["s0", "s1"]                 # the same list object, contents untouched


def test_everything_is_restored_after_an_exception():
    lib, ops = _fake_lib([MAIN] * 4), _fake_ops()
    before = (lib.stream_ptr, ops._flush_wgrad, ops.branch_stream, ops._branch_streams, ops._wgrad_stream)
    slept = []
    with pytest.raises(RuntimeError, match="boom"):
        with ss.serial_replay(ops, lambda: "main"), ss.launch_census(lib, ops), ss.delayed_launch(1, slept.append, lib):
            lib.stream_ptr()
            lib.stream_ptr()
            raise RuntimeError("boom")
    assert slept == [MAIN]
    assert (lib.stream_ptr, ops._flush_wgrad, ops.branch_stream, ops._branch_streams, ops._wgrad_stream) == before

    def bad_sleep(s):
        raise RuntimeError("sleep failed")
    with pytest.raises(RuntimeError, match="sleep failed"):
        with ss.delayed_launch(0, bad_sleep, lib):
            lib.stream_ptr()
    assert lib.stream_ptr is before[0]


def test_every_product_caller_reaches_stream_ptr_through_the_module():
    """The wrappers replace the attribute ``mmfusion.lib.stream_ptr``: a caller that bound the function at import time
    (``from .lib import stream_ptr``) would slip past the census.  None does."""
    import os
    import re
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simple-multimodal_amd")
    calls = 0
    for root, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith(".py"):
                continue
            src = open(os.path.join(root, f)).read()
            assert not re.search(r"import[^\n]*\bstream_ptr\b", src), f"{f} binds stream_ptr at import time"
            assert not re.search(r"=\s*(_?lib\.)?stream_ptr\s*(\n|#)", src), f"{f} keeps a reference to stream_ptr"
            bare = len(re.findall(r"(?<![\w.])stream_ptr\(\)", src))
            assert bare == 0 or f == "lib.py", f"{f} calls a bare stream_ptr()"
            calls += len(re.findall(r"stream_ptr\(\)", src))
    assert calls > 50                                          # (the walk did find the package)
