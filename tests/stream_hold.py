"""Making the ORDER of GPU work observable (tests/test_gpu_stream_rule.py; DESIGN.md, "Two kinds of ordering bug").

A test that enqueues two small calls on two streams and compares data cannot fail when a wait is missing: the calls
finish in tens of microseconds and rarely overlap, and a second call that runs to completion before the first has
started is a legal serial order.  Here the first call sits behind a HOLD, a bounded piece of device work that outlasts the
second call many times over, and the test asserts where the second call ended relative to the hold:

    h = hold(A); first enqueues on A          the first call cannot start before the hold is over
    second enqueues on B; evB behind it       (or second is a host-buffer call / an accumulator read, which blocks)
    assert not h.query()                      the hold outlasted every enqueue -- else the case proves nothing, and FAILS
    evB.synchronize(); assert h.query()       a second call that did not wait for the first ended inside the hold
    synchronize; compare all outputs bitwise  a second call that touched shared state BEFORE its wait got wrong data

Nothing here spins or waits on a flag: a hold is PASSES in-place passes over a HOLD_BYTES tensor.  Its length was chosen
from measurements on the MI355X (profiles/stream_rule/README.md): at least ten times the longest second call of the cases,
enqueue time included."""
import numpy as np
import pytest

HOLD_BYTES = 128 << 20          # one float32 tensor; a pass reads and writes it once
PASSES = 1000                   # profiles/stream_rule/README.md: measured pass time, longest second call, the factor
CANDIDATES = 8                  # streams tried as B before the fixture gives up

_hold_buffer = None


def _buffer():
    import torch
    global _hold_buffer
    if _hold_buffer is None:
        _hold_buffer = torch.ones(HOLD_BYTES // 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
    return _hold_buffer


def hold(stream):
    """Queue the blocker on `stream`; returns a torch event recorded right behind it."""
    import torch
    buf = _buffer()
    with torch.cuda.stream(stream):
        for _ in range(PASSES):
            buf.mul_(1.0001)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def _trivial_engine():
    """The engine and the arrays of `_trivial_unrank`, made once and BEFORE any hold is queued: creating an engine
    synchronises, and behind a queued hold that would wait the hold out."""
    import torch
    from tetrad_amd.engine import QuartetEngine
    if _trivial_unrank.engine is None:
        from tetrad_amd import synth
        _trivial_unrank.engine = QuartetEngine(0)
        _trivial_unrank.engine.set_data(*synth.simulate_tmparr(8, 64, seed=1))
        _trivial_unrank.ranks = torch.arange(64, dtype=torch.int64, device="cuda")
        _trivial_unrank.out = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
    return _trivial_unrank.engine


def _trivial_unrank(stream):
    """The smallest piece of the library that enqueues on a stream and promises no ordering: one unrank of 64 ranks."""
    _trivial_engine().unrank_dev(_trivial_unrank.ranks.data_ptr(), 64, _trivial_unrank.out.data_ptr(), stream.cuda_stream)


_trivial_unrank.engine = None


class Streams:
    """A, the stream that is held, and B, shown to run while A is held; `tried` = the candidates for B it took."""

    def __init__(self, A, B, tried):
        self.A, self.B, self.tried = A, B, tried


def runs_while_held(held, other):
    """Whether a trivial call on `other` finishes while `held` is held: the two are not serialised on one hardware queue.
    Everything the check needs exists before the hold is queued, so nothing but the enqueues stands between the hold and
    the query."""
    import torch
    _trivial_engine()
    _buffer()
    torch.cuda.synchronize()
    h = hold(held)
    _trivial_unrank(other)
    ev = torch.cuda.Event()
    ev.record(other)
    ev.synchronize()
    pending = not h.query()
    torch.cuda.synchronize()
    return pending


def concurrent_streams():
    """A and B such that work on B finishes while A is held; the number of candidates for B that were tried."""
    import torch
    A = torch.cuda.Stream()
    for tried in range(1, CANDIDATES + 1):
        B = torch.cuda.Stream()
        if runs_while_held(A, B):
            return Streams(A, B, tried)
    pytest.fail(f"none of {CANDIDATES} streams ran concurrently with a held one: every ordering case would pass vacuously")


@pytest.fixture(scope="module")
def streams():
    s = concurrent_streams()
    print(f"stream_hold: B is candidate {s.tried}")
    yield s
    if _trivial_unrank.engine is not None:
        _trivial_unrank.engine.close()
        _trivial_unrank.engine = None


def ordered(streams, first, second, check, second_kind="enqueue", expect_wait=True):
    """The one pattern of every case.  `first(stream_address)` enqueues on the held A.  `second(stream_address)` enqueues
    on B (second_kind "enqueue") or is a host-buffer call or an accumulator read that blocks (second_kind "host"; it gets
    B's address too, for reads that are preceded by an enqueue of their own).  `check()` compares the outputs once the
    device is idle.  With expect_wait=False the second call promises no ordering and must END INSIDE the hold."""
    import torch
    assert second_kind in ("enqueue", "host")
    A, B = streams.A, streams.B
    torch.cuda.synchronize()
    h = hold(A)
    first(A.cuda_stream)
    if second_kind == "host":
        assert not h.query(), "the hold ended before the host call was made: the case proves nothing"
        result = second(B.cuda_stream)
    else:
        result = second(B.cuda_stream)
        evB = torch.cuda.Event()
        evB.record(B)
        assert not h.query(), "the hold ended before the second call was enqueued: the case proves nothing"
        evB.synchronize()
    over = h.query()
    torch.cuda.synchronize()
    if expect_wait:
        assert over, "the second call finished while the first was still held: it did not wait for it"
    else:
        assert not over, "a call that touches only caller memory waited for work on another stream"
    check()
    return result


def assert_bitwise(got, want, what):
    """Arrays of one call, bit for bit."""
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: output {i}"
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{what}: output {i}")
