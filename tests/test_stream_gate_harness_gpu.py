"""The stream-order harness (tests/stream_gate.py) has teeth: stand-in "library calls" written in torch -- no library
code but the gate's own spin kernel is involved.  A call that does all its work on the current stream passes in both
modes; one that does part of it on the null stream is found in both; one that does part of it on a second side stream
without an event is found by ``late_producer``; one that synchronises the host first is reported as ``GateMissed``
unless it says so."""
import pytest
import torch

import stream_gate as sg

pytestmark = pytest.mark.gpu
N = 1 << 16


def _x(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, generator=g)


def _case(call, **kw):
    def run(ctx):
        x = ctx.input(_x(1), _x(2))
        return {"y": ctx.call(lambda: call(x), [x], **kw)}
    return run


def correct(x):
    y = torch.zeros_like(x)
    y.add_(x * 3)
    return y + 1


def part_on_null_stream(x):
    y = torch.zeros_like(x)  # (cleared on the caller's stream: what the later read sees when the null-stream part is late)
    with torch.cuda.stream(torch.cuda.default_stream()):
        y.add_(x * 3)
    return y + 1


def part_on_second_stream(x):
    y = torch.zeros_like(x)
    with torch.cuda.stream(sg.side_stream(1)):  # (no event in either direction)
        y.add_(x * 3)
    return y + 1


def syncs_first(x):
    torch.cuda.current_stream().synchronize()
    return correct(x)


@pytest.mark.parametrize("mode", sg.MODES)
def test_a_call_on_the_current_stream_passes(mode):
    lines = sg.check("stand-in correct", _case(correct), mode)
    assert len(lines) == 1 and "held=True" in lines[0]


@pytest.mark.parametrize("mode", sg.MODES)
def test_work_on_the_null_stream_is_found(mode):
    with pytest.raises(sg.StreamFinding, match="depends on the stream"):
        sg.check("stand-in null", _case(part_on_null_stream), mode)


def test_work_on_a_second_stream_without_an_event_is_found():
    with pytest.raises(sg.StreamFinding, match="depends on the stream"):
        sg.check("stand-in second", _case(part_on_second_stream), sg.LATE_PRODUCER)


def test_an_undeclared_host_synchronisation_is_a_missed_gate():
    with pytest.raises(sg.GateMissed, match="no longer held right after the enqueue"):
        sg.check("stand-in sync", _case(syncs_first), sg.LATE_PRODUCER)
    # declared: what comes before the synchronisation is gated, the rest is compared as usual
    lines = sg.check("stand-in sync", _case(syncs_first, syncs="test_stream_gate_harness_gpu.py syncs_first"), sg.LATE_PRODUCER)
    assert "held=False" in lines[0] and "syncs=" in lines[0]
    sg.check("stand-in sync", _case(syncs_first), sg.NULL_HELD)  # (this mode does not mind)


def test_a_case_that_is_not_deterministic_is_reported_as_such():
    def run(ctx):
        return {"y": ctx.call(lambda: torch.rand(N, device="cuda"))}
    with pytest.raises(sg.NotDeterministic):
        sg.check("stand-in random", run, sg.NULL_HELD)


def test_one_object_on_two_streams():
    """the two-stream driver: a stand-in with a buffer per stream passes, one that shares its buffer is found"""
    xa, xb = _x(3).cuda(), _x(4).cuda()

    class PerStream:
        def __init__(self):
            self.ws = {}

        def buf(self, x):
            return self.ws.setdefault(torch.cuda.current_stream().cuda_stream, torch.empty_like(x))

        def __call__(self, x):
            w = self.buf(x)
            w.copy_(x)
            sg.occupy(5, torch.cuda.current_stream())  # (a long kernel between the write and the read of the buffer)
            return {"y": w + 1}

    class Shared(PerStream):
        def buf(self, x):
            return self.ws.setdefault(0, torch.empty_like(x))

    sg.check_two_streams("stand-in per-stream", PerStream, lambda o: o(xa), lambda o: o(xb))
    with pytest.raises(sg.StreamFinding, match="two streams"):
        sg.check_two_streams("stand-in shared", Shared, lambda o: o(xa), lambda o: o(xb), rounds=2)
