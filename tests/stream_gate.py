"""Stream ordering (a plain module, imported by the test files, like tests/poison.py and tests/numerics.py).

Every device entry point takes the caller's stream, and the wrappers pass ``torch.cuda.current_stream()``.  On torch's
default stream (the legacy null stream) a kernel or copy issued on the wrong stream, a ``hipMemset`` where the ``Async``
form was meant, or a staging buffer reused too early still give the right answer: everything serialises anyway.  This
module makes such a mistake visible.  It runs a case on the default stream, freezes the bytes of its outputs
(``poison.freeze``), and runs it again on a non-blocking side stream under a gate: a bounded spin kernel of ONE workgroup
(``ppasr_debug_occupy_cus(1, G, stream)``) that holds a stream for ``G`` milliseconds while the rest of the chip is free.

``null_held``      the gate sits on the NULL stream before each call; the call is made on the side stream and its outputs
                   are copied on the side stream with no device-wide synchronise in between.  Whatever the library puts
                   on the null stream lands ``G`` ms late, and the side-stream work reads what is not produced yet.
                   Host-blocking uploads inside a wrapper do not disturb this mode.
``late_producer``  the inputs are device buffers that hold a DECOY (different, valid data of the same shape) while the
                   call is enqueued.  On the side stream: the gate, then ``buf.copy_(real)`` for every input, then the
                   call, then ``buf.copy_(decoy)`` again (work deferred past the return reads the decoy too).  Whatever
                   runs on another stream, or on the side stream without ordering, reads the decoy.  Right after the last
                   enqueue the gate must still be holding (an event recorded right behind the spin kernel has not
                   completed, so ``side.query() is False``), else the gate had run out
                   before the call was queued and the case proves nothing: ``GateMissed``.  A call that synchronises the
                   host by design says so (``syncs="<file>:<line> <what>"``); only what it enqueues before that
                   synchronisation is gated then.

``G`` = max(20 ms, 10 x the host wall time of the same call in the control run on the default stream), at most 500 ms
(the control is the second of the two reference runs, i.e. with modules loaded and the allocator warm).

A case is ``run(ctx) -> {name: tensor}``: it builds a fresh wrapper, registers its inputs with ``ctx.input(real, decoy)``
(-> the device buffer to hand to the call), makes each call under test inside ``ctx.call(fn, inputs)`` (-> what ``fn``
returns, its device tensors copied on the side stream right behind the call) and returns the defined regions of the
outputs (the definitions of the poison tests).  Decoys are always valid data: a mis-streamed
kernel must compute a wrong answer, never read out of bounds."""
import time

import torch

import poison

NULL_HELD = "null_held"
LATE_PRODUCER = "late_producer"
MODES = (NULL_HELD, LATE_PRODUCER)
G_MIN_MS, G_MAX_MS, G_FACTOR = 20, 500, 10


class StreamFinding(AssertionError):
    """A result depends on which stream the call was made on: part of its work is not ordered on the caller's stream."""


class GateMissed(AssertionError):
    """The gate was no longer holding when the call had been enqueued (an undeclared host synchronisation, or a gate
    shorter than the enqueue): the case proves nothing."""


NotDeterministic = poison.NotDeterministic

_SIDE = []


def side_stream(i=0):
    """One of the two non-blocking side streams this process uses.  Both are made on first use, one right after the other:
    torch hands its pooled streams out in turn, and neighbours in the pool do not share a hardware queue."""
    if not _SIDE:
        _SIDE.extend([torch.cuda.Stream(), torch.cuda.Stream()])
    return _SIDE[i]


def occupy(ms, stream=None):
    """Hold ``stream`` (None: the null stream) for ``ms`` milliseconds with one spinning workgroup."""
    from ppasr_amd import _lib
    assert 0 < ms <= G_MAX_MS
    _lib.check(_lib.load().ppasr_debug_occupy_cus(1, int(ms), None if stream is None else stream.cuda_stream))


def gate_ms(wall_s):
    return int(min(G_MAX_MS, max(G_MIN_MS, round(G_FACTOR * wall_s * 1e3))))


def _dev(t, like=None):
    t = torch.as_tensor(t)
    if like is not None:
        assert t.shape == like.shape and t.dtype == like.dtype, "a decoy has the shape and type of the real input"
    return t.cuda().contiguous()


def snapshot(out):
    """Copies of the tensors in what a call returned (tuple / list / dict / tensor), made on the current stream right
    behind the call: before anything -- the wrapper's destructor, say -- can wait for the device."""
    if isinstance(out, torch.Tensor):
        return out.clone() if out.is_cuda else out
    if isinstance(out, (tuple, list)):
        return type(out)(snapshot(v) for v in out)
    if isinstance(out, dict):
        return {k: snapshot(v) for k, v in out.items()}
    return out


class Ctx:
    """What ``run`` sees: ``mode`` ("reference", or one of MODES), ``input`` and ``call``."""

    def __init__(self, case, mode, gates=None, log=print):
        self.case, self.mode, self.log = case, mode, log
        self.gates = gates  # G per call of the case, from the control run
        self.walls = []     # reference: host wall time per call
        self.lines = []
        self._k = 0
        self.side = side_stream(0) if mode in MODES else None

    def input(self, real, decoy):
        """-> the device buffer the call reads.  Make every input of the case before its first ``call`` (an upload from
        pageable memory waits for the stream)."""
        real = _dev(real)
        buf = real.clone() if self.mode != LATE_PRODUCER else _dev(decoy, real).clone()
        buf._gate_real, buf._gate_decoy = real, (_dev(decoy, real) if self.mode == LATE_PRODUCER else None)
        return buf

    def call(self, fn, inputs=(), syncs=None, label=""):
        """Make one call (or several behind one gate) under the mode's gate; -> what ``fn`` returns."""
        k, self._k = self._k, self._k + 1
        if self.mode == "reference":
            t0 = time.perf_counter()
            out = fn()
            self.walls.append(time.perf_counter() - t0)
            return out
        assert k < len(self.gates), f"{self.case}: call {k} was not made in the reference run"
        G = self.gates[k]
        gate = torch.cuda.Event()  # recorded right behind the spin kernel: done <=> the gate no longer holds
        t0 = time.perf_counter()
        if self.mode == NULL_HELD:
            occupy(G, None)
            gate.record(torch.cuda.default_stream())
            out = snapshot(fn())
            enq = time.perf_counter() - t0
            held = not gate.query()
        else:
            occupy(G, self.side)
            gate.record(self.side)
            for b in inputs:
                b.copy_(b._gate_real, non_blocking=True)
            out = fn()
            for b in inputs:
                b.copy_(b._gate_decoy, non_blocking=True)
            out = snapshot(out)
            enq = time.perf_counter() - t0
            # (the gate itself, not merely the stream: a call that waited the gate out and then queued a little work
            # leaves the stream busy for a few microseconds; this implies ``side.query() is False``)
            held = not gate.query()
        line = (f"[gate] {self.case} {label or f'call {k}'} {self.mode} G={G}ms enqueue={enq * 1e3:.2f}ms held={held}"
                + (f" syncs={syncs!r}" if syncs else ""))
        self.lines.append(line)
        self.log(line)
        if self.mode == LATE_PRODUCER and not held and not syncs:
            self.side.synchronize()
            raise GateMissed(f"{self.case} {label or f'call {k}'}: the gate no longer held right after the enqueue "
                             f"(G={G} ms, enqueue {enq * 1e3:.2f} ms): the call synchronises the host and does not say so, "
                             f"or the gate is too short")
        return out


def _reference(case, run, log):
    def once():
        ctx = Ctx(case, "reference", log=log)
        outs = run(ctx)
        torch.cuda.synchronize()
        return poison.freeze(outs), ctx.walls

    (a, _), (b, walls) = once(), once()
    d = poison.differences(a, b)
    if d:
        raise NotDeterministic(f"{case}: not deterministic, two default-stream runs differ: " + "; ".join(d))
    return a, [gate_ms(w) for w in walls]


def reference(case, run, memo=None, log=print):
    """-> (frozen outputs of the case on the default stream, the gate per call), memoised per case in ``memo``"""
    return memo.get(case, lambda: _reference(case, run, log)) if memo is not None else _reference(case, run, log)


def check(case, run, mode, memo=None, log=print):
    """Reference on the default stream (twice: the control; memoised per case in ``memo``) -> the gated run on the side
    stream -> bytes compared.  -> the ``[gate]`` lines of the gated run."""
    assert mode in MODES, mode
    ref, gates = reference(case, run, memo, log)
    torch.cuda.synchronize()
    ctx = Ctx(case, mode, gates, log=log)
    try:
        with torch.cuda.stream(ctx.side):
            outs = run(ctx)
            copies = {k: v.clone() if v.is_cuda else v for k, v in outs.items()}  # on the side stream, nothing in between
            ctx.side.synchronize()
        got = poison.freeze(copies)
    finally:
        torch.cuda.synchronize()  # (the null-stream gates drain before the next case)
    d = poison.differences(ref, got)
    if d:
        raise StreamFinding(f"{case}: result depends on the stream ({mode}): " + "; ".join(d))
    return ctx.lines


def check_two_streams(case, build, call_a, call_b, rounds=3, hold_ms=G_MIN_MS, log=print):
    """One wrapper object, two streams: ``call_a(obj)`` and ``call_b(obj)`` (-> {name: tensor}; different batches, inputs
    made by ``build``) are enqueued alternately on two side streams, both held by a gate first so that their work runs
    side by side, with no synchronisation between them.  Every round's result must equal the serial reference's bytes."""
    obj = build()
    torch.cuda.synchronize()
    refs = []
    for call in (call_a, call_b):
        refs.append(poison.freeze(call(obj)))
        torch.cuda.synchronize()
    streams = (side_stream(0), side_stream(1))
    for s in streams:  # (each wrapper's first call on a stream allocates its workspace there: not behind the gate)
        s.synchronize()
    got = []
    try:
        for s in streams:
            occupy(hold_ms, s)
        for r in range(rounds):
            for i, call in enumerate((call_a, call_b)):
                with torch.cuda.stream(streams[i]):
                    got.append((r, i, {k: v.clone() for k, v in call(obj).items()}))
        held = [not s.query() for s in streams]
        for s in streams:
            s.synchronize()
    finally:
        torch.cuda.synchronize()
    log(f"[gate] {case} two_streams rounds={rounds} hold={hold_ms}ms held={held}")
    bad = []
    for r, i, outs in got:
        d = poison.differences(refs[i], poison.freeze(outs))
        if d:
            bad.append(f"round {r} stream {'ab'[i]}: " + "; ".join(d))
    if bad:
        raise StreamFinding(f"{case}: one object on two streams differs from the serial result: " + " | ".join(bad))
