"""Buffer-content independence (a plain module, imported by the test files, like tests/numerics.py).

Every device buffer the library works in -- workspace, outputs, beam-search state and scratch -- reaches it uninitialised
(``torch.empty`` in the wrappers, a caller-owned workspace in the C-ABI).  The rule the kernels keep by hand is: a value
that is masked, skipped or not yet written is never read into a result.  This module makes a violation visible:

* ``Session(pattern)`` replaces ``torch.empty`` / ``torch.empty_like`` so that every tensor they return on the watched
  device type is filled with a byte pattern, records those tensors, and refills the scratch a wrapper keeps between
  calls (``Session.scratch``);
* ``check(case, run, pattern, ...)`` runs ``run`` on zero-filled buffers twice (the control: the two results must be
  byte-identical, else the case is reported as "not deterministic"), then under the pattern, and compares the raw bytes
  of the defined output regions.  No tolerance anywhere.

Patterns (byte fills, so that they apply to any dtype):
  ``ff``     fp32 / fp16 / fp64 NaN, int32 -1: catches 0 x garbage, unmasked reads, accumulation into unwritten memory;
  ``7f``     fp32 3.39e38 (finite: x 0 hides it, any sum overflows), fp16 NaN, int32 2139062143: catches a missing clear
             of an int table whose "empty" marker is -1, which ``ff`` would let pass;
  ``a5``     fp32 -2.87e-16, the old guard sentinel: harmless, kept only to show in the CPU test that it has no teeth;
  ``stale``  no fill: the buffers hold what a different call on the same wrapper left there (``run`` makes that call
             first when ``session.stale``), the only case where stale ints look like valid indices;
  ``zero``   the clean reference.
"""
import contextlib

import torch

BYTES = {"zero": 0x00, "ff": 0xFF, "7f": 0x7F, "a5": 0xA5}
STALE = "stale"
PATTERNS = (STALE, "ff", "7f")  # what the GPU tests are parametrised over, most benign first

# attributes under which the wrappers keep scratch between calls (a tensor, or a dict of tensors per HIP stream), and
# attributes that lead to further wrapper objects with scratch of their own.  State that legitimately carries
# information between calls (_BeamState.buf, stream / group caches) is NOT listed: it is poisoned at allocation only.
SCRATCH_ATTRS = ("_ws", "_scratch")
OWNER_ATTRS = ("_scratch_stream", "_streams")


class NotDeterministic(AssertionError):
    """The control failed: two clean runs of the case differ, so the case cannot tell poison from noise."""


class PoisonFinding(AssertionError):
    """A result depends on what a scratch, state or output buffer held on entry."""


class PoisonMissed(AssertionError):
    """The pattern never reached the workspace: the case proves nothing."""


def fill(t, byte):
    """Fill the storage bytes of ``t`` with ``byte`` (any dtype)."""
    if t.numel():
        t.view(torch.uint8).fill_(byte)
    return t


def kept_scratch(obj):
    """The scratch tensors ``obj`` (a wrapper object, a module, or a list of them) keeps between calls."""
    out, seen = [], set()

    def walk(o):
        if o is None or id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):  # a buffer the test itself handed to the call (a beam-search state)
            if o.numel():
                out.append(o)
            return
        if isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
            return
        for a in SCRATCH_ATTRS:
            v = getattr(o, a, None)
            for t in (v.values() if isinstance(v, dict) else [v]):
                if isinstance(t, torch.Tensor) and t.numel():
                    out.append(t)
        for a in OWNER_ATTRS:
            walk(getattr(o, a, None))

    walk(obj)
    return out


def _span(t):
    return t.data_ptr(), t.numel() * t.element_size()


class Session:
    """One run under one pattern.  As a context manager it patches the two allocators (through pytest's ``monkeypatch``
    when given one, else by hand) for tensors on ``device_types``; host tensors stay untouched unless "cpu" is watched
    (the CPU stand-ins of tests/test_poison_harness_cpu.py)."""

    def __init__(self, pattern, monkeypatch=None, device_types=("cuda",)):
        assert pattern == STALE or pattern in BYTES, pattern
        self.pattern = pattern
        self.stale = pattern == STALE
        self.byte = None if self.stale else BYTES[pattern]
        self.device_types = tuple(device_types)
        self.filled = set()  # (address, bytes) of what this session filled (allocation or refill); no tensor is kept alive
        self._entry = {}  # stale: (address, bytes) of a kept scratch tensor -> copy of its bytes on entry to the next call
        self.reports = []  # what observe() saw, one entry per call of a multi-call case
        self._mp = monkeypatch
        self._stack = None

    # -- allocation poisoning ------------------------------------------------------------------------------------
    def _wrap(self, fn):
        def alloc(*a, **kw):
            t = fn(*a, **kw)
            if self.byte is not None and t.device.type in self.device_types and t.numel():
                fill(t, self.byte)
                self.filled.add(_span(t))
            return t
        alloc.__wrapped__ = fn
        return alloc

    def __enter__(self):
        self._stack = contextlib.ExitStack()
        if self._mp is not None:
            mp = self._stack.enter_context(self._mp.context())
            mp.setattr(torch, "empty", self._wrap(torch.empty))
            mp.setattr(torch, "empty_like", self._wrap(torch.empty_like))
        else:
            e, el = torch.empty, torch.empty_like
            torch.empty, torch.empty_like = self._wrap(e), self._wrap(el)

            def restore():
                torch.empty, torch.empty_like = e, el
            self._stack.callback(restore)
        return self

    def __exit__(self, *exc):
        self._stack.close()
        self.filled, self._entry = set(), {}
        return False

    # -- scratch kept between calls ------------------------------------------------------------------------------
    def scratch(self, obj):
        """Refill the scratch ``obj`` keeps between calls with the pattern (stale: leave it, but note its bytes so that
        ``report`` can tell what the next call wrote).  -> the tensors."""
        ts = kept_scratch(obj)
        for t in ts:
            if self.stale:
                self._entry[_span(t)] = t.view(torch.uint8).clone()  # (one copy per buffer: the earlier one is dropped)
            else:
                fill(t, self.byte)
                self.filled.add(_span(t))
        return ts

    # -- proof that the poison arrived, and what the call never wrote --------------------------------------------
    def report(self, obj):
        """-> dict(bytes, arrived, never_written) over the scratch ``obj`` keeps.  ``arrived``: every such tensor was
        filled by this session (stale: was noted on entry with non-zero bytes in it).  ``never_written``: share of its
        bytes that still hold the pattern (stale: that are unchanged) -- an upper bound, a write of the same byte counts."""
        ts = kept_scratch(obj)
        total = same = 0
        if obj is None:  # an entry point that keeps nothing: its buffers are the allocations of the call itself
            return dict(bytes=0, arrived=self.stale or (bool(self.filled) and self.byte != 0), never_written=0.0)
        arrived = bool(ts)
        for t in ts:
            b = t.view(torch.uint8)
            total += b.numel()
            if self.stale:
                e = self._entry.get(_span(t))
                if e is None or not bool(e.any()):
                    arrived = False
                    continue
                same += int((b == e).sum())
            else:
                if _span(t) not in self.filled:
                    arrived = False
                same += int((b == self.byte).sum())
        return dict(bytes=total, arrived=arrived and (self.stale or self.byte != 0), never_written=same / max(total, 1))

    def observe(self, obj, label=""):
        """``report(obj)`` right after one call of a multi-call case, kept in ``self.reports``."""
        r = self.report(obj)
        r["label"] = label
        self.reports.append(r)
        return r


# -- comparison ---------------------------------------------------------------------------------------------------------
def raw(t):
    """The bytes of a tensor (host copy, uint8), so that NaNs compare by pattern."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.uint8).reshape(-1).clone() if t.numel() else torch.zeros(0, dtype=torch.uint8)


def freeze(outputs):
    """{name: tensor} -> {name: (shape, dtype, bytes)}"""
    return {k: (tuple(v.shape), v.dtype, raw(v)) for k, v in outputs.items()}


def differences(ref, got):
    """Names (with the first differing element and the count) of the outputs whose bytes differ."""
    out = []
    if set(ref) != set(got):
        return [f"outputs {sorted(ref)} vs {sorted(got)}"]
    for k in ref:
        (s0, d0, b0), (s1, d1, b1) = ref[k], got[k]
        if s0 != s1 or d0 != d1:
            out.append(f"{k}: {s0} {d0} vs {s1} {d1}")
            continue
        ne = b0 != b1
        if bool(ne.any()):
            size = torch.empty(0, dtype=d0).element_size()
            idx = torch.nonzero(ne)[:, 0] // size
            first = int(idx[0])
            a = b0[first * size:(first + 1) * size].view(d0).item()
            b = b1[first * size:(first + 1) * size].view(d0).item()
            out.append(f"{k}{list(s0)}: {int(torch.unique(idx).numel())} elements differ, first at flat index {first}: "
                       f"clean {a!r} vs {b!r}")
    return out


# -- the case driver ----------------------------------------------------------------------------------------------------
def check(case, run, pattern, monkeypatch=None, memo=None, device_types=("cuda",), log=print):
    """``run(session) -> (outputs, owner)``: builds a fresh wrapper, makes the call under test and returns the defined
    regions of its outputs ({name: tensor}) and the wrapper object(s) / tensors whose kept scratch the call used (None:
    the entry point keeps nothing between calls; the pattern then reaches it through the allocators alone).  When
    ``session.stale`` it first makes a different call on the same wrapper and then calls ``session.scratch(owner)``;
    between the calls of a multi-call case it calls ``session.scratch(owner)`` as well (refill).

    Clean reference (zero fill, memoised per case in ``memo``) -> control -> the pattern's run, bytes compared."""
    def clean():
        with Session("zero", monkeypatch, device_types) as s:
            return freeze(run(s)[0])

    def reference():
        a, b = clean(), clean()
        d = differences(a, b)
        if d:
            raise NotDeterministic(f"{case}: not deterministic, two clean runs differ: " + "; ".join(d))
        return a

    ref = memo.get(case, reference) if memo is not None else reference()
    with Session(pattern, monkeypatch, device_types) as s:
        outs, owner = run(s)
        got = freeze(outs)
        reps = s.reports or [s.observe(owner)]
    for rep in reps:
        log(f"[poison] {case} {rep['label']} pattern={pattern} control=identical scratch_bytes={rep['bytes']} "
            f"arrived={rep['arrived']} never_written={100.0 * rep['never_written']:.1f}%")
    for rep in reps:
        if not rep["arrived"]:
            raise PoisonMissed(f"{case} {rep['label']}: pattern {pattern} did not reach the kept scratch "
                               f"({rep['bytes']} bytes)")
    d = differences(ref, got)
    if d:
        raise PoisonFinding(f"{case}: result depends on buffer contents (pattern {pattern}): " + "; ".join(d))
    return reps
