"""tests/poison.py has teeth: plain torch-CPU stand-ins of an entry point, each with one of the ways a kernel can let the
contents of an unwritten buffer into its result, are flagged by the pattern that is meant to catch them (and a correct
one by none); the "poison arrived" check and the run-to-run control fail when they should; and ppasr_amd allocates its
uninitialised device buffers through the two allocators the helper replaces."""
import os
import re

import pytest
import torch

import poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = ("cpu",)
T, D = 12, 8


def _inputs():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(T, D, generator=g) + 0.5
    valid = 7  # rows behind it are padding: the stand-ins must not let them into the result
    return x, valid


class MaskedProduct:
    """p * scratch with p == 0 on the masked rows of a scratch whose masked rows nobody wrote (the `vt` of the fused
    attention without its clear)."""
    alloc = staticmethod(lambda *a, **k: torch.empty(*a, **k))

    def __init__(self):
        self._ws = None

    def __call__(self, x, valid):
        if self._ws is None:
            self._ws = self.alloc(T, D, dtype=torch.float32)
        self._ws[:valid] = 2.0 * x[:valid]
        p = torch.zeros(T)
        p[:valid] = 1.0 / valid
        out = torch.empty(D, dtype=torch.float32)
        out[:] = (p[:, None] * self._ws).sum(0)
        return out


class Accumulate(MaskedProduct):
    """+= into a partial-sum buffer nobody cleared (a split launch's join that adds to the buffer instead of storing)."""

    def __call__(self, x, valid):
        if self._ws is None:
            self._ws = self.alloc(D, dtype=torch.float32)
        self._ws += 2.0 * x[:valid].sum(0)
        out = torch.empty(D, dtype=torch.float32)
        out[:] = self._ws
        return out


class IntTable(MaskedProduct):
    """A "child of this node" table where -1 (or 0: node 0 is the root, nobody's child) means none, consulted behind the
    part the stand-in cleared: a -1 fill passes as "empty", a large positive int is trusted as a node index."""

    def __call__(self, x, valid):
        if self._ws is None:
            self._ws = self.alloc(T, dtype=torch.int32)
        self._ws[:valid] = -1  # the clear stops at the valid rows ...
        out = torch.empty(D, dtype=torch.float32)
        out[:] = 0.0
        for t in range(T):  # ... the walk does not
            child = int(self._ws[t])
            out += x[child % T] if child > 0 else x[t]
        return out


class Correct(MaskedProduct):
    """Reads only what it wrote."""

    def __call__(self, x, valid):
        if self._ws is None:
            self._ws = self.alloc(T, D, dtype=torch.float32)
        self._ws[:valid] = 2.0 * x[:valid]
        out = torch.empty(D, dtype=torch.float32)
        out[:] = self._ws[:valid].sum(0) / valid
        return out


def _run(cls, **attrs):
    def run(session):
        m = cls()
        for k, v in attrs.items():
            setattr(m, k, v)
        x, valid = _inputs()
        if session.stale:  # another call first, on the same stand-in: all rows valid, other values
            m(x + 1.0, T)
            session.scratch(m)
        return {"out": m(x, valid)}, m
    return run


def _flags(cls, pattern, monkeypatch):
    try:
        poison.check(cls.__name__, _run(cls), pattern, monkeypatch, device_types=CPU, log=lambda s: None)
    except poison.PoisonFinding:
        return True
    return False


def test_ff_flags_the_masked_product_and_the_accumulation(monkeypatch):
    assert _flags(MaskedProduct, "ff", monkeypatch)
    assert _flags(Accumulate, "ff", monkeypatch)


def test_7f_flags_the_int_table_that_ff_lets_pass(monkeypatch):
    assert _flags(IntTable, "7f", monkeypatch)
    assert not _flags(IntTable, "ff", monkeypatch)  # -1 is the table's own "empty": why 0x7F is in the matrix


def test_the_old_guard_sentinel_does_not_flag_the_masked_product(monkeypatch):
    """0xA5 bytes are -2.87e-16 as fp32: 0 x that is -0.0, and the sum of the row is what it was."""
    assert not _flags(MaskedProduct, "a5", monkeypatch)
    # and 0 x 3.39e38 is 0 as well: 0x7F is for sums and int tables, 0xFF for products
    assert not _flags(MaskedProduct, "7f", monkeypatch)
    assert _flags(Accumulate, "7f", monkeypatch)


def test_stale_contents_pass_the_masked_product_and_flag_the_accumulation(monkeypatch):
    """What an earlier, larger call on the same stand-in left behind: finite floats, which 0 x hides (the reason the
    suite never saw such a read), but which a sum picks up."""
    assert not _flags(MaskedProduct, poison.STALE, monkeypatch)
    assert _flags(Accumulate, poison.STALE, monkeypatch)


@pytest.mark.parametrize("pattern", ["ff", "7f", "a5", poison.STALE])
def test_the_correct_stand_in_passes_every_pattern(pattern, monkeypatch, capsys):
    reps = poison.check("Correct", _run(Correct), pattern, monkeypatch, device_types=CPU)
    line = capsys.readouterr().out
    assert "control=identical" in line and "never_written=" in line and f"pattern={pattern}" in line
    assert all(r["arrived"] for r in reps)
    # rows behind `valid` are never written: (T - valid) / T of the scratch still holds the pattern
    # (an upper bound: a byte written with the pattern's own value counts as unwritten)
    # (stale: "unchanged since entry", and the earlier call's values share exponent bytes with this one's)
    assert (T - 7) / T <= reps[0]["never_written"] <= (T - 7) / T + (0.2 if pattern == poison.STALE else 0.03)


def test_poison_arrived_fails_when_the_scratch_was_not_allocated_through_the_patched_allocators(monkeypatch):
    with pytest.raises(poison.PoisonMissed):
        poison.check("Correct-zeros", _run(Correct, alloc=torch.zeros), "ff", monkeypatch, device_types=CPU,
                     log=lambda s: None)
    # host tensors are left alone when only device tensors are watched (the GPU tests' setting)
    with pytest.raises(poison.PoisonMissed):
        poison.check("Correct-host", _run(Correct), "ff", monkeypatch, log=lambda s: None)


def test_control_reports_run_to_run_noise_as_not_deterministic(monkeypatch):
    calls = [0]

    class Noisy(Correct):
        def __call__(self, x, valid):
            calls[0] += 1
            return Correct.__call__(self, x, valid) + 1e-7 * calls[0]

    with pytest.raises(poison.NotDeterministic, match="not deterministic"):
        poison.check("Noisy", _run(Noisy), "ff", monkeypatch, device_types=CPU, log=lambda s: None)


def test_memo_keeps_one_clean_reference_per_case(monkeypatch):
    from numerics import Memo
    built = [0]

    class Counted(Correct):
        def __init__(self):
            built[0] += 1
            Correct.__init__(self)

    memo = Memo()
    for pattern in ("ff", "7f"):
        poison.check("Counted", _run(Counted), pattern, monkeypatch, memo=memo, device_types=CPU, log=lambda s: None)
    assert built[0] == 2 + 2  # two clean runs once, one run per pattern


def test_allocators_are_restored_and_bytes_compare_nans_by_pattern(monkeypatch):
    e, el = torch.empty, torch.empty_like
    with poison.Session("ff", monkeypatch, CPU) as s:
        a = torch.empty(3, dtype=torch.float32)
        b = torch.empty_like(a, dtype=torch.int32)
        c = torch.zeros(3)
        assert bool(torch.isnan(a).all()) and b.tolist() == [-1, -1, -1] and not bool(c.any())
        assert len(s.filled) == 2
    assert torch.empty is e and torch.empty_like is el
    with poison.Session("7f", None, CPU):
        assert torch.empty(1, dtype=torch.int32).item() == 2139062143
        assert torch.empty(1, dtype=torch.float32).item() == pytest.approx(3.39e38, rel=1e-2)
    assert torch.empty is e and torch.empty_like is el
    nan = torch.full((2,), float("nan"))
    assert not poison.differences(poison.freeze({"x": nan}), poison.freeze({"x": nan.clone()}))
    assert poison.differences(poison.freeze({"x": torch.zeros(2)}), poison.freeze({"x": -torch.zeros(2)}))  # +0 vs -0


def test_kept_scratch_finds_what_the_wrappers_keep():
    class W:
        pass
    w, s1, s2 = W(), W(), W()
    w._ws = {1: torch.ones(2), 2: torch.ones(3)}
    s1._ws, s2._ws = torch.ones(4), None
    w._scratch_stream, w._streams = s1, [s1, s2]
    w.buf = torch.ones(5)  # carried state: not scratch
    got = poison.kept_scratch([w, torch.ones(6)])
    assert sorted(t.numel() for t in got) == [2, 3, 4, 6]


def test_ppasr_amd_allocates_uninitialised_buffers_only_with_empty_and_empty_like():
    """The allocation poisoning replaces torch.empty and torch.empty_like: any other way to get uninitialised memory
    (new_empty, empty_strided, the legacy constructors, resize_, an alias of torch.empty bound at import time) would
    slip past it."""
    banned = re.compile(r"new_empty|empty_strided|empty_permuted|empty_quantized|\.new\(|\.resize_\(|\.set_\("
                        r"|torch\.(cuda\.)?(Tensor|FloatTensor|DoubleTensor|HalfTensor|IntTensor|LongTensor|ByteTensor)\("
                        r"|from\s+torch\s+import|import\s+torch\s+as|=\s*torch\.empty(_like)?\s*$")
    wrappers, hits = 0, []
    for d, _, files in os.walk(os.path.join(ROOT, "ppasr_amd")):
        for f in files:
            if not f.endswith(".py"):
                continue
            for n, line in enumerate(open(os.path.join(d, f), encoding="utf-8"), 1):
                code = line.split("#", 1)[0]
                if banned.search(code):
                    hits.append(f"{os.path.relpath(os.path.join(d, f), ROOT)}:{n}: {line.strip()}")
                wrappers += len(re.findall(r"torch\.empty(_like)?\(", code))
    assert not hits, "\n".join(hits)
    assert wrappers >= 40  # (the check looked at the wrappers at all)
