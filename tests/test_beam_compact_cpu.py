"""CPU checks of the prefix-arena compaction's boundary: the header, the library and _lib.py agree on the five new calls;
every refusal of the C-ABI comes back with its code with no device; BeamSearchSessions(compact=...),
BeamSearchDecoder(compact=...) and StreamPool(beam_compact=...) validate before any device work."""
import ctypes
import os
import re

import pytest

from ppasr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPACT_CALLS = ["ppasr_ctc_beam_state_compact", "ppasr_beam_arena_compact", "ppasr_beam_arena_set_auto",
                 "ppasr_beam_arena_live_nodes", "ppasr_beam_arena_bytes"]


def _declarations():
    src = open(os.path.join(ROOT, "include", "ppasr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"PPASR_API\s+([a-z_ ]+?\**)\s*\b(ppasr_beam_arena_[a-z_]+|ppasr_ctc_beam_state_compact)\s*\(([^)]*)\)",
                         src):
        out[m.group(2)] = (m.group(1).strip(), [a.strip() for a in m.group(3).split(",") if a.strip()])
    return out


def test_header_library_and_binding_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(COMPACT_CALLS)
    lib = _lib.load()
    bound = {name: (restype, argtypes) for name, restype, argtypes in _lib.SYMBOLS}
    c_types = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "ppasr_status": ctypes.c_int}
    for name, (ret, args) in decl.items():
        assert hasattr(lib, name)
        restype, argtypes = bound[name]
        assert restype is c_types[ret], name
        assert len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):
            typ = a.rsplit(" ", 1)[0] if "*" not in a else "*"
            if typ == "*" or typ.startswith("ppasr_beam_pool"):
                assert t is ctypes.c_void_p or hasattr(t, "contents") or t.__name__.startswith("LP_"), (name, a, t)
            else:
                assert t is c_types[typ], (name, a, t)


def test_c_abi_refuses_before_any_device_work():
    lib = _lib.load()
    live = (ctypes.c_int32 * 4)()
    fake = ctypes.c_void_p(0x1000)  # (never dereferenced: every call below is refused by its arguments)
    big = int(lib.ppasr_ctc_beam_state_bytes(2, 16, 10))
    assert lib.ppasr_ctc_beam_state_compact(None, big, 2, 10, 0, live, None) == _lib.PPASR_EINVAL       # null state
    assert lib.ppasr_ctc_beam_state_compact(fake, big, 0, 10, 0, live, None) == _lib.PPASR_EINVAL       # B <= 0
    assert lib.ppasr_ctc_beam_state_compact(fake, big, -1, 10, 0, None, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_ctc_beam_state_compact(fake, big, 2, 0, 0, live, None) == _lib.PPASR_EINVAL        # beam_size < 1
    one = int(lib.ppasr_ctc_beam_state_bytes(1, 1, 10))
    assert lib.ppasr_ctc_beam_state_compact(fake, one - 1, 1, 10, 0, live, None) == _lib.PPASR_EINVAL   # < one frame
    assert lib.ppasr_ctc_beam_state_compact(fake, 2 * one - 1, 2, 10, 1, None, None) == _lib.PPASR_EINVAL
    ids = (ctypes.c_int * 1)(0)
    out = (ctypes.c_longlong * 1)()
    assert lib.ppasr_beam_arena_compact(None, ids, 1, out, None) == _lib.PPASR_EINVAL                   # null pool
    assert lib.ppasr_beam_arena_compact(None, None, -1, None, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_beam_arena_set_auto(None, 1) == _lib.PPASR_EINVAL
    assert lib.ppasr_beam_arena_live_nodes(None, 0) == -1
    assert lib.ppasr_beam_arena_bytes(None) == 0


def test_wrappers_validate_compact_without_a_device(monkeypatch):
    import torch
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchDecoder, BeamSearchSessions
    from ppasr_amd.serving import StreamPool
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    vocab = ["<blank>", "a", "b"]
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            BeamSearchSessions(2, 2.2, 4.3, 10, 0.99, 40, vocab, compact=bad)
        with pytest.raises(ValueError):
            BeamSearchDecoder(2.2, 4.3, 10, 0.99, 40, vocab, compact=bad)
        with pytest.raises(ValueError):
            StreamPool(None, vocab, 2, decoder="ctc_beam_search", beam_compact=bad)
    for ok in (True, False):
        with pytest.raises(_lib.PPASRHipError):  # valid arguments, no device: no CPU fallback
            BeamSearchSessions(2, 2.2, 4.3, 10, 0.99, 40, vocab, compact=ok)
        assert BeamSearchDecoder(2.2, 4.3, 10, 0.99, 40, vocab, compact=ok).compact is ok  # (no device until it decodes)
    # (model=None: every refusal comes before the model or a group is touched)
    with pytest.raises(ValueError):
        StreamPool(None, vocab, 2, decoder="ctc_greedy", beam_compact=True)        # a beam-search option
    with pytest.raises(ValueError):
        StreamPool(None, vocab, 2, decoder="ctc_beam_search", decoder_conf={"beam_compact": True})  # not a YAML key
