"""CPU checks of the beam-search session pool's boundary: the header, the library and _lib.py agree on the
ppasr_beam_pool_* calls; argument validation of the C-ABI, BeamSearchSessions and StreamPool fails before any device work;
the wrappers refuse to run without a device."""
import ctypes
import os
import re

import pytest

from ppasr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_CALLS = ["ppasr_beam_pool_create", "ppasr_beam_pool_destroy", "ppasr_beam_pool_reset", "ppasr_beam_pool_frames",
              "ppasr_beam_pool_capacity", "ppasr_beam_pool_status", "ppasr_beam_pool_workspace_bytes",
              "ppasr_beam_pool_decode"]


def _declarations():
    src = open(os.path.join(ROOT, "include", "ppasr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"PPASR_API\s+([a-z_ ]+?\**)\s*\b(ppasr_beam_pool_[a-z_]+)\s*\(([^)]*)\)", src):
        out[m.group(2)] = (m.group(1).strip(), [a.strip() for a in m.group(3).split(",") if a.strip()])
    return out


def test_header_library_and_binding_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(POOL_CALLS)
    lib = _lib.load()
    bound = {name: (restype, argtypes) for name, restype, argtypes in _lib.SYMBOLS}
    c_types = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong,
               "ppasr_status": ctypes.c_int}
    for name, (ret, args) in decl.items():
        assert hasattr(lib, name)
        restype, argtypes = bound[name]
        assert restype is c_types[ret], name
        assert len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):
            typ = a.rsplit(" ", 1)[0] if "*" not in a else "*"
            if typ == "*" or typ.startswith("ppasr_beam_pool") or typ.startswith("ppasr_lm_handle"):
                assert t is ctypes.c_void_p or hasattr(t, "contents") or t.__name__.startswith("LP_"), (name, a, t)
            else:
                assert t is c_types[typ], (name, a, t)


def test_c_abi_refuses_before_any_device_work():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.ppasr_beam_pool_create(2, 300, 10, 0.99, 40, 0, None, 0.0, 0.0, 16, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_beam_pool_create(0, 300, 10, 0.99, 40, 0, None, 0.0, 0.0, 16, ctypes.byref(h)) == _lib.PPASR_EINVAL
    assert lib.ppasr_beam_pool_create(2, 300, 10, 0.99, 40, 0, None, 0.0, 0.0, 0, ctypes.byref(h)) == _lib.PPASR_EINVAL
    for V, beam in [(1, 10), (16384, 10), (300, 0), (300, 513)]:
        assert lib.ppasr_beam_pool_create(2, V, beam, 0.99, 40, 0, None, 0.0, 0.0, 16, ctypes.byref(h)) == \
            _lib.PPASR_EUNSUPPORTED
        assert not h.value
    assert lib.ppasr_beam_pool_create(2, 300, 10, 0.99, 40, 300, None, 0.0, 0.0, 16, ctypes.byref(h)) == _lib.PPASR_EINVAL
    assert lib.ppasr_beam_pool_destroy(None) == _lib.PPASR_EINVAL
    assert lib.ppasr_beam_pool_reset(None, -1, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_beam_pool_frames(None, 0) == -1 and lib.ppasr_beam_pool_capacity(None, 0) == -1
    assert lib.ppasr_beam_pool_workspace_bytes(None, 1, 16) == 0
    ids = (ctypes.c_int * 1)(0)
    assert lib.ppasr_beam_pool_decode(None, ids, 1, None, 0, None, 8, None, None, None, None, 0, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_beam_pool_status(None, None, None) == _lib.PPASR_EINVAL


def test_beam_sessions_validate_arguments_without_a_device(monkeypatch):
    import torch
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    vocab = ["<blank>", "a", "b"]
    for kw in (dict(n_sessions=0), dict(init_frames=0), dict(beam_size=0), dict(cutoff_top_n=0), dict(blank_id=3),
               dict(vocab_list=["<blank>"]), dict(scorer=object(), language_model_path="x.arpa")):
        args = dict(n_sessions=2, alpha=2.2, beta=4.3, beam_size=10, cutoff_prob=0.99, cutoff_top_n=40, vocab_list=vocab)
        args.update(kw)
        with pytest.raises(ValueError):
            BeamSearchSessions(**args)
    with pytest.raises(_lib.PPASRHipError):  # valid arguments, no device: no CPU fallback
        BeamSearchSessions(2, 2.2, 4.3, 10, 0.99, 40, vocab)


def test_stream_pool_validates_the_decoder_before_any_device_work():
    from ppasr_amd.serving import StreamPool
    vocab = ["<blank>", "a", "b"]
    # (model=None: every refusal comes before the model or a group is touched)
    with pytest.raises(ValueError):
        StreamPool(None, vocab, 2, decoder="attention_rescoring")
    with pytest.raises(ValueError):
        StreamPool(None, vocab, 2, decoder="ctc_beam_search", decoder_conf={"beam_width": 10})
    with pytest.raises(ValueError):
        StreamPool(None, vocab, 2, decoder="ctc_greedy", decoder_conf={"beam_size": 10})
