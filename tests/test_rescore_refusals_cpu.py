"""Refusals of the rescoring entry points that come before any device work (no GPU needed), as tests/test_capi_cpu.py does
for the encoder: shapes the decoder kernels are not built for are refused at create, never emulated, and NULL handles /
arguments are rejected.  (The refusals of ppasr_rescore itself need a rescorer, i.e. a device: tests/test_rescore_gpu.py.)"""
import ctypes

import numpy as np
import pytest

from ppasr_amd import _lib


def _create(desc):
    lib = _lib.load()
    h = ctypes.c_void_p(0)
    blob = (_lib.WeightBlob * 1)()
    a = np.zeros(1, np.float32)
    blob[0].name, blob[0].data_host, blob[0].ndim = b"x", a.ctypes.data, 1
    blob[0].shape[0] = 1
    rc = lib.ppasr_rescorer_create(ctypes.byref(desc), blob, 1, ctypes.byref(h))
    assert not h.value
    return rc, lib.ppasr_last_error()


@pytest.mark.parametrize("desc", [
    _lib.RescorerDesc(100, 512, 8, 2048, 3, 3, 5000),   # another width
    _lib.RescorerDesc(100, 256, 8, 2048, 3, 3, 5000),   # another head count
    _lib.RescorerDesc(100, 256, 4, 1000, 3, 3, 5000),   # linear_units not a multiple of 256
    _lib.RescorerDesc(100, 256, 4, 2048, 0, 3, 5000),   # no left blocks
    _lib.RescorerDesc(100, 256, 4, 2048, 7, 0, 5000),   # more than 6
    _lib.RescorerDesc(100, 256, 4, 2048, 3, 7, 5000),
    _lib.RescorerDesc(1, 256, 4, 2048, 3, 3, 5000),     # V < 2
])
def test_unsupported_decoder_shapes_are_refused_at_create(desc):
    rc, msg = _create(desc)
    assert rc == _lib.PPASR_EUNSUPPORTED, msg
    assert b"attention decoder" in msg


def test_null_arguments():
    lib = _lib.load()
    assert lib.ppasr_rescorer_create(None, None, 0, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_rescorer_workspace_bytes(None, 1, 10, 1, 4) == 0
    assert lib.ppasr_rescorer_destroy(None) == _lib.PPASR_OK
    rc = lib.ppasr_rescore(None, None, None, 1, 1, None, None, None, 1, 1, 0.5, 0.0, None, None, None, None, None, None, None,
                           0, None)
    assert rc == _lib.PPASR_EINVAL and b"null" in lib.ppasr_last_error()
    with pytest.raises(_lib.PPASRHipError):
        _lib.check(lib.ppasr_set_memory_out(None, None, 0))


def test_python_wrapper_refuses_unbuilt_options_before_loading_anything():
    import torch
    if torch.cuda.is_available():
        from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
        for bad in (dict(normalize_before=False), dict(concat_after=True)):
            with pytest.raises(_lib.PPASRHipError) as e:
                AttentionRescorer({}, 100, dict(attention_heads=4, linear_units=1024, num_blocks=1, **bad))
            assert e.value.status == _lib.PPASR_EUNSUPPORTED
    else:
        from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
        with pytest.raises(_lib.PPASRHipError):  # no device: no fallback
            AttentionRescorer({}, 100, {})
