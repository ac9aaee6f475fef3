"""CPU checks of the batch-form fbank front-end's host side: ``ppasr_fbank_plan_batch`` needs no device and no handle, so the
segment table it fills -- sample, chunk and frame prefixes, output rows -- is checked here for every length around the window
and the 8192-sample chunk of the mean square."""
import ctypes

import numpy as np
import pytest
import torch

from ppasr_amd import _lib

EDGES = [8191, 8192, 8193, 16383, 16384, 16385, 24577]


def _plan(counts, sr=16000, t_max=0, length_ms=25.0, shift_ms=10.0):
    lib = _lib.load()
    n = len(counts)
    arr = (ctypes.c_int * max(n, 1))(*counts)
    table = (_lib.FbankSegment * max(n, 1))()
    chunks, frames = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.ppasr_fbank_plan_batch(sr, length_ms, shift_ms, ctypes.addressof(arr), n, t_max, ctypes.addressof(table),
                                    ctypes.byref(chunks), ctypes.byref(frames))
    return rc, list(table)[:n], chunks.value, frames.value


def _frames(n, sr):
    win, shift = sr // 40, sr // 100
    return 0 if n < win else 1 + (n - win) // shift


@pytest.mark.parametrize("sr,counts", [(16000, list(range(0, 1301))), (16000, EDGES), (8000, EDGES),
                                       (16000, [0, 399, 0, 8193, 400, 0]), (8000, list(range(0, 1301, 7)))])
def test_plan_prefixes(sr, counts):
    rc, table, chunks, frames = _plan(counts, sr)
    assert rc == _lib.PPASR_OK
    sample = chunk = frame = 0
    for b, (n, seg) in enumerate(zip(counts, table)):
        assert (seg.first_sample, seg.n_samples, seg.first_chunk, seg.first_frame) == (sample, n, chunk, frame), b
        assert seg.out_row == frame, b  # compact form: the output row is the compact frame number
        sample += n
        chunk += (n + 8191) // 8192
        frame += _frames(n, sr)
    assert (chunks, frames) == (chunk, frame)
    assert frames == sum(_frames(n, sr) for n in counts)


@pytest.mark.parametrize("sr", [16000, 8000])
def test_plan_padded_rows(sr):
    counts = EDGES + [0, sr // 40 - 1, sr // 40]
    t_max = max(_frames(n, sr) for n in counts)
    for stride in (t_max, t_max + 5):
        rc, table, chunks, frames = _plan(counts, sr, t_max=stride)
        assert rc == _lib.PPASR_OK
        assert [seg.out_row for seg in table] == [b * stride for b in range(len(counts))]
        # the compact numbering underneath does not change
        assert [seg.first_frame for seg in table] == list(np.cumsum([0] + [_frames(n, sr) for n in counts])[:-1])
        assert frames == sum(_frames(n, sr) for n in counts)


def test_plan_refusals():
    lib = _lib.load()
    rc, *_ = _plan([400, -1, 400])
    assert rc == _lib.PPASR_EINVAL and b"negative" in lib.ppasr_last_error()
    t_max = _frames(16385, 16000)
    assert _plan([400, 16385], t_max=t_max)[0] == _lib.PPASR_OK
    rc, *_ = _plan([400, 16385], t_max=t_max - 1)
    assert rc == _lib.PPASR_EINVAL and b"row stride" in lib.ppasr_last_error()
    with pytest.raises(_lib.PPASRHipError):
        _lib.check(rc)
    assert _plan([400], length_ms=0.0)[0] == _lib.PPASR_EINVAL
    # an empty batch and a batch of empty segments are legal
    assert _plan([])[0] == _lib.PPASR_OK and _plan([])[2:] == (0, 0)
    assert _plan([0, 0, 0])[2:] == (0, 0)


def test_batch_workspace_and_null_arguments():
    lib = _lib.load()
    assert lib.ppasr_fbank_batch_workspace_bytes(12, 9) >= (9 + 2 * 12) * 4
    assert lib.ppasr_fbank_batch_workspace_bytes(0, 0) > 0
    assert lib.ppasr_fbank_compute_batch(None, None, None, 1, 1, 1, 1, -20.0, None, None, 0, None) == _lib.PPASR_EINVAL
    assert ctypes.sizeof(_lib.FbankSegment) == 32


def test_featurize_many_refuses_to_run_without_gpu():
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    f = AudioFeaturizer(n_mels=80, sample_rate=16000)
    wavs = [np.zeros(1600, np.float32), np.zeros(100, np.float32)]
    if torch.cuda.is_available():  # (the suite on a GPU machine: the call runs; tests/test_fbank_batch_gpu.py checks it)
        assert f.featurize_many(wavs)[1].tolist() == [8, 0]
        return
    with pytest.raises(_lib.PPASRHipError):
        f.featurize(wavs[0])
    with pytest.raises(_lib.PPASRHipError):
        f.featurize_many(wavs)
    with pytest.raises(_lib.PPASRHipError):
        f.featurize_many(wavs, padded=True)
