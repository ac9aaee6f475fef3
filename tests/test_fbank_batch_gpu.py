"""GPU: the batch form of the fbank front-end (``AudioFeaturizer.featurize_many`` -> ``ppasr_fbank_compute_batch``, the
segment-table kernels of csrc/fbank.hip).  The reference of every check is the single-waveform call on the same build
(``featurize_device``), compared byte for byte: features, per-chunk sums of the mean square and the gain.  No tolerance
anywhere, except where the single-waveform call computes nothing to compare with (a segment without a frame): its gain is
held to ``db_gain`` within the 4 ulp tests/test_fbank_gpu.py allows the kernel's log10."""
import functools

import numpy as np
import pytest
import torch

import poison
from test_fbank_gpu import _audio

pytestmark = pytest.mark.gpu

# most lengths odd (unaligned packed offsets); 399 / 400 / 401, 559 / 560: zero, one, two frames at 16 kHz; 8191 .. 8193: the
# chunk boundary of the mean square; 16383: a full chunk followed by the depth-7 tail; 16385: three chunks
LENS = [0, 399, 400, 401, 559, 560, 8191, 8192, 8193, 16383, 16385, 20000]
SUBSET = [401, 8193, 16383, 20000]
ZERO_AT = 5  # this segment of a batch is silence


def _featurizer(n_mels=80, sr=16000, use_db=True):
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    return AudioFeaturizer(feature_method="fbank", n_mels=n_mels, sample_rate=sr, use_dB_normalization=use_db, target_dB=-20)


def _segments(lens, sr=16000, seed=0, zero_at=None):
    out = [_audio(max(lens) / sr + 0.01, seed=seed + 7 * i, sr=sr)[:n].copy() for i, n in enumerate(lens)]
    if zero_at is not None:
        out[zero_at][:] = 0.0
    assert [w.size for w in out] == list(lens)
    return out


def _raw(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _single(f, wav):
    """featurize_device on one waveform -> (feats, chunk-sum bytes, gain bytes); the last two None where that call
    computes none (no dB normalisation, or no frame)."""
    feats = f.featurize_device(wav).clone()
    if not f.use_db_normalization or feats.shape[0] == 0:
        return feats, None, None
    chunks = (wav.size + 8191) // 8192
    return feats, _raw(f._ws[:4 * chunks]), _raw(f._ws[4 * chunks:4 * chunks + 8])


@functools.lru_cache(maxsize=None)
def _reference(n_mels, sr, use_db, lens, seed, zero_at):
    """the single-waveform results of one batch, computed once"""
    f = _featurizer(n_mels, sr, use_db)
    wavs = _segments(lens, sr, seed, zero_at)
    return wavs, [_single(f, w) for w in wavs]


def _check_batch(f, wavs, refs, feats, counts):
    from ppasr_amd.data_utils.featurizer import db_gain
    torch.cuda.synchronize()
    assert counts.tolist() == [r[0].shape[0] for r in refs]
    assert feats.shape == (int(counts.sum()), refs[0][0].shape[1])
    ws = f._scratch["ws"]
    total_chunks = sum((w.size + 8191) // 8192 for w in wavs)
    row = chunk = 0
    for b, (w, (ref, sums, gain)) in enumerate(zip(wavs, refs)):
        t, c = ref.shape[0], (w.size + 8191) // 8192
        assert torch.equal(feats[row:row + t], ref), (b, w.size)
        if f.use_db_normalization:
            got_gain = ws[4 * total_chunks + 8 * b:4 * total_chunks + 8 * b + 8]
            if sums is not None:
                assert _raw(ws[4 * chunk:4 * (chunk + c)]) == sums, (b, w.size)
                assert _raw(got_gain) == gain, (b, w.size)
            elif w.size:  # no frame: nothing of the single call's to compare with
                acc = np.float32(0)
                for v in ws[4 * chunk:4 * (chunk + c)].view(torch.float32).cpu().numpy():
                    acc = np.float32(acc + v)
                assert acc.tobytes() == np.add.reduce(w ** 2).tobytes(), (b, w.size)
                g = np.float32(db_gain(w, -20))
                assert abs(float(got_gain.view(torch.float32)[0]) - float(g)) <= 4 * float(np.spacing(g)), (b, w.size)
        row += t
        chunk += c


@pytest.mark.parametrize("n_mels,sr,lens,zero_at", [(80, 16000, tuple(LENS), ZERO_AT), (40, 8000, tuple(SUBSET), None),
                                                    (128, 16000, tuple(SUBSET), None)],
                         ids=["80mel-16k", "40mel-8k", "128mel-16k"])
@pytest.mark.parametrize("use_db", [True, False], ids=["db", "nodb"])
def test_every_segment_equals_its_own_call(n_mels, sr, lens, zero_at, use_db):
    wavs, refs = _reference(n_mels, sr, use_db, lens, 3, zero_at)
    f = _featurizer(n_mels, sr, use_db)
    feats, counts = f.featurize_many(wavs)
    _check_batch(f, wavs, refs, feats, counts)
    assert sum(r[0].shape[0] > 0 for r in refs) >= 3


def test_a_segment_does_not_depend_on_its_neighbours():
    lens = (8193, 401, 16383)
    wavs, refs = _reference(80, 16000, True, lens, 11, None)
    others = _segments([777, 20000, 8192], seed=50)
    f = _featurizer()
    for order in ([0, 1, 2], [2, 0, 1]):
        feats, counts = f.featurize_many([wavs[i] for i in order])
        _check_batch(f, [wavs[i] for i in order], [refs[i] for i in order], feats, counts)
    batch = [others[0], wavs[0], others[1], wavs[1], wavs[2], others[2]]
    feats, counts = f.featurize_many(batch)
    torch.cuda.synchronize()
    starts = np.concatenate([[0], np.cumsum(counts)])
    for pos, i in ((1, 0), (3, 1), (4, 2)):
        assert torch.equal(feats[starts[pos]:starts[pos + 1]], refs[i][0]), (pos, i)


@pytest.mark.parametrize("pattern", ["ff", "7f"])
def test_padded_form(pattern):
    wavs, refs = _reference(80, 16000, True, tuple(LENS), 3, ZERO_AT)
    f = _featurizer()
    # a larger call first, so that the grow-only buffers hold large values past what the next call writes
    loud = [np.clip(40.0 * w, -1, 1) for w in _segments([30000, 25001, 20000] * 5, seed=90)]
    big, _ = f.featurize_many(loud, padded=True)
    assert float(big.abs().max()) > 5.0
    del big
    for t in f._scratch.values():
        if t.is_cuda:
            poison.fill(t, poison.BYTES[pattern])
    with poison.Session(pattern) as session:  # feats reaches the call filled with the pattern
        feats, lens = f.featurize_many(wavs, padded=True)
        assert session.filled
    torch.cuda.synchronize()
    t_max = max(r[0].shape[0] for r in refs)
    assert feats.shape == (len(wavs), t_max, 80) and lens.dtype == torch.int64
    assert lens.tolist() == [r[0].shape[0] for r in refs]
    for b, (ref, _, _) in enumerate(refs):
        t = ref.shape[0]
        assert torch.equal(feats[b, :t], ref), b
        assert not bool(feats[b, t:].contiguous().view(torch.int32).any()), b  # +0.0, bit for bit
    compact, _ = f.featurize_many(wavs)
    assert torch.equal(compact, torch.cat([feats[b, :int(lens[b])] for b in range(len(wavs))]))


@pytest.mark.parametrize("use_db", [True, False], ids=["db", "nodb"])
def test_two_calls_back_to_back(use_db):
    lens = (16385, 401, 8193, 20000)
    wavs_a, refs_a = _reference(80, 16000, use_db, lens, 21, None)
    wavs_b, refs_b = _reference(80, 16000, use_db, lens, 22, None)
    f = _featurizer(use_db=use_db)
    f.featurize_many(wavs_a)  # (buffers at their final size: the two calls below reuse them)
    torch.cuda.synchronize()
    fa, ca = f.featurize_many(wavs_a)
    fb, cb = f.featurize_many(wavs_b)  # same staging buffers, other data, no synchronisation in between
    torch.cuda.synchronize()
    for feats, counts, refs in ((fa, ca, refs_a), (fb, cb, refs_b)):
        assert torch.equal(feats, torch.cat([r[0] for r in refs]))
        assert counts.tolist() == [r[0].shape[0] for r in refs]
    assert not torch.equal(fa, fb)


@pytest.mark.parametrize("use_db,launches", [(True, 3), (False, 1)], ids=["db", "nodb"])
def test_launch_count_does_not_depend_on_the_batch(use_db, launches):
    from ppasr_amd import _lib
    f = _featurizer(use_db=use_db)
    wavs = _segments([401, 8193, 16383, 20000, 0, 399, 5000, 560], seed=31)
    for batch in (wavs, wavs[1:2]):
        f.featurize_many(batch)  # (handle, buffers)
        torch.cuda.synchronize()
        with _lib.kernel_profile() as kp:
            f.featurize_many(batch)
            torch.cuda.synchronize()
        assert sum(c for _, c in kp.kernels.values()) == launches, kp.kernels
        assert len(kp.kernels) == launches and all("batch" in k for k in kp.kernels), kp.kernels


def test_gain_refusal():
    f = _featurizer()
    wavs = _segments([8193, 1600, 401], seed=41)
    wavs[1] = np.full(1600, 1e-20, np.float32)  # mean square 1e-40: a gain of 380 dB
    with pytest.raises(ValueError):
        f.featurize_many(wavs)
    with pytest.raises(ValueError):
        f.featurize_many(wavs, padded=True)
    feats, counts = f.featurize_many([wavs[0], wavs[2]])  # the featurizer stays usable
    assert counts.tolist() == [49, 1]


@pytest.mark.parametrize("n", [400, 16383, 20000])
def test_batch_of_one_equals_featurize_device(n):
    f, g = _featurizer(), _featurizer()
    wav = _segments([n], seed=61)[0]
    feats, counts = f.featurize_many([wav])
    ref = g.featurize_device(wav)
    assert counts.tolist() == [ref.shape[0]] and torch.equal(feats, ref)
    assert np.float32(f.last_gains[0]).tobytes() == np.float32(g.last_gain).tobytes()
    padded, lens = f.featurize_many([wav], padded=True)
    assert padded.shape == (1, ref.shape[0], 80) and torch.equal(padded[0], ref) and lens.tolist() == [ref.shape[0]]
