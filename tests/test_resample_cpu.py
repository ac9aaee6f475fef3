"""CPU checks of the device resampler's host side (csrc/resample.hip, ``ppasr_resampler_*``): the filter table against
``up * firwin(...)`` placed by phase (tests/resample_cases.py), the geometry and the stream helpers against their integer
definitions, the refusals, and what ``AudioFeaturizer(resample=...)`` accepts.  No device is touched."""
import ctypes

import numpy as np
import pytest

import resample_cases as rc
from ppasr_amd import _lib

PAIRS = [(r, rc.MODEL_RATE) for r in rc.ALL_RATES] + [(16000, 8000), (8000, 44100), (16000, 15625)]


def _geometry(in_rate, out_rate):
    v = [ctypes.c_int(-7) for _ in range(5)]
    st = _lib.load().ppasr_resampler_geometry(in_rate, out_rate, *[ctypes.byref(x) for x in v])
    return st, [x.value for x in v]


@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_geometry(in_rate, out_rate):
    st, got = _geometry(in_rate, out_rate)
    g = rc.geometry(in_rate, out_rate)
    assert st == _lib.PPASR_OK
    assert got == [g["up"], g["down"], g["taps"], g["n_pre_pad"], g["n_pre_remove"]]
    if out_rate == rc.MODEL_RATE:
        assert g["taps"] == rc.TAPS[in_rate]
    assert _lib.RESAMPLE_TILE == rc.TILE


def test_largest_standard_table():
    sizes = {r: rc.geometry(r, rc.MODEL_RATE)["up"] * rc.geometry(r, rc.MODEL_RATE)["taps"] for r in rc.ALL_RATES}
    assert max(sizes, key=sizes.get) == 11025 and sizes[11025] == 640 * 21


@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_table_is_firwin_rounded_once(in_rate, out_rate):
    g = rc.geometry(in_rate, out_rate)
    want, real = rc.table64(in_rate, out_rate)
    got = np.full(want.shape, np.nan, np.float32)
    assert _lib.load().ppasr_resampler_table(in_rate, out_rate, got.ctypes.data) == _lib.PPASR_OK
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-12
    print("worst table err / bound", float((err / bound).max()), "rows x taps", want.shape)
    assert (err <= bound).all()
    assert (got[~real] == 0).all() and not np.signbit(got[~real]).any()  # the padding: exactly +0
    assert real.sum() == g["L"]  # every coefficient of h has one place
    # unit gain at 0 Hz: every phase's taps add up to ~1 for an interpolator's rows ... in all: sum(h) = up
    assert abs(float(got.astype(np.float64).sum()) - g["up"]) < 1e-4 * g["up"]


@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_out_len_ready_first_needed(in_rate, out_rate):
    lib = _lib.load()
    g = rc.geometry(in_rate, out_rate)
    for n in list(range(0, 40)) + [159, 160, 1000, 3333, 16000, 2 ** 31 - 1, 2 ** 31, 2 ** 35 + 12345, 2 ** 40 - 1, 2 ** 40]:
        assert lib.ppasr_resampler_out_len(in_rate, out_rate, n) == -(-n * g["up"] // g["down"]), n
        # ready(n): the first output that is NOT ready reads sample n or later, the one before it does not
        r = lib.ppasr_resampler_ready(in_rate, out_rate, n)
        assert r >= 0 and rc.q_of(in_rate, out_rate, r) >= n, n
        assert r == 0 or rc.q_of(in_rate, out_rate, r - 1) < n, n
        assert r <= lib.ppasr_resampler_out_len(in_rate, out_rate, n)
        assert lib.ppasr_resampler_first_needed(in_rate, out_rate, n) == rc.first_needed(in_rate, out_rate, n), n
    for n in (0, 1, 2, 5, 77, 500):
        assert lib.ppasr_resampler_ready(in_rate, out_rate, n) == rc.ready(in_rate, out_rate, n), n


def test_refusals_write_nothing():
    lib = _lib.load()
    buf = np.full(1024 * 64, np.nan, np.float32)
    h = ctypes.c_void_p()
    for in_rate, out_rate, want in [(16000, 16000, _lib.PPASR_EINVAL), (0, 16000, _lib.PPASR_EINVAL),
                                    (16000, 0, _lib.PPASR_EINVAL), (-8000, 16000, _lib.PPASR_EINVAL),
                                    (8000, -1, _lib.PPASR_EINVAL), (16001, 16000, _lib.PPASR_EUNSUPPORTED),
                                    (16000, 16001, _lib.PPASR_EUNSUPPORTED), (1, 1025, _lib.PPASR_EUNSUPPORTED)]:
        st, got = _geometry(in_rate, out_rate)
        assert st == want and got == [-7] * 5, (in_rate, out_rate)
        assert b"resampler" in lib.ppasr_last_error()
        assert lib.ppasr_resampler_table(in_rate, out_rate, buf.ctypes.data) == want
        assert np.isnan(buf).all()
        assert lib.ppasr_resampler_out_len(in_rate, out_rate, 100) == -1
        assert lib.ppasr_resampler_ready(in_rate, out_rate, 100) == -1
        assert lib.ppasr_resampler_first_needed(in_rate, out_rate, 100) == -1
        # create refuses the same before it touches a device
        assert lib.ppasr_resampler_create(in_rate, out_rate, ctypes.byref(h)) == want and not h.value
    assert _geometry(1024, 1)[0] == _lib.PPASR_OK and _geometry(1, 1024)[0] == _lib.PPASR_OK  # the cap itself is inside
    # null pointers
    v = [ctypes.c_int(-7) for _ in range(5)]
    for hole in range(5):
        args = [ctypes.byref(x) for x in v]
        args[hole] = None
        assert lib.ppasr_resampler_geometry(8000, 16000, *args) == _lib.PPASR_EINVAL
        assert [x.value for x in v] == [-7] * 5
    assert lib.ppasr_resampler_table(8000, 16000, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_resampler_create(8000, 16000, None) == _lib.PPASR_EINVAL
    assert b"null" in lib.ppasr_last_error()
    # counts outside 0 .. 2^40
    for n in (-1, 2 ** 40 + 1):
        assert lib.ppasr_resampler_out_len(8000, 16000, n) == -1
        assert lib.ppasr_resampler_ready(8000, 16000, n) == -1
        assert lib.ppasr_resampler_first_needed(8000, 16000, n) == -1
    # compute refuses a null handle and bad windows before any launch
    assert lib.ppasr_resample_compute(None, None, 0, 0, None, 0, 0, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_resample_compute_batch(None, None, None, 0, 0, None, None) == _lib.PPASR_EINVAL
    with pytest.raises(_lib.PPASRHipError) as e:
        _lib.check(lib.ppasr_resampler_create(16001, 16000, ctypes.byref(h)))
    assert e.value.status == _lib.PPASR_EUNSUPPORTED


def test_audio_featurizer_resample_option(monkeypatch):
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    # the host route constructs without loading the library
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded at construction")))
    assert AudioFeaturizer().resample_mode == "host"
    assert AudioFeaturizer(resample="host").resample_mode == "host"
    assert AudioFeaturizer(resample="device").resample_mode == "device"
    assert AudioFeaturizer(**dict(feature_method="fbank", sample_rate=16000, resample="device")).resample_mode == "device"
    for bad in ("gpu", "", None, True, "Device"):
        with pytest.raises(ValueError, match="resample"):
            AudioFeaturizer(resample=bad)


def test_foreign_rates_need_the_device_option():
    """refused before any device call, whether or not a device is there"""
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer, StreamResampler
    f = AudioFeaturizer()
    x = np.zeros(4000, np.float32)
    with pytest.raises(ValueError, match='resample="device"'):
        f.featurize_many([x, x], sample_rates=[16000, 8000])
    with pytest.raises(ValueError, match='resample="device"'):
        f.featurize_many([x], sample_rates=8000)
    with pytest.raises(ValueError, match='resample="device"'):
        StreamResampler(f, 8000)
    with pytest.raises(ValueError, match="2 sample rates for 1"):
        AudioFeaturizer(resample="device").featurize_many([x], sample_rates=[8000, 8000])
