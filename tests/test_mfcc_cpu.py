"""CPU checks of the MFCC form of the front-end (``feature_method='mfcc'``): the DCT and lifter tables ``ppasr_mfcc_create``
uploads, handed out by the host-only ``ppasr_mfcc_tables``, against their float64 statement (tests/mfcc_cases.py); the
refusals of the two calls; and what ``AudioFeaturizer`` accepts at construction.  No device is touched."""
import ctypes

import numpy as np
import pytest

import mfcc_cases as mc
from ppasr_amd import _lib

SHAPES = [(80, 40), (80, 13), (23, 13), (40, 40), (256, 256), (80, 1)]


def _tables(n_mels, n_mfcc, q=mc.LIFTER):
    lib = _lib.load()
    d = np.full((max(n_mels, 1), max(n_mfcc, 1)), np.nan, np.float32)
    l = np.full(max(n_mfcc, 1), np.nan, np.float32)
    rc = lib.ppasr_mfcc_tables(n_mels, n_mfcc, q, d.ctypes.data, l.ctypes.data)
    return rc, d, l


@pytest.mark.parametrize("n_mels,n_mfcc", SHAPES)
def test_tables_are_float64_rounded_once(n_mels, n_mfcc):
    rc, d, l = _tables(n_mels, n_mfcc)
    assert rc == _lib.PPASR_OK
    want_d, want_l = mc.dct_matrix(n_mels, n_mfcc), mc.lifter(n_mfcc)
    # one fp32 ulp per entry (relative 2^-23), + 1e-9 absolute for the cosines next to a zero, where the last bits of the
    # float64 argument decide the value
    err_d = np.abs(d.astype(np.float64) - want_d)
    err_l = np.abs(l.astype(np.float64) - want_l)
    print("worst D err / ulp", float((err_d / (2.0 ** -23 * np.abs(want_d) + 1e-9)).max()),
          "worst L err / ulp", float((err_l / (2.0 ** -23 * np.abs(want_l) + 1e-9)).max()))
    assert (err_d <= 2.0 ** -23 * np.abs(want_d) + 1e-9).all()
    assert (err_l <= 2.0 ** -23 * np.abs(want_l) + 1e-9).all()
    assert l[0] == 1.0
    assert (d[:, 0] == np.float32(np.sqrt(1.0 / n_mels))).all()


@pytest.mark.parametrize("n", [23, 40, 80, 256])
def test_square_table_is_orthonormal(n):
    rc, d, _ = _tables(n, n)
    assert rc == _lib.PPASR_OK
    d = d.astype(np.float64)
    assert np.abs(d.T @ d - np.eye(n)).max() < 1e-6


def test_lifter_zero_is_identity():
    rc, d, l = _tables(80, 40, 0.0)
    assert rc == _lib.PPASR_OK and (l == 1.0).all()
    rc, d22, l22 = _tables(80, 40)
    assert d.tobytes() == d22.tobytes()          # the lifter does not touch D
    assert l22[0] == 1.0 and l22[11] == 12.0     # 1 + 11 sin(pi / 2)
    assert l22[33] == -10.0                      # 1 + 11 sin(3 pi / 2): the lifter changes sign past k = 22


def test_refusals():
    lib = _lib.load()
    for n_mels, n_mfcc, q in [(80, 0, 22.0), (80, -3, 22.0), (80, 81, 22.0), (80, 40, -1.0), (0, 0, 22.0), (257, 40, 22.0),
                              (80, 40, float("nan")), (80, 40, float("inf"))]:
        rc, d, l = _tables(n_mels, n_mfcc, q)
        assert rc == _lib.PPASR_EINVAL, (n_mels, n_mfcc, q)
        assert np.isnan(d).all() and np.isnan(l).all()  # nothing written
    assert b"mfcc" in lib.ppasr_last_error()
    buf = np.zeros(80 * 40, np.float32)
    assert lib.ppasr_mfcc_tables(80, 40, 22.0, None, buf.ctypes.data) == _lib.PPASR_EINVAL
    assert lib.ppasr_mfcc_tables(80, 40, 22.0, buf.ctypes.data, None) == _lib.PPASR_EINVAL
    # ppasr_mfcc_create refuses the same arguments, and ppasr_fbank_create's, before it touches a device
    h = ctypes.c_void_p()
    for sr, n_mels, n_mfcc, length_ms, q in [(16000, 80, 0, 25.0, 22.0), (16000, 80, 81, 25.0, 22.0), (16000, 80, 40, 25.0, -0.5),
                                             (16000, 0, 0, 25.0, 22.0), (16000, 257, 40, 25.0, 22.0), (0, 80, 40, 25.0, 22.0),
                                             (16000, 80, 40, 0.0, 22.0)]:
        assert lib.ppasr_mfcc_create(sr, n_mels, n_mfcc, length_ms, 10.0, q, ctypes.byref(h)) == _lib.PPASR_EINVAL
        assert not h.value
    assert lib.ppasr_mfcc_create(16000, 80, 40, 25.0, 10.0, 22.0, None) == _lib.PPASR_EINVAL
    with pytest.raises(_lib.PPASRHipError):
        _lib.check(lib.ppasr_mfcc_create(16000, 80, 81, 25.0, 10.0, 22.0, ctypes.byref(h)))
    assert lib.ppasr_fbank_feature_dim(None) == 0


def test_audio_featurizer_accepts_mfcc():
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    f = AudioFeaturizer(feature_method="mfcc")  # the reference's defaults: 80 mel bins, 40 coefficients
    assert f.feature_dim == 40
    assert AudioFeaturizer(feature_method="mfcc", n_mels=23, n_mfcc=13, sample_rate=8000).feature_dim == 13
    assert AudioFeaturizer(feature_method="mfcc", n_mels=40, n_mfcc=40).feature_dim == 40
    # the fbank form does not look at n_mfcc
    assert AudioFeaturizer(feature_method="fbank", n_mels=64, n_mfcc=100).feature_dim == 64
    assert AudioFeaturizer(n_mels=80).feature_dim == 80


def test_audio_featurizer_refuses_more_coefficients_than_mel_bins():
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    with pytest.raises(AssertionError):  # paddleaudio.compliance.kaldi.mfcc asserts n_mfcc <= n_mels
        AudioFeaturizer(feature_method="mfcc", n_mels=40, n_mfcc=41)
    with pytest.raises(AssertionError):
        AudioFeaturizer(feature_method="mfcc", n_mels=80, n_mfcc=0)


def test_linear_is_still_not_built():
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    with pytest.raises(NotImplementedError, match="linear"):
        AudioFeaturizer(feature_method="linear")
    with pytest.raises(NotImplementedError):
        AudioFeaturizer(feature_method="spectrogram")

