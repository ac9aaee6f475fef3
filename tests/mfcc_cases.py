"""Helper of the MFCC tests (not a test): the float64 statement of the stage ``feature_method='mfcc'`` adds to the fbank
front-end -- Kaldi's MFCC with use_energy False, subtract_mean False, cepstral_lifter 22, what
``paddleaudio.compliance.kaldi.mfcc`` computes at the arguments ``audio_featurizer.py:109-115`` gives it -- and the two
error budgets the GPU tests hold csrc/fbank.hip to.  paddleaudio is not installable offline and the shim's ``mfcc`` is a
stub, so the path is parity unpinned like the fbank: the reference here is the published algorithm, in float64.

  D[m][0] = sqrt(1/M)      D[m][k] = sqrt(2/M) cos(pi/M (m + 1/2) k)      L[k] = 1 + (Q/2) sin(pi k / Q)  (1 when Q == 0)
  mfcc[t][k] = L[k] * sum_m logmel[t][m] D[m][k]
"""
import functools

import numpy as np

from oracle import fbank_oracle

LIFTER = 22.0
U = 2.0 ** -24  # unit roundoff of float32


def dct_matrix(n_mels, n_mfcc):
    m = np.arange(n_mels, dtype=np.float64)[:, None]
    k = np.arange(n_mfcc, dtype=np.float64)[None, :]
    d = np.sqrt(2.0 / n_mels) * np.cos(np.pi / n_mels * (m + 0.5) * k)
    d[:, 0] = np.sqrt(1.0 / n_mels)
    return d


def lifter(n_mfcc, q=LIFTER):
    k = np.arange(n_mfcc, dtype=np.float64)
    return 1.0 + 0.5 * q * np.sin(np.pi * k / q) if q > 0 else np.ones(n_mfcc)


@functools.lru_cache(maxsize=None)
def _fbank_ref(key, sr, n_mels, use_db):
    return fbank_oracle.featurize(np.frombuffer(key, np.float32), sr, n_mels, use_db, -20.0)


def fbank_ref(wav, sr, n_mels, use_db):
    """oracle/fbank_oracle.py on `wav`, float64 [T, n_mels]; computed once per (waveform, bank) and not to be modified"""
    return _fbank_ref(np.ascontiguousarray(wav, np.float32).tobytes(), sr, n_mels, bool(use_db))


def mfcc_oracle(wav, sr, n_mels, n_mfcc, use_db):
    """float64 [T, n_mfcc]: the sum over the mel axis is formed first, then multiplied by L[k]"""
    return (fbank_ref(wav, sr, n_mels, use_db) @ dct_matrix(n_mels, n_mfcc)) * lifter(n_mfcc)


def end_to_end_tol(ref_fbank, n_mfcc):
    """Budget of the whole front-end against float64: the project's fbank budget (tests/test_fbank_gpu.py: 2e-4 + 4e-5
    exp((rowmax - ref) / 2) per log-mel value) pushed through the linear map, plus the fp32 contraction (M fused
    multiply-adds on a table entry rounded once, one multiply by a lifter rounded once: (M + 2) u relative to the sum of
    magnitudes).  Derived, not measured.  L[k] is negative for 22 < k < 44 (40 coefficients reach k = 39), so the budget
    carries |L[k]|."""
    m = ref_fbank.shape[1]
    d, l = np.abs(dct_matrix(m, n_mfcc)), np.abs(lifter(n_mfcc))
    tol_fbank = 2e-4 + 4e-5 * np.exp(0.5 * (ref_fbank.max(axis=1, keepdims=True) - ref_fbank))
    return l * (tol_fbank @ d + (m + 2) * U * (np.abs(ref_fbank) @ d))


def stage_tol(fbank_gpu, n_mfcc):
    """Budget of the new stage alone, against (float64(fbank_gpu) @ D) * L on the fbank form's own output: fp32 products of
    fp32-rounded table entries, M accumulations in any order, the lifter's rounding and its multiply: (M + 3) u."""
    m = fbank_gpu.shape[1]
    d, l = np.abs(dct_matrix(m, n_mfcc)), np.abs(lifter(n_mfcc))
    return (m + 3) * U * l * (np.abs(fbank_gpu.astype(np.float64)) @ d)


def audio(seconds, seed=0, sr=16000):
    """`_audio` of tests/test_fbank_gpu.py"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(int(sr * seconds)) / sr
    x = 0.2 * np.sin(2 * np.pi * 180 * t) * (1 + 0.5 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * rng.standard_normal(t.shape)
    x += 0.1 * np.sin(2 * np.pi * (500 + 800 * t) * t)
    return x.astype(np.float32)
