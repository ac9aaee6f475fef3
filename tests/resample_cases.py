"""Cases and the float64 statement of the device resampler (csrc/resample.hip), shared by tests/test_resample_cpu.py and
tests/test_resample_gpu.py.  The oracle is what the host route has always computed: ``scipy.signal.resample_poly(x, up,
down, window=("kaiser", BETA))`` -- its filter design restated here step by step so that the table layout, the geometry and
the stream helpers can be checked against integer definitions."""
from math import gcd

import numpy as np

BETA = 14.769656459379492
TILE = 256  # PPASR_RESAMPLE_TILE: outputs per workgroup
MODEL_RATE = 16000
# -> 16 000: upsampling with T = 21; up = 1 and the longest rows; large up and down; the largest table
RATES = [8000, 48000, 44100, 11025]
ALL_RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000]
TAPS = {8000: 21, 11025: 21, 22050: 29, 24000: 32, 32000: 43, 44100: 58, 48000: 64}


def geometry(in_rate, out_rate):
    g = gcd(in_rate, out_rate)
    up, down = out_rate // g, in_rate // g
    half_len = 10 * max(up, down)
    L = 2 * half_len + 1
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    taps = -(-(L + n_pre_pad) // up)
    return dict(up=up, down=down, half_len=half_len, L=L, n_pre_pad=n_pre_pad, n_pre_remove=n_pre_remove, taps=taps)


def fir(in_rate, out_rate):
    """h = up * firwin(L, 1 / max(up, down), kaiser BETA), float64"""
    from scipy.signal import firwin
    g = geometry(in_rate, out_rate)
    return g["up"] * firwin(g["L"], 1.0 / max(g["up"], g["down"]), window=("kaiser", BETA))


def table64(in_rate, out_rate):
    """[up][taps] float64: table[p][t] = hp[p + t up], hp = [0] * n_pre_pad + h, zero past hp's end; and the mask of the
    entries that come from h"""
    g = geometry(in_rate, out_rate)
    hp = np.concatenate([np.zeros(g["n_pre_pad"]), fir(in_rate, out_rate)])
    flat = np.zeros(g["up"] * g["taps"])
    real = np.zeros(g["up"] * g["taps"], bool)
    idx = np.arange(g["up"])[:, None] + np.arange(g["taps"])[None, :] * g["up"]  # p + t up
    ok = idx < len(hp)
    flat.reshape(g["up"], g["taps"])[ok] = hp[idx[ok]]
    real.reshape(g["up"], g["taps"])[ok] = idx[ok] >= g["n_pre_pad"]
    return flat.reshape(g["up"], g["taps"]), real.reshape(g["up"], g["taps"])


def out_len(in_rate, out_rate, n_in):
    g = geometry(in_rate, out_rate)
    return -(-n_in * g["up"] // g["down"])


def q_of(in_rate, out_rate, m):
    """the highest sample index output m reads"""
    g = geometry(in_rate, out_rate)
    return (m + g["n_pre_remove"]) * g["down"] // g["up"]


def ready(in_rate, out_rate, n_in_total):
    """leading outputs whose reads all lie below n_in_total, by counting (small n only)"""
    m = 0
    while q_of(in_rate, out_rate, m) < n_in_total:
        m += 1
    return m


def first_needed(in_rate, out_rate, m):
    return max(0, q_of(in_rate, out_rate, m) - (geometry(in_rate, out_rate)["taps"] - 1))


def resample64(x, in_rate, out_rate):
    """float64 oracle of the float32 samples x"""
    from scipy.signal import resample_poly
    g = geometry(in_rate, out_rate)
    x = np.asarray(x, np.float32).astype(np.float64)
    if x.size == 0:
        return np.zeros(0)
    return resample_poly(x, g["up"], g["down"], window=("kaiser", BETA))


def abs_sum64(x, in_rate, out_rate):
    """S[m] = sum_k |h_k| |x_k| over output m's taps: the scale of a T-term dot product's rounding error"""
    from scipy.signal import resample_poly
    g = geometry(in_rate, out_rate)
    x = np.abs(np.asarray(x, np.float32).astype(np.float64))
    if x.size == 0:
        return np.zeros(0)
    return resample_poly(x, g["up"], g["down"], window=np.abs(fir(in_rate, out_rate)) / g["up"])


def lengths(in_rate, out_rate=MODEL_RATE):
    """input lengths: 0, 1, fewer than T samples, one tile of outputs - 1 / exactly / + 1, three tiles and an odd rest"""
    g = geometry(in_rate, out_rate)

    def n_for(n_out):  # the smallest input length with out_len >= n_out (an upsampler skips some output lengths)
        n = n_out * g["down"] // g["up"]
        while out_len(in_rate, out_rate, n) < n_out:
            n += 1
        while n > 0 and out_len(in_rate, out_rate, n - 1) >= n_out:
            n -= 1
        return n
    around = sorted({n_for(TILE - 1), n_for(TILE), n_for(TILE + 1), n_for(TILE + 1) + 1})
    return [0, 1, g["taps"] - 4] + around + [n_for(3 * TILE + 77)]


def signals(in_rate, out_rate, n, seed):
    """uniform noise, a full-scale sine at 0.45 x the lower Nyquist, a constant 1.0"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f = 0.45 * 0.5 * min(in_rate, out_rate)
    return {"noise": rng.uniform(-1.0, 1.0, n).astype(np.float32),
            "sine": np.sin(2.0 * np.pi * f * t / in_rate).astype(np.float32),
            "ones": np.ones(n, np.float32)}
