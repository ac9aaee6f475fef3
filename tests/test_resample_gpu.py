"""GPU: the device resampler (csrc/resample.hip) behind ``AudioFeaturizer(resample="device")``.
  1. against the float64 oracle (``scipy.signal.resample_poly``) at the a-priori bound of a T-term fp32 dot product;
  2. impulses: every output is the table entry it should pick, bit for bit;
  3. a stream cut into packets, and raw calls on arbitrary windows, equal the whole byte for byte;
  4. the batch form equals single calls;  5. nothing else is written, nothing depends on what the buffers held;
  6. featurize(x, sr) is featurize(resample(x)) exactly;  7. ``featurize_many(sample_rates=...)`` and its launch count;
  8.-10. ``StreamPool`` at foreign rates;  11. ``PPASRPredictor.predict`` with ``resample: device``."""
import ctypes
import io
import wave

import numpy as np
import pytest
import torch

import resample_cases as rc
from ppasr_amd import _lib
from ppasr_amd.utils.synth import conformer_state_dict, synth_vocabulary
from test_predictor_gpu import _audio, _cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(r, rc.MODEL_RATE) for r in rc.RATES] + [(16000, 8000)]
_made = {}


def _featurizer(out_rate=rc.MODEL_RATE, method="fbank", use_db=True, resample="device"):
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    key = (out_rate, method, use_db, resample)
    if key not in _made:
        _made[key] = AudioFeaturizer(feature_method=method, sample_rate=out_rate, use_dB_normalization=use_db, resample=resample)
    return _made[key]


def _wave(seconds, rate, seed):
    """`seconds` of audio at `rate` (the synthetic signal of the predictor tests, read at that rate)"""
    n = int(seconds * rate)
    return _audio(n / 16000.0 + 0.01, seed=seed)[:n]


def _table(in_rate, out_rate):
    g = rc.geometry(in_rate, out_rate)
    t = np.zeros((g["up"], g["taps"]), np.float32)
    assert _lib.load().ppasr_resampler_table(in_rate, out_rate, t.ctypes.data) == _lib.PPASR_OK
    return t, g


def _compute(f, in_rate, x_dev, in_first, n_in, out_dev, out_first, n_out):
    """a raw ppasr_resample_compute call on device tensors"""
    r, _ = f._resampler(in_rate)
    _lib.check(f._lib.ppasr_resample_compute(r, x_dev.data_ptr(), in_first, n_in, out_dev.data_ptr(), out_first, n_out,
                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_rate,out_rate", CASES)
def test_against_float64(in_rate, out_rate):
    """|err[m]| <= (T + 2) 2^-24 S[m] + 2^-24 |y[m]|, S[m] = sum_k |h_k| |x_k|: T roundings of the running sum (each at most
    half an ulp of a partial sum that S bounds), the table's rounding (one more term of 2^-24 S), slack of one, and the
    rounding of the result.  A sequential fp32 emulation sits at 0.09 - 0.26 of it."""
    f = _featurizer(out_rate)
    T = rc.geometry(in_rate, out_rate)["taps"]
    worst = {}
    for n in rc.lengths(in_rate, out_rate)[1:]:
        for name, x in rc.signals(in_rate, out_rate, n, seed=n).items():
            got = f.resample_device(x, in_rate).cpu().numpy()
            want, S = rc.resample64(x, in_rate, out_rate), rc.abs_sum64(x, in_rate, out_rate)
            assert got.dtype == np.float32 and got.shape == want.shape == (rc.out_len(in_rate, out_rate, n),)
            bound = (T + 2) * 2.0 ** -24 * S + 2.0 ** -24 * np.abs(want)
            err = np.abs(got.astype(np.float64) - want)
            ok = bound > 0
            ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert (err <= bound).all(), (n, name, ratio)
    print(f"{in_rate} -> {out_rate}: worst err / bound {worst}")
    assert f.resample_device(np.zeros(0, np.float32), in_rate).shape == (0,)


# ---- 2. impulses ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_rate,out_rate", CASES)
def test_impulses_pick_table_entries(in_rate, out_rate):
    f = _featurizer(out_rate)
    table, g = _table(in_rate, out_rate)
    n = rc.lengths(in_rate, out_rate)[-1]
    n_out = rc.out_len(in_rate, out_rate, n)
    m = np.arange(n_out, dtype=np.int64)
    k = (m + g["n_pre_remove"]) * g["down"]
    q, p = k // g["up"], k % g["up"]
    for i in (0, 1, n // 2 + 3, n - 1):
        x = np.zeros(n, np.float32)
        x[i] = 1.0
        got = f.resample_device(x, in_rate).cpu().numpy()
        t = q - i  # the tap of output m that meets sample i
        hit = (t >= 0) & (t < g["taps"])
        want = np.zeros(n_out, np.float32)
        want[hit] = table[p[hit], t[hit]]
        assert hit.any() and got.tobytes() == want.tobytes(), i  # (also: +0, never -0, away from the impulse)
    # every tap of every phase: output m meets an impulse at i with tap t of phase p where (i + t) up + p = (m +
    # n_pre_remove) down, so `down` consecutive impulse positions (up and down are coprime) meet every (p, t).  Deep inside
    # a stream, by raw calls on the window of outputs that can see the impulse.
    met = np.zeros(table.shape, bool)
    i0 = 5 * g["taps"] * g["down"] // g["up"] + 11
    cnt = (g["taps"] + 2) * g["up"] // g["down"] + 8
    xd = torch.zeros(i0 + g["down"], dtype=torch.float32, device=DEV)
    out = torch.empty(cnt, dtype=torch.float32, device=DEV)
    for i in range(i0, i0 + g["down"]):
        xd.zero_()
        xd[i] = 1.0
        out.fill_(7.0)
        m0 = i * g["up"] // g["down"] - g["n_pre_remove"] - 2
        assert m0 > 0
        _compute(f, in_rate, xd, 0, xd.numel(), out, m0, cnt)
        mm = m0 + np.arange(cnt, dtype=np.int64)
        kk = (mm + g["n_pre_remove"]) * g["down"]
        qq, pp = kk // g["up"], kk % g["up"]
        tt = qq - i
        hit = (tt >= 0) & (tt < g["taps"])
        assert not hit[0] and not hit[-1]  # the window holds every output that sees the impulse
        want = np.zeros(cnt, np.float32)
        want[hit] = table[pp[hit], tt[hit]]
        assert out.cpu().numpy().tobytes() == want.tobytes(), i
        met[pp[hit], tt[hit]] = True
    assert met.all()


# ---- 3. packets equal the whole -------------------------------------------------------------------------------------------
PACKETS = [1, 7, 159, 160, 1000, 3333]


@pytest.mark.parametrize("in_rate,out_rate", CASES)
def test_packets_equal_the_whole(in_rate, out_rate):
    from ppasr_amd.data_utils.featurizer import StreamResampler
    f = _featurizer(out_rate)
    x = rc.signals(in_rate, out_rate, int(0.3 * in_rate), seed=5)["noise"]
    whole = f.resample_device(x, in_rate).cpu().numpy()
    assert whole.size == rc.out_len(in_rate, out_rate, x.size)
    sr = StreamResampler(f, in_rate)
    parts, pos = [], 0
    for k in PACKETS + [x.size]:
        parts.append(sr.push(x[pos:pos + k]))
        assert parts[-1].dtype == np.float32
        pos += k
        assert sum(p.size for p in parts) == _lib.load().ppasr_resampler_ready(in_rate, out_rate, min(pos, x.size))
    assert sum(p.size for p in parts) == _lib.load().ppasr_resampler_ready(in_rate, out_rate, x.size) < whole.size
    parts.append(sr.flush())
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    assert sr.flush().size == 0
    with pytest.raises(ValueError):
        sr.push(x[:10])
    # the tail a stream keeps is bounded by the filter, not by the stream
    g = rc.geometry(in_rate, out_rate)
    assert sr._tail.size <= g["taps"] + g["down"] // g["up"] + 1

    # raw calls on arbitrary windows: any (in_first, out_first) whose window holds the outputs' support
    xd = torch.from_numpy(x).to(DEV)
    rng = np.random.default_rng(11)
    for _ in range(6):
        m0 = int(rng.integers(0, whole.size - 1))
        cnt = int(rng.integers(1, min(700, whole.size - m0) + 1))
        lo = rc.first_needed(in_rate, out_rate, m0)
        hi = min(rc.q_of(in_rate, out_rate, m0 + cnt - 1) + 1, x.size)
        lo = max(0, lo - int(rng.integers(0, 50)))
        hi = min(x.size, hi + int(rng.integers(0, 50)))
        out = torch.full((cnt,), 3.0, dtype=torch.float32, device=DEV)
        _compute(f, in_rate, xd[lo:hi].clone(), lo, hi - lo, out, m0, cnt)
        assert out.cpu().numpy().tobytes() == whole[m0:m0 + cnt].tobytes(), (m0, cnt, lo, hi)
    # a window that holds nothing: zeros; no outputs: nothing
    out = torch.full((16,), 3.0, dtype=torch.float32, device=DEV)
    _compute(f, in_rate, xd, 0, 0, out, 5, 16)
    assert (out == 0).all()
    out.fill_(3.0)
    _compute(f, in_rate, xd, 0, x.size, out, 5, 0)
    assert (out == 3.0).all()


def test_positions_past_2_to_the_31():
    """a stream position where (m + n_pre_remove) * down passes 2^31 (and 2^32): the window around it gives what the same
    samples give at the start of a stream, shifted by whole periods of the phase pattern"""
    in_rate, out_rate = 44100, rc.MODEL_RATE
    f = _featurizer(out_rate)
    g = rc.geometry(in_rate, out_rate)
    x = rc.signals(in_rate, out_rate, 4000, seed=9)["noise"]
    xd = torch.from_numpy(x).to(DEV)
    m0, cnt = 300, 900
    lo = rc.first_needed(in_rate, out_rate, m0)
    near = torch.empty(cnt, dtype=torch.float32, device=DEV)
    _compute(f, in_rate, xd[lo:].clone(), lo, x.size - lo, near, m0, cnt)
    periods = 2 ** 33 // g["down"]  # shifting outputs by periods * up shifts their reads by periods * down exactly
    far = torch.empty(cnt, dtype=torch.float32, device=DEV)
    _compute(f, in_rate, xd[lo:].clone(), lo + periods * g["down"], x.size - lo, far, m0 + periods * g["up"], cnt)
    assert (m0 + periods * g["up"]) * g["down"] > 2 ** 33
    assert far.cpu().numpy().tobytes() == near.cpu().numpy().tobytes()
    assert near.abs().max() > 0.1


# ---- 4. + 5. batch equals single; nothing else is written -----------------------------------------------------------------
GUARD = 8


def _batch(f, in_rate, out_rate, waves, fill_out, fill_stage):
    """six segments in one compute_batch, each output between guard words -> (the whole output buffer, segment table)"""
    n = len(waves)
    outs = [rc.out_len(in_rate, out_rate, w.size) for w in waves]
    total_in = sum(w.size for w in waves) + GUARD * (n + 1)
    stage = torch.full((total_in,), fill_stage, dtype=torch.float32, device=DEV)
    out = torch.full((sum(outs) + GUARD * (n + 1),), fill_out, dtype=torch.float32, device=DEV)
    table = (_lib.ResampleSegment * n)()
    at_in = at_out = GUARD
    for b, w in enumerate(waves):
        stage[at_in:at_in + w.size] = torch.from_numpy(w).to(DEV)
        table[b] = _lib.ResampleSegment(at_in, 0, w.size, at_out, 0, outs[b])
        at_in += w.size + GUARD
        at_out += outs[b] + GUARD
    tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    r, _ = f._resampler(in_rate)
    _lib.check(f._lib.ppasr_resample_compute_batch(r, stage.data_ptr(), tab.data_ptr(), n, max(outs), out.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy(), table, outs, stage.cpu().numpy()


@pytest.mark.parametrize("in_rate,out_rate", CASES)
def test_batch_equals_single_and_writes_nothing_else(in_rate, out_rate):
    f = _featurizer(out_rate)
    ns = rc.lengths(in_rate, out_rate)
    ns = [ns[0], ns[1], ns[2], ns[4], ns[5], ns[-1]]  # six segments, the empty one among them
    waves = [rc.signals(in_rate, out_rate, n, seed=40 + b)["noise"] for b, n in enumerate(ns)]
    nan_bits = np.float32(np.nan)
    got_a, table, outs, stage_a = _batch(f, in_rate, out_rate, waves, 1234.5, -77.0)
    got_b, _, _, _ = _batch(f, in_rate, out_rate, waves, float(nan_bits), 1e30)
    at = GUARD
    last = got_a[got_a.size - GUARD - outs[-1]:got_a.size - GUARD].copy()
    assert (got_a[:GUARD] == 1234.5).all() and np.isnan(got_b[:GUARD]).all()
    for b, w in enumerate(waves):
        single = f.resample_device(w, in_rate).cpu().numpy()
        assert single.size == outs[b]
        assert got_a[at:at + outs[b]].tobytes() == single.tobytes(), b
        assert got_b[at:at + outs[b]].tobytes() == single.tobytes(), b  # whatever the buffers held
        at += outs[b]
        assert (got_a[at:at + GUARD] == 1234.5).all() and np.isnan(got_b[at:at + GUARD]).all(), b  # the guard words
        at += GUARD
    assert at == got_a.size
    # the input side is read only
    at = 0
    for w in waves:
        assert (stage_a[at:at + GUARD] == -77.0).all()
        assert stage_a[at + GUARD:at + GUARD + w.size].tobytes() == w.tobytes()
        at += GUARD + w.size
    # single call between guard words
    x = torch.from_numpy(waves[-1]).to(DEV)
    out = torch.full((outs[-1] + 2 * GUARD,), -5.0, dtype=torch.float32, device=DEV)
    _compute(f, in_rate, x, 0, x.numel(), out[GUARD:], 0, outs[-1])
    o = out.cpu().numpy()
    assert (o[:GUARD] == -5.0).all() and (o[-GUARD:] == -5.0).all()
    assert o[GUARD:-GUARD].tobytes() == last.tobytes()


# ---- 6. composition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["fbank", "mfcc"])
@pytest.mark.parametrize("in_rate", [8000, 44100])
def test_featurize_is_featurize_of_resampled(method, in_rate):
    f = _featurizer(method=method)
    x = _wave(0.5, in_rate, seed=3)
    a = f.featurize_device(x, in_rate)
    gain_a = f.last_gain
    y = f.resample_device(x, in_rate).cpu()
    b = f.featurize_device(y, rc.MODEL_RATE)
    assert a.shape == b.shape and a.shape[0] >= 40 and a.shape[1] == f.feature_dim
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert gain_a == f.last_gain
    assert f.featurize(x, in_rate).tobytes() == a.cpu().numpy().tobytes()
    # the host route still answers, and differs only by the resampler's fp32 rounding
    h = _featurizer(method=method, resample="host").featurize(x, in_rate)
    assert h.shape == tuple(a.shape)


def test_unsupported_ratio_raises_from_the_library():
    f = _featurizer()
    with pytest.raises(_lib.PPASRHipError) as e:
        f.resample_device(np.zeros(100, np.float32), 16001)
    assert e.value.status == _lib.PPASR_EUNSUPPORTED
    with pytest.raises(_lib.PPASRHipError):
        f.featurize_many([np.zeros(100, np.float32)], sample_rates=[16001])
    with pytest.raises(ValueError, match='resample="device"'):
        _featurizer(resample="host").resample_device(np.zeros(100, np.float32), 8000)


# ---- 7. featurize_many ----------------------------------------------------------------------------------------------------
MANY_RATES = [8000, 16000, 48000, 8000, 44100]


@pytest.mark.parametrize("use_db,launches", [(True, 3), (False, 1)])
@pytest.mark.parametrize("padded", [False, True])
def test_featurize_many_mixed_rates(use_db, launches, padded):
    f = _featurizer(use_db=use_db)
    waves = [_wave(0.31 + 0.05 * b, r, seed=60 + b) for b, r in enumerate(MANY_RATES)]
    own = [f.featurize_device(w, r).cpu().numpy() for w, r in zip(waves, MANY_RATES)]
    gains = []
    if use_db:
        for w, r in zip(waves, MANY_RATES):
            f.featurize_device(w, r)
            gains.append(np.float32(f.last_gain))
    feats, counts = f.featurize_many(waves, padded=padded, sample_rates=MANY_RATES)  # (handles, buffers)
    torch.cuda.synchronize()
    with _lib.kernel_profile() as kp:
        feats, counts = f.featurize_many(waves, padded=padded, sample_rates=MANY_RATES)
        torch.cuda.synchronize()
    fb = {k: c for k, c in kp.kernels.items() if "resample" not in k}
    rs = {k: c for k, c in kp.kernels.items() if "resample" in k}
    # the fbank's usual launches + one batched resample launch per distinct foreign rate (8 k, 44.1 k, 48 k)
    assert sum(c for _, c in fb.values()) == launches and len(fb) == launches, kp.kernels
    assert sum(c for _, c in rs.values()) == 3 and all("batch" in k for k in rs), kp.kernels
    feats = feats.cpu().numpy()
    row = 0
    for b, o in enumerate(own):
        assert int(counts[b]) == o.shape[0] > 0
        got = feats[b, :o.shape[0]] if padded else feats[row:row + o.shape[0]]
        assert got.tobytes() == o.tobytes(), b
        if padded:
            assert (feats[b, o.shape[0]:] == 0).all()
        row += o.shape[0]
    if use_db:
        assert np.array_equal(f.last_gains, np.array(gains, np.float32))
    # all rates native: the usual count, no resample launch; a scalar rate; None
    native = [w for w, r in zip(waves, MANY_RATES) if r == 16000] + [_audio(0.4, seed=2)]
    want, want_counts = f.featurize_many(native, padded=padded)
    for rates in ([16000, 16000], 16000, None):
        with _lib.kernel_profile() as kp:
            got, got_counts = f.featurize_many(native, padded=padded, sample_rates=rates)
            torch.cuda.synchronize()
        assert sum(c for _, c in kp.kernels.values()) == launches and not any("resample" in k for k in kp.kernels), kp.kernels
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        assert np.array_equal(np.asarray(got_counts), np.asarray(want_counts))
    # one foreign rate for all
    f8, c8 = f.featurize_many([waves[0], waves[3]], sample_rates=8000)
    assert f8.cpu().numpy().tobytes() == np.concatenate([own[0], own[3]]).tobytes()


# ---- 8. - 10. the pool ----------------------------------------------------------------------------------------------------
V = 97
N = 4
POOL_PACKETS = [50, 800, 50, 1200, 50, 2500, 50, 5120]  # samples at 8 kHz; the 50-sample packets often complete no frame


@pytest.fixture(scope="module")
def model():
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    cfg = _cfg(L=1)
    return ConformerModel(80, V, streaming=True, encoder_conf=cfg["encoder_conf"],
                          state_dict=conformer_state_dict(vocab_size=V, num_blocks=1, seed=3), device=DEV)


def _pool(model, resample="device", **kw):
    from ppasr_amd.serving import StreamPool
    conf = dict(_cfg()["preprocess_conf"])
    if resample is not None:
        conf["resample"] = resample
    return StreamPool(model, synth_vocabulary(V), n_sessions=N, preprocess_conf=conf, **kw)


def _stream(s, rate, seconds=1.5):
    return _wave(seconds + 0.017 * s, rate, seed=80 + s)


def _rounds(rates):
    """-> [{session: packet}, ...] of float samples at rates[session]"""
    rounds = []
    for s, rate in enumerate(rates):
        w = _stream(s, rate)
        pos = r = 0
        while pos < w.size:
            part = w[pos:pos + POOL_PACKETS[(s + r) % len(POOL_PACKETS)] * rate // 8000]
            pos += part.size
            if len(rounds) <= r:
                rounds.append({})
            rounds[r][s] = part
            r += 1
    return rounds


def _host(feat):
    return None if feat is None else (feat.cpu().numpy() if isinstance(feat, torch.Tensor) else feat)


def _same_state(a, b, where):
    for s, (x, y) in enumerate(zip(a.sessions, b.sessions)):
        assert (x.remained_wav is None) == (y.remained_wav is None), (where, s)
        if x.remained_wav is not None:
            assert x.remained_wav.dtype == y.remained_wav.dtype == np.float32
            assert x.remained_wav.tobytes() == y.remained_wav.tobytes(), (where, s)
        fx, fy = _host(x.cached_feat), _host(y.cached_feat)
        assert (fx is None) == (fy is None), (where, s)
        if fx is not None:
            assert fx.shape == fy.shape and fx.tobytes() == fy.tobytes(), (where, s)


def test_pool_at_8k_equals_pool_fed_resampled(model):
    """pool A takes 8 kHz packets; pool B (no resample option at all) takes, packet for packet, what a StreamResampler
    made of them"""
    from ppasr_amd.data_utils.featurizer import StreamResampler
    a, b = _pool(model), _pool(model, resample=None)
    f = _featurizer()
    rs = [StreamResampler(f, 8000) for _ in range(N)]
    for r, packets in enumerate(_rounds([8000] * N)):
        for s, p in packets.items():
            a.feed(s, p, sample_rate=8000)
            b.feed(s, rs[s].push(p))
        _same_state(a, b, ("fed", r))
        ua, ub = a.step(), b.step()
        assert ua == ub, r
        _same_state(a, b, ("stepped", r))
    for s in range(N):
        rest = rs[s].flush()
        assert rest.size > 0
        b.feed(s, rest)
        got_a, got_b = a.finish(s), b.finish(s)
        assert got_a is not None and got_a == got_b, (s, got_a, got_b)
        assert a.sessions[s].frame_ids == b.sessions[s].frame_ids and len(a.sessions[s].frame_ids) >= 16, s
    _same_state(a, b, "finished")
    # reset drops the session's resampler and its rate
    a.reset(0)
    assert a.sessions[0].resampler is None and a.sessions[0].sample_rate is None
    a.feed(0, _stream(0, 16000)[:1600])  # the featurizer's rate now


def test_feed_equals_feed_many_on_mixed_rates(model):
    rates = [8000, 16000, 44100, 8000]
    a, b = _pool(model), _pool(model)
    for r, packets in enumerate(_rounds(rates)):
        for s, p in packets.items():
            a.feed(s, p, sample_rate=rates[s])
        if r % 2 == 0:
            b.feed_many(packets, sample_rate={s: rates[s] for s in packets if rates[s] != 16000})
        else:
            b.feed_many(packets, sample_rate=dict(enumerate(rates)))
        _same_state(a, b, ("fed", r))
        ua, ub = a.step(), b.step()
        assert ua == ub, r
        _same_state(a, b, ("stepped", r))
    for s in range(N):
        got_a, got_b = a.finish(s), b.finish(s)
        assert got_a is not None and got_a == got_b, (s, got_a, got_b)
        assert a.sessions[s].frame_ids == b.sessions[s].frame_ids, s
    _same_state(a, b, "finished")
    # one rate for all packets, one batched resample launch for them
    c = _pool(model)
    first = {s: _stream(s, 8000)[:4000] for s in range(N)}
    c.feed_many(first, sample_rate=8000)
    with _lib.kernel_profile() as kp:
        c.feed_many({s: _stream(s, 8000)[4000:8000] for s in range(N)}, sample_rate=8000)
        torch.cuda.synchronize()
    rs = {k: v for k, v in kp.kernels.items() if "resample" in k}
    assert sum(v[1] for v in rs.values()) == 1 and all("batch" in k for k in rs), kp.kernels


def _snapshot(pool):
    return [(None if s.remained_wav is None else s.remained_wav.tobytes(),
             None if s.cached_feat is None else _host(s.cached_feat).tobytes(), s.sample_rate, s.resampler,
             None if s.resampler is None else (s.resampler._tail.tobytes(), s.resampler._n_in, s.resampler._n_out))
            for s in pool.sessions]


def test_rate_change_and_missing_option_touch_nothing(model):
    a = _pool(model)
    p8, p16 = _stream(0, 8000)[:4000], _stream(1, 16000)[:8000]
    a.feed(0, p8, sample_rate=8000)
    a.feed(1, p16)
    before = _snapshot(a)
    with pytest.raises(ValueError, match="fixed by its first packet"):
        a.feed(0, p8, sample_rate=16000)
    with pytest.raises(ValueError, match="fixed by its first packet"):
        a.feed(0, p8)  # (None = the featurizer's rate)
    with pytest.raises(ValueError, match="fixed by its first packet"):
        a.feed(1, p16, sample_rate=8000)
    with pytest.raises(ValueError, match="fixed by its first packet"):
        a.feed_many({2: p8, 0: p8, 3: p16}, sample_rate={2: 8000, 0: 44100})
    with pytest.raises(_lib.PPASRHipError):  # the library's refusal, before any session changes
        a.feed_many({2: p8, 3: p16}, sample_rate={2: 16001})
    with pytest.raises(ValueError):  # a refused gain after the resampling: the resamplers keep their state
        a.feed_many({0: p8, 2: np.full(4000, 1e-20, np.float32)}, sample_rate=8000)
    assert _snapshot(a) == before
    h = _pool(model, resample="host")
    n = _pool(model, resample=None)
    for pool in (h, n):
        before = _snapshot(pool)
        with pytest.raises(ValueError, match='resample="device"'):
            pool.feed(0, p8, sample_rate=8000)
        with pytest.raises(ValueError, match='resample="device"'):
            pool.feed_many({0: p16, 1: p8}, sample_rate={1: 8000})
        assert _snapshot(pool) == before
        pool.feed(0, p16, sample_rate=16000)  # the featurizer's own rate needs no option


# ---- 11. predict ----------------------------------------------------------------------------------------------------------
def _wav_bytes(x, rate):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype(np.int16).tobytes())
    return buf.getvalue()


def test_predict_with_resample_device():
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer, load_audio, resample
    from ppasr_amd.predict import PPASRPredictor
    Vp = 300
    sd = conformer_state_dict(vocab_size=Vp, num_blocks=2, seed=3)
    data = _wav_bytes(_wave(1.2, 48000, seed=4), 48000)
    cfg_dev = _cfg()
    cfg_dev["preprocess_conf"]["resample"] = "device"
    p_dev = PPASRPredictor(configs=cfg_dev, state_dict=sd, vocab_list=synth_vocabulary(Vp), warmup=False)
    p_def = PPASRPredictor(configs=_cfg(), state_dict=sd, vocab_list=synth_vocabulary(Vp), warmup=False)
    assert p_dev._audio_featurizer.resample_mode == "device" and p_def._audio_featurizer.resample_mode == "host"
    got = p_dev.predict(data)
    assert isinstance(got["text"], str) and set(got) == {"text", "score"}
    # the default: the host route's features, byte for byte what the parent computes -- scipy in float64, then the fbank
    samples, sr = load_audio(data)
    assert sr == 48000
    want = AudioFeaturizer(**_cfg()["preprocess_conf"]).featurize(resample(samples, 48000, 16000), 16000)
    assert p_def._audio_featurizer.featurize(samples, sr).tobytes() == want.tobytes()
    ref = p_def.predict(data)
    assert ref == p_def.predict(data)
    # the two routes differ by fp32 rounding of the resampler only: same frames, nearly the same features
    fd = p_dev._audio_featurizer.featurize(samples, sr)
    assert fd.shape == want.shape and float(np.abs(fd - want).max()) < 0.5
    # ... and what predict returns is what it returns for the device-resampled samples at the model's rate
    y = p_dev._audio_featurizer.resample_device(samples, sr).cpu().numpy()
    assert y.size == samples.size // 3 and p_dev.predict(y, sample_rate=16000) == got
    # predict_long goes through predict
    assert p_dev.predict_long(data, speech_timestamps=[{"start": 0, "end": samples.size}])["text"] == got["text"]
