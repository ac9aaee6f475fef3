"""GPU: the MFCC form of the front-end (``AudioFeaturizer(feature_method='mfcc')`` -> ``ppasr_mfcc_create``, the kMfcc form of
the frame kernels of csrc/fbank.hip) -- against the float64 statement of Kaldi's MFCC end to end, against the fbank form's
own output for the added stage alone, at the edges of its thread mapping and its output rows, batch against single byte
for byte, and through PPASRPredictor / StreamPool.  Budgets: tests/mfcc_cases.py (derived there, not measured).  Parity
unpinned: paddleaudio is not importable offline and the shim's ``mfcc`` is a stub."""
import ctypes

import numpy as np
import pytest
import torch

import mfcc_cases as mc
from mfcc_cases import audio as _audio  # (`_audio` of tests/test_fbank_gpu.py, copied there)
from ppasr_amd.utils.synth import conformer_state_dict, synth_vocabulary

pytestmark = pytest.mark.gpu


def _featurizer(method, n_mels=80, n_mfcc=40, sr=16000, use_db=True):
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    return AudioFeaturizer(feature_method=method, n_mels=n_mels, n_mfcc=n_mfcc, sample_rate=sr, use_dB_normalization=use_db,
                           target_dB=-20)


# ---- 1. against float64, end to end ----------------------------------------------------------------------------------------
# (seconds, n_mels, n_mfcc, sr, use_db); none has an empty mel filter (an empty filter sits at the log floor, where the fbank
# budget is huge and the comparison shows nothing: 128 mels at 16 kHz does not belong here)
#
# max err / tol measured on an MI355X, in the order of the list: 0.0068, 0.0060, 0.0375, 0.0216, 0.0011, 0.0068, 0.0075, 0.0694,
# 0.0068 (NOTES.md section 26 has the table)
END_TO_END = [(2.0, 80, 40, 16000, True), (2.0, 80, 40, 16000, False), (10.0, 80, 40, 16000, True), (0.5123, 80, 40, 16000, True),
              (0.0251, 80, 40, 16000, True), (2.0, 80, 13, 16000, True), (2.0, 40, 40, 16000, True), (2.0, 23, 13, 8000, True),
              (2.0, 80, 1, 16000, True)]


@pytest.mark.parametrize("seconds,n_mels,n_mfcc,sr,use_db", END_TO_END,
                         ids=[f"{s}-{m}x{k}-{sr // 1000}k-{'db' if db else 'nodb'}" for s, m, k, sr, db in END_TO_END])
def test_mfcc_matches_float64(seconds, n_mels, n_mfcc, sr, use_db):
    wav = _audio(seconds, seed=int(seconds * 10), sr=sr)
    got = _featurizer("mfcc", n_mels, n_mfcc, sr, use_db).featurize(wav, sr)
    ref_fbank = mc.fbank_ref(wav, sr, n_mels, use_db)
    ref = mc.mfcc_oracle(wav, sr, n_mels, n_mfcc, use_db)
    assert got.dtype == np.float32 and got.shape == ref.shape == (1 + (len(wav) - sr // 40) // (sr // 100), n_mfcc)
    assert ref_fbank.min() > np.log(mc.fbank_oracle.EPS) + 1.0  # no filter at the floor
    err = np.abs(got.astype(np.float64) - ref)
    tol = mc.end_to_end_tol(ref_fbank, n_mfcc)
    print("max abs err", float(err.max()), "max err / tol", float((err / tol).max()))
    assert (err <= tol).all()


# ---- 2. the new stage alone, tight -----------------------------------------------------------------------------------------
# where the thread mapping can go wrong: fewer coefficients than a wave, one more mel bin than a wave and as many
# coefficients as a wave / one more, two full waves, the whole workgroup, one coefficient of 256 bins; 8 kHz: the 256-point FFT
STAGE = [(80, 40, 16000), (65, 64, 16000), (65, 65, 16000), (128, 128, 16000), (256, 256, 16000), (256, 1, 16000), (23, 13, 8000)]


@pytest.mark.parametrize("n_mels,n_mfcc,sr", STAGE, ids=[f"{m}x{k}-{sr // 1000}k" for m, k, sr in STAGE])
def test_stage_on_the_fbank_forms_own_output(n_mels, n_mfcc, sr):
    wav = _audio(1.0, seed=5, sr=sr)
    fbank = _featurizer("fbank", n_mels, n_mfcc, sr).featurize(wav, sr)
    got = _featurizer("mfcc", n_mels, n_mfcc, sr).featurize(wav, sr)
    assert got.shape == (fbank.shape[0], n_mfcc) and fbank.shape[1] == n_mels
    want = (fbank.astype(np.float64) @ mc.dct_matrix(n_mels, n_mfcc)) * mc.lifter(n_mfcc)
    err = np.abs(got.astype(np.float64) - want)
    tol = mc.stage_tol(fbank, n_mfcc)
    print("max abs err", float(err.max()), "max err / tol", float((err / tol).max()))
    assert (err <= tol).all()


# ---- 3. edges --------------------------------------------------------------------------------------------------------------
def test_shorter_than_one_window_and_silence():
    f = _featurizer("mfcc")
    out = f.featurize(np.zeros(399, np.float32))
    assert out.shape == (0, 40) and out.dtype == np.float32
    assert f.featurize_device(np.zeros(0, np.float32)).shape == (0, 40)
    z = f.featurize(np.zeros(16000, np.float32)).astype(np.float64)  # silence: every log-mel value at the floor
    assert z.shape == (98, 40)
    floor = np.full((98, 80), np.log(np.finfo(np.float32).eps), np.float32)
    tol = mc.stage_tol(floor, 40)
    want = np.zeros((98, 40))
    want[:, 0] = np.log(float(np.finfo(np.float32).eps)) * np.sqrt(80.0)  # L[0] sum_m floor sqrt(1/M); the cosines sum to 0
    print("max err / tol", float((np.abs(z - want) / tol).max()))
    assert (np.abs(z - want) <= tol).all()


SENTINEL = 12345.678


def _raw_handle(n_mels, n_mfcc, sr=16000):
    from ppasr_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.ppasr_mfcc_create(sr, n_mels, n_mfcc, 25.0, 10.0, mc.LIFTER, ctypes.byref(h)))
    assert lib.ppasr_fbank_feature_dim(h) == n_mfcc
    return lib, h


def _raw_single(lib, h, x, n_mfcc, tail, out_fill, ws_fill, use_db=1):
    """ppasr_fbank_compute on an MFCC handle into an output of frames * n_mfcc + tail floats pre-filled with out_fill"""
    from ppasr_amd import _lib
    n = int(x.numel())
    frames = int(lib.ppasr_fbank_frames(h, n))
    out = torch.full((frames * n_mfcc + tail,), out_fill, dtype=torch.float32, device="cuda:0")
    ws = torch.full((int(lib.ppasr_fbank_workspace_bytes(h, n)),), ws_fill, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.ppasr_fbank_compute(h, x.data_ptr(), n, use_db, -20.0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return frames, out


def _raw_batch(lib, h, wavs, n_mfcc, tail, out_fill, ws_fill, use_db=1):
    from ppasr_amd import _lib
    n = len(wavs)
    counts = (ctypes.c_int * n)(*[int(w.size) for w in wavs])
    table = (_lib.FbankSegment * n)()
    chunks, frames = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.ppasr_fbank_plan_batch(16000, 25.0, 10.0, ctypes.addressof(counts), n, 0, ctypes.addressof(table),
                                          ctypes.byref(chunks), ctypes.byref(frames)))
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to("cuda:0")
    x = torch.from_numpy(np.concatenate(wavs)).to("cuda:0")
    out = torch.full((frames.value * n_mfcc + tail,), out_fill, dtype=torch.float32, device="cuda:0")
    ws = torch.full((int(lib.ppasr_fbank_batch_workspace_bytes(n, chunks.value)),), ws_fill, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.ppasr_fbank_compute_batch(h, x.data_ptr(), table_dev.data_ptr(), n, chunks.value, frames.value, use_db, -20.0,
                                             out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return frames.value, out


@pytest.mark.parametrize("n_mels,n_mfcc", [(80, 40), (80, 1), (256, 13)])
def test_rows_are_n_mfcc_floats_and_nothing_else_is_written(n_mels, n_mfcc):
    """Through the raw C calls, n_mels spare floats behind the last row: a kernel that strides its rows by n_mels leaves
    early rows unwritten and runs over the end; one that stores n_mels values per row writes into the tail."""
    lib, h = _raw_handle(n_mels, n_mfcc)
    try:
        wav = _audio(0.5, seed=9)
        x = torch.from_numpy(wav).to("cuda:0")
        frames, out = _raw_single(lib, h, x, n_mfcc, n_mels, SENTINEL, 0xFF)
        assert frames == 48
        body, tail = out[:frames * n_mfcc], out[frames * n_mfcc:]
        assert bool((body != SENTINEL).all()) and bool(torch.isfinite(body).all())
        assert tail.numel() == n_mels and bool((tail == SENTINEL).all())
        # the same rows from the featurizer (which allocates exactly frames * n_mfcc floats)
        ref = _featurizer("mfcc", n_mels, n_mfcc).featurize_device(wav)
        assert torch.equal(body.view(frames, n_mfcc), ref)
        # batch kernel: three segments, compact rows
        wavs = [wav[:3000], wav[100:501], wav[:8000]]
        total, out_b = _raw_batch(lib, h, wavs, n_mfcc, n_mels, SENTINEL, 0xFF)
        assert total == 17 + 1 + 48
        body, tail = out_b[:total * n_mfcc], out_b[total * n_mfcc:]
        assert bool((body != SENTINEL).all()) and bool(torch.isfinite(body).all())
        assert tail.numel() == n_mels and bool((tail == SENTINEL).all())
    finally:
        lib.ppasr_fbank_destroy(h)


@pytest.mark.parametrize("use_db", [1, 0], ids=["db", "nodb"])
def test_result_does_not_depend_on_what_the_buffers_held(use_db):
    lib, h = _raw_handle(80, 40)
    try:
        wav = _audio(1.3, seed=13)
        x = torch.from_numpy(wav).to("cuda:0")
        _, a = _raw_single(lib, h, x, 40, 0, float("nan"), 0xFF, use_db)
        _, b = _raw_single(lib, h, x, 40, 0, 1.0e30, 0x7F, use_db)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert bool(torch.isfinite(a).all())
        wavs = [wav[:8193], wav[:401], wav[3:16388]]
        _, a = _raw_batch(lib, h, wavs, 40, 0, float("nan"), 0xFF, use_db)
        _, b = _raw_batch(lib, h, wavs, 40, 0, 1.0e30, 0x7F, use_db)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert bool(torch.isfinite(a).all())
    finally:
        lib.ppasr_fbank_destroy(h)


# ---- 4. batch equals single, byte for byte ---------------------------------------------------------------------------------
WIN = 400
LENS = [0, WIN - 1, WIN, 8191, 8192, 8193, 16385, 16003]


@pytest.mark.parametrize("use_db", [True, False], ids=["db", "nodb"])
def test_featurize_many_equals_featurize_device(use_db):
    base = _audio(1.1, seed=17)
    wavs = [base[i:i + n].copy() for i, n in enumerate(LENS)]  # (different audio per segment)
    single = _featurizer("mfcc", use_db=use_db)
    refs = [single.featurize_device(w).clone() for w in wavs]
    assert [r.shape[0] for r in refs] == [0, 0, 1, 49, 49, 49, 100, 98] and all(r.shape[1] == 40 for r in refs)
    f = _featurizer("mfcc", use_db=use_db)
    feats, counts = f.featurize_many(wavs)
    torch.cuda.synchronize()
    assert counts.tolist() == [r.shape[0] for r in refs] and feats.shape == (int(counts.sum()), 40)
    assert torch.equal(feats, torch.cat(refs))
    padded, lens = f.featurize_many(wavs, padded=True)
    torch.cuda.synchronize()
    assert padded.shape == (len(wavs), 100, 40) and lens.tolist() == counts.tolist()
    for b, r in enumerate(refs):
        assert torch.equal(padded[b, :r.shape[0]], r), b
        assert not bool(padded[b, r.shape[0]:].contiguous().view(torch.int32).any()), b  # +0.0, bit for bit
    if use_db:  # the gain stages are the fbank form's own: same kernels, same workspace layout
        g = _featurizer("fbank", use_db=True)
        g.featurize_many(wavs)
        assert f.last_gains.tobytes() == g.last_gains.tobytes() and f.last_gains.shape == (len(wavs),)
        single.featurize_device(wavs[-1])
        assert np.float32(single.last_gain).tobytes() == np.float32(f.last_gains[-1]).tobytes()


@pytest.mark.parametrize("use_db,launches", [(True, 3), (False, 1)], ids=["db", "nodb"])
def test_no_new_launches(use_db, launches):
    from ppasr_amd import _lib
    f = _featurizer("mfcc", use_db=use_db)
    wav = _audio(0.7, seed=19)
    f.featurize_device(wav)
    f.featurize_many([wav, wav[:5000]])  # (handle, buffers)
    torch.cuda.synchronize()
    with _lib.kernel_profile() as kp:
        f.featurize_device(wav)
        torch.cuda.synchronize()
    assert sum(c for _, c in kp.kernels.values()) == launches and len(kp.kernels) == launches, kp.kernels
    with _lib.kernel_profile() as kp:
        f.featurize_many([wav, wav[:5000]])
        torch.cuda.synchronize()
    assert sum(c for _, c in kp.kernels.values()) == launches and len(kp.kernels) == launches, kp.kernels
    assert all("batch" in k for k in kp.kernels), kp.kernels


# ---- 5. through the public surface -----------------------------------------------------------------------------------------
V = 300


def _cfg():
    return dict(encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15),
                preprocess_conf=dict(feature_method="mfcc", n_mels=80, n_mfcc=40, sample_rate=16000, use_dB_normalization=True,
                                     target_dB=-20),
                ctc_beam_search_decoder_conf=dict(alpha=2.2, beta=4.3, beam_size=10, num_processes=10, cutoff_prob=0.99,
                                                  cutoff_top_n=40, language_model_path=None),
                use_model="conformer", streaming=True, decoder="ctc_greedy", metrics_type="cer")


@pytest.fixture(scope="module")
def predictor():
    from ppasr_amd.predict import PPASRPredictor
    sd = conformer_state_dict(input_dim=40, vocab_size=V, num_blocks=2, seed=31, perturb_norm=True)
    return PPASRPredictor(configs=_cfg(), state_dict=sd, vocab_list=synth_vocabulary(V), warmup=False)


def test_predictor_serves_an_mfcc_model(predictor):
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    p = predictor
    model = p.predictor.model
    assert model.input_dim == 40 and p._audio_featurizer.feature_dim == 40
    wav = _audio(3.0, seed=4)
    res = p.predict(audio_data=wav)
    assert set(res) == {"text", "score"} and isinstance(res["text"], str)
    feat = AudioFeaturizer(**_cfg()["preprocess_conf"]).featurize(wav)
    assert feat.shape == (298, 40)
    probs = model.get_encoder_out(feat[None].astype(np.float32), np.array([feat.shape[0]], np.int64))
    torch.cuda.synchronize()
    assert p.decode(probs[0])[1] == res["text"]
    # streaming: 0.5 s PCM16 packets
    pcm = (np.clip(wav, -1, 1) * 32767).astype(np.int16).tobytes()
    step = 16000
    out, n_none = None, 0
    for i in range(0, len(pcm), step):
        r = p.predict_stream(audio_data=pcm[i:i + step], is_end=(i + step >= len(pcm)))
        n_none += r is None
        out = r or out
    assert out is not None and isinstance(out["text"], str) and n_none >= 1
    assert p.predictor.offset[0] > 0
    p.reset_stream()
    assert p.predictor.offset[0] == 0 and p.predictor.att_cache.shape == (0, 0, 0, 0)


def test_stream_pool_feed_and_feed_many_agree_on_mfcc(predictor):
    from ppasr_amd.serving import StreamPool
    model, vocab, pre = predictor.predictor.model, synth_vocabulary(V), _cfg()["preprocess_conf"]
    wavs = [_audio(2.4 + 0.07 * s, seed=40 + s) for s in range(3)]
    pcms = [(np.clip(w, -1, 1) * 32767).astype(np.int16).tobytes() for w in wavs]
    step = 16000  # 0.5 s packets
    a = StreamPool(model, vocab, n_sessions=3, preprocess_conf=pre)
    b = StreamPool(model, vocab, n_sessions=3, preprocess_conf=pre)
    assert a.featurizer.feature_dim == 40
    for i in range(0, max(len(x) for x in pcms), step):
        packets = {s: pcm[i:i + step] for s, pcm in enumerate(pcms) if i < len(pcm)}
        for s, pkt in packets.items():
            a.feed(s, pkt)
        b.feed_many(packets)
        for s in range(3):
            fa, fb = a.sessions[s].cached_feat, b.sessions[s].cached_feat
            assert fa.shape[2] == 40 and np.asarray(fa).tobytes() == fb.cpu().numpy().tobytes(), (i, s)
        assert a.step() == b.step(), i
    got_a, got_b = [a.finish(s) for s in range(3)], [b.finish(s) for s in range(3)]
    for s in range(3):
        assert got_a[s] is not None and got_a[s] == got_b[s], (s, got_a[s], got_b[s])
        assert a.sessions[s].frame_ids == b.sessions[s].frame_ids and len(a.sessions[s].frame_ids) >= 16, s
