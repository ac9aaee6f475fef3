"""Token timestamps end to end: PPASRPredictor.predict(..., timestamps=True), predict_long(..., timestamps=True) and
PPASRPredictor.align on the small synthetic checkpoints of the predictor tests, for the three decoders, DeepSpeech2 and
an Efficient-Conformer (whose stride layer doubles the frame step)."""
import numpy as np
import pytest

import decoder_cases as dc
from ppasr_amd.utils.synth import (conformer_state_dict, deepspeech2_state_dict, efficient_conformer_state_dict,
                                   synth_vocabulary)

pytestmark = pytest.mark.gpu
V = 300
CASES = ["ctc_greedy", "ctc_beam_search", "attention_rescoring", "deepspeech2", "efficient_conformer"]


def _audio(seconds, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(int(16000 * seconds)) / 16000.0
    x = 0.1 * np.sin(2 * np.pi * 220 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(t.shape)
    return x.astype(np.float32)


def _build(case):
    from ppasr_amd.predict import PPASRPredictor
    use_model = case if case in ("deepspeech2", "efficient_conformer") else "conformer"
    decoder = case if use_model == "conformer" else "ctc_greedy"
    enc = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
    if use_model == "deepspeech2":
        enc = dict(num_rnn_layers=2, rnn_size=1024, use_gru=False)
        sd = deepspeech2_state_dict(vocab_size=V, num_rnn_layers=2, streaming=True, seed=7)
    elif use_model == "efficient_conformer":
        enc = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                   cnn_module_norm="layer_norm", efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1],
                                                                     group_size=3, stride_kernel=True))
        sd = efficient_conformer_state_dict(vocab_size=V, num_blocks=4, seed=5, stride_layer_idx=1, group_layer_idx=(0, 1))
    else:
        sd = conformer_state_dict(vocab_size=V, num_blocks=2, seed=3)
        if decoder == "attention_rescoring":
            sd.update(dc.decoder_state_dict(77, V, 1024, 3, 3))
    cfg = dict(encoder_conf=enc,
               decoder_conf=dict(attention_heads=4, linear_units=1024, num_blocks=3, r_num_blocks=3),
               preprocess_conf=dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True,
                                    target_dB=-20),
               ctc_beam_search_decoder_conf=dict(alpha=2.2, beta=4.3, beam_size=10, num_processes=10, cutoff_prob=0.99,
                                                 cutoff_top_n=40, language_model_path=None),
               attention_rescoring_decoder_conf=dict(beam_size=5, ctc_weight=0.5, reverse_weight=0.3, cutoff_prob=0.99,
                                                     cutoff_top_n=40),
               use_model=use_model, streaming=True, decoder=decoder, metrics_type="cer")
    return PPASRPredictor(configs=cfg, state_dict=sd, vocab_list=synth_vocabulary(V), warmup=False)


_built = {}


@pytest.fixture
def predictor(request):
    case = request.param
    if case not in _built:
        _built[case] = _build(case)
    return case, _built[case]


def _check_entries(entries, text, duration, offset=0.0):
    assert "".join(e["text"] for e in entries) == text
    last = offset
    for e in entries:
        assert set(e) == {"text", "start", "end", "score"}
        assert offset <= e["start"] < e["end"] <= offset + duration + 1e-9, (e, duration)
        assert e["start"] >= last  # non-decreasing
        last = e["start"]
        assert 0.0 <= e["score"] <= 1.0


@pytest.mark.parametrize("predictor", CASES, indirect=True)
def test_timestamps(predictor):
    case, p = predictor
    wav = _audio(2.0, seed=4)
    duration = len(wav) / 16000.0
    plain = p.predict(audio_data=wav)
    assert set(plain) == {"text", "score"}
    res = p.predict(audio_data=wav, timestamps=True)
    assert set(res) == {"text", "score", "timestamps"}
    assert res["text"] == plain["text"] and res["score"] == plain["score"]  # the same decode, plus one alignment
    assert p.predict(audio_data=wav) == plain
    print(f"[timestamps] {case}: {len(res['timestamps'])} tokens, text {res['text']!r}")
    _check_entries(res["timestamps"], res["text"], duration)
    # the frame step: 4 x 10 ms, 8 x 10 ms behind the Efficient-Conformer's stride layer
    step = 0.08 if case == "efficient_conformer" else 0.04
    assert p.predictor.model.total_subsampling * 0.01 == pytest.approx(step)
    for e in res["timestamps"]:
        assert e["start"] / step == pytest.approx(round(e["start"] / step), abs=1e-6)
    # a transcript the caller supplies: the decoder's own text gives the decoder's own timestamps
    assert p.align(wav, plain["text"]) == res["timestamps"]
    # and any other one: five tokens with a repeat and the multi-character <unk> entry
    vocab = synth_vocabulary(V)
    other = vocab[7] + vocab[7] + "<unk>" + vocab[9] + vocab[8]
    entries = p.align(wav, other)
    assert [e["text"] for e in entries] == [vocab[7], vocab[7], "<unk>", vocab[9], vocab[8]]
    _check_entries(entries, other, duration)
    assert entries[0]["end"] < entries[1]["start"]  # a blank frame between the two equal tokens


@pytest.mark.parametrize("predictor", ["ctc_greedy", "ctc_beam_search"], indirect=True)
def test_predict_long_offsets_each_segment(predictor):
    case, p = predictor
    wav = np.concatenate([_audio(1.5, seed=1), _audio(1.0, seed=2), _audio(1.5, seed=3)])
    segs = [dict(start=0, end=24000), dict(start=40000, end=len(wav))]
    plain = p.predict_long(audio_data=wav, speech_timestamps=segs)
    assert set(plain) == {"text", "score"}
    res = p.predict_long(audio_data=wav, speech_timestamps=segs, timestamps=True)
    assert res["text"] == plain["text"] and res["score"] == plain["score"]
    want = []
    for s in segs:
        one = p.predict(audio_data=wav[s["start"]:s["end"]], timestamps=True)
        at = s["start"] / 16000.0
        _check_entries(one["timestamps"], one["text"], (s["end"] - s["start"]) / 16000.0)
        want += [dict(e, start=e["start"] + at, end=e["end"] + at) for e in one["timestamps"]]
    assert res["timestamps"] == want
    assert "".join(e["text"] for e in res["timestamps"]) == res["text"].replace("，", "")


@pytest.mark.parametrize("predictor", ["ctc_greedy"], indirect=True)
def test_align_refuses_what_cannot_be_aligned(predictor):
    _, p = predictor
    wav = _audio(1.0, seed=6)
    vocab = synth_vocabulary(V)
    with pytest.raises(ValueError, match="not in the vocabulary"):
        p.align(wav, vocab[5] + "q")
    frames = p.predictor.predict_device(*_features(p, wav)).shape[1]
    with pytest.raises(ValueError, match=rf"T = {frames} frames, {frames + 1} needed"):
        p.align(wav, "".join(vocab[2 + (i % 2)] for i in range(frames + 1)))
    # one token per frame still fits, and a transcript of one repeated character needs a blank between each pair
    fit = p.align(wav, "".join(vocab[2 + (i % 2)] for i in range(frames)))
    assert [(round(e["start"] / 0.04), round(e["end"] / 0.04)) for e in fit[:-1]] == [(i, i + 1) for i in range(frames - 1)]
    n = (frames + 1) // 2 + 1
    with pytest.raises(ValueError, match=rf"T = {frames} frames, {2 * n - 1} needed \({n} tokens, {n - 1} repeats\)"):
        p.align(wav, vocab[2] * n)
    assert p.align(wav, "") == []


def _features(p, wav):
    feat = np.asarray(p._audio_featurizer.featurize(wav, 16000), np.float32)[np.newaxis, :]
    return feat, np.array([feat.shape[1]], np.int64)
