"""`decoder: attention` end to end: PPASRPredictor on a synthetic checkpoint that carries decoder weights.  predict
returns the text of the device's best hypothesis (AttentionRescorer.decode on the same encoder output; the search itself is
held to float64 by tests/test_attention_decode_gpu.py); timestamps=True returns one entry per token; predict_stream,
StreamPool and DeepSpeech2 refuse the decoder; evaluate(decoder="attention") runs a two-batch set."""
import numpy as np
import pytest

import decoder_cases as dc
from ppasr_amd.utils.synth import conformer_state_dict, deepspeech2_state_dict, synth_vocabulary

pytestmark = pytest.mark.gpu
V, UNITS, BLOCKS = 300, 1024, (3, 0)
ATTENTION = dict(beam_size=4, max_steps=6)


def _cfg(use_model="conformer"):
    enc = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
    if use_model == "deepspeech2":
        enc = dict(num_rnn_layers=2, rnn_size=1024, use_gru=False)
    return dict(encoder_conf=enc,
                decoder_conf=dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0], r_num_blocks=BLOCKS[1]),
                preprocess_conf=dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True,
                                     target_dB=-20),
                attention_decoder_conf=dict(ATTENTION),
                use_model=use_model, streaming=True, decoder="attention", metrics_type="cer")


def _audio(seconds, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(int(16000 * seconds)) / 16000.0
    x = 0.1 * np.sin(2 * np.pi * 220 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(t.shape)
    return x.astype(np.float32)


def _checkpoint():
    sd = conformer_state_dict(vocab_size=V, num_blocks=2, seed=3)
    sd.update(dc.decoder_state_dict(78, V, UNITS, *BLOCKS))
    # a trained decoder never emits the CTC blank; a random one would, and a transcript with a blank cannot be aligned
    b = sd["decoder.left_decoder.output_layer.bias"].copy()
    b[0] -= 30.0
    sd["decoder.left_decoder.output_layer.bias"] = b
    return sd


@pytest.fixture(scope="module")
def predictor():
    from ppasr_amd.predict import PPASRPredictor
    return PPASRPredictor(configs=_cfg(), state_dict=_checkpoint(), vocab_list=synth_vocabulary(V), warmup=False)


def test_predict_returns_the_best_hypothesis_of_the_device_search(predictor):
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    p = predictor
    wav = _audio(1.2, seed=5)
    res = p.predict(audio_data=wav)
    assert set(res) == {"text", "score"}
    feat = AudioFeaturizer(**_cfg()["preprocess_conf"]).featurize(wav)
    x, lens = feat[None].astype(np.float32), np.array([feat.shape[0]], np.int64)
    _, memory = p.predictor.model.get_encoder_out(x, lens, return_memory=True)
    got = p.predictor.rescorer.decode(memory, None, **ATTENTION)
    n = int(got["lens"][0, 0])
    ids = got["tokens"][0, 0, :n].cpu().tolist()
    vocab = synth_vocabulary(V)
    assert 0 < n <= ATTENTION["max_steps"] and 0 not in ids
    assert res["text"] == "".join(vocab[i] for i in ids)
    assert res["score"] == float(got["scores"][0, 0])
    # predict_long goes the same way
    long = p.predict_long(audio_data=wav, speech_timestamps=[dict(start=0, end=len(wav))])
    assert long["text"] == res["text"]
    # timestamps: one entry per token of the decoded ids, in order, inside the utterance
    ts = p.predict(audio_data=wav, timestamps=True)
    assert ts["text"] == res["text"] and ts["score"] == res["score"]
    assert [e["text"] for e in ts["timestamps"]] == [vocab[i] for i in ids]
    starts = [e["start"] for e in ts["timestamps"]]
    assert starts == sorted(starts) and all(0.0 <= e["start"] < e["end"] <= 1.2 + 1e-9 for e in ts["timestamps"])


def test_default_max_steps_is_the_number_of_encoder_frames(predictor):
    r = predictor.predictor.rescorer
    assert r.default_max_steps(28) == 28 and r.default_max_steps(1000) == 255 and r.default_max_steps(0) == 1
    memory = np.random.default_rng(1).standard_normal((1, 9, 256)).astype(np.float32)
    assert tuple(r.decode(memory, None, beam_size=2)["tokens"].shape) == (1, 2, 9)


def test_streams_refuse_the_decoder(predictor):
    from ppasr_amd.serving import StreamPool
    with pytest.raises(NotImplementedError, match="decoder: attention scores whole utterances"):
        predictor.predict_stream(audio_data=_audio(0.5), is_end=False)
    with pytest.raises(ValueError, match="unknown decoder 'attention'"):
        StreamPool(None, synth_vocabulary(V), 2, decoder="attention")


def test_deepspeech2_is_refused():
    from ppasr_amd.predict import PPASRPredictor
    sd = deepspeech2_state_dict(vocab_size=120, num_rnn_layers=2, streaming=True, seed=7)
    with pytest.raises(ValueError, match="decoder: attention needs a Conformer-family model"):
        PPASRPredictor(configs=_cfg("deepspeech2"), state_dict=sd, vocab_list=synth_vocabulary(120), warmup=False)


def test_evaluate_takes_the_decoder(predictor):
    """ppasr_amd.evaluate with decoder="attention" over two batches: the mean error rate of attention_decode()'s texts"""
    from ppasr_amd.decoders import attention_decode
    from ppasr_amd.evaluate import evaluate
    from ppasr_amd.utils.metrics import cer, labels_to_string
    from ppasr_amd.utils.synth import synth_features
    model, rescorer = predictor.predictor.model, predictor.predictor.rescorer
    vocab = synth_vocabulary(V)
    batches, errs = [], []
    for seed, labels in ((13, [[5, 9, 17, 3, -1], [8, 8, 21, -1, -1]]), (14, [[7, 7, 2, -1, -1], [30, 4, 4, 4, 11]])):
        x, lens = synth_features(2, 99, lens=[99, 99], seed=seed)
        labels = np.array(labels, np.int64)
        batches.append((x, labels, lens, (labels >= 0).sum(1)))
        _, memory = model.get_encoder_out(x, lens, return_memory=True)
        texts = [t for _, t in attention_decode(model, rescorer, memory, None, vocab, **ATTENTION)]
        errs += [cer(t, l) for t, l in zip(texts, labels_to_string(labels, vocab, eos=len(vocab) - 1))]
    got = evaluate(model, batches, vocab, decoder="attention", rescorer=rescorer, attention_conf=ATTENTION)
    assert got == pytest.approx(float(np.mean(errs)), abs=1e-12)
    with pytest.raises(ValueError, match="rescorer"):
        evaluate(model, [], vocab, decoder="attention")
