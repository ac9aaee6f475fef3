"""`decoder: attention_rescoring` end to end: PPASRPredictor on a synthetic checkpoint that carries decoder weights.
predict returns the hypothesis the float64 pipeline picks (the library's own n-best -> tests/decoder_oracle.py in float64
-> argmax); predict_stream raises; a checkpoint without decoder.* raises the missing-weight error; DeepSpeech2 is refused;
a batch of 3 through attention_rescoring() equals three single calls."""
import numpy as np
import pytest
import torch

import decoder_cases as dc
from decoder_oracle import DecoderOracle
from ppasr_amd.utils.synth import conformer_state_dict, deepspeech2_state_dict, synth_vocabulary

pytestmark = pytest.mark.gpu
V, UNITS, BLOCKS = 300, 1024, (3, 3)
RESCORING = dict(beam_size=5, ctc_weight=0.5, reverse_weight=0.3, cutoff_prob=0.99, cutoff_top_n=40)


def _cfg(use_model="conformer"):
    enc = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
    if use_model == "deepspeech2":
        enc = dict(num_rnn_layers=2, rnn_size=1024, use_gru=False)
    return dict(encoder_conf=enc,
                decoder_conf=dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0], r_num_blocks=BLOCKS[1],
                                  dropout_rate=0.1, positional_dropout_rate=0.1, self_attention_dropout_rate=0.1,
                                  src_attention_dropout_rate=0.1),
                preprocess_conf=dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True,
                                     target_dB=-20),
                attention_rescoring_decoder_conf=dict(RESCORING),
                use_model=use_model, streaming=True, decoder="attention_rescoring", metrics_type="cer")


def _audio(seconds, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(int(16000 * seconds)) / 16000.0
    x = 0.1 * np.sin(2 * np.pi * 220 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(t.shape)
    return x.astype(np.float32)


def _checkpoint():
    sd = conformer_state_dict(vocab_size=V, num_blocks=2, seed=3)
    sd.update(dc.decoder_state_dict(77, V, UNITS, *BLOCKS))
    return sd


@pytest.fixture(scope="module")
def predictor():
    from ppasr_amd.predict import PPASRPredictor
    return PPASRPredictor(configs=_cfg(), state_dict=_checkpoint(), vocab_list=synth_vocabulary(V), warmup=False)


def test_predict_returns_the_float64_pipelines_choice(predictor):
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    from ppasr_amd.decoders.beam_search_decoder import beam_search_ids
    p = predictor
    wav = _audio(1.2, seed=5)
    res = p.predict(audio_data=wav)
    assert set(res) == {"text", "score"}
    # the float64 pipeline on the library's own n-best
    feat = AudioFeaturizer(**_cfg()["preprocess_conf"]).featurize(wav)
    x, lens = feat[None].astype(np.float32), np.array([feat.shape[0]], np.int64)
    probs, memory = p.predictor.model.get_encoder_out(x, lens, return_memory=True)
    tokens, hl, scores, _ = beam_search_ids(probs, RESCORING["beam_size"], RESCORING["cutoff_prob"], RESCORING["cutoff_top_n"],
                                            nbest=RESCORING["beam_size"])
    tokens, hl, scores = tokens.cpu().numpy(), hl.cpu().numpy(), scores.cpu().numpy()
    assert (hl >= 0).sum() >= 2
    ref = DecoderOracle(_checkpoint(), V, *BLOCKS, dtype=torch.float64).rescore(
        memory.cpu().numpy(), None, tokens, hl, scores, RESCORING["ctc_weight"], RESCORING["reverse_weight"])
    # (the choice is only defined where float64 itself has a clear winner: the margin rule of tests/decoder_cases.py)
    case = dict(L=tokens.shape[2] + 1)
    assert dc.top2_margin(ref["total"][0]) > dc.MARGIN_FACTOR * dc.score_tol(case, ref, 0, 2e-5)
    k = int(ref["best"][0])
    vocab = synth_vocabulary(V)
    assert res["text"] == "".join(vocab[i] for i in tokens[0, k, :hl[0, k]])
    tol = dc.score_tol(case, ref, 0, 2e-5)
    assert abs(res["score"] - ref["total"][0, k]) <= tol, (res["score"], ref["total"][0, k], tol)
    # predict_long goes the same way
    long = p.predict_long(audio_data=wav, speech_timestamps=[dict(start=0, end=len(wav))])
    assert long["text"] == res["text"]


def test_predict_stream_raises(predictor):
    with pytest.raises(NotImplementedError, match="attention_rescoring"):
        predictor.predict_stream(audio_data=_audio(0.5), is_end=False)


def test_checkpoint_without_decoder_weights_names_the_missing_one():
    from ppasr_amd import _lib
    from ppasr_amd.predict import PPASRPredictor
    sd = {k: v for k, v in _checkpoint().items() if not k.startswith("decoder.")}
    with pytest.raises(_lib.PPASRHipError, match="decoder.left_decoder") as e:
        PPASRPredictor(configs=_cfg(), state_dict=sd, vocab_list=synth_vocabulary(V), warmup=False)
    assert e.value.status == _lib.PPASR_EMISSING


def test_deepspeech2_is_refused():
    from ppasr_amd.predict import PPASRPredictor
    sd = deepspeech2_state_dict(vocab_size=120, num_rnn_layers=2, streaming=True, seed=7)
    with pytest.raises(ValueError, match="attention_rescoring"):
        PPASRPredictor(configs=_cfg("deepspeech2"), state_dict=sd, vocab_list=synth_vocabulary(120), warmup=False)


def test_batch_of_three_equals_three_single_calls(predictor):
    from ppasr_amd.decoders.attention_rescoring import attention_rescoring
    from ppasr_amd.utils.synth import synth_features
    model, rescorer = predictor.predictor.model, predictor.predictor.rescorer
    x, lens = synth_features(3, 131, lens=[131, 100, 60], seed=9)
    model.set_skip_padding(True)
    try:
        probs, memory = model.get_encoder_out(x, lens, return_memory=True)
    finally:
        model.set_skip_padding(False)
    out_lens = model.valid_out_frames(lens, 131)
    vocab = synth_vocabulary(V)
    batch = attention_rescoring(model, rescorer, probs, memory, out_lens, vocab, **RESCORING)
    assert len(batch) == 3
    for b in range(3):
        one = attention_rescoring(model, rescorer, probs[b:b + 1], memory[b:b + 1], out_lens[b:b + 1], vocab, **RESCORING)
        # (every packed row goes through the same arithmetic whatever else the call holds)
        assert one[0] == batch[b], b


def test_evaluate_takes_the_decoder(predictor):
    """ppasr_amd.evaluate with decoder="attention_rescoring": the mean error rate of attention_rescoring()'s texts"""
    from ppasr_amd.decoders.attention_rescoring import attention_rescoring
    from ppasr_amd.evaluate import evaluate
    from ppasr_amd.utils.metrics import cer, labels_to_string
    from ppasr_amd.utils.synth import synth_features
    model, rescorer = predictor.predictor.model, predictor.predictor.rescorer
    vocab = synth_vocabulary(V)
    x, lens = synth_features(2, 99, lens=[99, 99], seed=13)
    labels = np.array([[5, 9, 17, 3, -1], [8, 8, 21, -1, -1]], np.int64)
    got = evaluate(model, [(x, labels, lens, np.array([4, 3]))], vocab, decoder="attention_rescoring", rescorer=rescorer,
                   rescoring_conf=RESCORING)
    probs, memory = model.get_encoder_out(x, lens, return_memory=True)
    texts = [t for _, t in attention_rescoring(model, rescorer, probs, memory, None, vocab, **RESCORING)]
    want = np.mean([cer(t, l) for t, l in zip(texts, labels_to_string(labels, vocab, eos=len(vocab) - 1))])
    assert got == pytest.approx(float(want), abs=1e-12)
    with pytest.raises(ValueError, match="rescorer"):
        evaluate(model, [], vocab, decoder="attention_rescoring")
