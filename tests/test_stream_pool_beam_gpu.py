"""GPU: StreamPool(decoder="ctc_beam_search") behind every kind of session group -- staggered PCM streams decoded with one
beam-search launch per round.  The decoder half is exact (the probabilities each round produced, fed to one
BeamSearchDecoder per session, give the pool's text and score bit for bit); end to end every session equals its own
PPASRPredictor.predict_stream with the beam-search decoder."""
import numpy as np
import pytest

from lm_util import write_synthetic_arpa
from ppasr_amd.utils.synth import (conformer_state_dict, efficient_conformer_state_dict, squeezeformer_state_dict,
                                   synth_vocabulary)

from session_groups import predict_stream_reference

pytestmark = pytest.mark.gpu
V = 300


def _setup(family):
    from test_predictor_gpu import _cfg
    if family == "squeezeformer":
        cfg = _cfg(use_model="squeezeformer", L=4)
        cfg["encoder_conf"] = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=4, reduce_idx=1,
                                   recover_idx=3, feed_forward_expansion_factor=8, cnn_module_kernel=31)
        return cfg, squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=5)
    if family == "efficient_conformer":
        cfg = _cfg(use_model="efficient_conformer", L=4)
        cfg["encoder_conf"] = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                                   cnn_module_norm="layer_norm",
                                   efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1],
                                                       group_size=3, stride_kernel=True))
        return cfg, efficient_conformer_state_dict(vocab_size=V, num_blocks=4, seed=5, stride_layer_idx=1,
                                                   group_layer_idx=(0, 1))
    return _cfg(use_model="conformer", L=2), conformer_state_dict(vocab_size=V, num_blocks=2, seed=3)


def _group(family, model, n):
    if family == "squeezeformer":
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup
        return SqueezeformerStreamGroup(model, n)
    if family == "efficient_conformer":
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup
        return EfficientConformerStreamGroup(model, n)
    if family == "handles":
        from ppasr_amd.model_utils.conformer.model import StreamHandleSet
        return StreamHandleSet(model, n)
    return None  # make_stream_group's choice: ConformerStreamGroup


@pytest.mark.parametrize("family,scorer,beam", [("conformer", False, 300), ("conformer", True, 10),
                                                 ("handles", False, 10),
                                                 ("squeezeformer", False, 10), ("squeezeformer", True, 10),
                                                 ("efficient_conformer", False, 10), ("efficient_conformer", True, 10)])
def test_stream_pool_beam_search_equals_predict_stream(tmp_path, family, scorer, beam):
    from test_predictor_gpu import _audio
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchDecoder
    from ppasr_amd.serving import StreamPool
    vocab = synth_vocabulary(V)
    cfg, sd = _setup("conformer" if family == "handles" else family)
    cfg["decoder"] = "ctc_beam_search"
    conf = cfg["ctc_beam_search_decoder_conf"]
    conf["beam_size"] = beam
    if scorer:
        conf["language_model_path"] = write_synthetic_arpa(str(tmp_path / "lm.arpa"), vocab[2:150], order=3, seed=6)
    n = 3
    p, pcms, want = predict_stream_reference(cfg, sd, vocab, [_audio(2.4, seed=21), _audio(1.93, seed=22), _audio(3.1, seed=23)])
    step = 16000  # 0.5 s packets
    model = p.predictor.model
    pool = StreamPool(model, vocab, n_sessions=n, preprocess_conf=cfg["preprocess_conf"], group=_group(family, model, n),
                      decoder="ctc_beam_search", decoder_conf=dict(conf))
    rounds = []  # (sessions, probs) of every encoder round
    encode = pool.group.encode_chunks

    def spy(ids, chunks, want_probs=False):
        out = encode(ids, chunks, want_probs=want_probs)
        assert want_probs
        rounds.append((list(ids), out[2].clone()))
        return out
    pool.group.encode_chunks = spy
    # staggered: session 2 starts one packet late
    for i in range(0, max(len(x) for x in pcms) + step, step):
        for s, pcm in enumerate(pcms):
            j = i - step if s == 2 else i
            if 0 <= j < len(pcm):
                pool.feed(s, pcm[j:j + step])
        pool.step()
    got = [pool.finish(s) for s in range(n)]
    # decoder half, exact
    singles = [BeamSearchDecoder(vocab_list=vocab, **conf) for _ in range(n)]
    last = [None] * n
    for ids, probs in rounds:
        for k, s in enumerate(ids):
            last[s] = singles[s].decode_chunk(probs[k:k + 1], np.array([probs.shape[1]]))
    for s in range(n):
        assert got[s] is not None and got[s]["text"] == last[s][1] and got[s]["score"] == last[s][0], s
    # end to end
    for s in range(n):
        assert want[s] is not None and got[s]["text"] == want[s]["text"], (s, got[s], want[s])
        assert abs(got[s]["score"] - want[s]["score"]) <= 1e-4 * max(1.0, abs(want[s]["score"])), (s, got[s], want[s])
    # reset: both halves start again
    pool.reset(0)
    assert pool.beam.frames(0) == 0 and pool.sessions[0].result is None


def test_greedy_stays_the_default():
    from test_predictor_gpu import _cfg
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    from ppasr_amd.serving import StreamPool
    cfg = _cfg()
    model = ConformerModel(80, V, streaming=True, encoder_conf=cfg["encoder_conf"],
                           state_dict=conformer_state_dict(vocab_size=V, num_blocks=2, seed=3), device="cuda:0")
    pool = StreamPool(model, synth_vocabulary(V), n_sessions=2, preprocess_conf=cfg["preprocess_conf"])
    assert pool.decoder == "ctc_greedy" and pool.beam is None
