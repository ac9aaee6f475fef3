"""GPU: ``StreamPool.feed_many`` -- the listed sessions' packets featurized by one set of fbank launches, features kept on
the device -- leaves every session exactly where ``feed`` leaves it: buffered remainder and cached features byte for byte
after every packet round and every ``step``, and the same frame ids, text and score at the end.  No tolerance."""
import numpy as np
import pytest
import torch

from ppasr_amd.utils.synth import conformer_state_dict, synth_vocabulary
from test_predictor_gpu import _audio, _cfg

pytestmark = pytest.mark.gpu
V = 97
N = 5
# packet sizes in samples, walked cyclically, session s starting s places in; the 100-sample packets yield no frame on
# many calls (the remainder alone is multiplied by the call's gain then)
PACKETS = [100, 1600, 100, 2400, 100, 5000, 100, 10240]


@pytest.fixture(scope="module")
def model():
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    cfg = _cfg(L=1)
    return ConformerModel(80, V, streaming=True, encoder_conf=cfg["encoder_conf"],
                          state_dict=conformer_state_dict(vocab_size=V, num_blocks=1, seed=3), device="cuda:0")


def _pool(model, **kw):
    from ppasr_amd.serving import StreamPool
    return StreamPool(model, synth_vocabulary(V), n_sessions=N, preprocess_conf=_cfg()["preprocess_conf"], **kw)


def _rounds():
    """-> [{session: packet}, ...]: about 1.6 s of audio per session, as PCM16 bytes (even sessions) or float samples"""
    rounds = []
    for s in range(N):
        w = _audio(1.6 + 0.013 * s, seed=70 + s)
        pos = r = 0
        while pos < w.size:
            part = w[pos:pos + PACKETS[(s + r) % len(PACKETS)]]
            pos += part.size
            if len(rounds) <= r:
                rounds.append({})
            rounds[r][s] = (np.clip(part, -1, 1) * 32767).astype(np.int16).tobytes() if s % 2 == 0 else part
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


def _drive(a, b, feed_b):
    """pool a by feed, pool b by feed_b(pool, round, {session: packet}); state compared after every round and step"""
    for r, packets in enumerate(_rounds()):
        for s, p in packets.items():
            a.feed(s, p)
        feed_b(b, r, packets)
        _same_state(a, b, ("fed", r))
        ua, ub = a.step(), b.step()
        assert ua == ub, r
        _same_state(a, b, ("stepped", r))
    return [a.finish(s) for s in range(N)], [b.finish(s) for s in range(N)]


def _feed_many(pool, r, packets):
    pool.feed_many(packets)


def test_feed_many_equals_feed_greedy(model):
    a, b = _pool(model), _pool(model)
    got_a, got_b = _drive(a, b, _feed_many)
    _same_state(a, b, "finished")
    assert all(isinstance(s.cached_feat, torch.Tensor) and s.cached_feat.is_cuda for s in b.sessions)
    assert all(isinstance(s.cached_feat, np.ndarray) for s in a.sessions)
    for s in range(N):
        assert a.sessions[s].frame_ids == b.sessions[s].frame_ids and len(a.sessions[s].frame_ids) >= 16, s
        assert a.sessions[s].frame_probs == b.sessions[s].frame_probs, s
        assert got_a[s] is not None and got_a[s] == got_b[s], (s, got_a[s], got_b[s])


def test_feed_many_equals_feed_beam_search(model):
    kw = dict(decoder="ctc_beam_search", decoder_conf=dict(beam_size=10))
    a, b = _pool(model, **kw), _pool(model, **kw)
    got_a, got_b = _drive(a, b, _feed_many)
    for s in range(N):
        assert got_a[s] is not None and got_a[s]["text"] == got_b[s]["text"], (s, got_a[s], got_b[s])
        assert got_a[s]["score"] == got_b[s]["score"], (s, got_a[s], got_b[s])


def test_feed_and_feed_many_in_one_round(model):
    def mixed(pool, r, packets):
        alone = [s for s in packets if (s + r) % 3 == 0]  # which sessions go through feed changes from round to round
        for s in alone:
            pool.feed(s, packets[s])
        many = {s: p for s, p in packets.items() if s not in alone}
        if many:
            pool.feed_many(many)
    a, b = _pool(model), _pool(model)
    got_a, got_b = _drive(a, b, mixed)
    for s in range(N):
        assert a.sessions[s].frame_ids == b.sessions[s].frame_ids, s
        assert got_a[s] is not None and got_a[s] == got_b[s], (s, got_a[s], got_b[s])


def test_feed_many_refusals_change_no_session(model):
    a, b = _pool(model), _pool(model)
    first, again = _rounds()[:2]
    with pytest.raises(ValueError):  # refused gain, between sessions that would be accepted
        b.feed_many({0: first[0], 1: np.full(1600, 1e-20, np.float32), 2: first[2]})
    _same_state(a, b, "after the refused gain")
    for s, p in first.items():
        a.feed(s, p)
    b.feed_many(first)
    with pytest.raises(ValueError):
        b.feed_many({**again, N: again[0]})             # unknown index
    with pytest.raises(ValueError):
        b.feed_many({**again, -1: again[0]})
    with pytest.raises(ValueError):
        b.feed_many(list(again.items()) + [(2, again[2])])  # repeated index (a list of pairs: a dict cannot repeat a key)
    _same_state(a, b, "after the refusals")
    for s, p in again.items():
        a.feed(s, p)
    b.feed_many(again)
    _same_state(a, b, "fed again")
