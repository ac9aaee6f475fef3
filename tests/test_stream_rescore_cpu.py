"""Refusals of the streaming attention-rescoring interface that need no device: every one is raised before the model, a
group or the library is touched (model=None, an object built without its constructor)."""
import pytest

VOCAB = ["<blank>", "a", "b"]


class _Rescorer:
    """stands in for an AttentionRescorer: the refusals below come before it is read"""
    d_model = 256


def test_stream_pool_refuses_attention_rescoring_without_a_rescorer():
    from ppasr_amd.serving import StreamPool
    with pytest.raises(ValueError, match="rescorer"):
        StreamPool(None, VOCAB, 2, decoder="attention_rescoring")
    with pytest.raises(ValueError, match="rescorer"):
        StreamPool(None, VOCAB, 2, decoder="attention_rescoring", decoder_conf={"beam_size": 5})
    with pytest.raises(ValueError, match="rescorer"):  # and a rescorer belongs to that decoder alone
        StreamPool(None, VOCAB, 2, decoder="ctc_beam_search", rescorer=_Rescorer())


def test_stream_pool_refuses_a_language_model_timestamps_and_unknown_keys():
    from ppasr_amd.serving import StreamPool
    kw = dict(decoder="attention_rescoring", rescorer=_Rescorer())
    with pytest.raises(ValueError, match="language_model_path"):
        StreamPool(None, VOCAB, 2, decoder_conf={"language_model_path": "lm.klm"}, **kw)
    with pytest.raises(ValueError, match="timestamps"):
        StreamPool(None, VOCAB, 2, timestamps=True, **kw)
    with pytest.raises(ValueError, match="unknown decoder_conf keys"):
        StreamPool(None, VOCAB, 2, decoder_conf={"alpha": 1.0}, **kw)
    with pytest.raises(ValueError, match="unknown decoder_conf keys"):
        StreamPool(None, VOCAB, 2, decoder_conf={"beam_width": 5}, **kw)
    for bad in (0, -1.0, float("inf"), True, "30"):
        with pytest.raises(ValueError, match="memory_seconds"):
            StreamPool(None, VOCAB, 2, memory_seconds=bad, **kw)


def test_finish_many_belongs_to_the_rescoring_decoder():
    from ppasr_amd.serving import StreamPool
    pool = object.__new__(StreamPool)
    pool.memory = None
    with pytest.raises(ValueError, match="attention_rescoring"):
        pool.finish_many([0])


@pytest.mark.parametrize("nbest", [0, -1, 6, 2.0, True, None])
def test_nbest_out_of_range_is_refused_before_any_device_work(nbest):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    pool = object.__new__(BeamSearchSessions)  # (no device, no library: the check reads beam_size alone)
    pool.beam_size, pool.n_sessions = 5, 3
    with pytest.raises(ValueError, match="nbest"):
        pool.nbest([0, 1], nbest)


def test_nbest_refuses_a_bad_session_list():
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    pool = object.__new__(BeamSearchSessions)
    pool.beam_size, pool.n_sessions = 5, 3
    for bad in ([], [0, 0], [3], [-1]):
        with pytest.raises(ValueError, match="sessions"):
            pool.nbest(bad, 2)
