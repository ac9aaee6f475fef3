"""Token timestamps of streams, the parts that need no device: the greedy run-length builder against the float64 Viterbi
of tests/align_oracle.py, the workspace arithmetic of ppasr_ctc_align_arena, and the argument checks that come before
any device call.

Why the run-length builder may stand in for the alignment: the frame-wise argmax path is the best of ALL paths, and it
collapses to greedy's tokens, so it is the best path of those tokens; it is the only one when every frame's top-2 margin
is positive.  The tables admitted here have a float64 log-margin of at least 0.01 on every frame, far above what fp32
rounding of a softmax row can move, so begin, end and conf must be equal exactly."""
import ctypes

import numpy as np
import pytest

import align_oracle as ao
from ppasr_amd import _lib
from ppasr_amd.decoders.ctc_alignment import greedy_runs, token_entries

V = 7
SEEDS = [0, 1, 2, 3, 4]
MARGIN = 0.01


def table(seed, T):
    rng = np.random.default_rng(1000 * T + seed)
    z = rng.normal(size=(T, V)) * 3.0
    z[:, 0] += 4.0 * (rng.random(T) < 0.5)
    p = np.exp(z - z.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def admitted(p):
    top = np.sort(np.log(np.maximum(p.astype(np.float64), float(ao.FLT_MIN))), axis=1)
    return bool((top[:, -1] - top[:, -2] >= MARGIN).all())


@pytest.mark.parametrize("T", [1, 2, 17, 64])
def test_greedy_runs_are_the_float64_viterbi_of_greedys_own_tokens(T):
    n = 0
    for seed in SEEDS:
        p = table(seed, T)
        if not admitted(p):
            continue
        n += 1
        ids, spans = greedy_runs(p.argmax(1), p.max(1), 0)
        assert ids == ao.collapse(p.argmax(1).tolist(), 0)
        ref = ao.align(p, ids)
        assert ref["status"] == ao.OK
        assert [b for b, _, _ in spans] == ref["begin"].tolist() and [e for _, e, _ in spans] == ref["end"].tolist()
        assert np.asarray([c for _, _, c in spans], np.float32).tobytes() == ref["conf"].tobytes()
        assert all(isinstance(c, float) for _, _, c in spans)
    print(f"[greedy_runs] T={T}: {n} of {len(SEEDS)} seeds admitted")
    assert n >= 3  # (it cannot pass by admitting nothing)


def test_greedy_runs_edges():
    assert greedy_runs([], []) == ([], [])
    assert greedy_runs([0, 0, 0], [0.9, 0.8, 0.7]) == ([], [])
    # a blank between two equal ids keeps them apart; blank_index is honoured
    ids, spans = greedy_runs([3, 3, 0, 3, 5, 5, 5], [0.5, 0.75, 0.9, 0.25, 0.125, 0.5, 0.25])
    assert ids == [3, 3, 5] and spans == [(0, 2, 0.75), (3, 4, 0.25), (4, 7, 0.5)]
    ids, spans = greedy_runs([3, 0, 0, 3], [0.5, 0.25, 0.75, 0.5], blank_index=3)
    assert ids == [0] and spans == [(1, 3, 0.75)]


def test_token_entries_follow_the_predictors_rule():
    vocab = ["<blank>", "<unk>", "a", "<space>", "b"]
    got = token_entries([2, 3, 4], [(0, 2, 0.5), (2, 3, 0.25), (5, 9, 1.0)], vocab, 0.08, 0.7, space_as_blank=True)
    assert got == [{"text": "a", "start": 0.0, "end": 2 * 0.08, "score": 0.5},
                   {"text": " ", "start": 2 * 0.08, "end": 3 * 0.08, "score": 0.25},
                   {"text": "b", "start": 5 * 0.08, "end": 0.7, "score": 1.0}]  # the last end is clipped to the audio fed
    assert token_entries([3], [(0, 1, 0.5)], vocab, 0.04, 1.0)[0]["text"] == "<space>"


def test_arena_workspace_is_the_dense_calls():
    lib = _lib.load()
    al = lambda n: (n + 255) // 256 * 256
    for n, Tp, mt in [(1, 1, 0), (3, 17, 5), (5, 257, 255), (64, 750, 50), (2, 0, 3)]:
        stride = (mt + 3) // 4 * 4 + 4
        want = max(al(n * Tp * stride * 4) + al(n * Tp * 64 * 2) + al(n * 2 * mt * 4), 256)
        assert lib.ppasr_ctc_align_arena_workspace_bytes(n, Tp, mt) == want == lib.ppasr_ctc_align_workspace_bytes(n, Tp, mt)
    for bad in [(0, 4, 4), (-1, 4, 4), (2, -1, 4), (2, 4, -1), (2, 4, 256)]:
        assert lib.ppasr_ctc_align_arena_workspace_bytes(*bad) == 0


def test_arena_create_refuses_bad_shapes_before_any_device_call():
    lib = _lib.load()
    h = ctypes.c_void_p(1)
    for args in [(0, 5, 4, 4), (2, 1, 4, 4), (2, 5, 0, 4), (2, 5, 4, 0), (-1, 5, 4, 4), (2, 5, -4, 4),
                 (2, 4233, 16, 2 ** 24), (2, 2 ** 20, 2 ** 10, 2 ** 10), (2 ** 20 + 1, 5, 4, 4), (2, 5, 2 ** 20, 2 ** 11)]:
        h.value = 1
        assert lib.ppasr_prob_arena_create(*args, ctypes.byref(h)) == _lib.PPASR_EINVAL, args
        assert not h.value  # no handle comes back
        assert b"prob_arena_create" in lib.ppasr_last_error()
    assert lib.ppasr_prob_arena_create(2, 5, 4, 4, None) == _lib.PPASR_EINVAL
    assert lib.ppasr_prob_arena_destroy(None) == _lib.PPASR_OK
    # the calls on a missing arena
    assert lib.ppasr_prob_arena_frames(None, 0) == -1 and lib.ppasr_prob_arena_free_pages(None) == -1
    assert lib.ppasr_prob_arena_reset(None, 0) == _lib.PPASR_EINVAL
    assert lib.ppasr_prob_arena_read(None, 0, None, None) == _lib.PPASR_EINVAL
    from ppasr_amd.decoders.ctc_alignment import ProbArena
    for kw in (dict(n_sessions=0, V=5), dict(n_sessions=2, V=1), dict(n_sessions=2, V=5, page_frames=0),
               dict(n_sessions=2, V=5, n_pages=0)):
        with pytest.raises(ValueError):
            ProbArena(**kw)


def test_stream_pool_validates_the_timestamp_arguments_first():
    from ppasr_amd.serving import StreamPool
    vocab = ["<blank>", "<unk>", "a", "b"]
    for decoder in ("ctc_greedy", "ctc_beam_search"):
        for kw in (dict(timestamps="yes"), dict(timestamps=1), dict(timestamps=None),
                   dict(timestamps=True, table_seconds=0), dict(timestamps=True, table_seconds=-3.0),
                   dict(timestamps=True, table_seconds=float("nan")), dict(timestamps=True, table_seconds=float("inf")),
                   dict(timestamps=True, table_seconds="30"), dict(timestamps=True, table_seconds=True),
                   dict(timestamps=True, page_frames=0), dict(timestamps=True, page_frames=-16),
                   dict(timestamps=True, page_frames=1.5), dict(timestamps=True, page_frames=True),
                   dict(table_seconds=0), dict(page_frames=0)):
            with pytest.raises(ValueError, match="StreamPool: (timestamps|table_seconds|page_frames)"):
                StreamPool(None, vocab, 2, decoder=decoder, **kw)
