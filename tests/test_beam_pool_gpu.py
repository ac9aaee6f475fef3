"""GPU: beam-search session pools (ppasr_beam_pool_* / BeamSearchSessions) -- N streaming CTC prefix beam searches
advanced with one pruning and one search launch per call.  Every session must give, after every chunk, the tokens and
the score its own BeamSearchDecoder.decode_chunk sequence gives on the same chunks (bit for bit while it does not grow),
whatever subset of sessions the call lists."""
import ctypes

import numpy as np
import pytest
import torch

from lm_util import write_synthetic_arpa
from ppasr_amd import _lib
from test_ctc_beam_gpu import _oracle, _probs
from test_ctc_beam_wordlm_gpu import VOCAB as WVOCAB, WORDS, _spoken_probs

pytestmark = pytest.mark.gpu
GUARD = 1 << 20
SENTINEL = 0xA5


def _vocab(V):
    return ["<blank>"] + [chr(0x4E00 + i) for i in range(V - 1)]


def _singles(n, beam, cutoff_prob, top_n, vocab, lm=None, max_frames=5000):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchDecoder
    return [BeamSearchDecoder(2.2, 4.3, beam, cutoff_prob, top_n, vocab, language_model_path=lm,
                              max_stream_frames=max_frames) for _ in range(n)]


def _round(rng, ids, table_of, V, max_len=16):
    """chunks of 1..max_len frames per listed session -> (probs [n,T,V] padded, lens [n], per-session chunks)"""
    lens = rng.integers(1, max_len + 1, size=len(ids)).astype(np.int32)
    T = int(lens.max())
    probs = np.zeros((len(ids), T, V), np.float32)
    chunks = []
    for k, s in enumerate(ids):
        c = table_of(s, int(lens[k]))
        probs[k, :lens[k]] = c
        probs[k, lens[k]:] = 1.0 / V  # (padding: never read)
        chunks.append(c)
    return probs, lens, chunks


def _check_round(pool, singles, ids, probs, lens, chunks, exact=True, last=None):
    got = pool.decode_chunks(ids, torch.from_numpy(probs).cuda(), lens)
    for k, s in enumerate(ids):
        want = singles[s].decode_chunk(chunks[k][None], np.array([chunks[k].shape[0]]))
        if last is not None:
            last[s] = got[k][1]
        assert got[k][1] == want[1], (s, got[k], want)
        if exact:
            assert got[k][0] == want[0], (s, got[k][0], want[0])
        else:
            assert abs(got[k][0] - want[0]) < 1e-9 * max(1.0, abs(want[0])), (s, got[k][0], want[0])
    return got


def _drive(pool, singles, n, rounds, seed, V, table_of, subset_max=None, exact=True, hist=None, on_round=None, last=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    for r in range(rounds):
        if on_round:
            on_round(r)
        m = int(rng.integers(1, (subset_max or n) + 1))
        ids = [int(i) for i in rng.permutation(n)[:m]]
        probs, lens, chunks = _round(rng, ids, table_of, V)
        if hist is not None:
            for k, s in enumerate(ids):
                hist[s].append(chunks[k])
        _check_round(pool, singles, ids, probs, lens, chunks, exact, last)


def _random_tables(seed, V):
    rng = np.random.Generator(np.random.PCG64(seed))
    return lambda s, L: _probs(rng, L, V, "peaky")


def _oracle_text(lib, chunks, V, beam, cutoff_prob, top_n, vocab):
    h = lib.ctc_beam_oracle_create(V, beam, ctypes.c_double(cutoff_prob), top_n, 0)
    total = 0
    for c in chunks:
        c = np.ascontiguousarray(c, np.float32)
        lib.ctc_beam_oracle_next(h, c.ctypes.data_as(ctypes.c_void_p), c.shape[0])
        total += c.shape[0]
    L = max(total, 1)
    tk = np.empty((1, L), np.int32); ln = np.empty(1, np.int32); sc = np.empty(1, np.float64)
    lib.ctc_beam_oracle_result(h, 1, L, tk.ctypes.data_as(ctypes.c_void_p), ln.ctypes.data_as(ctypes.c_void_p),
                               sc.ctypes.data_as(ctypes.c_void_p))
    lib.ctc_beam_oracle_free(h)
    return "".join(vocab[i] for i in tk[0, :ln[0]])


# ---- 1. staggered subsets ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,beam,cutoff_prob,top_n", [(300, 10, 0.99, 40), (300, 300, 0.99, 40), (4233, 10, 0.99, 40),
                                                      (4233, 300, 0.99, 40),
                                                      (300, 10, 1.0, 40)])  # unpruned: wide records in the workspace
def test_staggered_subsets_equal_single_decoders(V, beam, cutoff_prob, top_n):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    n, rounds = 8, 20
    vocab = _vocab(V)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, cutoff_prob, top_n, vocab, init_frames=rounds * 16)
    singles = _singles(n, beam, cutoff_prob, top_n, vocab)
    hist, last = [[] for _ in range(n)], {}
    _drive(pool, singles, n, rounds, 100 + V + beam, V, _random_tables(V + beam, V), hist=hist, last=last)
    assert all(pool.capacity(s) == rounds * 16 for s in range(n))  # (no growth here: test 4)
    assert not pool.status().any()
    lib = _oracle()
    for s in range(n):  # every session once against the C oracle's streaming object
        if hist[s]:
            assert pool.frames(s) == sum(c.shape[0] for c in hist[s])
            want = _oracle_text(lib, hist[s], V, beam, cutoff_prob, top_n, vocab)
            assert last[s] == want, s


# ---- 2. scorers -------------------------------------------------------------------------------------------------------
def test_character_scorer_sessions_equal_single_decoders(tmp_path):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, beam, n = 300, 30, 6
    vocab = _vocab(V)
    arpa = write_synthetic_arpa(str(tmp_path / "c.arpa"), vocab[2:150], order=3, seed=4)
    singles = _singles(n, beam, 0.99, 40, vocab, lm=arpa)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, scorer=singles[0]._ext_scorer, init_frames=256)
    _drive(pool, singles, n, 12, 7, V, _random_tables(8, V))
    assert not pool.status().any()


def test_word_scorer_sessions_equal_single_decoders(tmp_path):
    """Word-based scorers run with node tables: a reset session's table must be empty again."""
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, beam, n = len(WVOCAB), 30, 4
    arpa = write_synthetic_arpa(str(tmp_path / "w.arpa"), WORDS, order=3, n_sent=300, sent_len=8, seed=2)
    singles = _singles(n, beam, 0.99, 40, WVOCAB, lm=arpa)
    pool = BeamSearchSessions(n, 1.9, 0.3, beam, 0.99, 40, WVOCAB, language_model_path=arpa, init_frames=512)
    for d in singles:
        d._ext_scorer.reset_params(1.9, 0.3)
    rng = np.random.Generator(np.random.PCG64(3))
    sentences = [["the", "cat", "sat", "on", "the", "mat"], ["where", "is", "the", "hat"], ["we", "were", "here"],
                 ["then", "there", "was", "news"]]
    tables = [_spoken_probs(rng, sentences[s], V) for s in range(n)]
    pos = [0] * n

    def table_of(s, L):
        t = tables[s][pos[s]:pos[s] + L]
        pos[s] += t.shape[0]
        if t.shape[0] < L:  # (past the sentence: blanks)
            pad = np.full((L - t.shape[0], V), 1e-4, np.float32)
            pad[:, 0] = 1.0
            t = np.concatenate([t, pad / pad.sum(-1, keepdims=True)])
        return t

    def on_round(r):
        if r == 6:  # reset mid-stream: the session's node table is cleared
            pool.reset(1)
            singles[1].reset_decoder()
            pos[1] = 0
    _drive(pool, singles, n, 14, 5, V, table_of, on_round=on_round)
    assert not pool.status().any()


# ---- 3. reset ---------------------------------------------------------------------------------------------------------
def test_reset_mid_stream_equals_a_fresh_decoder():
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, beam, n = 300, 20, 5
    vocab = _vocab(V)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, init_frames=512)
    singles = _singles(n, beam, 0.99, 40, vocab)

    def on_round(r):
        if r == 8:
            pool.reset(2)
            singles[2].reset_decoder()
            assert pool.frames(2) == 0
        if r == 14:
            pool.reset()
            for d in singles:
                d.reset_decoder()
            assert all(pool.frames(s) == 0 for s in range(n))
    _drive(pool, singles, n, 20, 11, V, _random_tables(12, V), on_round=on_round)


# ---- 4. growth --------------------------------------------------------------------------------------------------------
def test_one_session_grows_and_the_others_are_untouched():
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, beam, n = 300, 10, 4
    vocab = _vocab(V)
    rng = np.random.Generator(np.random.PCG64(21))
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, init_frames=8)
    singles = _singles(n, beam, 0.99, 40, vocab, max_frames=400)  # sized for the whole stream: never grow
    frames = [0] * n
    for r in range(13):
        ids = [0] + ([1, 2] if r < 4 else []) + ([3] if r == 5 else [])
        lens = np.array([16] + [2] * (len(ids) - 1), np.int32)
        chunks = [_probs(rng, int(L), V, "peaky") for L in lens]
        probs = np.zeros((len(ids), 16, V), np.float32)
        for k, c in enumerate(chunks):
            probs[k, :c.shape[0]] = c
        _check_round(pool, singles, ids, probs, lens, chunks, exact=False)
        for k, s in enumerate(ids):
            frames[s] += int(lens[k])
    assert frames[0] == 208 and pool.frames(0) == 208 and pool.capacity(0) >= 208
    assert [pool.capacity(s) for s in (1, 2, 3)] == [8, 8, 8]
    assert [pool.frames(s) for s in (1, 2, 3)] == [8, 8, 2]
    assert not pool.status().any()


# ---- 5. more sessions than CUs ----------------------------------------------------------------------------------------
def test_more_sessions_than_compute_units():
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, beam, n = 300, 10, 300
    vocab = _vocab(V)
    rng = np.random.Generator(np.random.PCG64(31))
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, init_frames=64)
    singles = _singles(n, beam, 0.99, 40, vocab, max_frames=64)
    for _ in range(2):
        ids = list(range(n))
        probs, lens, chunks = _round(rng, ids, lambda s, L: _probs(rng, L, V, "peaky"), V)
        _check_round(pool, singles, ids, probs, lens, chunks)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
def _raw_decode(pool, ids, probs, T, lens, ws, ws_bytes, max_tokens=64):
    lib = _lib.load()
    n = len(ids)
    tokens = torch.empty(n, max_tokens, dtype=torch.int32, device="cuda")
    ln = torch.empty(n, dtype=torch.int32, device="cuda")
    sc = torch.empty(n, dtype=torch.float64, device="cuda")
    c_ids = (ctypes.c_int * n)(*ids)
    fl = None if lens is None else np.ascontiguousarray(lens, np.int32)
    rc = lib.ppasr_beam_pool_decode(pool._h, c_ids, n, probs.data_ptr(), T,
                                    None if fl is None else fl.ctypes.data_as(ctypes.c_void_p), max_tokens,
                                    tokens.data_ptr(), ln.data_ptr(), sc.data_ptr(), ws, ws_bytes,
                                    torch.cuda.current_stream().cuda_stream)
    return rc, tokens, ln, sc


def test_refusals_change_no_session():
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    lib = _lib.load()
    V, beam, n = 300, 10, 4
    vocab = _vocab(V)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, init_frames=128)
    singles = _singles(n, beam, 0.99, 40, vocab)
    tables = _random_tables(41, V)
    _drive(pool, singles, n, 3, 40, V, tables)
    before = [pool.frames(s) for s in range(n)]
    T = 8
    probs = torch.from_numpy(np.stack([_probs(np.random.default_rng(s), T, V, "peaky") for s in range(2)])).cuda()
    need = int(lib.ppasr_beam_pool_workspace_bytes(pool._h, 2, T))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for ids, lens, nbytes, code in [([1, 1], None, need, _lib.PPASR_EINVAL),        # repeated session
                                    ([0, n], None, need, _lib.PPASR_EINVAL),        # out of range
                                    ([0, -1], None, need, _lib.PPASR_EINVAL),
                                    ([0, 1], [3, T + 1], need, _lib.PPASR_EINVAL),  # frame_lens > T
                                    ([0, 1], [3, -1], need, _lib.PPASR_EINVAL),
                                    ([0, 1], None, need - 1, _lib.PPASR_ENOSPACE)]:  # short workspace
        rc = _raw_decode(pool, ids, probs, T, lens, ws.data_ptr(), nbytes)[0]
        assert rc == code, (ids, lens, nbytes, rc)
        assert [pool.frames(s) for s in range(n)] == before
    for bad_V, bad_beam in [(16384, 10), (1, 10), (300, 513), (300, 0)]:  # what the search refuses: at create
        h = ctypes.c_void_p()
        assert lib.ppasr_beam_pool_create(2, bad_V, bad_beam, 0.99, 40, 0, None, 0.0, 0.0, 16, ctypes.byref(h)) in (
            _lib.PPASR_EUNSUPPORTED, _lib.PPASR_EINVAL)
        assert not h.value
    with pytest.raises(ValueError):
        pool.decode_chunks([0, 0], probs)
    _drive(pool, singles, n, 6, 42, V, tables)  # every session continues as if nothing had been asked
    assert not pool.status().any()


# ---- 7. workspace canary ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff_prob", [0.99, 1.0])
def test_workspace_canary(cutoff_prob):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    lib = _lib.load()
    V, beam, n, T = 300, 16, 5, 16
    vocab = _vocab(V)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, cutoff_prob, 40, vocab, init_frames=64)
    singles = _singles(n, beam, cutoff_prob, 40, vocab)
    rng = np.random.Generator(np.random.PCG64(51))
    for r in range(3):
        ids = [4, 0, 2] if r != 1 else [1, 3]
        chunks = [_probs(rng, T, V, "peaky") for _ in ids]
        probs = torch.from_numpy(np.stack(chunks)).cuda()
        need = int(lib.ppasr_beam_pool_workspace_bytes(pool._h, len(ids), T))
        assert need > 0
        buf = torch.full((need + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        rc, tokens, ln, sc = _raw_decode(pool, ids, probs, T, None, buf.data_ptr(), need, max_tokens=3 * T)
        assert rc == 0, lib.ppasr_last_error()
        torch.cuda.synchronize()
        assert bool((buf[need:] == SENTINEL).all())
        for k, s in enumerate(ids):
            want = singles[s].decode_chunk(chunks[k][None], np.array([T]))
            got = "".join(vocab[i] for i in tokens[k, :int(ln[k])].tolist())
            assert got == want[1] and float(sc[k]) == want[0]
