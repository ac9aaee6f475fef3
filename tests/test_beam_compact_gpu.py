"""GPU: compaction of the beam search's prefix arena (launch_beam_compact behind ppasr_ctc_beam_state_compact and
ppasr_beam_arena_*).  1: the kernel against a restatement on the host, word for word, and the search continued from the
compacted buffer against the one continued from an untouched copy, bit for bit.  2: a session pool compacted after every
round against single decoders and the C oracle.  3: the automatic policy.  4: node tables (word-based scorer) against the
C oracle with a dictionary.  5: refusals and BeamSearchDecoder(compact=True)."""
import ctypes

import numpy as np
import pytest
import torch

from lm_util import read_arpa, write_synthetic_arpa
from ppasr_amd import _lib
from test_beam_pool_gpu import _check_round, _drive, _oracle_text, _random_tables, _singles, _vocab
from test_ctc_beam_gpu import _oracle, _probs
from test_ctc_beam_lm_gpu import _oracle_lm_decode
from test_ctc_beam_wordlm_gpu import VOCAB as WVOCAB, WORDS, _dictionary, _oracle_word_decode, _spoken_probs

pytestmark = pytest.mark.gpu

# ---- the state layout of csrc/ctc_beam.h, restated ----
ARRAYS = 7 + (6 - 1)  # kBeamStateArrays = 7 + (kLmMaxOrder - 1)
ARENA = 3             # kArenaWords: parent id, character, dictionary state


class _Layout:
    def __init__(self, F, beam):
        self.beam = beam
        self.max_nodes = 1 + (F + 1) * beam
        self.fixed = (2 + ARRAYS * beam + 1) & ~1                      # beam_fixed_words
        self.arena_words = (ARENA * self.max_nodes + 1) & ~1            # beam_arena_words
        self.block = self.fixed + self.arena_words + 3 * 2 * self.max_nodes  # ... + 3 * beam_table_slots


def _live_set(blk, lay):
    """-> (n_beam, n_nodes, live [n_nodes] bool): the root, the beam entries' nodes and their ancestors through word 0."""
    nb, n = int(blk[0]), int(blk[1])
    arena = blk[lay.fixed:lay.fixed + ARENA * n].reshape(n, ARENA)
    live = np.zeros(n, bool)
    live[0] = True
    for v in blk[2:2 + nb]:
        v = int(v)
        while not live[v]:
            live[v] = True
            v = int(arena[v, 0])
    return nb, n, live


def _compact_host(words, B, lay):
    """The canonical compacted form of every block -> (expected words, mask of the words it specifies, live counts)."""
    want = words.copy()
    mask = np.zeros(words.shape, bool)
    mask[B * lay.block:] = True  # status words and everything behind the blocks: unchanged
    counts = []
    for u in range(B):
        o = u * lay.block
        blk = words[o:o + lay.block]
        mask[o:o + lay.fixed] = True
        if words[B * lay.block + u] != 0:  # exhausted: untouched, arena included
            mask[o:o + lay.fixed + lay.arena_words] = True
            counts.append(-1)
            continue
        nb, n, live = _live_set(blk, lay)
        new = np.cumsum(live) - 1
        L = int(live.sum())
        rows = blk[lay.fixed:lay.fixed + ARENA * n].reshape(n, ARENA)[live].copy()
        rows[1:, 0] = new[rows[1:, 0]]  # (the root's parent sentinel stays)
        out = want[o:o + lay.block]
        out[lay.fixed:lay.fixed + ARENA * L] = rows.reshape(-1)
        mask[o + lay.fixed:o + lay.fixed + ARENA * L] = True
        out[1] = L
        out[2:2 + nb] = new[blk[2:2 + nb]]
        par = blk[2 + 2 * lay.beam:2 + 2 * lay.beam + nb]
        is_id = (par >= 0) & (par < n)
        out[2 + 2 * lay.beam:2 + 2 * lay.beam + nb] = np.where(is_id, new[np.clip(par, 0, n - 1)], par)
        assert live[par[is_id]].all()
        counts.append(L)
    return want, mask, counts


class _Raw:
    """ppasr_ctc_beam_search_ws / ppasr_ctc_beam_state_compact on a state tensor of this test's own."""

    def __init__(self, B, F, V, beam):
        self.lib = _lib.load()
        self.B, self.F, self.V, self.beam = B, F, V, beam
        self.lay = _Layout(F, beam)
        self.nbytes = int(self.lib.ppasr_ctc_beam_state_bytes(B, F, beam))
        assert self.nbytes >= 4 * (B * self.lay.block + B)
        # (filled with a pattern: neither the search nor the compaction may rely on what the buffer held)
        self.buf = torch.full((self.nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
        self.total = 0

    def words(self, buf=None):
        return (self.buf if buf is None else buf).cpu().numpy().view(np.int32).copy()

    def search(self, probs, lens, init, buf=None):
        buf = self.buf if buf is None else buf
        B, T, V = probs.shape
        p = torch.from_numpy(probs).cuda()
        fl = torch.from_numpy(np.asarray(lens, np.int32)).cuda()
        nbest, L = self.beam, self.total + T
        tokens = torch.empty(B, nbest, L, dtype=torch.int32, device="cuda")
        ln = torch.empty(B, nbest, dtype=torch.int32, device="cuda")
        sc = torch.empty(B, nbest, dtype=torch.float64, device="cuda")
        need = int(self.lib.ppasr_ctc_beam_scratch_bytes(B, T, V, self.beam, 0.99, 40))
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
        _lib.check(self.lib.ppasr_ctc_beam_search_ws(p.data_ptr(), fl.data_ptr(), B, T, V, self.beam, 0.99, 40, 0, nbest, L,
                                                     tokens.data_ptr(), ln.data_ptr(), sc.data_ptr(), buf.data_ptr(),
                                                     self.nbytes, 1 if init else 0, None, 0.0, 0.0,
                                                     scratch.data_ptr() if need else None, need,
                                                     torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return tokens.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()

    def compact(self, buf=None):
        buf = self.buf if buf is None else buf
        live = np.full(self.B, -7, np.int32)
        _lib.check(self.lib.ppasr_ctc_beam_state_compact(buf.data_ptr(), self.nbytes, self.B, self.beam, 0,
                                                         live.ctypes.data_as(ctypes.c_void_p),
                                                         torch.cuda.current_stream().cuda_stream))
        return [int(v) for v in live]


# ---- 1. the kernel, word for word ---------------------------------------------------------------------------------------
# (V, beam, frame capacity, frames per chunk, chunks before the compaction, frames of each block per chunk)
CASES = {
    "three-blocks": (300, 10, 160, 16, 5, [16, 7, 0]),    # 801 / 351 / 1 ids: two tiles, one tile, the root alone (L == 1)
    "one-frame": (300, 64, 16, 1, 1, [1, 1]),             # at most 41 hypotheses: n_beam < beam
    "beam-300": (300, 300, 64, 10, 2, [10, 6]),           # about 6 000 ids: twelve tiles, live rows move across their borders
    "exhausted": (300, 10, 16, 16, 2, [16, 4]),           # block 0 runs out of arena in its 17th frame: left untouched, -1
}


@pytest.mark.parametrize("fast", ["1", "0"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_equals_host_restatement_and_the_search_continues_bit_for_bit(case, fast, monkeypatch):
    monkeypatch.setenv("PPASR_BEAM_FAST", fast)
    V, beam, F, T, k, lens = CASES[case]
    B = len(lens)
    rng = np.random.Generator(np.random.PCG64(len(case) * 131 + beam))
    raw = _Raw(B, F, V, beam)
    lay = raw.lay
    for i in range(k):
        raw.search(np.stack([_probs(rng, T, V, "peaky") for _ in range(B)]), lens, init=i == 0)
        raw.total += T
    before = raw.words()
    status = before[B * lay.block:B * lay.block + B]
    assert (status != 0).tolist() == ([True, False] if case == "exhausted" else [False] * B)
    untouched = raw.buf.clone()
    want, mask, counts = _compact_host(before, B, lay)
    print(f"{case}: n_beam {[int(before[u * lay.block]) for u in range(B)]} "
          f"n_nodes {[int(before[u * lay.block + 1]) for u in range(B)]} live {counts}")
    if case == "three-blocks":
        assert counts[2] == 1 and before[2 * lay.block + 1] == 1
    if case == "one-frame":
        assert all(before[u * lay.block] < beam for u in range(B))
    if case == "beam-300":
        assert before[1] > 8 * 512  # (many tiles)
    got_counts = raw.compact()
    after = raw.words()
    assert got_counts == counts
    for u in range(B):
        o = u * lay.block
        assert after[o] == want[o] and after[o + 1] == want[o + 1], u                          # st[0], st[1]
        assert np.array_equal(after[o + 2:o + lay.fixed], want[o + 2:o + lay.fixed]), u            # every beam array
        L = max(counts[u], 0)
        assert np.array_equal(after[o + lay.fixed:o + lay.fixed + ARENA * L], want[o + lay.fixed:o + lay.fixed + ARENA * L]), u
    assert np.array_equal(after[B * lay.block:], before[B * lay.block:])                          # status, all bytes behind
    assert np.array_equal(after[mask], want[mask])
    # a second compaction right away changes nothing
    assert raw.compact() == counts
    again = raw.words()
    assert np.array_equal(again[mask], want[mask])
    if case == "exhausted":
        return  # (block 0 has stopped consuming frames)
    # the search continues from the compacted buffer exactly as from the untouched one
    for i in range(3):
        probs = np.stack([_probs(rng, T, V, "peaky") for _ in range(B)])
        a = raw.search(probs, [T] * B, init=False)
        b = raw.search(probs, [T] * B, init=False, buf=untouched)
        raw.total += T
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (case, i)
    assert not raw.words()[B * lay.block:B * lay.block + B].any()


# ---- 2. a pool compacted after every round ------------------------------------------------------------------------------
@pytest.mark.parametrize("V,beam,cutoff_prob", [(300, 10, 0.99), (300, 300, 0.99), (4233, 300, 0.99), (300, 10, 1.0)])
def test_pool_compacted_every_round_equals_single_decoders_and_the_oracle(V, beam, cutoff_prob):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    n, rounds = 8, 20
    vocab = _vocab(V)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, cutoff_prob, 40, vocab, init_frames=rounds * 16)
    singles = _singles(n, beam, cutoff_prob, 40, vocab)
    hist, last = [[] for _ in range(n)], {}
    bytes0 = pool.arena_bytes()
    assert bytes0 > 0

    def on_round(r):
        if r:
            live = pool.compact()
            assert len(live) == n and all(v >= 1 for v in live)
            assert [pool.live_nodes(s) for s in range(n)] == live
    _drive(pool, singles, n, rounds, 100 + V + beam, V, _random_tables(V + beam, V), hist=hist, last=last, on_round=on_round)
    assert all(pool.capacity(s) == rounds * 16 for s in range(n)) and pool.arena_bytes() == bytes0  # (no block moved)
    assert not pool.status().any()
    lib = _oracle()
    for s in range(n):
        if hist[s]:
            assert pool.frames(s) == sum(c.shape[0] for c in hist[s])  # (cumulative, whatever was compacted)
            assert last[s] == _oracle_text(lib, hist[s], V, beam, cutoff_prob, 40, vocab), s


def test_pool_with_a_character_scorer_compacted_every_round(tmp_path):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, beam, n = 300, 30, 6
    vocab = _vocab(V)
    arpa = write_synthetic_arpa(str(tmp_path / "c.arpa"), vocab[2:150], order=3, seed=4)
    singles = _singles(n, beam, 0.99, 40, vocab, lm=arpa)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, scorer=singles[0]._ext_scorer, init_frames=256)
    hist, last = [[] for _ in range(n)], {}
    _drive(pool, singles, n, 12, 7, V, _random_tables(8, V), hist=hist, last=last,
           on_round=lambda r: pool.compact() if r else None)
    assert not pool.status().any() and all(pool.capacity(s) == 256 for s in range(n))
    lib, lm = _oracle(), read_arpa(arpa, vocab)
    for s in range(n):
        if hist[s]:
            ref = _oracle_lm_decode(lib, hist[s], V, beam, 0.99, 40, lm, 2.2, 4.3, 1)
            assert last[s] == "".join(vocab[i] for i in ref[0][0]), s


def test_partial_lists_and_reset():
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, beam, n = 300, 10, 6
    vocab = _vocab(V)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, init_frames=512)
    singles = _singles(n, beam, 0.99, 40, vocab)
    listed = [4, 0, 2]

    def on_round(r):
        if r == 0:
            return
        live = pool.compact(listed)
        assert [pool.live_nodes(s) for s in listed] == live and all(v >= 1 for v in live)
        assert all(pool.live_nodes(s) == 0 for s in range(n) if s not in listed)  # the unlisted ones: never compacted
        if r == 9:
            pool.reset(2)
            singles[2].reset_decoder()
            assert pool.live_nodes(2) == 0 and pool.frames(2) == 0
    _drive(pool, singles, n, 16, 61, V, _random_tables(62, V), on_round=on_round)  # (every session against its decoder)
    assert all(pool.capacity(s) == 512 for s in range(n))
    assert not pool.status().any()


# ---- 3. the automatic policy --------------------------------------------------------------------------------------------
def _host_live_count(decoder, beam):
    st = decoder._state
    lay = _Layout(st.max_frames, beam)
    blk = st.buf.cpu().numpy().view(np.int32)[:lay.block]
    return int(_live_set(blk, lay)[2].sum())


@pytest.mark.parametrize("beam", [10, 300])
def test_automatic_policy_keeps_a_long_stream_bounded(beam):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, n, rounds, T = 300, 4, 40, 16
    vocab = _vocab(V)
    rng = np.random.Generator(np.random.PCG64(71 + beam))
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, init_frames=16, compact=True)
    twin = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, init_frames=16)
    singles = _singles(n, beam, 0.99, 40, vocab, max_frames=rounds * T + 16)  # sized for the whole stream: never grow
    used, cap, n_compactions = 0, 16, 0
    for r in range(rounds):
        ids = [0] + ([1, 2, 3] if r < 2 else [])
        lens = np.array([T] + [2] * (len(ids) - 1), np.int32)
        chunks = [_probs(rng, int(L), V, "peaky") for L in lens]
        probs = np.zeros((len(ids), T, V), np.float32)
        for k, c in enumerate(chunks):
            probs[k, :c.shape[0]] = c
        # the rule of the pool's accounting, restated: compact when the chunk does not fit; keep the block if half of it
        # stays free behind the chunk, else double until it does
        moved, live = False, None
        if used + T > cap:
            live = _host_live_count(singles[0], beam)  # (session 0's own decoder holds the same search at this point)
            used = (live - 1 + beam - 1) // beam
            n_compactions += 1
            while 2 * (used + T) > cap:
                cap *= 2
                moved = True
        mine = _check_round(pool, singles, ids, probs, lens, chunks, exact=not moved)
        used += T
        if live is not None:
            assert pool.live_nodes(0) == live, r
        assert pool.capacity(0) == cap, (r, pool.capacity(0), cap)
        theirs = twin.decode_chunks(ids, torch.from_numpy(probs).cuda(), lens)
        assert [t[1] for t in theirs] == [m[1] for m in mine], r
    print(f"beam {beam}: {n_compactions} compactions, capacity {cap} frames against {twin.capacity(0)}, "
          f"{pool.arena_bytes()} bytes against {twin.arena_bytes()}")
    assert n_compactions >= 2
    assert pool.frames(0) == rounds * T and twin.capacity(0) >= 640
    assert pool.arena_bytes() < twin.arena_bytes()
    assert [pool.capacity(s) for s in (1, 2, 3)] == [16, 16, 16]
    assert [pool.live_nodes(s) for s in (1, 2, 3)] == [0, 0, 0]
    assert not pool.status().any()


# ---- 4. node tables -----------------------------------------------------------------------------------------------------
def test_word_scorer_sessions_compacted_every_round_equal_the_oracle_with_a_dictionary(tmp_path):
    """Word-based scorers keep a node table, which a compaction rebuilds.  The reference is the C oracle with a dictionary
    (it deletes dead prefixes as a compacted search does); on these inputs the single decoders agree with it too."""
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
    hist, last = [[] for _ in range(n)], {}

    def table_of(s, L):
        t = tables[s][pos[s]:pos[s] + L]
        pos[s] += t.shape[0]
        if t.shape[0] < L:  # (past the sentence: blanks)
            pad = np.full((L - t.shape[0], V), 1e-4, np.float32)
            pad[:, 0] = 1.0
            t = np.concatenate([t, pad / pad.sum(-1, keepdims=True)])
        return t

    def on_round(r):
        if r:
            assert all(v >= 1 for v in pool.compact())
        if r == 6:  # reset mid-stream: the session's node table is cleared
            pool.reset(1)
            singles[1].reset_decoder()
            pos[1] = 0
            hist[1].clear()
            assert pool.live_nodes(1) == 0
    _drive(pool, singles, n, 14, 5, V, table_of, on_round=on_round, hist=hist, last=last)
    assert not pool.status().any()
    lib, lm = _oracle(), read_arpa(arpa, WVOCAB)
    dic = _dictionary(lm)
    for s in range(n):
        if hist[s]:
            ref = _oracle_word_decode(lib, hist[s], V, beam, 0.99, 40, lm, dic, 1.9, 0.3, 1)
            assert last[s] == "".join(WVOCAB[i] for i in ref[0][0]), s


# ---- 5. refusals; BeamSearchDecoder(compact=True) -------------------------------------------------------------------------
def test_refused_compactions_change_no_session():
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    lib = _lib.load()
    V, beam, n = 300, 10, 4
    vocab = _vocab(V)
    pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, init_frames=128)
    singles = _singles(n, beam, 0.99, 40, vocab)
    tables = _random_tables(81, V)
    _drive(pool, singles, n, 3, 80, V, tables)
    stream = torch.cuda.current_stream().cuda_stream
    out = (ctypes.c_longlong * 4)(*[-5] * 4)
    for ids in ([1, 1], [0, n], [0, -1], [0, 1, 2, 3, 0]):
        rc = lib.ppasr_beam_arena_compact(pool._h, (ctypes.c_int * len(ids))(*ids), len(ids), out, stream)
        assert rc == _lib.PPASR_EINVAL, ids
    assert lib.ppasr_beam_arena_compact(pool._h, (ctypes.c_int * 1)(0), 0, out, stream) == _lib.PPASR_EINVAL
    assert list(out) == [-5] * 4 and all(pool.live_nodes(s) == 0 for s in range(n))
    assert lib.ppasr_beam_arena_live_nodes(pool._h, n) == -1 and lib.ppasr_beam_arena_live_nodes(pool._h, -1) == -1
    with pytest.raises(ValueError):
        pool.compact([2, 2])
    with pytest.raises(ValueError):
        pool.live_nodes(n)
    _drive(pool, singles, n, 4, 82, V, tables)  # every session continues as if nothing had been asked
    assert lib.ppasr_beam_arena_compact(pool._h, None, -1, None, stream) == 0  # (no list: all sessions)
    assert all(pool.live_nodes(s) >= 1 for s in range(n))
    _drive(pool, singles, n, 2, 83, V, tables)
    assert not pool.status().any()


def test_decoder_object_compacts_before_it_grows():
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchDecoder
    rng = np.random.Generator(np.random.PCG64(15))
    V, beam = 200, 8
    vocab = _vocab(V)
    p = _probs(rng, 150, V, "peaky")
    small = BeamSearchDecoder(2.2, 4.3, beam, 0.99, 40, vocab, max_stream_frames=16, compact=True)
    plain = BeamSearchDecoder(2.2, 4.3, beam, 0.99, 40, vocab, max_stream_frames=16)
    big = BeamSearchDecoder(2.2, 4.3, beam, 0.99, 40, vocab, max_stream_frames=400)
    for s in range(0, 150, 13):
        chunk = np.ascontiguousarray(p[s:s + 13])
        a = small.decode_chunk(chunk[None], np.array([chunk.shape[0]]))
        b = big.decode_chunk(chunk[None], np.array([chunk.shape[0]]))
        c = plain.decode_chunk(chunk[None], np.array([chunk.shape[0]]))
        assert a[1] == b[1] == c[1] and abs(a[0] - b[0]) < 1e-9 * max(1.0, abs(b[0])), s
    assert plain._state.max_frames >= 150
    assert small._state.buf.numel() < plain._state.buf.numel()
    assert small._state.total == 150 and small._state.frames < small._state.total
