"""No decoder or fbank result depends on what the state, scratch and output buffers held on entry (tests/poison.py):
the greedy decoder, the prefix beam search (one-shot, chunked through one state buffer, grown past its capacity, with
HBM element lists, with a character and a word scorer), the beam-search session pool across reset(slot), and the fbank
front end -- n-best tokens, lengths and scores / features byte for byte against the same calls on zero-filled buffers.

``stale``: the state buffer under test first carries ANOTHER search (other probabilities, the same beam) and is then
started over with init_state = 1; the HBM scratch and the pool's blocks and workspace likewise.  The growth cases add
nothing under ``stale`` about the GROWN buffer: it is a new allocation whose contents the test does not control (what
the allocator hands back), so its foreign contents are tested by the 0xFF / 0x7F patterns only.

Defined regions (include/ppasr_hip.h): all of tokens (-1 padded; the rows of hypotheses that do not exist are -1 too),
lens (-1 = no such hypothesis) and scores (0 for such a hypothesis)."""
import numpy as np
import pytest
import torch

import numerics as nm
import poison
from lm_util import write_synthetic_arpa
from test_ctc_beam_gpu import _probs
from test_ctc_beam_wordlm_gpu import VOCAB as WVOCAB, WORDS, _spoken_probs
from test_fbank_gpu import _audio

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()


def _vocab(V):
    return ["<blank>"] + [chr(0x4E00 + i) for i in range(V - 1)]


def _batch(seed, B, T, V, kind="peaky"):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(np.stack([_probs(rng, T, V, kind) for _ in range(B)])).cuda()


def _defined(tokens, lens, scores):
    """an n-best result is defined in full: a hypothesis that does not exist has lens -1, score 0 and -1 tokens"""
    return {"tokens": tokens, "lens": lens, "scores": scores}


# ---- greedy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("frame_lens", [None, [50, 1, 0, 37]], ids=["all-rows", "lens-50-1-0-37"])
def test_ctc_greedy(frame_lens, pattern, monkeypatch):
    from ppasr_amd.decoders.ctc_greedy_decoder import greedy_decode_ids
    p = _batch(5, 4, 50, 131)

    def run(s):
        if s.stale:
            greedy_decode_ids(_batch(6, 6, 80, 131), None)
        tokens, n, score, fa, fp = greedy_decode_ids(p, frame_lens)
        torch.cuda.synchronize()
        outs = {"tokens": tokens, "n_tokens": n, "score": score}
        if frame_lens is None:  # (the per-frame stage is the call's workspace: every row is written when every row is decoded)
            outs.update(frame_argmax=fa, frame_maxprob=fp)
        return outs, None

    poison.check(f"ctc_greedy {frame_lens}", run, pattern, monkeypatch, MEMO)


# ---- prefix beam search ------------------------------------------------------------------------------------------------
def _search(s, bsd, p, beam, nbest, frame_lens, chunks, cutoff=(0.99, 40), scorer=None, other=None, max_frames=None,
            growable=False):
    """One search over `p` in `chunks` calls on one state buffer; stale: `other` is searched on the same buffer first."""
    B, T, _ = p.shape
    dev = p.device
    if s.pattern == "zero":
        bsd._scratch.clear()  # the clean reference starts without kept scratch, like a fresh process
    st = bsd._BeamState(B, max_frames or T, beam, dev)
    st.growable = growable
    if s.stale:
        o = other if other is not None else p.flip(1)
        bsd.beam_search_ids(o[:, :st.max_frames], beam, cutoff[0], cutoff[1], 0, nbest=nbest, state=st, ext_scorer=scorer)
        st.fresh, st.frames = True, 0
        s.scratch([st.buf, bsd])
    outs = {}
    step = (T + chunks - 1) // chunks
    # (stale and growing: the grown buffer is a new allocation, nothing of this test's making is in it)
    watch = not (s.stale and growable)
    for k in range(chunks):
        fl = None if frame_lens is None else np.clip(np.asarray(frame_lens) - k * step, 0, min(step, T - k * step))
        if not s.stale:
            s.scratch(bsd)  # (the state buffer carries the search between chunks: filled at allocation only)
        tokens, lens, scores, st = bsd.beam_search_ids(p[:, k * step:(k + 1) * step], beam, cutoff[0], cutoff[1], 0,
                                                       frame_lens=fl, nbest=nbest, state=st, ext_scorer=scorer)
        if watch:
            s.observe([st.buf, bsd], f"chunk {k}")
        torch.cuda.synchronize()
        outs.update({f"{k}/{n}": v for n, v in _defined(tokens, lens, scores).items()})
    return outs, ([st.buf, bsd] if watch else None)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("chunks", [1, 3], ids=["one-shot", "chunked"])
@pytest.mark.parametrize("beam,nbest", [(10, 10), (16, 4), (300, 5)])
def test_beam_search(beam, nbest, chunks, pattern, monkeypatch):
    """a batch that holds a 0-frame and a 1-frame utterance"""
    from ppasr_amd.decoders import beam_search_decoder as bsd
    p, other = _batch(beam, 4, 42, 131), _batch(beam + 1, 4, 42, 131, "flat")

    def run(s):
        return _search(s, bsd, p, beam, nbest, [42, 1, 0, 29], chunks, other=other)

    poison.check(f"beam_search beam={beam} chunks={chunks}", run, pattern, monkeypatch, MEMO)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("beam", [10, 300])
def test_beam_search_grows_past_max_stream_frames(beam, pattern, monkeypatch):
    """three chunks of 16 frames into a state sized for 16: ppasr_ctc_beam_state_grow moves the search into a new
    torch.empty buffer twice"""
    from ppasr_amd.decoders import beam_search_decoder as bsd
    p = _batch(beam + 7, 2, 48, 131)

    def run(s):
        return _search(s, bsd, p, beam, 3, None, 3, max_frames=16, growable=True)

    poison.check(f"beam_search grow beam={beam}", run, pattern, monkeypatch, MEMO)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("cutoff_prob", [0.99, 1.0])
@pytest.mark.parametrize("beam", [10, 300])
def test_beam_search_large_vocabulary(beam, cutoff_prob, pattern, monkeypatch):
    """V = 4233; cutoff_prob = 1.0 keeps every character of every frame: pruning records and element lists in HBM scratch"""
    from ppasr_amd.decoders import beam_search_decoder as bsd
    p, other = _batch(3, 2, 14, 4233), _batch(4, 2, 14, 4233, "flat")

    def run(s):
        outs, owner = _search(s, bsd, p, beam, 3, [14, 9], 2, cutoff=(cutoff_prob, 40), other=other)
        if cutoff_prob >= 1.0:
            assert bsd._scratch, "the unpruned search must go through the HBM scratch"
        return outs, owner

    poison.check(f"beam_search V=4233 beam={beam} cutoff={cutoff_prob}", run, pattern, monkeypatch, MEMO)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("kind", ["char", "word"])
def test_beam_search_with_scorer(kind, pattern, monkeypatch, tmp_path):
    from ppasr_amd.decoders import beam_search_decoder as bsd
    rng = np.random.Generator(np.random.PCG64(17))
    if kind == "char":
        vocab = _vocab(200)
        arpa = write_synthetic_arpa(str(tmp_path / "c.arpa"), vocab[2:150], order=3, seed=4)
        p, other, lens, alpha, beta, beam = _batch(8, 3, 40, 200, "flat"), _batch(9, 3, 40, 200), [40, 1, 0], 2.2, 4.3, 16
    else:  # word-based scorers run with node tables in the state buffer
        vocab = WVOCAB
        arpa = write_synthetic_arpa(str(tmp_path / "w.arpa"), WORDS, order=3, n_sent=300, sent_len=8, seed=2)
        tabs = [_spoken_probs(rng, sent, len(vocab)) for sent in (["the", "cat", "sat"], ["where", "is", "the", "hat"], ["we"])]
        T = max(t.shape[0] for t in tabs)
        batch = np.full((3, T, len(vocab)), 1.0 / len(vocab), np.float32)
        for b, t in enumerate(tabs):
            batch[b, :t.shape[0]] = t
        p, lens, alpha, beta, beam = torch.from_numpy(batch).cuda(), [t.shape[0] for t in tabs], 1.9, 0.3, 30
        other = p.flip(0).contiguous()

    def run(s):
        scorer = bsd.Scorer(alpha, beta, arpa, vocab)
        return _search(s, bsd, p, beam, 3, lens, 2, scorer=scorer, other=other)

    poison.check(f"beam_search {kind} scorer", run, pattern, monkeypatch, MEMO)


# ---- session pool ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("cutoff_prob", [0.99, 1.0])
def test_beam_pool_across_reset(cutoff_prob, pattern, monkeypatch):
    """Three sessions, one of them reset mid-stream and started over (in every pattern); stale: every block first carries
    another, longer stream.  The clean reference runs the restarted session in a slot nothing used before."""
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V, beam = 300, 20
    vocab = _vocab(V)
    tabs = _batch(31, 3, 16 * 5, V).cpu()
    other = _batch(32, 3, 16 * 7, V, "flat").cpu()

    def run(s):
        clean = s.pattern == "zero"
        pool = BeamSearchSessions(4 if clean else 3, 2.2, 4.3, beam, cutoff_prob, 40, vocab, init_frames=64)
        if s.stale:
            for k in range(7):
                pool.decode_chunks([0, 1, 2], other[:, 16 * k:16 * k + 16])
            pool.reset()
        text, scores = [], []
        for k in range(5):
            if k == 2 and not clean:
                pool.reset(1)
            mid = tabs[1, 16 * k:16 * k + 16] if k < 2 else tabs[0, 16 * (k - 2):16 * (k - 2) + 16]
            chunk = torch.stack([tabs[0, 16 * k:16 * k + 16], mid, tabs[2, 16 * k:16 * k + 16]])
            ids = [0, 3 if clean and k >= 2 else 1, 2] if k != 3 else [2, 0]  # (round 3 lists a subset)
            s.scratch(pool)
            got = pool.decode_chunks(ids, chunk if k != 3 else chunk[[2, 0]], lens=[16, 11, 16] if k == 1 else None)
            if kept := poison.kept_scratch(pool):
                s.observe(kept, f"round {k}")
            scores += [g[0] for g in got]
            text += [g[1] for g in got]
        assert not pool.status().any()
        outs = {"scores": torch.tensor(scores, dtype=torch.float64),
                "text": torch.tensor(list("\n".join(text).encode("utf-8")), dtype=torch.uint8)}
        return outs, (poison.kept_scratch(pool) or None)

    poison.check(f"beam_pool cutoff={cutoff_prob}", run, pattern, monkeypatch, MEMO)


# ---- fbank -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("use_db", [True, False])
def test_fbank(use_db, pattern, monkeypatch):
    """two sample counts, one of them not a multiple of the 8192-sample chunk of the gain's sum of squares"""
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    waves = [_audio(2.0, seed=3)[:16384], _audio(2.0, seed=4)[:11825]]  # 2 x 8192 samples; 8192 + 3633

    def run(s):
        f = AudioFeaturizer(n_mels=80, sample_rate=16000, use_dB_normalization=use_db, target_dB=-20)
        if s.stale:
            f.featurize_device(_audio(2.5, seed=5))
        outs = {}
        for i, w in enumerate(waves):
            s.scratch(f)
            outs[f"{i}/feats"] = f.featurize_device(w)
            s.observe(f, f"wave {i}")
            if use_db:
                outs[f"{i}/gain"] = torch.tensor([f.last_gain], dtype=torch.float64)
        return outs, f

    poison.check(f"fbank use_db={use_db}", run, pattern, monkeypatch, MEMO)
