"""Attention rescoring at end of stream: the encoder output of streaming rounds in a paged arena
(ppasr_encode_chunk_group_mem / ppasr_encode_chunk_mem), the gather of many sessions (ppasr_prob_arena_read_many), the
n-best list of a beam-search pool (ppasr_beam_sessions_nbest) and StreamPool(decoder="attention_rescoring").

Memory against the float64 oracle's forward_chunk, utt_rel at F32_BUDGET.  Worst values on the MI355X: see NOTES 41."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import decoder_cases as dc
import poison
import stream_rescore_cases as sc
from decoder_oracle import DecoderOracle
from numerics import F32_BUDGET, utt_rel
from ppasr_amd import _lib
from ppasr_amd.utils.synth import synth_vocabulary

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RESCORING = dict(beam_size=5, ctc_weight=0.5, reverse_weight=0.3, cutoff_prob=0.99, cutoff_top_n=40)
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _sd():
    return memo("sd", sc.checkpoint)


def _model():
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    return memo("model", lambda: ConformerModel(80, sc.V, streaming=True, encoder_conf=sc.ENC, state_dict=_sd(), device="cuda:0"))


def _rescorer():
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    return memo("rescorer", lambda: AttentionRescorer(_sd(), sc.V, decoder_conf=dict(sc.DEC)))


def _feats():
    return memo("feats", sc.features)


def _ref_memory():
    return memo("ref_memory", lambda: sc.oracle_memory(_sd(), _feats()))


def _arena(n_sessions, page_frames, n_pages, width=256):
    from ppasr_amd.decoders.ctc_alignment import ProbArena
    return ProbArena(n_sessions, width, page_frames=page_frames, n_pages=n_pages, device="cuda:0")


def _run_rounds(arena):
    """the five sessions' rounds on a fresh group -> (group, [(fa, fp, probs)] per round)"""
    from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
    feats, group, outs = _feats(), ConformerStreamGroup(_model(), 5), []
    for names, w, frames in sc.rounds(feats):
        x = np.concatenate([sc.windows(feats[n])[w] for n in names], 0)
        ids = [sc.SLOT[n] for n in names]
        kw = {} if arena is None else dict(memory_arena=arena, memory_frames=frames)
        outs.append(group.encode_chunks(ids, x, want_probs=True, **kw))
    torch.cuda.synchronize()
    return group, outs


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("page_frames", sc.PAGE_FRAMES)
def test_group_memory_matches_the_float64_oracle_and_changes_no_output(page_frames):
    ref = _ref_memory()
    total = sum(r.shape[0] for r in ref.values())
    arena = _arena(5, page_frames, sum(-(-r.shape[0] // page_frames) for r in ref.values()))
    _, outs = _run_rounds(arena)
    plain = memo("plain_rounds", lambda: _run_rounds(None)[1])
    for got, want in zip(outs, plain):
        for g, w in zip(got, want):
            assert _same_bytes(g, w)
    assert arena.free_pages() == 0
    worst = 0.0
    for name, slot in sc.SLOT.items():
        assert arena.frames(slot) == ref[name].shape[0], name
        err = utt_rel(arena.read(slot), ref[name])
        print(f"memory {name} page_frames={page_frames}: utt_rel {err:.3e}")
        worst = max(worst, err)
    print(f"memory worst page_frames={page_frames}: {worst:.3e} over {total} frames (budget {F32_BUDGET:.0e})")
    assert worst <= F32_BUDGET


def test_handle_memory_matches_the_oracle_and_changes_no_output():
    model, feats, ref = _model(), _feats(), _ref_memory()
    arena = _arena(2, 5, 16)
    s, twin = model.new_stream(), model.new_stream()
    for w in sc.windows(feats["B"]):
        got = s.encode_chunk(w, -16, want_probs=True, want_frames=True, memory_arena=arena, memory_session=1)
        want = twin.encode_chunk(w, -16, want_probs=True, want_frames=True)
        for g, t in zip(got, want):
            assert _same_bytes(g, t)
    assert arena.frames(1) == ref["B"].shape[0] and arena.frames(0) == 0
    err = utt_rel(arena.read(1), ref["B"])
    print(f"handle memory B: utt_rel {err:.3e}")
    assert err <= F32_BUDGET


def test_mem_refusals_change_nothing():
    from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
    model, feats = _model(), _feats()
    x = np.concatenate([sc.windows(feats[n])[0] for n in ("A", "B", "C")], 0)
    group, twin = ConformerStreamGroup(model, 3), ConformerStreamGroup(model, 3)
    small = _arena(3, 5, 8)  # the round needs 3 x ceil(16 / 5) = 12 pages
    with pytest.raises(_lib.PPASRHipError) as e:
        group.encode_chunks([0, 1, 2], x, want_probs=True, memory_arena=small)
    assert e.value.status == _lib.PPASR_ENOSPACE
    assert small.free_pages() == 8 and all(small.frames(i) == 0 and group.offset(i) == 0 for i in range(3))
    for bad, status in ((_arena(3, 5, 12, width=67), _lib.PPASR_EINVAL), (_arena(2, 5, 12), _lib.PPASR_EINVAL)):
        with pytest.raises(_lib.PPASRHipError) as e:
            group.encode_chunks([0, 1, 2], x, memory_arena=bad)
        assert e.value.status == status
    big = _arena(3, 5, 12)
    for frames in ([16, 17, 16], [16, -1, 16]):
        with pytest.raises(_lib.PPASRHipError) as e:
            group.encode_chunks([0, 1, 2], x, memory_arena=big, memory_frames=frames)
        assert e.value.status == _lib.PPASR_EINVAL
    assert big.free_pages() == 12 and all(group.offset(i) == 0 for i in range(3))
    # the refused rounds left the group where its twin is: the same round on a large enough arena gives the twin's result
    got = group.encode_chunks([0, 1, 2], x, want_probs=True, memory_arena=big)
    want = twin.encode_chunks([0, 1, 2], x, want_probs=True)
    for g, w in zip(got, want):
        assert _same_bytes(g, w)
    assert big.free_pages() == 0


def _routes():
    spec = importlib.util.spec_from_file_location("make_stream_routes", os.path.join(HERE, "golden", "make_stream_routes.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


@pytest.mark.parametrize("family", ["efficient", "squeezeformer"])
def test_other_families_are_refused_and_keep_their_state(family):
    """Squeezeformer and Efficient-Conformer groups and handles take no memory arena: PPASR_EUNSUPPORTED
    before any device work, the group and the arena as they were, and the plain round still runs."""
    from ppasr_amd.utils.synth import synth_features
    mk = _routes()
    model = mk._model(family)
    x, _ = synth_features(2, 67, seed=3)
    group, twin, arena = mk._group(family, model, 2), mk._group(family, model, 2), _arena(2, 5, 16)
    with pytest.raises(_lib.PPASRHipError) as e:
        group.encode_chunks([0, 1], x, want_probs=True, memory_arena=arena)
    assert e.value.status == _lib.PPASR_EUNSUPPORTED
    with pytest.raises(_lib.PPASRHipError) as e:
        model.new_stream().encode_chunk(x[:1], -16, memory_arena=arena)
    assert e.value.status == _lib.PPASR_EUNSUPPORTED
    assert arena.free_pages() == 16 and group.offset(0) == 0 and group.offset(1) == 0
    for g, t in zip(group.encode_chunks([0, 1], x, want_probs=True), twin.encode_chunks([0, 1], x, want_probs=True)):
        assert _same_bytes(g, t)


@pytest.mark.parametrize("case", ["group1-67", "group3-67"])
def test_an_arena_adds_exactly_one_launch(case):
    from ppasr_amd._lib import kernel_profile
    from ppasr_amd.utils.synth import synth_features
    mk = _routes()
    with open(os.path.join(HERE, "golden", "stream_routes.json")) as f:
        gold = json.load(f)[f"conformer/{case}"]
    assert mk.record("conformer", case) == gold  # without an arena: the fixture
    _, sessions, frames, _ = mk.CASES[case]
    model = mk._model("conformer")
    x, _ = synth_features(len(sessions), 2 * frames, seed=700 + frames)
    group, arena = mk._group("conformer", model, 4), _arena(4, 5, 64)
    step = lambda r: group.encode_chunks(sessions, x[:, r * frames:(r + 1) * frames], want_probs=True, memory_arena=arena)
    step(0)
    with kernel_profile(max_entries=512) as kp:
        step(1)
    torch.cuda.synchronize()
    got = {name: n for name, (_ms, n) in kp.kernels.items()}
    extra = {k: got.get(k, 0) - gold.get(k, 0) for k in set(got) | set(gold) if got.get(k, 0) != gold.get(k, 0)}
    assert len(extra) == 1 and list(extra.values()) == [1] and "k_memory_append" in list(extra)[0], extra


def test_read_many_equals_per_session_reads():
    arena = _arena(5, 5, 40)
    _run_rounds(arena)
    lib = _lib.load()
    ids = [3, 0, 4, 1]
    longest = max(arena.frames(i) for i in ids)
    for Tp in (None, longest + 3):
        dense, lens = arena.read_many(ids, Tp)
        assert lens.cpu().tolist() == [arena.frames(i) for i in ids]
        for k, i in enumerate(ids):
            n = arena.frames(i)
            assert _same_bytes(dense[k, :n], arena.read(i))
            assert not dense[k, n:].view(torch.int32).any()
    # what the destination held changes no result
    ref_dense, ref_lens = arena.read_many(ids, longest + 3)
    for byte in (0xFF, 0x7F):
        dense, lens = torch.empty_like(ref_dense), torch.empty_like(ref_lens)
        poison.fill(dense, byte)
        poison.fill(lens, byte)
        c_ids = (ctypes.c_int * len(ids))(*ids)
        _lib.check(lib.ppasr_prob_arena_read_many(arena._h, c_ids, len(ids), longest + 3, dense.data_ptr(), lens.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
        assert _same_bytes(dense, ref_dense) and _same_bytes(lens, ref_lens)
    stream = torch.cuda.current_stream().cuda_stream
    d, l = ref_dense.data_ptr(), ref_lens.data_ptr()
    for bad_ids, n, Tp, dp, lp in (([0, 1], 2, longest - 1, d, l), ([0, 0], 2, longest, d, l), ([0, 5], 2, longest, d, l),
                                   ([0], 0, longest, d, l), ([0, 1], 2, longest, None, l), ([0, 1], 2, longest, d, None)):
        rc = lib.ppasr_prob_arena_read_many(arena._h, (ctypes.c_int * len(bad_ids))(*bad_ids), n, Tp, dp, lp, stream)
        assert rc == _lib.PPASR_EINVAL, (bad_ids, n, Tp)
    with pytest.raises(ValueError):
        arena.read_many([0, 1], longest - 1)


@pytest.mark.parametrize("beam", [5, 8])
def test_pool_nbest_is_the_search_on_the_whole_table_and_leaves_the_pool_alone(beam):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions, beam_search_ids
    rng = np.random.Generator(np.random.PCG64(11))
    lens = [37, 23, 30]
    logits = 3.0 * rng.standard_normal((3, 37, sc.V)).astype(np.float32)
    probs = torch.softmax(torch.from_numpy(logits), -1).to("cuda:0")
    vocab = synth_vocabulary(sc.V)
    mk = lambda: BeamSearchSessions(4, 0.0, 0.0, beam, 0.99, 40, vocab, init_frames=16)
    pool, twin = mk(), mk()
    ids = [2, 0, 3]
    for p in (pool, twin):
        for a in range(0, 30, 10):
            p.decode_chunks(ids, probs[:, a:a + 10], lens=[min(max(n - a, 0), 10) for n in lens])
    fl = torch.tensor([min(n, 30) for n in lens], dtype=torch.int32)
    for K in (1, 3, beam):
        rt, rl, rs, _ = beam_search_ids(probs[:, :30], beam, 0.99, 40, 0, frame_lens=fl, nbest=K)
        tokens, hl, scores = pool.nbest(ids, K, max_tokens=rt.shape[2])
        assert torch.equal(tokens.cpu(), rt.cpu()) and torch.equal(hl.cpu(), rl.cpu())
        assert _same_bytes(scores.cpu(), rs.cpu())
    got = pool.decode_chunks(ids, probs[:, 30:37], lens=[min(max(n - 30, 0), 7) for n in lens], return_ids=True)
    want = twin.decode_chunks(ids, probs[:, 30:37], lens=[min(max(n - 30, 0), 7) for n in lens], return_ids=True)
    assert got == want
    assert [pool.frames(i) for i in ids] == [twin.frames(i) for i in ids]
    for K in (0, beam + 1):
        with pytest.raises(ValueError):
            pool.nbest(ids, K)
    lib = _lib.load()
    t, l, s = pool.nbest(ids, 1, max_tokens=4)
    rc = lib.ppasr_beam_sessions_nbest(pool._h, (ctypes.c_int * 3)(*ids), 3, beam + 1, 4, t.data_ptr(), l.data_ptr(), s.data_ptr(),
                                   None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.PPASR_EINVAL


# ---- StreamPool(decoder="attention_rescoring") ----
SECONDS = dict(A=1.45, B=1.9, C=0.9)


def _pool(decoder="attention_rescoring", **kw):
    from ppasr_amd.serving import StreamPool
    pre = dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True, target_dB=-20)
    if decoder == "attention_rescoring":
        kw = dict(dict(rescorer=_rescorer(), decoder_conf=dict(RESCORING), page_frames=5), **kw)
    return StreamPool(_model(), synth_vocabulary(sc.V), 3, preprocess_conf=pre, decoder=decoder, **kw)


def _feed(pool, partial=None):
    """the three sessions' audio in 0.4 s packets, a step after every packet -> per-session list of round results"""
    seen = {0: [], 1: [], 2: []}
    wavs = [sc.audio(SECONDS[n], seed=5 + k) for k, n in enumerate("ABC")]
    for a in range(0, max(len(w) for w in wavs), 6400):
        for i, w in enumerate(wavs):
            if a < len(w):
                pool.feed(i, w[a:a + 6400])
        for i, r in pool.step().items():
            seen[i].append(r)
    return seen


def test_round_results_are_a_ctc_beam_search_pools():
    bs = {k: v for k, v in RESCORING.items() if k in ("beam_size", "cutoff_prob", "cutoff_top_n")}
    got, want = _feed(_pool()), _feed(_pool("ctc_beam_search", decoder_conf=bs))
    assert got == want and all(got[i] for i in got)


def test_finish_many_totals_match_float64_and_equal_single_finishes():
    pool, twin = _pool(), _pool()
    _feed(pool)
    _feed(twin)
    batch = pool.finish_many([0, 1, 2])
    single = [twin.finish(i) for i in range(3)]
    assert batch == single  # (every packed row goes through the same arithmetic whatever else the call holds)
    tokens, hl, scores = [t.cpu().numpy() for t in pool.beam.nbest([0, 1, 2], RESCORING["beam_size"], max_tokens=64)]
    memory, mlens = pool.memory.read_many([0, 1, 2])
    oracle = DecoderOracle(_sd(), sc.V, *sc.BLOCKS, dtype=torch.float64)
    ref = oracle.rescore(memory.cpu().numpy(), mlens.cpu().numpy(), tokens, hl, scores, RESCORING["ctc_weight"],
                         RESCORING["reverse_weight"])
    vocab = synth_vocabulary(sc.V)
    case = dict(L=tokens.shape[2] + 1)
    for b in range(3):
        tol = dc.score_tol(case, ref, b, 2e-5)
        margin = dc.top2_margin(ref["total"][b])
        k = int(ref["best"][b])
        print(f"session {b}: total {batch[b]['score']:.9f} ref {ref['total'][b, k]:.9f} tol {tol:.3e} margin {margin:.3e}")
        assert batch[b]["rescored"] is True and set(batch[b]) == {"text", "score", "rescored"}
        assert margin > dc.MARGIN_FACTOR * tol, (b, margin, tol)
        assert batch[b]["text"] == "".join(vocab[i] for i in tokens[b, k, :hl[b, k]])
        assert abs(batch[b]["score"] - ref["total"][b, k]) <= tol, (b, batch[b]["score"], ref["total"][b, k], tol)


def test_overflow_keeps_the_ctc_result_and_reset_reuses_the_pages():
    small = _pool(memory_seconds=0.6)  # 15 frames: 3 pages of 5 per session, the first round's 16 frames do not fit
    seen = _feed(small)
    out = small.finish(1)
    assert out["rescored"] is False and out["memory_overflow"] is True
    last = small.sessions[1].result
    assert (out["text"], out["score"]) == (last["text"], last["score"])
    assert small.memory.free_pages() == 9
    # page reuse: a new stream in a used slot gives what a fresh pool gives
    pool, fresh = _pool(), _pool()
    _feed(pool)
    first = pool.finish_many([0, 1, 2])
    free = pool.memory.free_pages()
    for i in range(3):
        pool.reset(i)
    assert pool.memory.free_pages() > free and pool.memory.free_pages() == pool.memory.n_pages
    _feed(pool)
    _feed(fresh)
    assert pool.finish_many([2, 0, 1]) == fresh.finish_many([2, 0, 1])
    assert pool.finish_many([0, 1, 2]) == first
