"""Token timestamps of streams end to end: StreamPool(timestamps=True) and PPASRPredictor.predict_stream(timestamps=True) on
a 2-block synthetic Conformer with V = 120 (the builders of test_predict_timestamps_gpu.py), one Efficient-Conformer and
one DeepSpeech2 pool.  Three sessions of 1.0, 2.3 and 3.1 s are fed in interleaved 0.32 s packets.

Everything is exact.  Texts and scores are those of a pool without timestamps; the table a pool keeps is, word for word,
what the encoder rounds returned; and the timestamps are ``ctc_align_ids`` of the session's ids on that table, turned into
seconds by PPASRPredictor._token_times' rule (frame x total_subsampling x 10 ms, the end clipped to the audio fed)."""
import numpy as np
import pytest
import torch

import numerics as nm
from test_predict_timestamps_gpu import _audio
from ppasr_amd import _lib
from ppasr_amd.decoders import ctc_alignment as ca
from ppasr_amd.utils.synth import (conformer_state_dict, deepspeech2_state_dict, efficient_conformer_state_dict,
                                   synth_vocabulary)

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
V = 120
VOCAB = synth_vocabulary(V)
SECONDS = (1.0, 2.3, 3.1)
PACKET = int(0.32 * 16000) * 2  # bytes of PCM16
PROBE = 5                       # the packet behind which the partial hypotheses are aligned (1.92 s fed)
BEAM_CONF = dict(alpha=2.2, beta=4.3, beam_size=10, num_processes=10, cutoff_prob=0.99, cutoff_top_n=40,
                 language_model_path=None)


def _cfg(use_model, decoder):
    enc = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
    if use_model == "deepspeech2":
        enc = dict(num_rnn_layers=2, rnn_size=1024, use_gru=False)
    elif use_model == "efficient_conformer":
        enc = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                   cnn_module_norm="layer_norm", efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1],
                                                                     group_size=3, stride_kernel=True))
    return dict(encoder_conf=enc,
                preprocess_conf=dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True,
                                     target_dB=-20),
                ctc_beam_search_decoder_conf=dict(BEAM_CONF), use_model=use_model, streaming=True, decoder=decoder,
                metrics_type="cer")


def predictor(use_model="conformer", decoder="ctc_greedy"):
    def make():
        from ppasr_amd.predict import PPASRPredictor
        if use_model == "deepspeech2":
            sd = deepspeech2_state_dict(vocab_size=V, num_rnn_layers=2, streaming=True, seed=7)
        elif use_model == "efficient_conformer":
            sd = efficient_conformer_state_dict(vocab_size=V, num_blocks=4, seed=5, stride_layer_idx=1, group_layer_idx=(0, 1))
        else:
            sd = conformer_state_dict(vocab_size=V, num_blocks=2, seed=3)
        return PPASRPredictor(configs=_cfg(use_model, decoder), state_dict=sd, vocab_list=VOCAB, warmup=False)
    return MEMO.get(("predictor", use_model, decoder), make)


def pcms():
    return MEMO.get("pcm", lambda: [(np.clip(_audio(s, seed=40 + i), -1, 1) * 32767).astype(np.int16).tobytes()
                                    for i, s in enumerate(SECONDS)])


def make_pool(use_model, decoder, n=3, group=None, **kw):
    from ppasr_amd.serving import StreamPool
    p = predictor(use_model, "ctc_greedy")
    if decoder == "ctc_beam_search":
        kw["decoder_conf"] = dict(BEAM_CONF)
    model = p.predictor.model
    return StreamPool(model, VOCAB, n_sessions=n, preprocess_conf=_cfg(use_model, decoder)["preprocess_conf"], decoder=decoder,
                      group=group(model, n) if group else None, **kw)


def watch(pool):
    """-> per session the probability chunks the encoder rounds return, captured behind the pool's own call"""
    chunks = [[] for _ in pool.sessions]
    encode = pool.group.encode_chunks

    def spy(ids, x, want_probs=False):
        out = encode(ids, x, want_probs=want_probs)
        if want_probs:
            for k, s in enumerate(ids):
                chunks[s].append(out[2][k].clone())
        return out
    pool.group.encode_chunks = spy
    return chunks


def drive(pool, audio, sessions=None, chunks=None):
    """Interleaved 0.32 s packets, a step behind every packet row, then finish in session order.
    -> dict(log: every result a step or a finish gave, final: finish's dicts, mid: what was known behind packet PROBE)"""
    sessions = list(range(len(audio))) if sessions is None else sessions
    log, mid = [], {}
    for i in range(max(len(a) for a in audio) // PACKET + 1):
        for s, a in zip(sessions, audio):
            if i * PACKET < len(a):
                pool.feed(s, a[i * PACKET:(i + 1) * PACKET])
        log += [(s, r["text"], r["score"]) for s, r in sorted(pool.step().items())]
        if i == PROBE and pool.with_timestamps:
            for s, a in zip(sessions, audio):
                if pool.sessions[s].result is not None:
                    mid[s] = dict(stamps=pool.timestamps(s), text=pool.sessions[s].result["text"],
                                  fed=min(len(a), (i + 1) * PACKET) / 2 / 16000.0,
                                  frames=None if not chunks else sum(int(c.shape[0]) for c in chunks[s]))
    final = [pool.finish(s) for s in sessions]
    log += [(s, r["text"], r["score"]) for s, r in zip(sessions, final)]
    return dict(log=log, final=final, mid=mid)


def plain_run(use_model, decoder, group=None):
    return MEMO.get(("plain", use_model, decoder), lambda: drive(make_pool(use_model, decoder, group=group), pcms()))


def beam_run(use_model="conformer", group=None):
    """the beam-search pool with timestamps, watched: its results, its rounds' tables, and the pool itself"""
    def make():
        pool = make_pool(use_model, "ctc_beam_search", group=group, timestamps=True)
        chunks = watch(pool)
        run = drive(pool, pcms(), chunks=chunks)
        run.update(pool=pool, tables=[torch.cat(c) for c in chunks],
                   kept=[pool.session_probs(s).clone() for s in range(3)])
        return run
    return MEMO.get(("beam", use_model), make)


def expected(table, text, greedy, step, fed):
    """ctc_align_ids of the text's ids on a dense table [T, V], in seconds"""
    ids = ca.text_to_ids(text, VOCAB, space_token=greedy)
    n = len(ids)
    if n == 0:
        return []
    out = ca.ctc_align_ids(table[None], np.asarray(ids, np.int32).reshape(1, n), np.asarray([n], np.int32))
    assert int(out["status"][0]) == 0
    b, e, c = (out[k][0].cpu().numpy() for k in ("begin", "end", "conf"))
    return [{"text": VOCAB[i].replace("<space>", " ") if greedy else VOCAB[i], "start": int(b[l]) * step,
             "end": min(int(e[l]) * step, fed), "score": float(c[l])} for l, i in enumerate(ids)]


def check_entries(entries, text, fed):
    assert "".join(e["text"] for e in entries) == text  # one entry per token
    last = 0.0
    for e in entries:
        assert set(e) == {"text", "start", "end", "score"}
        assert last <= e["start"] < e["end"] <= fed + 1e-12, (e, last, fed)  # ordered, not overlapping, inside the audio
        last = e["end"]
        assert 0.0 < e["score"] <= 1.0


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def check_pool_run(run, plain, tables, greedy, step):
    # (i) the texts and scores of every step and finish are those of a pool without timestamps
    assert run["log"] == plain["log"]
    assert len({s for s, _, _ in run["log"]}) == 3 and any(t for _, t, _ in run["log"])
    for s, (got, want) in enumerate(zip(run["final"], plain["final"])):
        assert set(want) == {"text", "score"} and set(got) == {"text", "score", "timestamps"}
        fed = len(pcms()[s]) / 2 / 16000.0
        # (iii) the final list is the alignment of the final ids on the session's dense table
        assert got["timestamps"] == expected(tables[s], got["text"], greedy, step, fed), s
        check_entries(got["timestamps"], got["text"], fed)
        print(f"[stream timestamps] session {s}: {len(got['timestamps'])} tokens in {tables[s].shape[0]} frames, {fed:.2f} s")
    assert sum(len(r["timestamps"]) for r in run["final"]) > 0


# ---- the pool, both decoders ---------------------------------------------------------------------------------------------
def test_beam_search_pool():
    run, plain = beam_run(), plain_run("conformer", "ctc_beam_search")
    pool = run["pool"]
    assert pool.arena is not None and pool.frame_seconds == pytest.approx(0.04)
    # (ii) the table the pool kept is what the encoder rounds returned, word for word
    for s in range(3):
        assert np.array_equal(bits(run["kept"][s]), bits(run["tables"][s])), s
        assert run["tables"][s].shape[0] == pool.arena.frames(s) > 0
    check_pool_run(run, plain, run["tables"], False, 0.04)
    # (iv) mid-stream: the partial ids on the table so far
    assert sorted(run["mid"]) == [0, 1, 2]
    for s, m in run["mid"].items():
        assert 0 < m["frames"] <= run["tables"][s].shape[0]
        assert m["stamps"] == expected(run["tables"][s][:m["frames"]], m["text"], False, 0.04, m["fed"]), s
        check_entries(m["stamps"], m["text"], m["fed"])
    assert any(m["frames"] < run["tables"][s].shape[0] and m["stamps"] for s, m in run["mid"].items())


def test_greedy_pool_needs_no_table():
    plain = plain_run("conformer", "ctc_greedy")
    pool = make_pool("conformer", "ctc_greedy", timestamps=True)
    assert pool.arena is None and pool.beam is None
    run = drive(pool, pcms())
    tables = beam_run()["tables"]  # the same model, the same packets: the same rounds
    check_pool_run(run, plain, tables, True, 0.04)
    beam_mid = beam_run()["mid"]
    for s, m in run["mid"].items():
        assert m["stamps"] == expected(tables[s][:beam_mid[s]["frames"]], m["text"], True, 0.04, m["fed"]), s
    with pytest.raises(ValueError):
        pool.session_probs(0)
    with pytest.raises(ValueError):
        make_pool("conformer", "ctc_greedy").timestamps(0)


# ---- (v) reset -----------------------------------------------------------------------------------------------------------
def test_reset_returns_the_pages_and_the_slot_starts_again():
    first = beam_run()
    pool = make_pool("conformer", "ctc_beam_search", timestamps=True)
    total = pool.arena.free_pages()
    assert total == 3 * pool.session_pages == 3 * 47  # 30 s at 25 frames a second in pages of 16
    audio = pcms()
    drive(pool, [audio[1], audio[2]], sessions=[0, 2])
    assert pool.arena.free_pages() < total
    held2 = -(-pool.arena.frames(2) // 16)
    pool.reset(0)
    assert pool.arena.frames(0) == 0 and pool.arena.free_pages() == total - held2
    pool.reset(2)
    assert pool.arena.free_pages() == total
    assert pool.timestamps(0) == []
    # a second utterance on the slots: as on a fresh pool
    again = drive(pool, audio)
    assert again["log"] == first["log"] and again["final"] == first["final"]
    for s in range(3):
        assert np.array_equal(bits(pool.session_probs(s)), bits(first["tables"][s]))


# ---- (vi) overflow -------------------------------------------------------------------------------------------------------
def test_a_session_that_outgrows_its_table_keeps_its_text():
    first = beam_run()
    frames = [t.shape[0] for t in first["tables"]]
    assert frames[1] <= 64 < frames[2]  # 2.56 s = 64 frames = 4 pages hold the two shorter sessions only
    pool = make_pool("conformer", "ctc_beam_search", timestamps=True, table_seconds=2.56)
    assert pool.session_pages == 4 and pool.arena.free_pages() == 12
    run = drive(pool, pcms())
    assert run["log"] == first["log"]  # no text or score moves, and nothing is raised inside a round
    for s in (0, 1):
        assert run["final"][s] == first["final"][s]
    assert run["final"][2] == dict(text=first["final"][2]["text"], score=first["final"][2]["score"], timestamps=None,
                                   table_overflow=True)
    assert pool.timestamps(2) is None and pool.arena.frames(2) == 0 and tuple(pool.session_probs(2).shape) == (0, V)
    pool.reset(2)
    assert pool.timestamps(2) == [] and pool.arena.free_pages() == 12 - sum(-(-f // 16) for f in frames[:2])


# ---- launches ------------------------------------------------------------------------------------------------------------
def one_round_launches(timestamps, n):
    pool = make_pool("conformer", "ctc_beam_search", timestamps=timestamps)
    audio = pcms()[2]
    for s in range(n):
        pool.feed(s, audio[:int(0.8 * 16000) * 2])  # one full window each
    torch.cuda.synchronize()
    with _lib.kernel_profile() as kp:
        updated = pool.step()
    assert sorted(updated) == list(range(n))
    return kp.kernels


@pytest.mark.parametrize("n", [1, 3])
def test_the_table_costs_one_launch_per_round(n):
    off, on = one_round_launches(False, n), one_round_launches(True, n)
    count = lambda k: sum(c for _, c in k.values())
    extra = {name: c for name, (_, c) in on.items() if name not in off}
    print(f"[stream timestamps] n={n}: {count(off)} launches without the table, {count(on)} with it; new: {extra}")
    assert count(on) == count(off) + 1
    assert list(extra.values()) == [1] and "arena_append_kernel" in next(iter(extra))
    base = MEMO.get("launches", lambda: count(off))  # the same for one session and for three
    assert count(off) == base


# ---- predict_stream ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", ["ctc_greedy", "ctc_beam_search"])
def test_predict_stream(decoder):
    p = predictor("conformer", decoder)
    greedy = decoder == "ctc_greedy"
    audio = pcms()[1]
    packets = [audio[i:i + PACKET] for i in range(0, len(audio), PACKET)]

    def stream(**kw):
        p.reset_stream()
        return [p.predict_stream(audio_data=x, is_end=(k == len(packets) - 1), **kw) for k, x in enumerate(packets)]

    plain = stream()
    chunks = []
    handle = p.predictor._stream
    encode = handle.encode_chunk

    def spy(*a, **kw):
        out = encode(*a, **kw)
        chunks.append(out[0].clone())
        return out
    handle.encode_chunk = spy
    try:
        got = stream(timestamps=True)
        table = torch.cat(chunks)
        del chunks[:]
        again = stream(timestamps=True)  # reset_stream, then a second utterance
    finally:
        del handle.encode_chunk
    strip = lambda r: None if r is None else {k: r[k] for k in ("text", "score")}
    assert [strip(r) for r in got] == plain and plain[-1] is not None
    assert all(r is None or set(r) == {"text", "score", "timestamps"} for r in got)
    fed = len(audio) / 2 / 16000.0
    assert got[-1]["timestamps"] == expected(table, got[-1]["text"], greedy, 0.04, fed)
    check_entries(got[-1]["timestamps"], got[-1]["text"], fed)
    assert len(got[-1]["timestamps"]) > 0
    assert again == got
    p.reset_stream()
    assert stream() == plain  # and the keyword leaves nothing behind


def test_predict_stream_refuses_deepspeech2():
    p = predictor("deepspeech2", "ctc_greedy")
    p.reset_stream()
    with pytest.raises(NotImplementedError, match="DeepSpeech2"):
        p.predict_stream(audio_data=pcms()[0][:PACKET], timestamps=True)
    p.reset_stream()


# ---- the other families --------------------------------------------------------------------------------------------------
def _eff_group(model, n):
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup
    return EfficientConformerStreamGroup(model, n)


@pytest.mark.parametrize("use_model,group,step", [("efficient_conformer", _eff_group, 0.08), ("deepspeech2", None, 0.04)])
def test_other_families(use_model, group, step):
    run = beam_run(use_model, group)
    plain = plain_run(use_model, "ctc_beam_search", group)
    pool = run["pool"]
    assert pool.frame_seconds == pytest.approx(step)
    for s in range(3):
        assert np.array_equal(bits(run["kept"][s]), bits(run["tables"][s])), s
    check_pool_run(run, plain, run["tables"], False, step)
    for r in run["final"]:
        for e in r["timestamps"]:  # the model's own frame grid
            assert e["start"] / step == pytest.approx(round(e["start"] / step), abs=1e-6)
