"""Every entry point does all its work on the caller's stream (tests/stream_gate.py): each case runs on torch's default
stream, then on a non-blocking side stream under the ``null_held`` and the ``late_producer`` gate, and every defined
output region must have the same bytes.  Shapes, builders and defined regions are those of the buffer-contents tests
(tests/test_buffer_contents_*.py); the inputs are device tensors, so that no wrapper blocks on an upload, and the decoys
are valid inputs of the same shape (features of another seed, lengths and token ids in range).

Declared synchronisations (``syncs=``; the call then cannot stay behind the gate, its bytes are compared all the same):
  csrc/capi.hip:672            ppasr_encode reads the fp16x3 guard counters back when the guard is on
  model_utils/conformer/model.py:415   ConformerStream.load_caches waits for its temporaries' copies
  csrc/capi_internal.h:79      StagingRing::acquire waits for the entry's last reader: the 9th call queued behind one gate
  data_utils/featurizer.py:253 featurize_device keeps its upload alive until the kernels have run
  data_utils/featurizer.py:376 featurize_many takes host waveforms and reads the gains back
  data_utils/featurizer.py:215 StreamResampler.push / flush take and return host samples
  decoders/beam_search_decoder.py:441  BeamSearchSessions.decode_chunks returns host results
  csrc/capi_decode.hip:222     ppasr_ctc_beam_state_compact reads the live node counts back
  serving.py                   StreamPool.step / finish take host audio and return host results"""
import numpy as np
import pytest
import torch

import numerics as nm
import stream_gate as sg
import test_align_gpu as tag
import test_buffer_contents_gpu as bc
import test_buffer_contents_stream_gpu as bcs
import test_ragged_gpu as rg
from test_buffer_contents_decoders_gpu import _batch, _vocab
from ppasr_amd.utils.synth import synth_features

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
V = 131
GUARD_SYNC = "csrc/capi.hip:672 ppasr_encode reads the fp16x3 guard counters back (guard on)"
RING_SYNC = "csrc/capi_internal.h:79 StagingRing::acquire waits for the entry's last reader (9th call behind one gate)"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _pair(ctx, B, T, lens, F, seed):
    """features and lengths of the case, their decoys: other features, the lengths in another order"""
    x, la = synth_features(B, T, n_mels=F, lens=lens, seed=seed)
    xd, _ = synth_features(B, T, n_mels=F, lens=lens, seed=seed + 7919)
    return ctx.input(_t(x), _t(xd)), ctx.input(_t(la).long(), _t(np.roll(la, 1)).long()), [int(v) for v in la]


# ---- batched encode ----------------------------------------------------------------------------------------------------
ENC_SHAPES = [("2x131", 2, 131, [131, 36]), ("3x400", 3, 400, [400, 133, 36])]
ENC_ROUTES = [r for r in bc.ROUTES if r[0] in ("default", "ffn_split=0", "ffn_split=2", "row_block=16", "front_fused=0",
                                                "front_fused=1", "skip+hint")] + [
    ("f16x3+row_block=32+guard", dict(gemm="f16x3", row_block=32, guard=True)),
    ("f16x3+row_block=32", dict(gemm="f16x3", row_block=32, guard=False))]


def _encode(model, x, la, knobs):
    p, l = model.get_encoder_out(x, la, return_logits=True)
    t, n, sc = model.encode_greedy(x, la, trim_to_length=bool(knobs.get("skip")))
    return dict(probs=p, logits=l, tokens=t, n_tokens=n, score=sc)


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("shape", ENC_SHAPES, ids=[s[0] for s in ENC_SHAPES])
@pytest.mark.parametrize("family", list(rg.FAMILIES))
def test_batched_encode(family, shape, mode):
    name, B, T, lens = shape

    def run(ctx):
        model = rg.FAMILIES[family](V)[0]
        x, la, host_lens = _pair(ctx, B, T, lens, model.input_dim, B * 1000 + T)
        outs = {}
        for route, knobs in ENC_ROUTES:
            ok = bc._apply(model, knobs, host_lens)
            if ok and "guard" in knobs:
                ok = bc._accepted(lambda: model.set_gemm_guard(knobs["guard"]))
            got = {}
            if ok:
                ok = bc._accepted(lambda: got.update(ctx.call(lambda: _encode(model, x, la, knobs), [x, la], label=route,
                                                              syncs=GUARD_SYNC if knobs.get("guard") else None)))
            if not ok:  # (what a handle refuses it refuses in every run alike)
                outs[route + "/refused"] = torch.zeros(1)
                continue
            outs.update({f"{route}/{k}": v for k, v in got.items()})
        bc._accepted(lambda: model.set_gemm_guard(True))
        assert any(not k.endswith("/refused") for k in outs)
        return outs

    sg.check(f"encode {family} {name}", run, mode, MEMO)


# ---- DeepSpeech2 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("B", [1, 3, 6])
@pytest.mark.parametrize("streaming", [True, False], ids=["streaming", "bidirectional"])
@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
def test_deepspeech2(gru, streaming, B, mode, monkeypatch):
    """two calls, the second one starting from the first one's state boxes; the per-step recurrence in every run (the gate
    holds a CU: the persistent recurrence would give up, a legitimate last-bit difference)"""
    monkeypatch.setenv("PPASR_DS2_PERSIST", "0")
    T = 67
    lens = [T] + [int(v) for v in np.linspace(60, 9, B - 1)]

    def run(ctx):
        m = bc._ds2(streaming, gru)
        # (the second call's utterances are shorter: rows the first call wrote lie behind its lengths)
        ins = [_pair(ctx, B, T, [n - 24 * k if n > 30 else n for n in lens], 80, 300 + 10 * B + k)[:2] for k in range(2)]
        outs, h, c = {}, None, None
        for k, (x, la) in enumerate(ins):
            probs, out_lens, h, c = ctx.call(lambda: m.get_encoder_out_chunk(x, la, h, c), [x, la])
            outs.update({f"{k}/probs": probs, f"{k}/out_lens": out_lens, f"{k}/h": h, f"{k}/c": c})
        return outs

    kind = ("gru" if gru else "lstm") + ("-streaming" if streaming else "-bidirectional")
    sg.check(f"ds2 {kind} B={B}", run, mode, MEMO)


# ---- stream handles ----------------------------------------------------------------------------------------------------
LOAD_SYNC = "model_utils/conformer/model.py:415 ConformerStream.load_caches waits for its temporaries' copies"


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("required", [-16, 32])
@pytest.mark.parametrize("family", bcs.HANDLES)
def test_stream_handle(family, required, mode):
    """The handle is created and its first chunk issued at once, inside the gate; the caches are exported after every
    chunk; after two chunks they are imported into a second handle that then runs the third chunk as well; the first
    handle is reset after the third chunk and starts over."""
    real, decoy = bcs._feats(1, 227, 31), bcs._feats(1, 227, 9031)

    def run(ctx):
        model = rg.FAMILIES[family](V)[0]
        x = ctx.input(real, decoy)
        box, outs = {}, {}

        def chunk(s, a, b, create=False):
            if create:
                box[s] = model.new_stream()
            probs, fa, fp = box[s].encode_chunk(x[:, a:b], required, want_frames=True)
            att, cnn = box[s].export_caches()
            return dict(probs=probs, frame_argmax=fa, frame_maxprob=fp, att_cache=att, cnn_cache=cnn)

        def record(tag_, got, s):
            outs.update({f"{tag_}/{k}": v for k, v in got.items()})
            outs[f"{tag_}/offset"] = torch.tensor([box[s].offset, box[s].cache_frames])

        for k, (a, b) in enumerate(bcs.WINDOWS[:2]):
            got = ctx.call(lambda: chunk("one", a, b, create=k == 0), [x], label=f"chunk {k}")
            record(k, got, "one")
        att, cnn = outs["1/att_cache"], outs["1/cnn_cache"]

        def second():
            box["two"] = model.new_stream()
            box["two"].load_caches(att, cnn, box["one"].offset)
            return chunk("two", *bcs.WINDOWS[2])

        record("2/imported", ctx.call(second, [x], syncs=LOAD_SYNC, label="import + chunk 2"), "two")
        record(2, ctx.call(lambda: chunk("one", *bcs.WINDOWS[2]), [x], label="chunk 2"), "one")

        def restart():
            box["one"].reset()
            return chunk("one", *bcs.WINDOWS[0])

        record("restart", ctx.call(restart, [x], label="reset + chunk 0"), "one")
        record(3, ctx.call(lambda: chunk("two", *bcs.WINDOWS[3]), [x], label="chunk 3"), "two")
        return outs

    sg.check(f"stream {family} required={required}", run, mode, MEMO)


# ---- session groups ----------------------------------------------------------------------------------------------------
def _group_run(family, n_rounds_behind_one_gate=0):
    rounds = bcs.ROUNDS if not n_rounds_behind_one_gate else \
        [([[0, 2], [1], [0, 1, 2], [2, 1], [0]][r % 5], 67) for r in range(n_rounds_behind_one_gate)]
    n_frames = 64 * len(rounds) + 67
    real = [bcs._feats(1, n_frames, 50 + u) for u in range(3)]
    decoy = [bcs._feats(1, n_frames, 9050 + u) for u in range(3)]

    def run(ctx):
        model = bcs._group_model(family)
        utts = [ctx.input(r, d) for r, d in zip(real, decoy)]
        box, outs, pos = {}, {}, [0, 0, 0]

        def one_round(r, act, T):
            if "g" not in box:
                box["g"] = bcs._group(family, model)  # (created inside the gate: its clears come right before round 0)
            if r == 3 and not n_rounds_behind_one_gate:
                box["g"].reset(1)  # one slot starts over mid-stream while the others carry on
                pos[1] = 0
            chunk = torch.cat([utts[i][:, 64 * pos[i]:64 * pos[i] + T] for i in act], 0)
            fa, fp, probs = box["g"].encode_chunks(act, chunk, want_probs=True)
            for i in act:
                pos[i] += 1
            return {f"{r}/probs": probs, f"{r}/frame_argmax": fa, f"{r}/frame_maxprob": fp}

        if n_rounds_behind_one_gate:
            def all_rounds():
                got = {}
                for r, (act, T) in enumerate(rounds):
                    got.update(one_round(r, act, T))
                return got
            outs.update(ctx.call(all_rounds, utts, syncs=RING_SYNC, label=f"{len(rounds)} rounds"))
        else:
            for r, (act, T) in enumerate(rounds):
                outs.update(ctx.call(lambda: one_round(r, act, T), utts, label=f"round {r} {act}"))
                outs[f"{r}/offsets"] = torch.tensor([box["g"].offset(i) for i in act])
        return outs
    return run


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("family", bcs.GROUPS)
def test_session_group(family, mode):
    sg.check(f"group {family}", _group_run(family), mode, MEMO)


@pytest.mark.parametrize("family", ["conformer", "squeezeformer", "deepspeech2-lstm"])
def test_ten_group_rounds_behind_one_gate(family):
    """two more than the staging ring holds: the 9th acquire must wait for round 0 (behind the gate), not overwrite the
    descriptors round 0 has yet to read -- the rounds list different sessions, so an overwritten entry changes the bytes"""
    sg.check(f"group {family} 10 rounds", _group_run(family, 10), sg.LATE_PRODUCER, MEMO)


# ---- decoders ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("frame_lens", [None, [50, 1, 0, 37]], ids=["all-rows", "lens-50-1-0-37"])
def test_ctc_greedy(frame_lens, mode):
    from ppasr_amd.decoders.ctc_greedy_decoder import greedy_decode_ids
    real, decoy = _batch(5, 4, 50, 131), _batch(6, 4, 50, 131, "flat")

    def run(ctx):
        p = ctx.input(real, decoy)
        fl = None if frame_lens is None else ctx.input(torch.tensor(frame_lens, dtype=torch.int32),
                                                       torch.tensor(frame_lens[::-1], dtype=torch.int32))
        tokens, n, score, fa, fp = ctx.call(lambda: greedy_decode_ids(p, fl), [p] + ([] if fl is None else [fl]))
        outs = {"tokens": tokens, "n_tokens": n, "score": score}
        if frame_lens is None:
            outs.update(frame_argmax=fa, frame_maxprob=fp)
        return outs

    sg.check(f"ctc_greedy {frame_lens}", run, mode, MEMO)


COMPACT_SYNC = "csrc/capi_decode.hip:222 ppasr_ctc_beam_state_compact reads the live node counts back"


def _search_run(real, decoy, beam, nbest, frame_lens, chunks, cutoff=(0.99, 40), scorer=None, max_frames=None, growable=False,
                compact=False):
    """One search over `real` in `chunks` calls on one state buffer (test_buffer_contents_decoders_gpu._search)."""
    from ppasr_amd.decoders import beam_search_decoder as bsd
    B, T, _ = real.shape
    step = (T + chunks - 1) // chunks

    def run(ctx):
        p = ctx.input(real, decoy)
        fls = []
        for k in range(chunks):
            if frame_lens is None:
                fls.append(None)
                continue
            fl = np.clip(np.asarray(frame_lens) - k * step, 0, min(step, T - k * step)).astype(np.int32)
            fls.append(ctx.input(_t(fl), _t(np.roll(fl, 1))))
        sc = scorer() if scorer is not None else None
        st = bsd._BeamState(B, max_frames or T, beam, p.device)
        st.growable, st.compact = growable, compact
        outs = {}
        for k in range(chunks):
            def call():
                return bsd.beam_search_ids(p[:, k * step:(k + 1) * step], beam, cutoff[0], cutoff[1], 0, frame_lens=fls[k],
                                           nbest=nbest, state=st, ext_scorer=sc)[:3]
            tokens, lens, scores = ctx.call(call, [p] + ([] if fls[k] is None else [fls[k]]), label=f"chunk {k}",
                                            syncs=COMPACT_SYNC if compact and k else None)
            outs.update({f"{k}/tokens": tokens, f"{k}/lens": lens, f"{k}/scores": scores})
        return outs
    return run


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("cutoff_prob", [0.99, 1.0])
@pytest.mark.parametrize("chunks", [1, 3], ids=["one-shot", "chunked"])
@pytest.mark.parametrize("beam", [10, 300])
def test_beam_search(beam, chunks, cutoff_prob, mode):
    real, decoy = _batch(beam, 3, 50, 300), _batch(beam + 1, 3, 50, 300, "flat")
    run = _search_run(real, decoy, beam, 3, [50, 1, 29], chunks, cutoff=(cutoff_prob, 40))
    sg.check(f"beam_search beam={beam} chunks={chunks} cutoff={cutoff_prob}", run, mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
def test_beam_search_large_vocabulary(mode):
    real, decoy = _batch(3, 2, 14, 4233), _batch(4, 2, 14, 4233, "flat")
    sg.check("beam_search V=4233", _search_run(real, decoy, 10, 3, [14, 9], 2, cutoff=(1.0, 40)), mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
def test_beam_search_grows_past_max_stream_frames(mode):
    real, decoy = _batch(17, 2, 48, 300), _batch(18, 2, 48, 300, "flat")
    sg.check("beam_search grow", _search_run(real, decoy, 10, 3, None, 3, max_frames=16, growable=True), mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
def test_beam_search_compacts_its_arena(mode):
    """a full state buffer is compacted (one read-back) before it grows: chunks 1 and 2 of 16 frames into a state for 16"""
    real, decoy = _batch(19, 2, 48, 300), _batch(20, 2, 48, 300, "flat")
    run = _search_run(real, decoy, 10, 3, None, 3, max_frames=16, growable=True, compact=True)
    sg.check("beam_search compact", run, mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("kind", ["char", "word"])
def test_beam_search_with_scorer(kind, mode, tmp_path):
    from lm_util import write_synthetic_arpa
    from test_ctc_beam_wordlm_gpu import VOCAB as WVOCAB, WORDS, _spoken_probs
    from ppasr_amd.decoders import beam_search_decoder as bsd
    rng = np.random.Generator(np.random.PCG64(17))
    if kind == "char":
        vocab = _vocab(200)
        arpa = write_synthetic_arpa(str(tmp_path / "c.arpa"), vocab[2:150], order=3, seed=4)
        real, decoy, lens, alpha, beta, beam = _batch(8, 3, 40, 200, "flat"), _batch(9, 3, 40, 200), [40, 1, 0], 2.2, 4.3, 16
    else:
        vocab = WVOCAB
        arpa = write_synthetic_arpa(str(tmp_path / "w.arpa"), WORDS, order=3, n_sent=300, sent_len=8, seed=2)
        tabs = [_spoken_probs(rng, sent, len(vocab)) for sent in (["the", "cat", "sat"], ["where", "is", "the", "hat"], ["we"])]
        T = max(t.shape[0] for t in tabs)
        batch = np.full((3, T, len(vocab)), 1.0 / len(vocab), np.float32)
        for b, t in enumerate(tabs):
            batch[b, :t.shape[0]] = t
        real, lens, alpha, beta, beam = torch.from_numpy(batch).cuda(), [t.shape[0] for t in tabs], 1.9, 0.3, 30
        decoy = real.flip(0).contiguous()
    run = _search_run(real, decoy, beam, 3, lens, 2, scorer=lambda: bsd.Scorer(alpha, beta, arpa, vocab))
    sg.check(f"beam_search {kind} scorer", run, mode, MEMO)


POOL_SYNC = "decoders/beam_search_decoder.py:441 BeamSearchSessions.decode_chunks returns host results (one read-back per call)"


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("behind_one_gate", [False, True], ids=["gate-per-call", "10-calls-one-gate"])
def test_beam_pool(behind_one_gate, mode):
    """three sessions, staggered subsets, a reset, one session growing past init_frames (16-frame chunks into 32)"""
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    Vp, beam, n_calls = 300, 20, 10
    real, decoy = _batch(31, 3, 16 * n_calls, Vp), _batch(32, 3, 16 * n_calls, Vp, "flat")
    acts = [[0, 1, 2], [2, 0], [1], [0, 1, 2], [0], [2, 1], [0, 1, 2], [0], [1, 2], [0, 2, 1]]

    def run(ctx):
        tabs = ctx.input(real, decoy)
        pool = BeamSearchSessions(3, 2.2, 4.3, beam, 0.99, 40, _vocab(Vp), init_frames=32)
        scores, text = [], []

        def call(k):
            if k == 4:
                pool.reset(1)
            got = pool.decode_chunks(acts[k], torch.stack([tabs[i, 16 * k:16 * k + 16] for i in acts[k]]))
            scores.extend(g[0] for g in got)
            text.extend(g[1] for g in got)

        if behind_one_gate:
            ctx.call(lambda: [call(k) for k in range(n_calls)] and None, [tabs], syncs=POOL_SYNC, label=f"{n_calls} calls")
        else:
            for k in range(n_calls):
                ctx.call(lambda: call(k), [tabs], syncs=POOL_SYNC, label=f"call {k}")
        assert not pool.status().any()
        return {"scores": torch.tensor(scores, dtype=torch.float64),
                "text": torch.tensor(list("\n".join(text).encode("utf-8")), dtype=torch.uint8)}

    sg.check(f"beam_pool one_gate={behind_one_gate}", run, mode, MEMO)


STEP_SYNC = "serving.py StreamPool.step / finish take host audio and return host results (read-backs in every round)"


@pytest.mark.parametrize("mode", sg.MODES)
def test_stream_pool_with_timestamps(mode):
    """three rounds of interleaved packets and finish: front end, session group, beam pool, probability arena and the
    alignment that reads it, all on the caller's stream"""
    import test_stream_timestamps_gpu as tst
    audio = tst.pcms()

    def run(ctx):
        pool = tst.make_pool("conformer", "ctc_beam_search", timestamps=True)
        log = []

        def packets(i):
            for s, a in enumerate(audio):
                if i * tst.PACKET < len(a):
                    pool.feed(s, a[i * tst.PACKET:(i + 1) * tst.PACKET])
            return sorted(pool.step().items())

        for i in range(3):
            log += [(s, sorted(r.items())) for s, r in ctx.call(lambda: packets(i), syncs=STEP_SYNC, label=f"round {i}")]
        final = ctx.call(lambda: [pool.finish(s) for s in range(len(audio))], syncs=STEP_SYNC, label="finish")
        log += [sorted(r.items()) for r in final]
        return {"log": torch.tensor(list(repr(log).encode("utf-8")), dtype=torch.uint8)}

    sg.check("stream pool timestamps", run, mode, MEMO)


# ---- front end ---------------------------------------------------------------------------------------------------------
FBANK_SYNC = "data_utils/featurizer.py:253 featurize_device keeps its upload alive until the kernels have run"


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("method", ["fbank", "mfcc"])
def test_front_end(method, mode):
    from test_fbank_gpu import _audio
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    real, decoy = _t(_audio(0.5, seed=3)), _t(_audio(0.5, seed=4))

    def run(ctx):
        f = AudioFeaturizer(feature_method=method, n_mels=80, sample_rate=16000, use_dB_normalization=True, target_dB=-20)
        w = ctx.input(real, decoy)
        feats = ctx.call(lambda: f.featurize_device(w), [w], syncs=FBANK_SYNC)
        return {"feats": feats, "gain": torch.tensor([f.last_gain], dtype=torch.float64)}

    sg.check(f"front {method}", run, mode, MEMO)


MANY_SYNC = "data_utils/featurizer.py:376 featurize_many takes host waveforms and reads the gains back"
PACKET_SYNC = "data_utils/featurizer.py:215 StreamResampler takes host packets and returns host samples (one download per packet)"


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("method", ["fbank", "mfcc"])
def test_front_end_many(method, mode):
    """host waveforms in, one packed upload: only what the call enqueues before its read-back is gated"""
    from test_fbank_gpu import _audio
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    waves = [_audio(0.5, seed=5), _audio(0.5, seed=6)[:5000], _audio(0.5, seed=7)[:7321]]

    def run(ctx):
        f = AudioFeaturizer(feature_method=method, n_mels=80, sample_rate=16000, use_dB_normalization=True, target_dB=-20)
        feats, lens = ctx.call(lambda: f.featurize_many(waves, padded=True), syncs=MANY_SYNC)
        return {"feats": feats, "lens": lens, "gains": torch.as_tensor(np.asarray(f.last_gains))}

    sg.check(f"front many {method}", run, mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("rate", [8000, 44100])
def test_resample_whole(rate, mode):
    from test_fbank_gpu import _audio
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    n = rate // 2
    real, decoy = _t(_audio(1.0, seed=8)[:n]), _t(_audio(1.0, seed=9)[:n])

    def run(ctx):
        f = AudioFeaturizer(n_mels=80, sample_rate=16000, resample="device")
        f._resampler(rate)  # (the filter table is built and uploaded at creation, outside the gate)
        w = ctx.input(real, decoy)
        return {"y": ctx.call(lambda: f.resample_device(w, rate), [w])}

    sg.check(f"resample {rate}", run, mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("rate", [8000, 44100])
def test_resample_packets(rate, mode):
    from test_fbank_gpu import _audio
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer, StreamResampler
    x = _audio(1.0, seed=10)[:rate // 2]
    cuts = [0, 1, 800, 801, 2400, x.size]

    def run(ctx):
        f = AudioFeaturizer(n_mels=80, sample_rate=16000, resample="device")
        r = StreamResampler(f, rate)
        outs = {}
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            outs[f"push{k}"] = torch.from_numpy(ctx.call(lambda: r.push(x[a:b]), syncs=PACKET_SYNC, label=f"push {k}").copy())
        outs["flush"] = torch.from_numpy(ctx.call(r.flush, syncs=PACKET_SYNC, label="flush").copy())
        return outs

    sg.check(f"resample packets {rate}", run, mode, MEMO)


# ---- alignment and the CTC loss ----------------------------------------------------------------------------------------
def _align_batch(seed, Va=67, T=33, bad=True):
    """B = 3, T = 33: a good utterance, an infeasible one (more frames needed than it has) and one with a bad id"""
    rng = np.random.default_rng(seed)
    probs = np.stack([tag.softmax_table(rng, T, Va) for _ in range(3)])
    toks = [tag.random_tokens(rng, 17, T, Va), [4, 4, 4, 9], tag.random_tokens(rng, 5, 20, Va)]
    lens = np.asarray([T, 5 if bad else 9, 20], np.int32)
    if bad:
        toks[2][2] = Va
    tk, nt = tag.pack_tokens(toks, 17, pad=0)
    return probs, tk, nt, lens


def _align_inputs(ctx, seed=91):
    real, decoy = _align_batch(seed), _align_batch(seed + 1, bad=False)
    return [ctx.input(_t(r), _t(d)) for r, d in zip(real, decoy)]


@pytest.mark.parametrize("mode", sg.MODES)
def test_ctc_align(mode):
    from ppasr_amd.decoders import ctc_alignment as ca

    def run(ctx):
        p, tk, nt, fl = ins = _align_inputs(ctx)
        out = ctx.call(lambda: ca.ctc_align_ids(p, tk, nt, fl), ins)
        assert out["status"].tolist() == [0, 1, 2]
        return {k: out[k] for k in tag.OUT_NAMES}

    sg.check("ctc_align 3x33", run, mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
def test_ctc_nll(mode):
    from ppasr_amd.model_utils import loss as ml

    def run(ctx):
        p, tk, nt, fl = ins = _align_inputs(ctx)
        out = ctx.call(lambda: ml.ctc_nll(p, tk, nt, fl), ins)
        assert out["status"].tolist() == [0, 1, 2]
        return {k: out[k] for k in ("nll", "status")}

    sg.check("ctc_nll 3x33", run, mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
def test_prob_arena(mode):
    """appends over page edges (P = 4, rounds of 7 rows), read, and the alignment that reads the pages; 7 staged calls
    behind the first gate, one fewer than the staging ring holds"""
    from ppasr_amd.decoders import ctc_alignment as ca
    Va, P = 67, 4

    def run(ctx):
        p, tk, nt, _ = ins = _align_inputs(ctx, 95)
        arena = ca.ProbArena(3, Va, page_frames=P, n_pages=3 * 9)

        def fill():
            for a in range(0, 33, 7):  # session 0: 33 frames, 1: 7, 2: 21
                c = min(7, 33 - a)
                arena.append([2, 0, 1], torch.stack([p[2, a:a + c], p[0, a:a + c], p[1, a:a + c]]),
                             frames=[c if a < 21 else 0, c, c if a < 7 else 0])
            return {f"read{s}": arena.read(s) for s in (0, 2)}

        outs = ctx.call(fill, ins, label="5 appends + 2 reads")
        assert [arena.frames(s) for s in range(3)] == [33, 7, 21]
        out = ctx.call(lambda: arena.align_ids([0, 1, 2], tk, nt), ins, label="align")
        outs.update({k: out[k] for k in tag.OUT_NAMES})
        return outs

    sg.check("prob_arena P=4", run, mode, MEMO)


def test_ten_arena_appends_behind_one_gate():
    """two more staged calls than the ring holds: the 9th acquire waits for the first append (behind the gate) and does not
    overwrite the page table it has yet to read; every append lists other sessions and rows"""
    from ppasr_amd.decoders import ctc_alignment as ca
    Va, P = 67, 4

    def run(ctx):
        p = ctx.input(*(_t(_align_batch(seed, bad=False)[0]) for seed in (97, 98)))
        arena = ca.ProbArena(3, Va, page_frames=P, n_pages=3 * 9)

        def fill():
            for k in range(10):
                act = [[0, 1, 2], [2, 0], [1], [0, 2], [1, 0]][k % 5]
                arena.append(act, torch.stack([p[s, 3 * k:3 * k + 3] for s in act]))
            return {f"read{s}": arena.read(s) for s in range(3)}

        return ctx.call(fill, [p], syncs=RING_SYNC, label="10 appends + 3 reads")

    sg.check("prob_arena 10 appends", run, sg.LATE_PRODUCER, MEMO)


# ---- attention rescoring and the attention loss ------------------------------------------------------------------------
RESCORE = "v67_l17_n3_b3_t33"


def _rescore_inputs(ctx, loss):
    import decoder_cases as dc
    case = dc.CASES[RESCORE]
    inp, other = dc.case_inputs(case), dc.case_inputs(dict(case, seed=case["seed"] + 1))
    if loss:
        keys = ("memory", "out_lens", "labels", "label_lens")
        pick = lambda d: dict(memory=d["memory"], out_lens=d["out_lens"], labels=np.ascontiguousarray(d["tokens"][:, 0]),
                              label_lens=np.ascontiguousarray(d["lens"][:, 0]))
        inp, other = pick(inp), pick(other)
    else:
        keys = ("memory", "out_lens", "tokens", "lens", "ctc_scores")
    return case, [ctx.input(_t(np.asarray(inp[k])), _t(np.asarray(other[k]))) for k in keys]


@pytest.mark.parametrize("mode", sg.MODES)
def test_attention_rescorer(mode):
    import test_rescore_gpu as trg

    def run(ctx):
        r = trg.rescorer(RESCORE)
        case, ins = _rescore_inputs(ctx, loss=False)
        got = ctx.call(lambda: r.rescore(*ins, case["ctc_weight"], case["reverse_weight"], return_token_logp=True,
                                         return_logits=True), ins)
        return dict(got)

    sg.check("rescore " + RESCORE, run, mode, MEMO)


@pytest.mark.parametrize("mode", sg.MODES)
def test_attention_loss(mode):
    import test_att_loss_gpu as tal

    def run(ctx):
        r = tal.rescorer(RESCORE)
        case, ins = _rescore_inputs(ctx, loss=True)
        return dict(ctx.call(lambda: r.loss(*ins, 0.1, case["reverse_weight"]), ins))

    sg.check("att_loss " + RESCORE, run, mode, MEMO)


# ---- hypothesis records ------------------------------------------------------------------------------------------------
def _scores(k, rng):
    """float64 scores that carry the bit patterns of NaN (two payloads), -0.0, +-inf and a denormal"""
    s = torch.from_numpy(rng.normal(size=k) * 50.0)
    special = torch.from_numpy(np.array([0x7FF8000000000001, 0xFFF0DEADBEEF0001, 0x8000000000000000, 0x7FF0000000000000,
                                         0xFFF0000000000000, 0x0000000000000001], np.uint64).view(np.float64))
    s[:min(k, special.numel())] = special[:min(k, special.numel())]
    return s[torch.from_numpy(rng.permutation(k))].contiguous()


def _host_pack(rec, tokens, n, score, index, row0, cols, extra):
    """the host expressions of parallel.RaggedPlan._record / pack_hypotheses, on CPU tensors"""
    k, w = tokens.shape[0], min(int(tokens.shape[1]), cols)
    rec[row0:row0 + k, :cols] = -1
    rec[row0:row0 + k, :w] = tokens[:, :w].to(torch.int32)
    rec[row0:row0 + k, cols] = n.to(torch.int32)
    # (a fresh array: one strided element counts as contiguous and cannot be viewed as words)
    rec[row0:row0 + k, cols + 1:cols + 3] = torch.from_numpy(score.to(torch.float64).numpy().copy()).view(torch.int32).view(k, 2)
    if extra == 4:
        rec[row0:row0 + k, cols + 3] = -1 if index is None else index
    return rec


def _host_unpack(out, order, cols, extra):
    """parallel.RaggedPlan._unpack / unpack_hypotheses on CPU tensors"""
    g = out if order is None else out[order]
    # (fresh arrays: a slice of ONE row counts as contiguous as it is and cannot be viewed as doubles or bytes)
    fresh = lambda t: torch.from_numpy(t.numpy().copy())
    score = fresh(g[:, cols + 1:cols + 3]).view(torch.float64).view(-1)
    index = g[:, cols + 3] if extra == 4 else torch.full((g.shape[0],), -1, dtype=torch.int32)
    return fresh(g[:, :cols]), fresh(g[:, cols]), score, fresh(index)


# (k, L, cols, extra, row0, rows, with index, with order): L < / == / > cols; k (cols + extra) and N (cols + 1) at 255, 256, 257
HYP = [(4, 9, 13, 3, 0, 4, False, False), (4, 13, 13, 3, 0, 4, False, True), (4, 20, 13, 3, 0, 4, False, False),
       (3, 7, 11, 4, 2, 7, True, True), (3, 11, 11, 4, 4, 7, False, True), (3, 15, 11, 4, 0, 7, True, False),
       (1, 252, 252, 3, 0, 1, False, False), (1, 253, 253, 3, 0, 1, False, False), (1, 254, 254, 3, 0, 1, False, False),
       (5, 30, 47, 4, 1, 7, True, True), (16, 12, 12, 4, 0, 16, True, True), (16, 13, 13, 3, 0, 16, False, True),
       (15, 16, 16, 3, 0, 15, False, True), (16, 15, 15, 4, 0, 16, True, False), (1, 300, 256, 3, 0, 1, False, False),
       (1, 255, 255, 4, 0, 1, True, False)]


def _hyp_inputs(cfg, seed):
    k, L, cols, extra, row0, rows, with_index, with_order = cfg
    rng = np.random.default_rng(seed)
    n = torch.from_numpy(rng.integers(0, min(L, cols) + 1, size=(k, 3)).astype(np.int32))  # (column 0 of a [k][nbest] output)
    tokens = torch.from_numpy(rng.integers(1, 5000, size=(k, L + 5)).astype(np.int32))     # (row stride L + 5)
    for r in range(k):
        tokens[r, int(n[r, 0]):] = -1
    score = torch.stack([_scores(k, rng), torch.zeros(k, dtype=torch.float64)], 1)          # (element stride 2)
    index = torch.from_numpy(rng.permutation(1000)[:k].astype(np.int32))
    order = torch.from_numpy(rng.permutation(rows)[:max(rows - 1, 1)].astype(np.int64))
    return dict(tokens=tokens, n=n, score=score, index=index, order=order)


def _hyp_case(cfg, seed=0):
    from ppasr_amd import parallel
    k, L, cols, extra, row0, rows, with_index, with_order = cfg

    def run(ctx):
        real, decoy = _hyp_inputs(cfg, 1000 + seed), _hyp_inputs(cfg, 2000 + seed)
        d = {key: ctx.input(real[key], decoy[key]) for key in real}
        ins = list(d.values())

        def pack():
            rec = torch.full((rows, cols + extra), -1, dtype=torch.int32, device="cuda")
            parallel._hip_pack(d["tokens"][:, :L], d["n"][:, 0], d["score"][:, 0], d["index"] if with_index else None, rec,
                               row0, cols, extra)
            return rec

        rec = ctx.call(pack, ins, label="pack")
        order = d["order"] if with_order else None
        n_rows = int(order.shape[0]) if with_order else rows
        # (the unpack reads a record that is an input of its own: the packed one of this case, real and decoy alike)
        rec_in = ctx.input(_host_pack(torch.full((rows, cols + extra), -1, dtype=torch.int32), real["tokens"][:, :L],
                                      real["n"][:, 0], real["score"][:, 0], real["index"] if with_index else None, row0, cols,
                                      extra),
                           _host_pack(torch.full((rows, cols + extra), -7, dtype=torch.int32), decoy["tokens"][:, :L],
                                      decoy["n"][:, 0], decoy["score"][:, 0], decoy["index"], row0, cols, extra))
        tk, nn, sc, ix = ctx.call(lambda: parallel._hip_unpack(rec_in, order, n_rows, cols, extra, want_index=True),
                                  [rec_in] + ([order] if with_order else []), label="unpack")
        return dict(rec=rec, tokens=tk, n_tokens=nn, score=sc, index=ix)
    return run


def _hyp_expected(cfg, seed=0):
    k, L, cols, extra, row0, rows, with_index, with_order = cfg
    real = _hyp_inputs(cfg, 1000 + seed)
    rec = _host_pack(torch.full((rows, cols + extra), -1, dtype=torch.int32), real["tokens"][:, :L], real["n"][:, 0],
                     real["score"][:, 0], real["index"] if with_index else None, row0, cols, extra)
    tk, nn, sc, ix = _host_unpack(rec, real["order"] if with_order else None, cols, extra)
    return dict(rec=rec, tokens=tk, n_tokens=nn, score=sc, index=ix)


@pytest.mark.parametrize("cfg", HYP, ids=["k{}-L{}-cols{}-x{}-row{}of{}-i{:d}-o{:d}".format(*c) for c in HYP])
def test_hyp_pack_and_unpack_equal_the_host_expressions(cfg):
    """ppasr_hyp_pack / ppasr_hyp_unpack against the host tensor expressions of parallel.py, byte for byte: on the default
    stream (the reference of the gated runs is compared with the host result first), then under both gates"""
    import poison
    on_default_stream, _ = sg.reference(f"hyp {cfg}", _hyp_case(cfg), MEMO)
    d = poison.differences(poison.freeze(_hyp_expected(cfg)), on_default_stream)
    assert not d, "; ".join(d)
    for mode in sg.MODES:
        sg.check(f"hyp {cfg}", _hyp_case(cfg), mode, MEMO)


def test_hyp_records_equal_pack_hypotheses_on_the_host():
    """the public pair: device records == the host path of the same functions, rows and bits"""
    import poison
    from ppasr_amd import parallel
    real = _hyp_inputs((6, 21, 21, 3, 0, 6, False, False), 7)
    tokens, n, score = real["tokens"][:, :21].contiguous(), real["n"][:, 0].contiguous(), real["score"][:, 0].contiguous()
    host = parallel.pack_hypotheses(tokens, n, score)
    dev = parallel.pack_hypotheses(tokens.cuda(), n.cuda(), score.cuda())
    names = ("tokens", "n_tokens", "score")
    back_h = dict(zip(names, (t.contiguous() for t in parallel.unpack_hypotheses(host))))
    back_d = dict(zip(names, parallel.unpack_hypotheses(dev)))
    torch.cuda.synchronize()
    d = poison.differences(poison.freeze(dict(back_h, rec=host)), poison.freeze(dict(back_d, rec=dev)))
    assert not d, "; ".join(d)


# ---- one object, two streams -------------------------------------------------------------------------------------------
def _dev_feats(B, T, lens, F, seed):
    x, la = synth_features(B, T, n_mels=F, lens=lens, seed=seed)
    return _t(x).cuda(), _t(la).long().cuda()


@pytest.mark.parametrize("family", list(rg.FAMILIES))
def test_one_model_on_two_streams(family):
    """what tools/bench_configs.py does: two different batches encoded alternately on two streams, no synchronisation
    between them; the workspace is kept per stream, the handle is only read during an encode"""
    box = {}

    def build():
        m = rg.FAMILIES[family](V)[0]
        box["a"] = _dev_feats(2, 131, [131, 36], m.input_dim, 501)
        box["b"] = _dev_feats(3, 200, [200, 133, 36], m.input_dim, 502)
        return m

    def call(which):
        return lambda m: _encode(m, *box[which], {})

    sg.check_two_streams(f"two streams encode {family}", build, call("a"), call("b"))


def test_the_aligner_on_two_streams():
    from ppasr_amd.decoders import ctc_alignment as ca
    a = [_t(v).cuda() for v in _align_batch(91)]
    b = [_t(v).cuda() for v in _align_batch(92, T=65, bad=False)]
    pick = lambda out: {k: out[k] for k in tag.OUT_NAMES}
    sg.check_two_streams("two streams ctc_align", lambda: ca, lambda m: pick(m.ctc_align_ids(*a)),
                         lambda m: pick(m.ctc_align_ids(*b)))


def test_the_rescorer_on_two_streams():
    import decoder_cases as dc
    import test_rescore_gpu as trg
    case = dc.CASES[RESCORE]
    keys = ("memory", "out_lens", "tokens", "lens", "ctc_scores")
    a, b = ([_t(np.asarray(d[k])).cuda() for k in keys]
            for d in (dc.case_inputs(case), dc.case_inputs(dict(case, seed=case["seed"] + 1))))
    go = lambda ins: lambda r: dict(r.rescore(*ins, case["ctc_weight"], case["reverse_weight"], return_token_logp=True))
    sg.check_two_streams("two streams rescore", lambda: trg.rescorer(RESCORE), go(a), go(b))
