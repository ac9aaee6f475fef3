"""Streaming serving throughput: N independent Conformer sessions (device-resident caches), each fed 0.64 s chunks, on N HIP
streams from one host thread.  Prints the aggregate audio-seconds/s and the single-session chunk latency.

  --squeezeformer            the Squeezeformer section instead (not part of the default run): the shipped configuration (configs/squeezeformer.yml of
                             PPASR: 12 blocks, reduce before 5, recover before 11, kernel 31), SqueezeformerStreamGroup
                             against StreamHandleSet at n = 1 / 8 / 64 / 256, measured alternately in this process
  --sq-rounds R --sessions N only R group rounds of N sessions (after model set-up, nothing else): run it under
                             `rocprofv3 --kernel-trace --stats` at two R and subtract for the dispatches per round
  --efficient-conformer      the same section for the Efficient-Conformer: the shipped configuration
                             (configs/efficient_conformer.yml of PPASR: 12 blocks, stride layer 3, grouped attention on
                             layers 0-3 with group size 3, kernel 15 -> 7), EfficientConformerStreamGroup against
                             StreamHandleSet
  --eff-rounds R --sessions N  R Efficient-Conformer group rounds of N sessions, for the dispatch count as above
  --deepspeech2 [--gru]      the same section for DeepSpeech2: the shipped configuration (configs/deepspeech2.yml of PPASR:
                             streaming, 5 x 1024 LSTM; --gru: nn.GRU layers), DeepSpeech2StreamGroup against one
                             get_encoder_out_chunk call per session that carries its own h / c boxes (what
                             predict_chunk_deepspeech does), one 67-frame window per session per round
  --ds2-rounds R --sessions N [--gru]  R DeepSpeech2 group rounds of N sessions, for the dispatch count as above
  --general                  the same section for the general layer route: the shipped configs/conformer.yml, streaming,
                             with output_size 512 and attention_heads 8 (the YAML's own suggestion for large datasets),
                             GeneralConformerStreamGroup against StreamHandleSet (one stream handle per session)
  --gen-rounds R --sessions N  R general-route group rounds of N sessions, for the dispatch count as above
  --decoder beam             the beam-search session pool (BeamSearchSessions, one pruning + one search launch per round)
                             against N BeamSearchDecoder objects: the decode stage of one 16-frame round at n = 8 / 64 /
                             256 / 300, beam 10 and the shipped beam 300 (cutoff 0.99 / 40), without and with a synthetic
                             character ARPA scorer; then pool rounds end to end (Conformer group + beam pool)
  --decoder beam --stream-frames F [--compact] [--sessions N] [--beam B] [--scorer]
                             one long stream of F frames per session in 16-frame rounds through the pool (init_frames 16):
                             the decode stage per round (median, 10th / 90th percentile), block moves, arena_bytes() at the
                             end and the time of an explicit compact() of the F-frame arenas.  --compact: a second pool with
                             compact=True takes the same rounds, alternately in this process; adds its rounds with a
                             compaction (count, time) and the time of a compact() at the arena sizes the policy leaves
  --beam-rounds R --sessions N [--compact]  R pool decode rounds of N sessions at beam 300 (no scorer), for a rocprofv3
                             kernel trace (--compact: the pool has compact=True; 16 frames of room, so it compacts)
  --front [--rounds R]       the audio front stage of a serving round on the Conformer group with greedy decoding, n = 8 / 64 /
                             256 sessions and one 0.64 s packet per session per round: N x StreamPool.feed against one
                             StreamPool.feed_many, the front stage alone and the whole round (front + step), the two
                             variants alternating round by round in this process after warm-up; one JSON line per n with the
                             median and the 10th / 90th percentile over R rounds (default 12)"""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppasr_amd.model_utils.conformer.model import ConformerModel
from ppasr_amd.utils.synth import DEFAULT_VOCAB_SIZE, conformer_state_dict, synth_features


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def squeezeformer_model():
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel
    from ppasr_amd.utils.synth import squeezeformer_state_dict
    V = DEFAULT_VOCAB_SIZE
    conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=12, reduce_idx=5, recover_idx=11,
                feed_forward_expansion_factor=8, cnn_module_kernel=31)
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=12, seed=1234)
    return SqueezeformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


def efficient_conformer_model():
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel
    from ppasr_amd.utils.synth import efficient_conformer_state_dict
    V = DEFAULT_VOCAB_SIZE
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, cnn_module_kernel=15,
                cnn_module_norm="layer_norm",
                efficient_conf=dict(stride_layer_idx=[3], stride=[2], group_layer_idx=[0, 1, 2, 3], group_size=3))
    sd = efficient_conformer_state_dict(vocab_size=V, seed=1234)
    return EfficientConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


def deepspeech2_model(gru=False):
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
    from ppasr_amd.utils.synth import deepspeech2_state_dict
    V = DEFAULT_VOCAB_SIZE
    sd = deepspeech2_state_dict(vocab_size=V, num_rnn_layers=5, rnn_size=1024, streaming=True, seed=1234, use_gru=gru)
    return DeepSpeech2Model(80, V, streaming=True, encoder_conf=dict(num_rnn_layers=5, rnn_size=1024, use_gru=gru),
                            state_dict=sd, device="cuda:0")


def general_model():
    """configs/conformer.yml (12 blocks, kernel 15, rel_pos, swish) at output_size 512 / 8 heads: the general layer route."""
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "conformer.yml")) as f:
        conf = dict(yaml.safe_load(f)["encoder_conf"], output_size=512, attention_heads=8)
    V = DEFAULT_VOCAB_SIZE
    sd = conformer_state_dict(vocab_size=V, num_blocks=conf["num_blocks"], seed=1234, output_size=512, attention_heads=8,
                              cnn_module_kernel=conf["cnn_module_kernel"])
    return ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


class Ds2BoxSessions:
    """The group's interface over per-session get_encoder_out_chunk calls, each with its own h / c boxes (the only way to
    serve N DeepSpeech2 streams without a group: N single-utterance calls per round)."""

    def __init__(self, model, n_sessions, max_frames=0):
        self.model, self.n_sessions = model, int(n_sessions)
        self.boxes = [(None, None)] * self.n_sessions

    def reset(self, session=-1):
        for i in (range(self.n_sessions) if int(session) < 0 else [int(session)]):
            self.boxes[i] = (None, None)

    def encode_chunks(self, sessions, speech, want_probs=False):
        lens = np.full(1, int(speech.shape[1]), np.int64)
        out = []
        for k, s in enumerate(sessions):
            probs, _, h, c = self.model.get_encoder_out_chunk(speech[k:k + 1], lens, *self.boxes[s])
            self.boxes[s] = (h, c)
            out.append(probs)
        return out


def group_section(family, model, group_cls, n_chunks=8, sizes=(1, 8, 64, 256), reps=3, baseline=None):
    """ms per round and audio-s/s of one 0.64 s chunk per session per round: the group (one set of launches per round)
    and StreamHandleSet (one stream handle per session, what make_stream_group gives this family; `baseline`: another
    per-session class with its interface) at the same n, measured alternately (warm-up, then `reps` timed passes of each;
    the median is printed)."""
    from ppasr_amd.model_utils.conformer.model import StreamHandleSet
    baseline = baseline or ("handle_set", StreamHandleSet)
    x, _ = synth_features(1, 67, seed=5)
    chunk = torch.from_numpy(x).cuda()
    for n in sizes:
        batch = chunk.repeat(n, 1, 1).contiguous()
        ids = list(range(n))
        kinds = {"group": group_cls(model, n, max_frames=16 * (n_chunks + 2)),
                 baseline[0]: baseline[1](model, n)}
        times = {k: [] for k in kinds}
        for rep in range(reps + 1):  # rep 0 = warm-up
            for k, g in kinds.items():
                g.reset()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(n_chunks):
                    g.encode_chunks(ids, batch)
                torch.cuda.synchronize()
                if rep:
                    times[k].append(time.perf_counter() - t)
        for k in kinds:
            dt = float(np.median(times[k]))
            print(json.dumps({"family": family, "route": k, "sessions": n,
                              "ms_per_chunk_round": round(dt / n_chunks * 1e3, 3),
                              "audio_s_per_s": round(n * n_chunks * 0.64 / dt, 1)}), flush=True)
        del kinds


def _beam_probs(n, T, V, seed):
    """peaky synthetic posteriors (a character held for 3 frames, blank-heavy), [n, T, V] on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn(n, T, V, device="cuda", generator=g)
    idx = torch.randint(0, V, (n, (T + 2) // 3), device="cuda", generator=g).repeat_interleave(3, 1)[:, :T]
    logits.scatter_add_(2, idx[..., None], torch.full((n, T, 1), 6.0, device="cuda"))
    logits[..., 0] += 7.0 * (torch.rand(n, T, device="cuda", generator=g) < 0.4)
    return torch.softmax(logits, -1).contiguous()


def _beam_scorer(V):
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from lm_util import write_synthetic_arpa
    from ppasr_amd.decoders.beam_search_decoder import Scorer
    vocab = [chr(0x4E00 + i) for i in range(V)]
    path = os.path.join(tempfile.mkdtemp(), "bench.arpa")
    write_synthetic_arpa(path, vocab[2:400], order=3, seed=1)
    return vocab, path, Scorer


def beam_section(sizes=(8, 64, 256, 300), rounds=4, reps=2, T=16):
    """ms per round of the decode stage (one 16-frame chunk per session): the session pool against N decoder objects,
    measured alternately (warm-up, then `reps` timed passes of `rounds` rounds each; the median is printed)."""
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchDecoder, BeamSearchSessions
    V = DEFAULT_VOCAB_SIZE
    vocab, arpa, Scorer = _beam_scorer(V)
    for beam, lm in ((10, False), (300, False), (10, True), (300, True)):
        scorer = Scorer(2.2, 4.3, arpa, vocab) if lm else None
        for n in sizes:
            probs = _beam_probs(n, T, V, seed=n)
            pool = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, scorer=scorer, init_frames=T * (rounds + 1))
            decs = [BeamSearchDecoder(2.2, 4.3, beam, 0.99, 40, vocab, max_stream_frames=T * (rounds + 1)) for _ in range(n)]
            for d in decs:
                d._ext_scorer = scorer
            ids, lens = list(range(n)), np.full(1, T, np.int32)
            times = {"pool": [], "decoders": []}
            for rep in range(reps + 1):  # rep 0 = warm-up
                pool.reset()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(rounds):
                    pool.decode_chunks(ids, probs)
                torch.cuda.synchronize()
                if rep:
                    times["pool"].append(time.perf_counter() - t)
                for d in decs:
                    d.reset_decoder()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(rounds):
                    for k, d in enumerate(decs):
                        d.decode_chunk(probs[k:k + 1], lens)
                torch.cuda.synchronize()
                if rep:
                    times["decoders"].append(time.perf_counter() - t)
            out = {k: round(float(np.median(v)) / rounds * 1e3, 3) for k, v in times.items()}
            print(json.dumps({"section": "beam_decode", "beam": beam, "cutoff": [0.99, 40], "scorer": "arpa3" if lm else None,
                              "sessions": n, "pool_ms_per_round": out["pool"], "decoders_ms_per_round": out["decoders"],
                              "speedup": round(out["decoders"] / out["pool"], 2)}), flush=True)
            del pool, decs


def beam_end_to_end(sizes=(8, 64, 256), n_chunks=8, reps=2):
    """ms per round of one 0.64 s chunk per session: Conformer group + beam pool (beam 300, cutoff 0.99 / 40, no scorer)
    against the group alone; the chunk's probabilities go to the pool on the same stream."""
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
    model = ConformerModel(80, DEFAULT_VOCAB_SIZE, streaming=True, device="cuda:0",
                           encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12,
                                             cnn_module_kernel=15),
                           state_dict=conformer_state_dict(vocab_size=DEFAULT_VOCAB_SIZE, num_blocks=12, seed=1234))
    vocab = [chr(0x4E00 + i) for i in range(DEFAULT_VOCAB_SIZE)]
    x, _ = synth_features(1, 67, seed=5)
    chunk = torch.from_numpy(x).cuda()
    for n in sizes:
        batch = chunk.repeat(n, 1, 1).contiguous()
        ids = list(range(n))
        g = ConformerStreamGroup(model, n, max_frames=16 * (n_chunks + 2))
        pool = BeamSearchSessions(n, 2.2, 4.3, 300, 0.99, 40, vocab, init_frames=16 * (n_chunks + 2))
        times = {"group": [], "group+beam": []}
        for rep in range(reps + 1):
            for k in times:
                g.reset()
                pool.reset()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(n_chunks):
                    if k == "group":
                        g.encode_chunks(ids, batch)[0].cpu()  # (the greedy pool's copy-back)
                    else:
                        pool.decode_chunks(ids, g.encode_chunks(ids, batch, want_probs=True)[2])
                torch.cuda.synchronize()
                if rep:
                    times[k].append(time.perf_counter() - t)
        print(json.dumps({"section": "beam_end_to_end", "sessions": n, **{
            f"{k}_ms_per_round": round(float(np.median(v)) / n_chunks * 1e3, 3) for k, v in times.items()}}), flush=True)
        del g, pool


def beam_long_streams(n, beam, lm, frames, compact, T=16):
    """One stream of `frames` frames per session, 16 frames per round; the pool without compaction and (compact) one with
    it take every round one after the other, so both see the same machine state."""
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    V = DEFAULT_VOCAB_SIZE
    vocab, arpa, Scorer = _beam_scorer(V)
    scorer = Scorer(2.2, 4.3, arpa, vocab) if lm else None
    sides = {"off": BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, scorer=scorer, init_frames=T)}
    if compact:
        sides["on"] = BeamSearchSessions(n, 2.2, 4.3, beam, 0.99, 40, vocab, scorer=scorer, init_frames=T, compact=True)
    tables = [_beam_probs(n, T, V, seed=100 + k) for k in range(8)]  # (a cycle of 8 rounds: new characters every round)
    ids = list(range(n))
    ms = {k: [] for k in sides}
    event = {k: [] for k in sides}  # per round: 0 plain, 1 a compaction ran, 2 ... and / or a block moved
    for k, pool in sides.items():  # warm-up on sessions that are reset afterwards
        pool.decode_chunks(ids, tables[0])
        pool.reset()
    torch.cuda.synchronize()
    for r in range(frames // T):
        for k, pool in sides.items():
            caps = [pool.capacity(s) for s in ids]
            live = [pool.live_nodes(s) for s in ids]
            used_before = pool.arena_bytes()
            torch.cuda.synchronize()
            t = time.perf_counter()
            pool.decode_chunks(ids, tables[r % len(tables)])
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t) * 1e3)
            moved = pool.arena_bytes() != used_before or [pool.capacity(s) for s in ids] != caps
            event[k].append(2 if moved else 1 if [pool.live_nodes(s) for s in ids] != live else 0)
    for k, pool in sides.items():
        t_all, ev = np.asarray(ms[k]), np.asarray(event[k])
        plain = t_all[ev == 0]
        torch.cuda.synchronize()
        t = time.perf_counter()
        live = pool.compact()
        explicit_ms = (time.perf_counter() - t) * 1e3
        out = {"section": "beam_long_streams", "side": k, "sessions": n, "beam": beam, "scorer": "arpa3" if lm else None,
               "stream_frames": frames, "rounds": len(t_all),
               "round_ms_median": round(float(np.median(t_all)), 3),
               "round_ms_p10_p90": [round(float(np.percentile(t_all, q)), 3) for q in (10, 90)],
               "plain_round_ms_median": round(float(np.median(plain)), 3) if plain.size else None,
               "rounds_with_block_moves": int((ev == 2).sum()),
               "rounds_with_compaction_only": int((ev == 1).sum()),
               "compaction_round_ms_median": round(float(np.median(t_all[ev == 1])), 3) if (ev == 1).any() else None,
               "move_round_ms_median": round(float(np.median(t_all[ev == 2])), 3) if (ev == 2).any() else None,
               "capacity_frames_max": max(pool.capacity(s) for s in ids), "arena_bytes": pool.arena_bytes(),
               "explicit_compact_ms": round(explicit_ms, 3), "explicit_compact_live_nodes_max": max(live)}
        print(json.dumps(out), flush=True)


def front_section(sizes=(8, 64, 256), rounds=12, warmup=3, packet=10240):
    """ms of the front stage (packets -> cached features) and of the whole round (front + step) per variant; a host clock
    around work that ends in a device synchronise.  Both pools take the same packets, one round each in turn."""
    from ppasr_amd.serving import StreamPool
    from ppasr_amd.utils.synth import synth_vocabulary
    V = DEFAULT_VOCAB_SIZE
    model = ConformerModel(80, V, streaming=True, device="cuda:0",
                           encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12,
                                             cnn_module_kernel=15),
                           state_dict=conformer_state_dict(vocab_size=V, num_blocks=12, seed=1234))
    vocab = synth_vocabulary(V)
    total = warmup + rounds
    for n in sizes:
        rng = np.random.Generator(np.random.PCG64(n))
        t = np.arange(4 * packet) / 16000.0
        audio = (0.1 * np.sin(2 * np.pi * (150 + 3 * np.arange(n))[:, None] * t) + 0.03 * rng.standard_normal((n, t.size)))
        audio = audio.astype(np.float32)
        pools = {k: StreamPool(model, vocab, n_sessions=n, max_seconds=0.64 * total + 2.0) for k in ("feed", "feed_many")}
        front = {k: [] for k in pools}
        whole = {k: [] for k in pools}
        windows = {k: 0 for k in pools}
        for r in range(total):
            lo = (r % 4) * packet
            packets = {i: audio[i, lo:lo + packet] for i in range(n)}
            for k, pool in pools.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k == "feed":
                    for i, p in packets.items():
                        pool.feed(i, p)
                else:
                    pool.feed_many(packets)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                updated = pool.step()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if r >= warmup:
                    front[k].append((t1 - t0) * 1e3)
                    whole[k].append((t2 - t0) * 1e3)
                    windows[k] += len(updated)
        same = all(a.frame_ids == b.frame_ids for a, b in zip(pools["feed"].sessions, pools["feed_many"].sessions))
        out = {"section": "front_batch", "sessions": n, "packet_s": packet / 16000.0, "rounds": rounds,
               "sessions_advanced_per_round": round(windows["feed"] / rounds, 1), "same_frame_ids": bool(same)}
        for k in pools:
            out[k] = {"front_ms_median": round(float(np.median(front[k])), 3),
                      "front_ms_p10_p90": [round(float(np.percentile(front[k], q)), 3) for q in (10, 90)],
                      "round_ms_median": round(float(np.median(whole[k])), 3),
                      "round_ms_p10_p90": [round(float(np.percentile(whole[k], q)), 3) for q in (10, 90)]}
        out["front_ratio"] = round(out["feed"]["front_ms_median"] / out["feed_many"]["front_ms_median"], 2)
        out["round_ratio"] = round(out["feed"]["round_ms_median"] / out["feed_many"]["round_ms_median"], 2)
        print(json.dumps(out), flush=True)
        del pools


if "--front" in sys.argv:
    front_section(rounds=_arg("--rounds", 12))
    sys.exit(0)

if "--stream-frames" in sys.argv and _arg("--decoder", "greedy") == "beam":
    beam_long_streams(_arg("--sessions", 64), _arg("--beam", 300), "--scorer" in sys.argv, _arg("--stream-frames", 4000),
                      "--compact" in sys.argv)
    sys.exit(0)

if "--beam-rounds" in sys.argv:
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    _n, _R = _arg("--sessions", 64), _arg("--beam-rounds", 4)
    _vocab = [chr(0x4E00 + i) for i in range(DEFAULT_VOCAB_SIZE)]
    _compact = "--compact" in sys.argv
    _pool = BeamSearchSessions(_n, 2.2, 4.3, 300, 0.99, 40, _vocab, init_frames=16 if _compact else 16 * (_R + 1),
                               compact=_compact)
    _p = _beam_probs(_n, 16, DEFAULT_VOCAB_SIZE, seed=3)
    for _ in range(_R):
        _pool.decode_chunks(list(range(_n)), _p)
    torch.cuda.synchronize()
    print(json.dumps({"beam_rounds": _R, "sessions": _n}))
    sys.exit(0)

if "--decoder" in sys.argv and _arg("--decoder", "greedy") == "beam":
    beam_section()
    beam_end_to_end()
    sys.exit(0)

for _flag in ("--sq-rounds", "--eff-rounds", "--ds2-rounds", "--gen-rounds"):
    if _flag in sys.argv:
        if _flag == "--sq-rounds":
            from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup as _cls
            _model = squeezeformer_model()
        elif _flag == "--ds2-rounds":
            from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2StreamGroup as _cls
            _model = deepspeech2_model(gru="--gru" in sys.argv)
        elif _flag == "--gen-rounds":
            from ppasr_amd.model_utils.conformer.model import GeneralConformerStreamGroup as _cls
            _model = general_model()
        else:
            from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup as _cls
            _model = efficient_conformer_model()
        _n, _R = _arg("--sessions", 1), _arg(_flag, 10)
        _g = _cls(_model, _n, max_frames=16 * (_R + 2))
        _batch = torch.from_numpy(synth_features(1, 67, seed=5)[0]).cuda().repeat(_n, 1, 1).contiguous()
        torch.cuda.synchronize()
        for _ in range(_R):
            _g.encode_chunks(list(range(_n)), _batch)
        torch.cuda.synchronize()
        print(json.dumps({_flag[2:].replace("-", "_"): _R, "sessions": _n}), flush=True)
        sys.exit(0)
if "--squeezeformer" in sys.argv:
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup
    group_section("squeezeformer", squeezeformer_model(), SqueezeformerStreamGroup)
    sys.exit(0)
if "--deepspeech2" in sys.argv:
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2StreamGroup
    _gru = "--gru" in sys.argv
    group_section("deepspeech2_gru" if _gru else "deepspeech2", deepspeech2_model(_gru), DeepSpeech2StreamGroup, n_chunks=4,
                  baseline=("per_session_calls", Ds2BoxSessions))
    sys.exit(0)
if "--general" in sys.argv:
    # (caches: the group holds 16 x (8 + 2) frames per session -- 12 layers x K + V x 512 floats = 48 KB per frame; a
    #  stream handle holds max_len = 5 000 frames, 245 MB, so 256 handles take 63 GB)
    from ppasr_amd.model_utils.conformer.model import GeneralConformerStreamGroup
    group_section("conformer_512", general_model(), GeneralConformerStreamGroup)
    sys.exit(0)
if "--efficient-conformer" in sys.argv:
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup
    group_section("efficient_conformer", efficient_conformer_model(), EfficientConformerStreamGroup)
    sys.exit(0)

V = DEFAULT_VOCAB_SIZE
conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, cnn_module_kernel=15)
sd = conformer_state_dict(vocab_size=V, num_blocks=12, seed=1234)
model = ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
x, _ = synth_features(1, 67, seed=5)
chunk = torch.from_numpy(x).cuda()
n_chunks = 10
for n_sessions in (1, 8, 32, 64):
    sessions = [model.new_stream() for _ in range(n_sessions)]
    streams = [torch.cuda.Stream() for _ in range(n_sessions)]
    for rep in range(2):  # first repetition = warm-up
        for s in sessions:
            s.reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n_chunks):
            for s, st in zip(sessions, streams):
                with torch.cuda.stream(st):
                    s.encode_chunk(chunk, -16, want_probs=False, want_frames=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    audio = n_sessions * n_chunks * 0.64
    print(json.dumps({"sessions": n_sessions, "ms_per_chunk_round": round(dt / n_chunks * 1e3, 2),
                      "audio_s_per_s": round(audio / dt, 1)}), flush=True)

# ---- the same sessions advanced as ONE group call per chunk round ----
from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
for n_sessions in (8, 64, 256, 496):
    group = ConformerStreamGroup(model, n_sessions, max_frames=16 * (n_chunks * 2 + 2))
    batch = chunk.repeat(n_sessions, 1, 1).contiguous()
    ids = list(range(n_sessions))
    for rep in range(2):
        group.reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n_chunks):
            group.encode_chunks(ids, batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    print(json.dumps({"group_sessions": n_sessions, "ms_per_chunk_round": round(dt / n_chunks * 1e3, 2),
                      "audio_s_per_s": round(n_sessions * n_chunks * 0.64 / dt, 1)}), flush=True)
    del group

# ---- the opt-in fp16 x3 GEMM mode (ppasr_set_gemm_mode): the chunk's split-route kernels run their units on that route ----
model.set_gemm_mode("f16x3")
for n_sessions in (1, 8):
    sessions = [model.new_stream() for _ in range(n_sessions)]
    streams = [torch.cuda.Stream() for _ in range(n_sessions)]
    for rep in range(2):
        for s in sessions:
            s.reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n_chunks):
            for s, st in zip(sessions, streams):
                with torch.cuda.stream(st):
                    s.encode_chunk(chunk, -16, want_probs=False, want_frames=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    print(json.dumps({"gemm": "f16x3", "sessions": n_sessions, "ms_per_chunk_round": round(dt / n_chunks * 1e3, 2),
                      "audio_s_per_s": round(n_sessions * n_chunks * 0.64 / dt, 1)}), flush=True)
for n_sessions in (8, 64):
    group = ConformerStreamGroup(model, n_sessions, max_frames=16 * (n_chunks * 2 + 2))
    batch = chunk.repeat(n_sessions, 1, 1).contiguous()
    ids = list(range(n_sessions))
    for rep in range(2):
        group.reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n_chunks):
            group.encode_chunks(ids, batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    print(json.dumps({"gemm": "f16x3", "group_sessions": n_sessions, "ms_per_chunk_round": round(dt / n_chunks * 1e3, 2),
                      "audio_s_per_s": round(n_sessions * n_chunks * 0.64 / dt, 1)}), flush=True)
    del group
