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
  --eff-rounds R --sessions N  R Efficient-Conformer group rounds of N sessions, for the dispatch count as above"""
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


def group_section(family, model, group_cls, n_chunks=8, sizes=(1, 8, 64, 256), reps=3):
    """ms per round and audio-s/s of one 0.64 s chunk per session per round: the group (one set of launches per round)
    and StreamHandleSet (one stream handle per session, what make_stream_group gives this family) at the same n,
    measured alternately (warm-up, then `reps` timed passes of each; the median is printed)."""
    from ppasr_amd.model_utils.conformer.model import StreamHandleSet
    x, _ = synth_features(1, 67, seed=5)
    chunk = torch.from_numpy(x).cuda()
    for n in sizes:
        batch = chunk.repeat(n, 1, 1).contiguous()
        ids = list(range(n))
        kinds = {"group": group_cls(model, n, max_frames=16 * (n_chunks + 2)),
                 "handle_set": StreamHandleSet(model, n)}
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


for _flag in ("--sq-rounds", "--eff-rounds"):
    if _flag in sys.argv:
        if _flag == "--sq-rounds":
            from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup as _cls
            _model = squeezeformer_model()
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
