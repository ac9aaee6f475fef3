"""Streaming attention rescoring measured; one JSON line per record, run on one otherwise idle MI355X:

    python tools/bench_stream_rescore.py [--reps R] [--warmup W] [--out profiles/stream_rescore.jsonl]

  rounds  (a) one Conformer session-group round (12 blocks, V = 4233, 67-frame windows -> 16 frames per session) at 8 / 64 /
          256 sessions, without and with a memory arena (``ppasr_encode_chunk_group_mem``: one more launch).
  finish  (b) the end of stream for 1 / 8 / 64 sessions that each hold 250 memory frames, beam 10: ``finish_many`` (the
          pool's n-best, one gather, one ``ppasr_rescore`` call, one read-back) against the only route without the arena:
          the same utterances encoded again offline (1003 feature frames each) plus ``attention_rescoring``.
The variants alternate inside one process, round by round; a host clock around work that ends in a device synchronise;
W warm-up rounds, then median and 10th / 90th percentile over R.  The decoder is synthetic (tests/decoder_cases.py)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ppasr_amd import _lib  # noqa: E402

V, C, UNITS, BLOCKS, BEAM = 4233, 16, 2048, (3, 3), 10
CONF = dict(beam_size=BEAM, ctc_weight=0.5, reverse_weight=0.3, cutoff_prob=0.99, cutoff_top_n=40)


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "p10_p90_ms": [round(float(np.percentile(ms, q)), 3) for q in (10, 90)]}


def rounds_section(model, N, reps, warmup, emit):
    from ppasr_amd.decoders.ctc_alignment import ProbArena
    from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
    from ppasr_amd.utils.synth import synth_features
    total = reps + warmup + 2
    groups = {"off": ConformerStreamGroup(model, N, max_frames=C * total + 32),
              "arena": ConformerStreamGroup(model, N, max_frames=C * total + 32)}
    arena = ProbArena(N, 256, page_frames=16, n_pages=N * total, device="cuda:0")
    x, _ = synth_features(N, 67, seed=11)
    chunks = torch.as_tensor(np.asarray(x, np.float32)).to("cuda:0")
    ids = list(range(N))
    kw = {"off": {}, "arena": dict(memory_arena=arena)}
    ms = {k: [] for k in groups}
    for r in range(warmup + reps):
        for name in (("off", "arena") if r % 2 == 0 else ("arena", "off")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            groups[name].encode_chunks(ids, chunks, want_probs=True, **kw[name])
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    launches, append_ms = {}, None
    for name, group in groups.items():
        with _lib.kernel_profile(max_entries=512) as kp:
            group.encode_chunks(ids, chunks, want_probs=True, **kw[name])
            torch.cuda.synchronize()
        launches[name] = int(sum(c for _, c in kp.kernels.values()))
        if name == "arena":
            append_ms = [round(t, 4) for k, (t, c) in kp.kernels.items() if "k_memory_append" in k]
    emit({"section": "rounds", "sessions": N, "frames_per_round": C, "V": V, "blocks": 12, "reps": reps,
          "off": _stats(ms["off"]), "arena": _stats(ms["arena"]), "launches_per_round": launches,
          "k_memory_append_ms": append_ms, "arena_minus_off_ms": round(float(np.median(ms["arena"]) - np.median(ms["off"])), 3)})


def finish_section(model, rescorer, vocab, n, reps, warmup, emit):
    from ppasr_amd.decoders.attention_rescoring import attention_rescoring
    from ppasr_amd.serving import StreamPool
    from ppasr_amd.utils.synth import synth_features
    T, F = 250, 1003  # ((1003 - 1) / 2 - 1) / 2 = 250
    x, lens = synth_features(n, F, seed=5)
    x = torch.as_tensor(np.asarray(x, np.float32)).to("cuda:0")
    probs, memory = model.get_encoder_out(x, lens, return_memory=True)
    assert probs.shape[1] == T
    # a pool at the end of n streams of 250 frames: the offline encode's rows as its memory and its beam search's table
    pool = StreamPool(model, vocab, n, decoder="attention_rescoring", rescorer=rescorer, decoder_conf=dict(CONF),
                      memory_seconds=T * 0.04)
    ids = list(range(n))
    for a in range(0, T, C):
        pool.memory.append(ids, memory[:, a:a + C].contiguous())
        res = pool.beam.decode_chunks(ids, probs[:, a:a + C].contiguous())
    for i, (score, text) in zip(ids, res):
        pool.sessions[i].result = {"text": text, "score": score}

    def offline():
        p, m = model.get_encoder_out(x, lens, return_memory=True)
        return attention_rescoring(model, rescorer, p, m, None, vocab, **CONF)

    ms = {"finish_many": [], "offline": []}
    out = {}
    for r in range(warmup + reps):
        for name in (("finish_many", "offline") if r % 2 == 0 else ("offline", "finish_many")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = pool.finish_many(ids) if name == "finish_many" else offline()
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    same = [o["text"] for o in out["finish_many"]] == [t for _, t in out["offline"]]
    emit({"section": "finish", "sessions": n, "memory_frames": T, "beam": BEAM, "V": V, "reps": reps,
          "finish_many": _stats(ms["finish_many"]), "offline_reencode_and_rescore": _stats(ms["offline"]),
          "ratio_offline_over_finish_many": round(float(np.median(ms["offline"]) / np.median(ms["finish_many"])), 2),
          "rescored": all(o["rescored"] for o in out["finish_many"]), "texts_equal": same})


if __name__ == "__main__":
    import decoder_cases as dc
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    from ppasr_amd.utils.synth import conformer_state_dict, synth_vocabulary
    reps, warmup = _arg("--reps", 20), _arg("--warmup", 3)
    path = _arg("--out", None, str)
    sd = conformer_state_dict(vocab_size=V, num_blocks=12, seed=1234)
    sd.update(dc.decoder_state_dict(4321, V, UNITS, *BLOCKS))
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, cnn_module_kernel=15)
    model = ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    rescorer = AttentionRescorer(sd, V, decoder_conf=dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0],
                                                          r_num_blocks=BLOCKS[1]))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "a", encoding="utf-8") as f:
                f.write(line + "\n")

    for N in (8, 64, 256):
        rounds_section(model, N, reps, warmup, emit)
    for n in (1, 8, 64):
        finish_section(model, rescorer, synth_vocabulary(V), n, reps, warmup, emit)
