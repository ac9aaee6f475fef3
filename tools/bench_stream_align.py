"""Token timestamps of streams measured; one JSON line per section, run on one otherwise idle MI355X:

    python tools/bench_stream_align.py [--reps R] [--warmup W] [--out profiles/stream_align_rounds.jsonl]

  rounds  (a) one StreamPool round of 64 Conformer sessions (12 blocks, V = 4233, beam 10, 16 output frames per session):
          ``timestamps=False``; ``timestamps=True`` (the round's probabilities go into the ProbArena with one launch); and
          the workaround a user would write without the arena: a pool without timestamps whose round copies every
          session's slice of the round's table and appends it to a Python list (one copy launch per session).
  finish  (b) end of stream for 64 sessions x 750 frames x 30-50 tokens: one ``ProbArena.align`` call for all of them
          against ``torch.cat`` of a session's list plus ``align_one`` for every session in turn.
The variants alternate inside one process, round by round; a host clock around work that ends in a device synchronise;
W warm-up rounds, then median and 10th / 90th percentile over R."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ppasr_amd import _lib  # noqa: E402
from ppasr_amd.serving import StreamPool  # noqa: E402

V, N, C = 4233, 64, 16
BEAM = dict(alpha=2.2, beta=4.3, beam_size=10, num_processes=10, cutoff_prob=0.99, cutoff_top_n=40, language_model_path=None)


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "p10_p90_ms": [round(float(np.percentile(ms, q)), 3) for q in (10, 90)]}


class SlicesPool(StreamPool):
    """The workaround: keep every session's rows of every round as a tensor of its own"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.kept = [[] for _ in self.sessions]

    def _advance(self, ids, chunks):
        _, _, probs = self.group.encode_chunks(ids, chunks, want_probs=True)
        for k, i in enumerate(ids):
            self.kept[i].append(probs[k].clone())  # (a view would be overwritten by the next round)
        return [{"text": text, "score": score} for score, text in self.beam.decode_chunks(ids, probs)]


def rounds_section(reps, warmup, emit):
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    from ppasr_amd.utils.synth import conformer_state_dict, synth_features, synth_vocabulary
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, cnn_module_kernel=15)
    model = ConformerModel(80, V, streaming=True, encoder_conf=conf,
                           state_dict=conformer_state_dict(vocab_size=V, num_blocks=12, seed=1234), device="cuda:0")
    vocab = synth_vocabulary(V)
    seconds = 0.64 * (reps + warmup + 2)
    kw = dict(n_sessions=N, max_seconds=seconds + 2.0, decoder="ctc_beam_search", decoder_conf=dict(BEAM))
    pools = {"off": StreamPool(model, vocab, **kw),
             "arena": StreamPool(model, vocab, timestamps=True, table_seconds=seconds, **kw),
             "slices": SlicesPool(model, vocab, **kw)}
    x, _ = synth_features(N, 67, seed=11)
    chunks = torch.as_tensor(np.asarray(x, np.float32)).to("cuda:0")
    ids = list(range(N))
    ms = {k: [] for k in pools}
    for r in range(warmup + reps):
        for name in (list(pools) if r % 2 == 0 else list(pools)[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pools[name]._advance(ids, chunks)
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    launches = {}
    for name, pool in pools.items():
        with _lib.kernel_profile() as kp:
            pool._advance(ids, chunks)
            torch.cuda.synchronize()
        launches[name] = int(sum(c for _, c in kp.kernels.values()))
        if name == "arena":
            append_ms = [round(t, 4) for k, (t, c) in kp.kernels.items() if "arena_append_kernel" in k]
    same = all(bool((pools["arena"].session_probs(s) == torch.cat(pools["slices"].kept[s])).all()) for s in (0, N - 1))
    emit({"section": "rounds", "sessions": N, "frames_per_round": C, "V": V, "beam": 10, "blocks": 12, "reps": reps,
          "off": _stats(ms["off"]), "arena": _stats(ms["arena"]), "slices": _stats(ms["slices"]),
          "library_launches_per_round": launches, "torch_copy_launches_per_round_slices": N,
          "arena_append_kernel_ms": append_ms, "arena_minus_off_ms": round(float(np.median(ms["arena"]) - np.median(ms["off"])), 3),
          "slices_minus_off_ms": round(float(np.median(ms["slices"]) - np.median(ms["off"])), 3),
          "arena_not_slower_than_slices": bool(np.median(ms["arena"]) <= np.median(ms["slices"])),
          "tables_equal": same})


def finish_section(reps, warmup, emit):
    from ppasr_amd.decoders.ctc_alignment import ProbArena, align_one
    T = 750
    g = torch.Generator(device="cuda:0").manual_seed(3)
    arena = ProbArena(N, V, page_frames=16, n_pages=N * 47)
    kept = [[] for _ in range(N)]
    ids = list(range(N))
    for t0 in range(0, T, C):
        z = torch.randn(N, C, V, generator=g, device="cuda:0") * 3.0
        z[:, :, 0] += 4.0 * (torch.rand(N, C, generator=g, device="cuda:0") < 0.5)
        probs = torch.softmax(z, dim=2)
        f = min(C, T - t0)
        arena.append(ids, probs, [f] * N)
        for s in ids:
            kept[s].append(probs[s, :f].clone())
    rng = np.random.default_rng(4)
    toks = [rng.integers(1, V, rng.integers(30, 51)).tolist() for _ in ids]
    ms = {"arena": [], "cat": []}
    out = {}
    for r in range(warmup + reps):
        for name in (("arena", "cat") if r % 2 == 0 else ("cat", "arena")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "arena":
                out[name] = arena.align(ids, toks)
            else:
                out[name] = [align_one(torch.cat(kept[s]), toks[s]) for s in ids]
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    with _lib.kernel_profile() as kp:
        arena.align(ids, toks)
        torch.cuda.synchronize()
    kernels = {k.split("(")[0].split("::")[-1]: [round(t, 4), int(c)] for k, (t, c) in sorted(kp.kernels.items())}
    emit({"section": "finish", "sessions": N, "frames": T, "V": V, "tokens": "30-50", "reps": reps,
          "arena_one_call": _stats(ms["arena"]), "cat_and_align_per_session": _stats(ms["cat"]),
          "arena_kernels_ms_launches": kernels,
          "ratio_cat_over_arena": round(float(np.median(ms["cat"]) / np.median(ms["arena"])), 2),
          "arena_not_slower_than_cat": bool(np.median(ms["arena"]) <= np.median(ms["cat"])),
          "results_equal": out["arena"] == out["cat"]})


if __name__ == "__main__":
    reps, warmup = _arg("--reps", 20), _arg("--warmup", 3)
    path = _arg("--out", None, str)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "a", encoding="utf-8") as f:
                f.write(line + "\n")

    rounds_section(reps, warmup, emit)
    finish_section(reps, warmup, emit)
