"""CTC forced alignment (csrc/ctc_align.hip) measured; one JSON line per section, run on one otherwise idle MI355X:

    python tools/bench_align.py [--reps R] [--warmup W] [--out profiles/align_rounds.jsonl]

Workloads: the rescorer's headline shape (B = 32 utterances x 250 frames x V = 4233, 30-50 tokens each) and one 30 s
utterance (750 frames) at 255 tokens.
  align     ``ppasr_ctc_align`` through ``ctc_align_ids`` on a device-resident table, the kernels' own time per kernel
            (dispatch-attached events), and what a user would otherwise do: download the table and run the same Viterbi
            in numpy on the host (tests/align_oracle.py in float32, utterance by utterance; the download is timed with it
            and also on its own).
  predict   ``PPASRPredictor.predict`` of one 10 s waveform with and without ``timestamps=True`` (12-block Conformer,
            ctc_greedy and ctc_beam_search), and the alignment's share of the call with timestamps.
A host clock around work that ends in a device synchronise; W warm-up calls, then median and 10th / 90th percentile over R."""
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

V = 4233


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "p10_p90_ms": [round(float(np.percentile(ms, q)), 3) for q in (10, 90)]}


def _timed(fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _case(B, Tp, lo, hi, seed):
    """a softmax table with the blank raised on half the frames, and lo..hi random tokens per utterance"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = torch.randn(B, Tp, V, generator=g) * 3.0
    z[:, :, 0] += 4.0 * (torch.rand(B, Tp, generator=g) < 0.5)
    probs = torch.softmax(z, dim=2).to("cuda:0")
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, B).astype(np.int32)
    tokens = np.full((B, hi), -1, np.int32)
    for b in range(B):
        tokens[b, :lens[b]] = rng.integers(1, V, lens[b])
    return probs, torch.from_numpy(tokens).to("cuda:0"), torch.from_numpy(lens).to("cuda:0"), tokens, lens


def align_section(B, Tp, lo, hi, reps, warmup, emit):
    import align_oracle as ao
    from ppasr_amd.decoders.ctc_alignment import ctc_align_ids
    probs, tk, nt, tk_np, nt_np = _case(B, Tp, lo, hi, seed=B + Tp)
    hip = _timed(lambda: ctc_align_ids(probs, tk, nt), reps, warmup)
    with _lib.kernel_profile() as kp:
        out = ctc_align_ids(probs, tk, nt)
        torch.cuda.synchronize()

    def host():
        p = probs.cpu().numpy()
        return [ao.align(p[b], tk_np[b, :nt_np[b]], dtype=np.float32, max_tokens=hi) for b in range(B)]

    host_ms = _timed(host, max(reps // 2, 3), 1)
    down = _timed(lambda: probs.cpu(), reps, warmup)
    ref = host()
    ft = out["frame_token"].cpu().numpy()
    kernels = {k.split("(")[0].split("::")[-1]: [round(ms, 4), int(c)] for k, (ms, c) in sorted(kp.kernels.items())}
    emit({"section": "align", "B": B, "Tp": Tp, "V": V, "tokens": f"{lo}-{hi}" if lo != hi else str(hi), "reps": reps,
          "hip": _stats(hip), "kernels_ms_launches": kernels,
          "kernel_ms_total": round(sum(v[0] for v in kernels.values()), 4),
          "numpy_f32_host_with_download": _stats(host_ms), "download_alone": _stats(down),
          "ratio_host_over_hip": round(float(np.median(host_ms) / np.median(hip)), 1),
          "all_status_ok": bool((out["status"] == 0).all()),
          "utterances_with_the_host_walks_path": int(sum((ft[b] == ref[b]["frame_token"]).all() for b in range(B)))})


def predict_section(reps, warmup, emit):
    from ppasr_amd.predict import PPASRPredictor
    from ppasr_amd.utils.synth import conformer_state_dict, synth_vocabulary
    sd = conformer_state_dict(vocab_size=V, num_blocks=12, seed=1234)
    rng = np.random.Generator(np.random.PCG64(5))
    t = np.arange(160000) / 16000.0
    wav = (0.1 * np.sin(2 * np.pi * 220 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(t.shape))
    wav = wav.astype(np.float32)
    out = {"section": "predict", "seconds": 10.0, "V": V, "reps": reps}
    for dec in ("ctc_greedy", "ctc_beam_search"):
        cfg = dict(encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, cnn_module_kernel=15),
                   preprocess_conf=dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True,
                                        target_dB=-20),
                   ctc_beam_search_decoder_conf=dict(alpha=2.2, beta=4.3, beam_size=10, num_processes=10, cutoff_prob=0.99,
                                                     cutoff_top_n=40, language_model_path=None),
                   use_model="conformer", streaming=True, decoder=dec, metrics_type="cer")
        p = PPASRPredictor(configs=cfg, state_dict=sd, vocab_list=synth_vocabulary(V), warmup=False)
        plain = _timed(lambda: p.predict(audio_data=wav), reps, warmup)
        stamped = _timed(lambda: p.predict(audio_data=wav, timestamps=True), reps, warmup)
        n = len(p.predict(audio_data=wav, timestamps=True)["timestamps"])
        out[dec] = {"tokens": n, "predict": _stats(plain), "predict_timestamps": _stats(stamped),
                    "alignment_share_of_predict_timestamps": round(
                        float((np.median(stamped) - np.median(plain)) / np.median(stamped)), 3)}
    emit(out)


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

    align_section(32, 250, 30, 50, reps, warmup, emit)
    align_section(1, 750, 255, 255, reps, warmup, emit)
    predict_section(reps, warmup, emit)
