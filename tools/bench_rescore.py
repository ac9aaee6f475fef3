"""Attention rescoring (csrc/rescore_kernels.hip) measured; one JSON line per section, run on one otherwise idle MI355X:

    python tools/bench_rescore.py [--reps R] [--warmup W] [--out profiles/rescore_rounds.jsonl]

Workloads: the headline shape (B = 32 utterances of 10 s -> T' = 249, V = 4233, nbest 10, hypotheses of 30-50 tokens, 3 + 3
decoder blocks of 1024 units) and B = 1.
  rescore   ``ppasr_rescore`` alone on synthetic hypotheses, against the same decoder run by tests/decoder_oracle.py
            (``rescore_batched``, float32, torch on the same device: rocBLAS GEMMs over padded [B * nbest, L] rows with the
            [.., V] logits materialised -- the only available stand-in for "the reference on this GPU"); the kernels' own
            time per kernel (dispatch-attached events) and launches per call.
  decode    on the probabilities of a synthetic 12-block Conformer: beam search (beam 10) alone, and beam search +
            rescoring (``attention_rescoring``).
  predict   the whole ``PPASRPredictor.predict`` of one 10 s waveform with ctc_greedy, ctc_beam_search (beam 10) and
            attention_rescoring (B = 1 only: predict takes one utterance).
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

V, TP, NBEST, UNITS, BLOCKS = 4233, 249, 10, 1024, (3, 3)
DEC_CONF = dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0], r_num_blocks=BLOCKS[1])
WEIGHTS = dict(ctc_weight=0.5, reverse_weight=0.3)


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


def _hyps(B, seed, mt=50):
    rng = np.random.default_rng(seed)
    lens = rng.integers(30, mt + 1, (B, NBEST)).astype(np.int32)
    tokens = np.full((B, NBEST, mt), -1, np.int32)
    for b in range(B):
        for k in range(NBEST):
            tokens[b, k, :lens[b, k]] = rng.integers(1, V - 1, lens[b, k])
    ctc = np.cumsum(rng.uniform(0.5, 6.0, (B, NBEST)), axis=1)
    memory = rng.standard_normal((B, TP, 256)).astype(np.float32)
    dev = "cuda:0"
    return (torch.from_numpy(memory).to(dev), torch.from_numpy(tokens).to(dev), torch.from_numpy(lens).to(dev),
            torch.from_numpy(ctc).to(dev))


def rescore_section(B, sd, reps, warmup, emit):
    from decoder_oracle import DecoderOracle
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    r = AttentionRescorer(sd, V, DEC_CONF)
    memory, tokens, lens, ctc = _hyps(B, seed=B)
    hip = _timed(lambda: r.rescore(memory, None, tokens, lens, ctc, **WEIGHTS), reps, warmup)
    with _lib.kernel_profile() as kp:
        res = r.rescore(memory, None, tokens, lens, ctc, **WEIGHTS)
        torch.cuda.synchronize()
    o32 = DecoderOracle(sd, V, *BLOCKS, dtype=torch.float32).to("cuda:0")
    with torch.no_grad():
        tor = _timed(lambda: o32.rescore_batched(memory, None, tokens, lens, ctc, **WEIGHTS), reps, warmup)
        t_att, t_r, t_total, t_best = o32.rescore_batched(memory, None, tokens, lens, ctc, **WEIGHTS)
    kernels = {k.split("(")[0].split("::")[-1]: [round(ms, 3), int(c)] for k, (ms, c) in sorted(kp.kernels.items())}
    emit({"section": "rescore", "B": B, "Tp": TP, "V": V, "nbest": NBEST, "tokens": "30-50", "blocks": list(BLOCKS),
          "rows": int((lens + 1).sum()) * 2, "reps": reps, "hip": _stats(hip), "torch_f32_padded": _stats(tor),
          "ratio_torch_over_hip": round(float(np.median(tor) / np.median(hip)), 2),
          "kernels_ms_launches": kernels, "kernel_ms_total": round(sum(v[0] for v in kernels.values()), 3),
          "launches": int(sum(v[1] for v in kernels.values())),
          "max_abs_total_difference_to_torch": round(float((res["total"] - t_total).abs().max()), 6),
          "same_best": bool((res["best"] == t_best).all())})


def decode_section(B, sd, reps, warmup, emit):
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer, attention_rescoring
    from ppasr_amd.decoders.beam_search_decoder import beam_search_ids
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    from ppasr_amd.utils.synth import synth_features, synth_vocabulary
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, cnn_module_kernel=15)
    model = ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    r = AttentionRescorer(sd, V, DEC_CONF)
    x, lens = synth_features(B, 1000, seed=20240 + B)
    probs, memory = model.get_encoder_out(x, lens, return_memory=True)
    vocab = synth_vocabulary(V)
    beam = _timed(lambda: beam_search_ids(probs, NBEST, 0.99, 40, nbest=NBEST), reps, warmup)
    both = _timed(lambda: attention_rescoring(model, r, probs, memory, None, vocab, beam_size=NBEST, **WEIGHTS), reps, warmup)
    _, hl, _, _ = beam_search_ids(probs, NBEST, 0.99, 40, nbest=NBEST)
    emit({"section": "decode", "B": B, "Tp": int(probs.shape[1]), "V": V, "beam": NBEST, "reps": reps,
          "hypothesis_tokens_mean": round(float(hl[hl >= 0].float().mean()), 1),
          "beam_search": _stats(beam), "beam_search_plus_rescoring": _stats(both)})


def predict_section(sd, reps, warmup, emit):
    from ppasr_amd.predict import PPASRPredictor
    from ppasr_amd.utils.synth import synth_vocabulary
    rng = np.random.Generator(np.random.PCG64(5))
    t = np.arange(160000) / 16000.0
    wav = (0.1 * np.sin(2 * np.pi * 220 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(t.shape))
    wav = wav.astype(np.float32)
    out = {"section": "predict", "seconds": 10.0, "V": V, "reps": reps}
    for dec in ("ctc_greedy", "ctc_beam_search", "attention_rescoring"):
        cfg = dict(encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, cnn_module_kernel=15),
                   decoder_conf=dict(DEC_CONF),
                   preprocess_conf=dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True,
                                        target_dB=-20),
                   ctc_beam_search_decoder_conf=dict(alpha=2.2, beta=4.3, beam_size=NBEST, num_processes=10, cutoff_prob=0.99,
                                                     cutoff_top_n=40, language_model_path=None),
                   attention_rescoring_decoder_conf=dict(beam_size=NBEST, cutoff_prob=0.99, cutoff_top_n=40, **WEIGHTS),
                   use_model="conformer", streaming=True, decoder=dec, metrics_type="cer")
        p = PPASRPredictor(configs=cfg, state_dict=sd, vocab_list=synth_vocabulary(V), warmup=False)
        out[dec] = _stats(_timed(lambda: p.predict(audio_data=wav), reps, warmup))
    emit(out)


if __name__ == "__main__":
    import decoder_cases as dc
    from ppasr_amd.utils.synth import conformer_state_dict
    reps, warmup = _arg("--reps", 10), _arg("--warmup", 3)
    path = _arg("--out", None, str)
    sd = conformer_state_dict(vocab_size=V, num_blocks=12, seed=1234)
    sd.update(dc.decoder_state_dict(4321, V, UNITS, *BLOCKS))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if path:
            with open(path, "a", encoding="utf-8") as f:
                f.write(line + "\n")

    for B in (32, 1):
        rescore_section(B, sd, reps, warmup, emit)
    for B in (32, 1):
        decode_section(B, sd, reps, warmup, emit)
    predict_section(sd, reps, warmup, emit)
