"""The loss half of evaluation (csrc/ctc_loss.hip, k_dec_output<true> of csrc/rescore_kernels.hip) measured; one JSON line per
section, run on one otherwise idle MI355X:

    python tools/bench_loss.py [--reps R] [--warmup W] [--out profiles/loss_device_vs_torch.jsonl]

  ctc_nll    32 utterances x 250 frames x V = 4233 with 40-token labels on the device-resident table: ``ctc_nll`` against
             ``torch.nn.functional.ctc_loss`` (fp32, log of the same table, reduction none) on the same device, and against
             the route a caller had before: download the table, ``ctc_loss`` on the CPU.
  att_loss   ``AttentionRescorer.loss`` at 32 x 40 tokens (3 + 3 blocks of 1024 units, T' = 249) against the same decoder run
             by tests/decoder_oracle.py (``rescore_batched`` with nbest 1, float32, torch on the same device: padded rows,
             the [B, L, V] logits materialised, log_softmax and the targets' gather) plus the smoothed target and
             ``kl_div`` on a [B, L, V] tensor per direction, timed separately and added.
  evaluate   ``evaluate(return_loss=True)`` per batch of 32 x 10 s against ``evaluate()`` (the default call runs the code
             path it ran before the loss half existed): the price of the loss half.
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

V, TP, UNITS, BLOCKS, B, TOKENS = 4233, 249, 1024, (3, 3), 32, 40
DEC_CONF = dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0], r_num_blocks=BLOCKS[1])
LOSS = dict(ctc_weight=0.3, lsm_weight=0.1, reverse_weight=0.3)


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


def _kernels(kp):
    return {k.split("(")[0].split("::")[-1]: [round(ms, 3), int(c)] for k, (ms, c) in sorted(kp.kernels.items())}


def ctc_section(reps, warmup, emit):
    from ppasr_amd.model_utils.loss import ctc_nll
    rng = np.random.default_rng(1)
    T = 250
    probs = torch.softmax(torch.from_numpy(rng.standard_normal((B, T, V)).astype(np.float32) * 3.0).cuda(), -1)
    labels = torch.from_numpy(rng.integers(1, V, (B, TOKENS)).astype(np.int32)).cuda()
    lens = torch.full((B,), TOKENS, dtype=torch.int32, device="cuda")
    frames = torch.full((B,), T, dtype=torch.int32, device="cuda")
    hip = _timed(lambda: ctc_nll(probs, labels, lens, frames), reps, warmup)
    with _lib.kernel_profile() as kp:
        mine = ctc_nll(probs, labels, lens, frames)["nll"]
        torch.cuda.synchronize()

    def torch_dev():
        lp = torch.log(torch.clamp(probs, min=torch.finfo(torch.float32).tiny)).transpose(0, 1)
        return torch.nn.functional.ctc_loss(lp, labels.long(), frames.long(), lens.long(), blank=0, reduction="none")

    def torch_cpu():
        p = probs.cpu()
        lp = torch.log(torch.clamp(p, min=torch.finfo(torch.float32).tiny)).transpose(0, 1)
        return torch.nn.functional.ctc_loss(lp, labels.cpu().long(), frames.cpu().long(), lens.cpu().long(), blank=0,
                                            reduction="none")

    dev = _timed(torch_dev, reps, warmup)
    cpu = _timed(torch_cpu, reps, warmup)
    emit({"section": "ctc_nll", "B": B, "T": T, "V": V, "tokens": TOKENS, "reps": reps, "hip": _stats(hip),
          "torch_same_device": _stats(dev), "download_plus_torch_cpu": _stats(cpu),
          "ratio_torch_device_over_hip": round(float(np.median(dev) / np.median(hip)), 2),
          "ratio_cpu_route_over_hip": round(float(np.median(cpu) / np.median(hip)), 2),
          "kernels_ms_launches": _kernels(kp),
          "max_abs_difference_to_torch_device": round(float((mine - torch_dev()).abs().max()), 6)})


def att_section(sd, reps, warmup, emit):
    from decoder_oracle import DecoderOracle
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    rng = np.random.default_rng(2)
    r = AttentionRescorer(sd, V, DEC_CONF)
    memory = torch.from_numpy(rng.standard_normal((B, TP, 256)).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(1, V - 1, (B, TOKENS)).astype(np.int32)).cuda()
    lens = torch.full((B,), TOKENS, dtype=torch.int32, device="cuda")
    lsm, rw = LOSS["lsm_weight"], LOSS["reverse_weight"]
    hip = _timed(lambda: r.loss(memory, None, labels, lens, lsm, rw), reps, warmup)
    with _lib.kernel_profile() as kp:
        r.loss(memory, None, labels, lens, lsm, rw)
        torch.cuda.synchronize()
    plain = _timed(lambda: r.rescore(memory, None, labels[:, None], lens[:, None], torch.zeros(B, 1, dtype=torch.float64), 0.0,
                                     rw), reps, warmup)
    o32 = DecoderOracle(sd, V, *BLOCKS, dtype=torch.float32).to("cuda:0")
    zeros = torch.zeros(B, 1, dtype=torch.float64, device="cuda")
    with torch.no_grad():
        dec = _timed(lambda: o32.rescore_batched(memory, None, labels[:, None], lens[:, None], zeros, 0.0, rw), reps, warmup)
    logits = torch.from_numpy(rng.standard_normal((B * (TOKENS + 1), V)).astype(np.float32)).cuda()
    target = torch.from_numpy(rng.integers(1, V, B * (TOKENS + 1))).cuda()

    def kl():  # label_smoothing_loss.py:68-91 on the materialised logits, once per direction
        for _ in range(2):
            t = torch.full_like(logits, lsm / (V - 1))
            t.scatter_(1, target[:, None], 1.0 - lsm)
            torch.nn.functional.kl_div(torch.log_softmax(logits, 1), t, reduction="none").sum()

    klt = _timed(kl, reps, warmup)
    tor = float(np.median(dec) + np.median(klt))
    emit({"section": "att_loss", "B": B, "Tp": TP, "V": V, "tokens": TOKENS, "blocks": list(BLOCKS), "reps": reps,
          "hip_loss": _stats(hip), "hip_rescore_same_rows": _stats(plain), "torch_f32_decoder": _stats(dec),
          "torch_f32_kl_div": _stats(klt), "torch_total_median_ms": round(tor, 3),
          "ratio_torch_over_hip": round(tor / float(np.median(hip)), 2), "kernels_ms_launches": _kernels(kp)})


def evaluate_section(sd, reps, warmup, emit):
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    from ppasr_amd.evaluate import evaluate
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    from ppasr_amd.utils.synth import synth_features, synth_vocabulary
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12, cnn_module_kernel=15)
    model = ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    r = AttentionRescorer(sd, V, DEC_CONF)
    vocab = synth_vocabulary(V)
    rng = np.random.default_rng(3)
    x, lens = synth_features(B, 1000, seed=20240 + B)
    labels = rng.integers(1, V - 1, (B, TOKENS)).astype(np.int64)
    batches = [(x, labels, lens, np.full(B, TOKENS, np.int64))]
    base = _timed(lambda: evaluate(model, batches, vocab), reps, warmup)
    one_stream = _timed(lambda: evaluate(model, batches, vocab, overlap_decode=False), reps, warmup)
    ctc_only = _timed(lambda: evaluate(model, batches, vocab, return_loss=True, loss_conf=dict(ctc_weight=1.0)), reps, warmup)
    full = _timed(lambda: evaluate(model, batches, vocab, return_loss=True, loss_conf=LOSS, rescorer=r), reps, warmup)
    emit({"section": "evaluate", "B": B, "frames": 1000, "V": V, "tokens": TOKENS, "decoder": "ctc_greedy", "reps": reps,
          "evaluate": _stats(base), "evaluate_one_stream": _stats(one_stream), "return_loss_ctc_only": _stats(ctc_only),
          "return_loss_ctc_and_attention": _stats(full),
          "price_ms_per_batch": round(float(np.median(full) - np.median(base)), 3)})


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

    ctc_section(reps, warmup, emit)
    att_section(sd, reps, warmup, emit)
    evaluate_section(sd, reps, warmup, emit)
