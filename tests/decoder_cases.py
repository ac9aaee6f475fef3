"""Seeded synthetic attention decoders under the reference's parameter names, and the case table of the rescoring tests.

Everything is regenerated from a seed: weights (decoder_state_dict), encoder memories, hypotheses and CTC scores
(inputs).  LayerNorm gains / biases and the embedding are non-trivial, and the output layer is scaled so that the
log-probabilities of a row spread over several nats.

A case is admitted only if, for every utterance, the float64 top-2 margin of `total` exceeds MARGIN_FACTOR x the score
tolerance (score_tol): then `best` must equal the float64 argmax (tests/test_rescore_oracle_cpu.py asserts it for the
whole table, so nothing is skipped at run time)."""
import numpy as np

import numerics

D, HEADS = 256, 4
MARGIN_FACTOR = 100.0


def decoder_state_dict(seed, V, units, num_blocks, r_num_blocks, d=D):
    rng = np.random.default_rng(seed)
    sd = {}

    def lin(name, k, n, gain=1.0):
        sd[name + ".weight"] = (rng.standard_normal((k, n)) * (gain / np.sqrt(k))).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(n) * 0.1).astype(np.float32)

    def norm(name):
        sd[name + ".weight"] = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)
        sd[name + ".bias"] = (0.1 * rng.standard_normal(d)).astype(np.float32)

    for side, blocks in (("left", num_blocks), ("right", r_num_blocks)):
        p = f"decoder.{side}_decoder"
        sd[p + ".embed.0.weight"] = (rng.standard_normal((V, d)) * 0.3).astype(np.float32)
        norm(p + ".after_norm")
        lin(p + ".output_layer", d, V, gain=2.5)  # logits of a row spread over ~ +-8
        for i in range(blocks):
            lp = f"{p}.decoders.{i}"
            for att in ("self_attn", "src_attn"):
                for m in ("linear_q", "linear_k", "linear_v", "linear_out"):
                    lin(f"{lp}.{att}.{m}", d, d, gain=1.5 if m in ("linear_q", "linear_k") else 1.0)
            lin(lp + ".feed_forward.w_1", d, units)
            lin(lp + ".feed_forward.w_2", units, d)
            for nm in ("norm1", "norm2", "norm3"):
                norm(f"{lp}.{nm}")
    return sd


# name -> case.  L = max_tokens + 1; `short`: out_lens < Tp for some utterances; hyp lengths are mixed, with the empty
# hypothesis and absent ones (lens = -1) in every case that has room for them.
def _c(seed, V, L, nbest, B, Tp, blocks, units, rw, short=True):
    return dict(seed=seed, V=V, L=L, nbest=nbest, B=B, Tp=Tp, blocks=blocks, units=units, reverse_weight=rw, short=short,
                ctc_weight=0.5)


CASES = {
    "v67_l17_n3_b3_t33": _c(1, 67, 17, 3, 3, 33, (3, 3), 1024, 0.3),
    "v67_l1_n1_b1_t1": _c(2, 67, 1, 1, 1, 1, (1, 0), 1024, 0.0, short=False),
    "v67_l2_n3_b1_t31": _c(3, 67, 2, 3, 1, 31, (3, 3), 2048, 0.3),
    "v67_l16_n10_b3_t100": _c(4, 67, 16, 10, 3, 100, (3, 3), 1024, 0.3),
    "v67_l33_n3_b1_t33": _c(5, 67, 33, 3, 1, 33, (6, 2), 2048, 0.3),
    "v67_l65_n10_b3_t31": _c(6, 67, 65, 10, 3, 31, (3, 3), 1024, 0.3),
    "v67_l64_n3_b1_t100": _c(7, 67, 64, 3, 1, 100, (1, 0), 2048, 0.0),
    "v4233_l17_n3_b3_t33": _c(8, 4233, 17, 3, 3, 33, (3, 3), 1024, 0.3),
    "v4233_l33_n10_b1_t100": _c(9, 4233, 33, 10, 1, 100, (3, 3), 1024, 0.0),
    "v4233_l65_n3_b3_t31": _c(10, 4233, 65, 3, 3, 31, (6, 2), 2048, 0.3),
    "v4233_l1_n3_b1_t1": _c(11, 4233, 1, 3, 1, 1, (3, 3), 1024, 0.3, short=False),
    "v4233_l16_n1_b3_t33": _c(12, 4233, 16, 1, 3, 33, (1, 0), 1024, 0.0),
}
FIXTURE_CASES = ("v67_l17_n3_b3_t33", "v67_l2_n3_b1_t31", "v67_l33_n3_b1_t33")  # tests/golden/ref_decoder.npz


def weights(case):
    return decoder_state_dict(1000 + case["seed"], case["V"], case["units"], *case["blocks"])


def inputs(case):
    """-> dict(memory [B, Tp, D] f32, out_lens [B] i32, tokens [B, nbest, L - 1] i32, lens [B, nbest] i32,
    ctc_scores [B, nbest] f64).  Tokens are 1 .. V - 2 (0 = blank and V - 1 = sos / eos never appear in a CTC hypothesis);
    slots behind a hypothesis hold -1, as ppasr_ctc_beam_search leaves them."""
    rng = np.random.default_rng(case["seed"])
    B, nbest, L, Tp, V = case["B"], case["nbest"], case["L"], case["Tp"], case["V"]
    mt = L - 1
    memory = rng.standard_normal((B, Tp, D)).astype(np.float32)
    out_lens = np.full(B, Tp, np.int32)
    if case["short"] and Tp > 1:
        for b in range(B):
            if b % 2 == 0:
                out_lens[b] = max(1, int(rng.integers(Tp // 2, Tp)))
    tokens = np.full((B, nbest, max(mt, 1)), -1, np.int32)[:, :, :mt]
    lens = np.zeros((B, nbest), np.int32)
    for b in range(B):
        for k in range(nbest):
            n = int(rng.integers(0, mt + 1))
            if k == 0:
                n = mt  # the longest row count L is reached in every utterance
            if nbest >= 3 and k == 1:
                n = 0  # the empty hypothesis
            if nbest >= 3 and k == nbest - 1:
                n = -1  # absent
            lens[b, k] = n
            if n > 0:
                tokens[b, k, :n] = rng.integers(1, V - 1, n)
    ctc = np.cumsum(rng.uniform(0.5, 6.0, (B, nbest)), axis=1) + rng.uniform(0.0, 30.0, (B, 1))
    return dict(memory=memory, out_lens=out_lens, tokens=np.ascontiguousarray(tokens), lens=lens,
                ctc_scores=ctc.astype(np.float64))


def poison_memory(inp, value=np.nan):
    """a copy of the memory with `value` behind every utterance's out_lens"""
    m = inp["memory"].copy()
    for b, n in enumerate(inp["out_lens"]):
        m[b, int(n):] = value
    return m


def logit_scale(ref, b):
    """max |logit - row mean| over utterance b's rows: the scale one row's log-probability error is measured in"""
    lg = ref["logits"][b]
    return float(np.abs(lg - lg.mean(-1, keepdims=True)).max())


def score_tol(case, ref, b, budget):
    """tolerance of a sequence score of utterance b: up to L summed log-probabilities, each within budget x scale"""
    return budget * case["L"] * max(logit_scale(ref, b), 1.0)


def top2_margin(total_row):
    t = np.sort(total_row[np.isfinite(total_row)])
    return np.inf if t.size < 2 else float(t[-1] - t[-2])


def errors(case, got, ref):
    """the three comparisons of tests/test_rescore_gpu.py: logits (utt_rel), token log-probabilities over the row's logit
    scale, scores over their tolerance's scale -> (e_logits, e_logp, e_score)"""
    B = case["B"]
    e_lg = numerics.utt_rel(np.reshape(got["logits"], (B, -1, case["V"])), np.reshape(ref["logits"], (B, -1, case["V"])))
    e_lp = e_sc = 0.0
    for b in range(B):
        scale = max(logit_scale(ref, b), 1e-30)
        e_lp = max(e_lp, float(np.abs(got["token_logp"][b] - ref["token_logp"][b]).max() / scale))
        fin = np.isfinite(ref["total"][b])
        d = max(np.abs(got[k][b][fin] - ref[k][b][fin]).max() if fin.any() else 0.0 for k in ("att", "r_att", "total"))
        e_sc = max(e_sc, float(d / (case["L"] * max(scale, 1.0))))
    return e_lg, e_lp, e_sc
