"""Seeded synthetic attention decoders under the reference's parameter names, and the case table of the rescoring tests.

Everything is regenerated from a seed: weights (decoder_state_dict), encoder memories, hypotheses and CTC scores
(inputs).  LayerNorm gains / biases and the embedding are non-trivial, and the output layer is scaled so that the
log-probabilities of a row spread over several nats.

A case is admitted only if, for every utterance, the float64 top-2 margin of `total` exceeds MARGIN_FACTOR x the score
tolerance (score_tol): then `best` must equal the float64 argmax (tests/test_rescore_oracle_cpu.py asserts it for the
whole table, so nothing is skipped at run time).

EDGE_CASES (constructed inputs on the kernels' tile edges) and TRAINED_CASES (weights that leave the random
initialisation in one respect: trained_like) follow the drawn table; tests/test_rescore_edges_gpu.py runs them."""
import contextlib

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
    sd = decoder_state_dict(1000 + case["seed"], case["V"], case["units"], *case["blocks"])
    if case.get("trained"):
        sd = trained_like(sd, *case["trained"])
    return sd


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


# ---- edge cases: constructed, not drawn -----------------------------------------------------------------------------------
# Each case places its inputs on one edge of the kernels of csrc/rescore_kernels.hip, at the smallest shape that reaches
# it.  Fields beyond those of CASES:
#   group     what the case is about (tests/test_rescore_oracle_cpu.py pairs each oracle mutation with a group)
#   out_lens  explicit valid memory frames per utterance (default: all Tp)
#   over      (utterance, value): a second call with out_lens[utterance] = value > Tp must equal this one byte for byte
#   lens      explicit hypothesis lengths [B][nbest] (default: the longest, the empty one, ..., an absent one)
#   force     token ids every utterance's first hypothesis carries, so that each occurs as a target of both directions
#   tie       (i, j): hypothesis j is a copy of hypothesis i -- tokens, length and CTC score -- and the pair leads the rest
#   lead      per utterance the hypothesis whose CTC score is set 400 below the others', so that it wins
#   ctc_step  scale of the CTC score steps between hypotheses (default 1)
#   max_len   positional table length of the rescorer (default: the library's)
#   trained   (kind, level) of trained_like()
def _e(group, seed, V=67, L=9, nbest=3, B=2, Tp=33, blocks=(1, 1), units=256, rw=0.3, cw=0.5, **kw):
    return dict(group=group, seed=seed, V=V, L=L, nbest=nbest, B=B, Tp=Tp, blocks=blocks, units=units, reverse_weight=rw,
                ctc_weight=cw, short=False, **kw)


KEY_COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 128, 129)  # around the 8 key slices of a row and the 64-key tile of k_dec_cross_attn
FORCED_COLUMNS = (1, 31, 32, 255, 256)  # and V - 2: wave and tile edges of k_dec_output's columns


def _forced(V):
    return tuple(sorted({c for c in FORCED_COLUMNS + (V - 2,) if 1 <= c <= V - 2}))


def _vocab(seed, V):
    if V == 2:  # no token between blank and sos / eos: only empty and absent hypotheses
        return _e("vocab", seed, V=2, L=3, lens=[[0, 0, -1], [0, -1, 0]])
    return _e("vocab", seed, V=V, force=_forced(V))


EDGE_CASES = {
    # cross-attention key tiles
    "keys_b10_t129": _e("keys", 101, L=5, B=10, Tp=129, out_lens=list(KEY_COUNTS), over=(9, 1000)),
    # right decoder deeper than the left; total without att; total without the CTC score
    "blocks_1_3": _e("blocks", 111, blocks=(1, 3), rw=0.3),
    "blocks_2_6_rw1": _e("blocks", 112, blocks=(2, 6), rw=1.0, lead=[0, 1]),
    "blocks_3_3_cw0": _e("blocks", 113, blocks=(3, 3), cw=0.0),
    # FFN width: one chunk, an odd multiple, the limit
    "units_256": _e("units", 121, units=256),
    "units_768": _e("units", 122, units=768, lead=[0, 0]),
    "units_4096": _e("units", 123, units=4096),
    # vocabulary tiles of the output layer
    "vocab_2": _vocab(131, 2),
    "vocab_3": _vocab(132, 3),
    "vocab_32": _vocab(133, 32),
    "vocab_33": _vocab(134, 33),
    "vocab_256": _vocab(135, 256),
    "vocab_257": _vocab(136, 257),
    "vocab_512": _vocab(137, 512),
    # the row table: a group without rows first / in the middle / last, no row at all, nbest beyond k_dec_score's block,
    # groups that end exactly on a tile (17 + 8 + 7 = 32 rows, 17 + 17 + 17 + 13 = 64 rows), L = max_len
    "rows_absent_u0": _e("rows", 141, B=4, lens=[[-1, -1, -1], [8, 0, 3], [8, 2, -1], [8, 0, 5]]),
    "rows_absent_u2": _e("rows", 141, B=4, lens=[[8, 0, 3], [8, 2, -1], [-1, -1, -1], [8, 0, 5]]),
    "rows_absent_u3": _e("rows", 141, B=4, lens=[[8, 0, 3], [8, 2, -1], [8, 0, 5], [-1, -1, -1]]),
    "rows_all_absent": _e("rows", 142, B=4, lens=[[-1, -1, -1]] * 4),
    "rows_n70_l2": _e("rows", 143, L=2, nbest=70, lead=[66, 68]),  # the winners sit behind the block's first stride
    "rows_32_and_64": _e("rows", 144, L=17, nbest=4, lens=[[16, 7, 6, -1], [16, 16, 16, 12]]),
    "rows_l17_maxlen17": _e("rows", 145, L=17, max_len=17),
    # exact ties: `best` is the lower index
    "tie_0_1": _e("tie", 151, L=5, nbest=4, lens=[[4, 4, 2, 0], [3, 3, 4, -1]], tie=(0, 1)),
    "tie_1_3": _e("tie", 152, L=5, nbest=4, lens=[[4, 2, 0, 2], [0, 4, 3, 4]], tie=(1, 3)),
    "tie_8_9": _e("tie", 153, L=5, nbest=10, lens=[[4, 0, 1, 2, 3, 4, -1, 2, 3, 3], [1, 2, 3, 4, 0, -1, 4, 3, 4, 4]], tie=(8, 9)),
    # the reordering test's case: (3, 3) blocks, mixed lengths with an empty and an absent hypothesis
    "reorder_b3_n5": _e("reorder", 161, B=3, nbest=5, blocks=(3, 3), units=1024,
                        lens=[[8, 0, 3, -1, 5], [2, 8, -1, 0, 7], [0, 6, 8, 1, -1]], out_lens=[33, 20, 29]),
}


def edge_inputs(case):
    """inputs() for a case of EDGE_CASES / TRAINED_CASES: the same dict, built from the case's explicit fields; only the
    memory, the free tokens and the CTC score steps are drawn."""
    rng = np.random.default_rng(case["seed"])
    B, nbest, L, Tp, V = case["B"], case["nbest"], case["L"], case["Tp"], case["V"]
    mt = L - 1
    memory = rng.standard_normal((B, Tp, D)).astype(np.float32)
    out_lens = np.asarray(case.get("out_lens", [Tp] * B), np.int32)
    assert out_lens.shape == (B,)
    if "lens" in case:
        lens = np.asarray(case["lens"], np.int32)
    else:
        lens = rng.integers(0, mt + 1, (B, nbest)).astype(np.int32)
        lens[:, 0] = mt
        if nbest >= 3:
            lens[:, 1] = 0
            lens[:, nbest - 1] = -1
    assert lens.shape == (B, nbest) and lens.max() <= mt
    tokens = np.full((B, nbest, max(mt, 1)), -1, np.int32)[:, :, :mt]
    for b in range(B):
        for k in range(nbest):
            n = int(lens[b, k])
            if n > 0:
                tokens[b, k, :n] = rng.integers(1, V - 1, n)
        force = case.get("force", ())
        if force:
            assert lens[b, 0] == mt >= len(force)
            tokens[b, 0, (np.arange(len(force)) + b) % mt] = force
    ctc = np.cumsum(rng.uniform(0.5, 6.0, (B, nbest)) * case.get("ctc_step", 1.0), axis=1) + rng.uniform(0.0, 30.0, (B, 1))
    for b, k in enumerate(case.get("lead", ())):
        assert lens[b, k] >= 0
        ctc[b, k] = ctc[b].min() - 400.0  # (a random decoder gives a token about -7)
    if "tie" in case:
        i, j = case["tie"]
        others = [k for k in range(nbest) if k not in (i, j)]
        ctc[:, others] += 200.0  # the pair leads whatever the decoders say about <= L tokens
        tokens[:, j], lens[:, j], ctc[:, j] = tokens[:, i], lens[:, i], ctc[:, i]
    return dict(memory=memory, out_lens=out_lens, tokens=np.ascontiguousarray(tokens), lens=lens,
                ctc_scores=ctc.astype(np.float64))


def case_inputs(case):
    return edge_inputs(case) if "group" in case else inputs(case)


def expected_best(case, ref):
    """the float64 argmax (numpy: the lowest index of the largest total, which is the lower duplicate of a tie case)"""
    return np.asarray(ref["total"]).argmax(1).astype(np.int32)


# ---- trained-like weights --------------------------------------------------------------------------------------------------
def trained_like(sd, kind, level):
    """A new state dict that leaves the random initialisation in ONE respect (the arrays it changes are copies):
      offset  `level` added to every embedding column and to every linear_out / w_2 bias: the residual stream of every
              row moves by 16 x level at the embedding and by 3 x level per block, so every LayerNorm sees
              |row mean| >> row std
      sharp   linear_q / linear_k weights of both attentions x level: scores grow by level^2, attention is near one-hot
      wide    output_layer.weight x level: logits of about +- 8 x level"""
    ends = {"offset": ("embed.0.weight", ".linear_out.bias", ".w_2.bias"), "sharp": (".linear_q.weight", ".linear_k.weight"),
            "wide": ("output_layer.weight",)}[kind]
    out = dict(sd)
    for k, v in sd.items():
        if k.endswith(ends):
            a = np.asarray(v, np.float32)
            out[k] = np.ascontiguousarray(a + np.float32(level) if kind == "offset" else a * np.float32(level))
    return out


@contextlib.contextmanager
def conditioning(oracle):
    """Records on `oracle` (float64) while the block runs -> dict: "ln" the smallest |row mean| / row std over every
    LayerNorm input row, "score" the largest max - min of an attention row's scores over the keys it sees, "logit" the
    largest max - min of a row's logits."""
    rec = {"ln": np.inf, "score": 0.0, "logit": 0.0}
    oracle.rec = rec
    try:
        yield rec
    finally:
        oracle.rec = None


REACHED = {"offset": lambda rec: rec["ln"], "sharp": lambda rec: rec["score"], "wide": lambda rec: rec["logit"]}


def _t(seed, kind, level, floor, **kw):
    return _e("trained", seed, L=17, B=2, blocks=(2, 2), units=1024, trained=(kind, level), floor=floor, **kw)


# Levels, chosen on the CPU (V 67, L 17, nbest 3, B 2, Tp 33, blocks (2, 2)); e32 = the float32 oracle's (logits,
# log-probabilities, scores) errors against float64, `reached` what conditioning() measured, `floor` what the CPU test
# asserts of it:
#   plain      e32 (5e-7, 5e-7, 3e-8); reached: |mean| / std 4e-4, score spread 16, logit spread 16
#   offset 16  e32 (8.0e-6, 5.1e-6, 1.0e-6)  |mean| / std >= 48    ln_one_pass 18 / 21 / 3 x tol
#   offset 64  e32 (3.7e-5, 3.0e-5, 3.8e-6)  |mean| / std >= 193   ln_one_pass 67 / 63 / 21 x tol
#   sharp 4    e32 (2.0e-6, 2.5e-6, 1.2e-7)  score spread 277      softmax_without_max > 1000 x tol
#   sharp 8    e32 (4.8e-6, 2.7e-6, 1.3e-7)  score spread 1088     softmax_without_max > 1000 x tol
#   wide 12    e32 (7.6e-7, 6.1e-7, 5.8e-8)  logit spread 199, lowest log-probability -136   softmax_without_max: NaN
#   wide 16    e32 (6.6e-7, 7.3e-7, 4.8e-8)  logit spread 265, lowest log-probability -181   softmax_without_max: NaN
# Not chosen: offset 8 (|mean| / std 24) leaves ln_one_pass at 6.7 x tol only; sharp 3 (spread 156) keeps every
# |score| under 88, where an fp32 softmax without its maximum is still exact, and wide 6 (spread 99) likewise.  Every
# tolerance stays far below numerics.TOL_CAP (the largest is 4 x 3.7e-5).  The kinds are not combined: all three at once
# (offset 32, sharp 8, wide 12) measured a logits e32 of 3.8e-4, four times which is above TOL_CAP.
TRAINED_CASES = {
    "offset_16": _t(171, "offset", 16.0, 40.0),
    "offset_64": _t(171, "offset", 64.0, 150.0),
    "sharp_4": _t(171, "sharp", 4.0, 200.0),
    "sharp_8": _t(171, "sharp", 8.0, 800.0),
    "wide_12": _t(171, "wide", 12.0, 150.0, ctc_step=10.0),
    "wide_16": _t(171, "wide", 16.0, 200.0, ctc_step=10.0),
}
ALL_EDGE_CASES = dict(EDGE_CASES, **TRAINED_CASES)
