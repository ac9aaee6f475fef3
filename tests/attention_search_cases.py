"""Case tables of the attention beam-search tests.  Everything is regenerated from a seed: the decoder
(decoder_cases.decoder_state_dict, plus `eos_bias` added to the output bias of the eos column, which sets how soon
hypotheses end) and the encoder memory.

CASES        drawn cases for the replay and final-hypothesis checks (no exact equality with float64 is demanded)
EXACT_CASES  the named exact class: beams of 1 to 4 whose smallest float64 gap over all steps -- at the beam cut and
             between kept neighbours -- is at least EXACT_FACTOR x the score tolerance, and on which the float32 oracle's
             search returns the float64 search's tokens, order and flags (tests/test_attention_search_oracle_cpu.py asserts
             both for every case, so nothing is skipped at run time).  On these the device must equal the float64 search.
             `ends` states what the case is in the class for: "first" (a hypothesis ends at step 1: the empty one), "mixed"
             (rows end at different steps, some never), "all" (every row ends before max_steps), "never" (no row ends)."""
import numpy as np

import decoder_cases as dc
import numerics as nm

EXACT_FACTOR = 4.0


def _c(seed, V, N, B, Tp, P, blocks=(1, 0), units=256, eos_bias=0.0, out_lens=None, **kw):
    return dict(seed=seed, V=V, N=N, B=B, Tp=Tp, P=P, blocks=blocks, units=units, eos_bias=eos_bias, out_lens=out_lens, **kw)


CASES = {
    "v67_n3_b2_t33_p12": _c(1, 67, 3, 2, 33, 12, (3, 3), 1024, 3.0, out_lens=[33, 20]),
    "v67_n10_b4_t50_p10": _c(2, 67, 10, 4, 50, 10, (2, 0), 512, 4.0, out_lens=[50, 7, 31, 1]),
    "v257_n8_b2_t33_p9": _c(3, 257, 8, 2, 33, 9, (1, 1), 256, 5.0),
    "v4233_n10_b2_t33_p8": _c(4, 4233, 10, 2, 33, 8, (1, 0), 256, 9.0, out_lens=[20, 33]),
    "v67_n1_b3_t9_p12": _c(5, 67, 1, 3, 9, 12, (1, 0), 256, 3.0),
    "v67_n4_b9_t17_p20": _c(6, 67, 4, 9, 17, 20, (1, 0), 256, 0.0),  # 36 rows: two tiles
}

def _x(ends, seed, V, N, eos_bias):
    return _c(seed, V, N, 2, 17, 12, (1, 0), 256, eos_bias, ends=ends)


# Chosen by a seed scan on the CPU (seeds 100 .. 139 per row of settings; float64 gaps and the float32 search, see the
# module docstring).  Beside each case: the smallest gap over the tolerance the scan printed (tolerance about 2e-3).
EXACT_CASES = {
    "first_n2": _x("first", 102, 67, 2, 9.0),      # 452
    "first_n3": _x("first", 103, 67, 3, 10.0),     # 196
    "mixed_n2_a": _x("mixed", 110, 67, 2, 3.0),    # 16.5
    "mixed_n2_b": _x("mixed", 104, 67, 2, 3.0),    # 12.6
    "all_n3": _x("all", 103, 67, 3, 4.0),          # 29.9
    "all_n4": _x("all", 100, 67, 4, 7.0),          # 36.3
    "all_n4_v131": _x("all", 107, 131, 4, 5.0),    # 12.0
    "mixed_n2_early": _x("mixed", 108, 67, 2, 3.0),  # 56.1: one utterance is done at step 3, the other runs all 12
    "never_n1": _x("never", 104, 67, 1, 2.0),      # 74.7
    "never_n2": _x("never", 125, 67, 2, -30.0),    # 4.8 (of 40 seeds at beams 2 and 3 without an eos, three passed 4)
}


def weights(case):
    sd = dc.decoder_state_dict(3000 + case["seed"], case["V"], case["units"], *case["blocks"])
    b = sd["decoder.left_decoder.output_layer.bias"].copy()
    b[case["V"] - 1] += np.float32(case["eos_bias"])
    for c in case.get("force", ()):  # (edge cases: winners in chosen columns)
        b[c] += np.float32(12.0)
    sd["decoder.left_decoder.output_layer.bias"] = b
    return sd


def conf(case, **kw):
    return dict(attention_heads=dc.HEADS, linear_units=case["units"], num_blocks=case["blocks"][0],
                r_num_blocks=case["blocks"][1], **kw)


def inputs(case):
    """-> dict(memory [B, Tp, D] f32, out_lens [B] i32)"""
    rng = np.random.default_rng(7000 + case["seed"])
    B, Tp = case["B"], case["Tp"]
    memory = rng.standard_normal((B, Tp, dc.D)).astype(np.float32)
    out_lens = np.asarray(case["out_lens"] if case["out_lens"] is not None else [Tp] * B, np.int32)
    assert out_lens.shape == (B,)
    return dict(memory=memory, out_lens=out_lens)


def score_tol(case, scale, budget=nm.F32_BUDGET):
    """tolerance of a sequence score: up to max_steps + 1 summed log-probabilities, each within budget x the logit scale
    (decoder_cases.score_tol with L = max_steps + 1)"""
    return budget * (case["P"] + 1) * max(scale, 1.0)


# ---- the reference's own incremental step (tests/golden/ref_decoder_steps.npz, made by make_attention_step_goldens.py) ----
STEP_CASES = ("v67_n3_b2_t33_p12", "v257_n8_b2_t33_p9", "v67_n1_b3_t9_p12")
PREFIX_LEN = 6


def step_prefix(case, b):
    """the fixed prefix of utterance b the fixture was made with: tokens 0 .. V - 2 from the case's seed"""
    return np.random.default_rng(9000 + 10 * case["seed"] + b).integers(0, case["V"] - 1, PREFIX_LEN).tolist()


# ---- exact ties ------------------------------------------------------------------------------------------------------------
TIE_PAIR = (5, 9)  # the two vocabulary entries of a tie case
TIE_CASES = {
    # first kind: identical output columns (weights and bias).  Their log-probabilities are equal in every row; the lower
    # id ranks first.
    "tie_columns": _c(49, 67, 2, 1, 9, 4, (1, 0), 256, -30.0, tie="columns", lift=8.0),  # (a larger lift leaves the rows
    # of different parents within 1e-5 of each other: 15 seeds x 4 lifts scanned, this one has 267 x the tolerance)
    # second kind: identical embedding rows as well.  The rows [.., 5] and [.., 9] are then the same row twice, their
    # candidates tie ACROSS parents at the next step, and the lower k * N + j wins.
    "tie_rows": _c(42, 67, 2, 1, 9, 4, (1, 0), 256, -30.0, tie="rows"),
    "tie_rows_n3": _c(43, 67, 3, 2, 9, 3, (1, 0), 256, -30.0, tie="rows"),
}


def tie_weights(case):
    """weights(case) with the output column of TIE_PAIR[1] made a copy of TIE_PAIR[0]'s and both lifted by 20, so that the
    pair leads every row (case["lift"]: another lift); tie = "rows": the embedding row copied too"""
    sd = weights(case)
    a, b = TIE_PAIR
    w = sd["decoder.left_decoder.output_layer.weight"].copy()
    bias = sd["decoder.left_decoder.output_layer.bias"].copy()
    w[:, b] = w[:, a]
    bias[a] += np.float32(case.get("lift", 20.0))
    bias[b] = bias[a]
    sd["decoder.left_decoder.output_layer.weight"], sd["decoder.left_decoder.output_layer.bias"] = w, bias
    if case["tie"] == "rows":
        e = sd["decoder.left_decoder.embed.0.weight"].copy()
        e[b] = e[a]
        sd["decoder.left_decoder.embed.0.weight"] = e
    return sd


def case_weights(case):
    return tie_weights(case) if case.get("tie") else weights(case)


# ---- edge cases: constructed, at the smallest shape that reaches each edge of csrc/attn_decode.hip -------------------------
# 1 block, units 256, V = 67 unless said.  `force`: columns whose output bias is lifted by 12, so that a row's N largest
# entries sit on the wave and tile edges of the output layer's columns (and on eos).
def _e(seed, V=67, N=2, B=1, Tp=9, P=4, blocks=(1, 0), units=256, eos_bias=0.0, **kw):
    return _c(seed, V, N, B, Tp, P, blocks, units, eos_bias, **kw)


def _forced(V):
    return tuple(sorted({c for c in (0, 31, 32, 255, 256, V - 2, V - 1) if 0 <= c < V}))


KEY_COUNTS = (1, 7, 8, 9, 63, 64, 65, 129)  # cross-attention keys around the 64-key chunk of k_ad_attn
EDGE_CASES = {
    # prefix lengths across the self-attention's 64-key chunk and at the row limit; eos suppressed, so every step runs
    **{f"steps_{P}": _e(201 + i, P=P, eos_bias=-30.0) for i, P in enumerate((63, 64, 65, 129, 255))},
    # cross keys: every count in one batch, NaN behind out_lens (the tests poison the memory)
    "keys_b8_t129": _e(211, B=8, Tp=129, out_lens=list(KEY_COUNTS)),
    # dense row tiles: R = B x N = 31, 32, 33, 64, 65
    "rows_31": _e(221, N=1, B=31, Tp=5, P=3), "rows_32": _e(222, N=2, B=16, Tp=5, P=3),
    "rows_33": _e(223, N=3, B=11, Tp=5, P=3), "rows_64": _e(224, N=2, B=32, Tp=5, P=3),
    "rows_65": _e(225, N=5, B=13, Tp=5, P=3),
    # the widest beam (1 and 10 are in CASES)
    "beam_32": _e(231, N=32, B=2, eos_bias=3.0),
    # vocabulary tiles of the output layer and of the top-N pass, winners forced onto their edges
    "vocab_2": _e(241, V=2, N=2, P=3, eos_bias=-1.0),
    "vocab_33": _e(242, V=33, N=3, P=3, force=_forced(33)),  # (three forced columns: 0, 31 and eos = 32)
    **{f"vocab_{V}": _e(243 + i, V=V, N=4, P=3, force=_forced(V)) for i, V in enumerate((256, 257, 4233))},
    # decoder depth and FFN width ((3, 3), (2, 0), (1, 1), (1, 0) at 1024 / 512 / 256 units are in CASES)
    "blocks_6_2": _e(251, blocks=(6, 2), N=3, B=2, eos_bias=3.0),
    "units_768": _e(261, units=768, N=3, B=2, eos_bias=3.0),
    "units_4096": _e(262, units=4096, N=3, B=2, eos_bias=3.0),
}
