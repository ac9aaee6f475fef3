"""The yardstick of the rescoring tests, checked on the CPU: tests/decoder_oracle.py in float64 against the REFERENCE's
own BiTransformerDecoder (tests/golden/ref_decoder.npz, made by tests/golden/make_decoder_goldens.py), the score formula
on a hand-computable case, the margin condition that makes `best` a fair test over the whole case table, and the
mutations each of which the budget must see.

The same for the constructed edge cases and the trained-like weights of tests/test_rescore_edges_gpu.py
(decoder_cases.EDGE_CASES / TRAINED_CASES): what the edge table covers, a clear winner or an exact tie in every
utterance, the conditioning each trained-like case states, its admission by the float32 oracle's own error, and one
pairing of every edge mutation with the cases that must see it."""
import os

import numpy as np
import pytest
import torch

import decoder_cases as dc
import numerics as nm
from decoder_oracle import EDGE_MUTATIONS, MUTATIONS, DecoderOracle

HERE = os.path.dirname(os.path.abspath(__file__))
SCORE_BUDGET = nm.F32_BUDGET  # the budget tests/test_rescore_gpu.py starts from
_memo = nm.Memo()


def oracle(case, dtype=torch.float64, mut=None):
    return DecoderOracle(dc.weights(case), case["V"], *case["blocks"], heads=dc.HEADS, dtype=dtype, mut=mut)


def run(name, dtype=torch.float64, mut=None):
    def go():
        case = dc.CASES[name]
        inp = dc.inputs(case)
        return oracle(case, dtype, mut).rescore(inp["memory"], inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"],
                                                case["ctc_weight"], case["reverse_weight"])
    return _memo.get((name, dtype, mut), go)


def valid_rows(case, inp, logits, side):
    """[B, nbest, 2, L, V] -> the valid rows of one side in (b, n, position) order, as the fixture stores them"""
    rows = []
    for b in range(case["B"]):
        for k in range(case["nbest"]):
            n = int(inp["lens"][b, k])
            if n >= 0:
                rows.append(logits[b, k, side, :n + 1])
    return np.concatenate(rows)


@pytest.mark.parametrize("name", dc.FIXTURE_CASES)
def test_float64_restatement_matches_the_reference_decoder(name):
    """Their difference is the fp32 rounding of the reference itself: bounded by the float32 restatement's own distance
    to float64 times FLOOR_FACTOR."""
    gold = np.load(os.path.join(HERE, "golden", "ref_decoder.npz"))
    case = dc.CASES[name]
    inp = dc.inputs(case)
    r64, r32 = run(name), run(name, torch.float32)
    for side, key in ((0, "l_x"), (1, "r_x")):
        if side == 1 and case["reverse_weight"] == 0:
            assert gold[f"{name}/{key}"].shape[0] == 0
            continue
        ref = gold[f"{name}/{key}"]
        a64, a32 = valid_rows(case, inp, r64["logits"], side), valid_rows(case, inp, r32["logits"], side)
        assert ref.shape == a64.shape
        floor = nm.rel(a32, a64)
        err = nm.rel(ref, a64)
        print(f"{name} {key}: reference vs float64 {err:.2e}, float32 restatement vs float64 {floor:.2e}")
        assert floor < nm.F32_BUDGET / 2  # the fp32 floor itself sits well inside the budget
        assert err <= nm.FLOOR_FACTOR * floor, (err, floor)


def test_score_formula_on_a_hand_computable_case():
    """One block, V = 3 (tokens: 0 blank, 1, sos = eos = 2), all weights zero except the output layer's bias: every row's
    logits are that bias, so every log-probability is log_softmax(bias) and the scores follow by hand."""
    V = 3
    sd = dc.decoder_state_dict(5, V, 1024, 1, 1)
    for k in sd:
        if not k.endswith(("norm1.weight", "norm2.weight", "norm3.weight", "after_norm.weight")):
            sd[k] = np.zeros_like(sd[k])
    bias_l, bias_r = np.array([0.0, 1.0, 2.0]), np.array([1.0, 0.0, -1.0])
    sd["decoder.left_decoder.output_layer.bias"] = bias_l.astype(np.float32)
    sd["decoder.right_decoder.output_layer.bias"] = bias_r.astype(np.float32)
    lp_l = bias_l - np.log(np.exp(bias_l).sum())
    lp_r = bias_r - np.log(np.exp(bias_r).sum())
    o = DecoderOracle(sd, V, 1, 1)
    memory = np.ones((1, 4, dc.D), np.float32)
    tokens = np.array([[[1, 1, 0], [1, -1, -1], [-1, -1, -1], [-1, -1, -1]]], np.int32)
    lens = np.array([[3, 1, 0, -1]], np.int32)
    ctc = np.array([[2.0, 4.0, 9.0, 0.0]])
    cw, rw = 0.5, 0.3
    r = o.rescore(memory, np.array([3], np.int32), tokens, lens, ctc, cw, rw)
    att = np.array([2 * lp_l[1] + lp_l[0] + lp_l[2], lp_l[1] + lp_l[2], lp_l[2]])
    r_att = np.array([2 * lp_r[1] + lp_r[0] + lp_r[2], lp_r[1] + lp_r[2], lp_r[2]])
    np.testing.assert_allclose(r["att"][0, :3], att, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["r_att"][0, :3], r_att, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["total"][0, :3], (1 - rw) * att + rw * r_att - cw * ctc[0, :3], rtol=0, atol=1e-12)
    assert r["total"][0, 3] == -np.inf and r["att"][0, 3] == 0 and r["r_att"][0, 3] == 0
    assert r["best"][0] == int(np.argmax(r["total"][0]))
    # reverse_weight 0: the right decoder takes no part
    r0 = o.rescore(memory, None, tokens, lens, ctc, cw, 0.0)
    np.testing.assert_allclose(r0["total"][0, :3], att - cw * ctc[0, :3], rtol=0, atol=1e-12)
    assert not r0["r_att"].any() and not r0["token_logp"][:, :, 1].any()


def test_every_case_has_a_clear_winner():
    """`best` is compared with the float64 argmax in every case: admitted only with a top-2 margin of MARGIN_FACTOR x the
    score tolerance in every utterance."""
    for name, case in dc.CASES.items():
        ref = run(name)
        for b in range(case["B"]):
            margin = dc.top2_margin(ref["total"][b])
            tol = dc.score_tol(case, ref, b, SCORE_BUDGET)
            assert margin > dc.MARGIN_FACTOR * tol, (name, b, margin, tol)


def test_case_table_covers_the_grid():
    cs = dc.CASES.values()
    assert {c["V"] for c in cs} == {67, 4233}
    assert {c["L"] for c in cs} == {1, 2, 16, 17, 33, 64, 65}
    assert {c["nbest"] for c in cs} == {1, 3, 10} and {c["B"] for c in cs} == {1, 3}
    assert {c["Tp"] for c in cs} == {1, 31, 33, 100}
    assert {c["blocks"] for c in cs} == {(3, 3), (1, 0), (6, 2)} and {c["units"] for c in cs} == {1024, 2048}
    assert {c["reverse_weight"] for c in cs} == {0.0, 0.3}
    for name, c in dc.CASES.items():
        inp = dc.inputs(c)
        if c["short"]:
            assert (inp["out_lens"] < c["Tp"]).any(), name
        if c["nbest"] >= 3:
            assert (inp["lens"] == 0).any() and (inp["lens"] < 0).any(), name
        assert inp["lens"].max() == c["L"] - 1


errors = dc.errors


MUT_CASES = ("v67_l17_n3_b3_t33", "v67_l2_n3_b1_t31", "v67_l33_n3_b1_t33")


@pytest.mark.parametrize("mut", MUTATIONS)
def test_each_mutation_leaves_the_budget(mut):
    worst = 0.0
    for name in MUT_CASES:
        worst = max(worst, max(errors(dc.CASES[name], run(name, mut=mut), run(name))))
    print(f"{mut}: worst error {worst:.2e} ({worst / SCORE_BUDGET:.0f} x the budget)")
    assert worst >= 5 * SCORE_BUDGET, (mut, worst)


def test_float32_restatement_sits_inside_the_budget():
    for name in MUT_CASES:
        e = errors(dc.CASES[name], run(name, torch.float32), run(name))
        print(name, ["%.2e" % v for v in e])
        assert max(e) < SCORE_BUDGET / 2, (name, e)


@pytest.mark.parametrize("name", ["v67_l17_n3_b3_t33", "v67_l1_n1_b1_t1", "v67_l64_n3_b1_t100"])
def test_batched_restatement_equals_the_per_hypothesis_one(name):
    """rescore_batched (padded, the reference's own way; the torch stand-in of tools/bench_rescore.py) against rescore:
    the same float64 arithmetic in another order"""
    case = dc.CASES[name]
    inp = dc.inputs(case)
    ref = run(name)
    t = {k: torch.as_tensor(v) for k, v in inp.items()}
    att, r_att, total, best = oracle(case).rescore_batched(t["memory"], t["out_lens"], t["tokens"], t["lens"], t["ctc_scores"],
                                                           case["ctc_weight"], case["reverse_weight"])
    np.testing.assert_allclose(att.numpy(), ref["att"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(r_att.numpy(), ref["r_att"], rtol=0, atol=1e-9)
    fin = np.isfinite(ref["total"])
    assert np.array_equal(np.isfinite(total.numpy()), fin)
    np.testing.assert_allclose(total.numpy()[fin], ref["total"][fin], rtol=0, atol=1e-9)
    assert np.array_equal(best.numpy(), ref["best"])


# ---- edge cases and trained-like weights -----------------------------------------------------------------------------------
def run_edge(name, dtype=torch.float64, mut=None):
    def go():
        case = dc.ALL_EDGE_CASES[name]
        inp = dc.edge_inputs(case)
        return oracle(case, dtype, mut).rescore(inp["memory"], inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"],
                                                case["ctc_weight"], case["reverse_weight"])
    return _memo.get(("edge", name, dtype, mut), go)


def group(g):
    return [n for n, c in dc.ALL_EDGE_CASES.items() if c["group"] == g]


def trained_tols(name):
    """per comparison: numerics.tol(budget, e32) with e32 of the float32 oracle on that very case"""
    e32 = errors(dc.TRAINED_CASES[name], run_edge(name, torch.float32), run_edge(name))
    return e32, tuple(nm.tol(nm.F32_BUDGET, e) for e in e32)


def test_edge_table_covers_the_edges():
    E = dc.EDGE_CASES
    for name, c in E.items():
        assert c["B"] <= 4 or name == "keys_b10_t129", name
        assert max(c["blocks"]) <= 2 or c["group"] in ("blocks", "reorder"), name
        assert c["L"] <= 17, name
    keys = E["keys_b10_t129"]
    assert keys["Tp"] == 129 and tuple(keys["out_lens"]) == (0, 1, 7, 8, 9, 63, 64, 65, 128, 129) and keys["over"][1] > 129
    assert {(E[n]["blocks"], E[n]["reverse_weight"], E[n]["ctc_weight"]) for n in group("blocks")} == {
        ((1, 3), 0.3, 0.5), ((2, 6), 1.0, 0.5), ((3, 3), 0.3, 0.0)}
    assert {E[n]["units"] for n in group("units")} == {256, 768, 4096}
    assert {E[n]["V"] for n in group("vocab")} == {2, 3, 32, 33, 256, 257, 512}
    for n in group("vocab"):  # every forced column is a target of both directions (the right targets are the reversed tokens)
        c, inp = E[n], dc.edge_inputs(E[n])
        assert c["reverse_weight"] > 0
        want = {col for col in (1, 31, 32, 255, 256, c["V"] - 2) if 1 <= col <= c["V"] - 2}
        for b in range(c["B"]):
            seen = {int(t) for k in range(c["nbest"]) for t in inp["tokens"][b, k, :max(int(inp["lens"][b, k]), 0)]}
            assert want <= seen, (n, b, want - seen)
            assert all(1 <= t <= c["V"] - 2 for t in seen), n
        if c["V"] == 2:
            assert inp["lens"].max() == 0 and (inp["lens"] < 0).any()
    # the row table
    absent = [int(np.nonzero((np.asarray(E[n]["lens"]) < 0).all(1))[0][0]) for n in ("rows_absent_u0", "rows_absent_u2", "rows_absent_u3")]
    assert absent == [0, 2, 3] and all(E[n]["B"] == 4 for n in ("rows_absent_u0", "rows_absent_u2", "rows_absent_u3"))
    assert (np.asarray(E["rows_all_absent"]["lens"]) < 0).all()
    assert E["rows_n70_l2"]["nbest"] == 70 and E["rows_n70_l2"]["L"] == 2
    assert (run_edge("rows_n70_l2")["best"] >= 64).all()  # the winner is behind the first 64 hypotheses
    rows = (np.asarray(E["rows_32_and_64"]["lens"]) + 1).clip(min=0).sum(1)
    assert rows.tolist() == [32, 64]
    assert E["rows_l17_maxlen17"]["max_len"] == E["rows_l17_maxlen17"]["L"] == 17
    assert dc.edge_inputs(E["rows_l17_maxlen17"])["lens"].max() == 16
    assert {(E[n]["tie"], E[n]["nbest"]) for n in group("tie")} == {((0, 1), 4), ((1, 3), 4), ((8, 9), 10)}
    r = E["reorder_b3_n5"]
    assert (r["blocks"], r["B"], r["nbest"]) == ((3, 3), 3, 5)
    assert all(0 in row and -1 in row for row in r["lens"])


def test_every_edge_case_has_a_clear_winner_or_an_exact_tie():
    """The margin rule of test_every_case_has_a_clear_winner at each case's own score tolerance, in every utterance with
    at least two finite totals.  Tie cases: the two duplicates are equal in every input, lead the rest by that margin,
    and the expected `best` is the lower index."""
    for name, case in dc.ALL_EDGE_CASES.items():
        ref = run_edge(name)
        budget = trained_tols(name)[1][2] if name in dc.TRAINED_CASES else SCORE_BUDGET
        inp = dc.edge_inputs(case)
        for b in range(case["B"]):
            total = ref["total"][b]
            need = dc.MARGIN_FACTOR * dc.score_tol(case, ref, b, budget)
            if "tie" in case:
                i, j = case["tie"]
                assert i < j and np.array_equal(inp["tokens"][b, i], inp["tokens"][b, j])
                assert inp["lens"][b, i] == inp["lens"][b, j] >= 0 and inp["ctc_scores"][b, i] == inp["ctc_scores"][b, j]
                assert total[i] == total[j]
                rest = np.delete(total, [i, j])
                assert np.isfinite(rest).any() and total[i] - rest.max() > need, (name, b)
                assert dc.expected_best(case, ref)[b] == i
            else:
                assert dc.top2_margin(total) > need, (name, b, dc.top2_margin(total), need)
        assert np.array_equal(dc.expected_best(case, ref), ref["best"])


def test_absent_conventions_of_the_oracle():
    ref = run_edge("rows_all_absent")
    assert np.isneginf(ref["total"]).all() and not ref["att"].any() and not ref["r_att"].any() and not ref["best"].any()
    assert not ref["token_logp"].any() and not ref["logits"].any()


# mutation -> the cases that must see it (last_index_on_tie, best_among_first_64: by a different `best`)
EDGE_TEETH = {
    "cross_keys_first_tile_only": ["keys_b10_t129"],
    "cross_every_eighth_slice_dropped": ["keys_b10_t129"],
    "right_reads_left_kv_slot": ["blocks_1_3", "blocks_2_6_rw1"],
    "ffn_last_chunk_dropped": ["units_256", "units_768", "units_4096"],
    "target_column_mod_256": ["vocab_257", "vocab_512"],
    "vocab_padded_columns_counted": ["vocab_2", "vocab_3", "vocab_32", "vocab_33", "vocab_257"],
    "last_index_on_tie": ["tie_0_1", "tie_1_3", "tie_8_9"],
    "best_among_first_64": ["rows_n70_l2"],
    "ln_one_pass": ["offset_16", "offset_64"],
    "softmax_without_max": ["sharp_4", "sharp_8", "wide_12", "wide_16"],
}


def over_tolerance(e, tols):
    """largest error / tolerance of the three comparisons; a NaN counts as infinitely far out"""
    return max(np.inf if not np.isfinite(v) else v / t for v, t in zip(e, tols))


@pytest.mark.parametrize("mut", EDGE_MUTATIONS)
def test_each_edge_mutation_leaves_the_tolerance(mut):
    """every paired case, not only one of them, sees its mutation by at least 5 x its tolerance"""
    assert set(EDGE_TEETH) == set(EDGE_MUTATIONS)
    for name in EDGE_TEETH[mut]:
        case, ref, bad = dc.ALL_EDGE_CASES[name], run_edge(name), run_edge(name, mut=mut)
        if mut == "last_index_on_tie":
            assert not np.array_equal(bad["best"], ref["best"]) and np.array_equal(bad["best"], [case["tie"][1]] * case["B"])
            continue
        if mut == "best_among_first_64":
            assert (bad["best"] != ref["best"]).all() and (ref["best"] >= 64).all()
            continue
        tols = trained_tols(name)[1] if name in dc.TRAINED_CASES else (SCORE_BUDGET,) * 3
        ratio = over_tolerance(errors(case, bad, ref), tols)
        print(f"{mut} on {name}: {ratio:.1f} x the tolerance")
        assert ratio >= 5.0, (mut, name, ratio)


def test_key_mutations_are_seen_only_past_their_edge():
    """the key-count case is what sees them: utterances of <= 64 keys (<= 7 keys) are untouched by the two mutations"""
    case, ref = dc.EDGE_CASES["keys_b10_t129"], run_edge("keys_b10_t129")
    for mut, clean in (("cross_keys_first_tile_only", 64), ("cross_every_eighth_slice_dropped", 7)):
        bad = run_edge("keys_b10_t129", mut=mut)
        for b, n in enumerate(case["out_lens"]):
            same = np.array_equal(bad["logits"][b], ref["logits"][b])
            assert same == (n <= clean), (mut, b, n)


@pytest.mark.parametrize("name", list(dc.TRAINED_CASES))
def test_trained_like_cases_reach_their_conditioning_and_are_admitted(name):
    case = dc.TRAINED_CASES[name]
    inp = dc.edge_inputs(case)
    o = oracle(case)
    with dc.conditioning(o) as rec:
        o.rescore(inp["memory"], inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"], case["ctc_weight"],
                  case["reverse_weight"])
    plain = oracle(dict(case, trained=None))
    with dc.conditioning(plain) as rec0:
        plain.rescore(inp["memory"], inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"], case["ctc_weight"],
                      case["reverse_weight"])
    kind = case["trained"][0]
    reached, centred = dc.REACHED[kind](rec), dc.REACHED[kind](rec0)
    e32, tols = trained_tols(name)
    print(f"{name}: reached {reached:.3g} (floor {case['floor']}, plain weights {centred:.3g}); e32 "
          + " ".join("%.1e" % v for v in e32) + "; tol " + " ".join("%.1e" % v for v in tols))
    assert reached >= case["floor"] and centred < case["floor"] / 5
    assert all(np.isfinite(v) for v in e32) and max(tols) <= nm.TOL_CAP, (e32, tols)
    if kind == "wide":
        assert run_edge(name)["token_logp"].min() < -100.0
