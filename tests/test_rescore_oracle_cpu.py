"""The yardstick of the rescoring tests, checked on the CPU: tests/decoder_oracle.py in float64 against the REFERENCE's
own BiTransformerDecoder (tests/golden/ref_decoder.npz, made by tests/golden/make_decoder_goldens.py), the score formula
on a hand-computable case, the margin condition that makes `best` a fair test over the whole case table, and the
mutations each of which the budget must see."""
import os

import numpy as np
import pytest
import torch

import decoder_cases as dc
import numerics as nm
from decoder_oracle import MUTATIONS, DecoderOracle

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
