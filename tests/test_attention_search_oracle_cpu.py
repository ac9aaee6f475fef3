"""The yardstick of the attention beam-search tests, checked on the CPU: the float64 step against the REFERENCE's own
`forward_one_step` with its cache (tests/golden/ref_decoder_steps.npz), the search on a hand-computable case, the named
exact class (attention_search_cases.EXACT_CASES: float64 gaps and the float32 search), the tie cases, and the mutations
each of which the replay or the exact class must see."""
import os

import numpy as np
import pytest
import torch

import attention_search_cases as ac
import attention_search_oracle as so
import decoder_cases as dc
import numerics as nm
from decoder_oracle import DecoderOracle

HERE = os.path.dirname(os.path.abspath(__file__))
_memo = nm.Memo()


def oracle(case, dtype=torch.float64, mut=None):
    return DecoderOracle(ac.case_weights(case), case["V"], *case["blocks"], heads=dc.HEADS, dtype=dtype, mut=mut)


def run(case_name, case, dtype=torch.float64, mut=None, dec_mut=None, **kw):
    """the search of every utterance of a case -> list of result dicts"""
    def go():
        inp = ac.inputs(case)
        o = oracle(case, dtype, dec_mut)
        return [so.search(o, inp["memory"][b], inp["out_lens"][b], case["N"], case["P"], mut=mut, **kw)
                for b in range(case["B"])]
    return _memo.get((case_name, dtype, mut, dec_mut, tuple(sorted(kw.items()))), go)


def same_hypotheses(a, b):
    return all(x["tokens"] == y["tokens"] and np.array_equal(x["ended"], y["ended"]) and x["steps"] == y["steps"]
               for x, y in zip(a, b))


@pytest.mark.parametrize("name", ac.STEP_CASES)
def test_float64_step_matches_the_reference_forward_one_step(name):
    """Their difference is the fp32 rounding of the reference itself: bounded by the float32 restatement's own distance
    to float64 times FLOOR_FACTOR (log-probabilities over the row's logit scale)."""
    gold = np.load(os.path.join(HERE, "golden", "ref_decoder_steps.npz"))[f"{name}/logp"]
    case = ac.CASES[name]
    inp = ac.inputs(case)
    o64, o32 = oracle(case), oracle(case, torch.float32)
    assert gold.shape == (case["B"], ac.PREFIX_LEN + 1, case["V"])
    for b in range(case["B"]):
        pre = ac.step_prefix(case, b)
        lg64 = o64.logits(inp["memory"][b], inp["out_lens"][b], pre)
        a64 = torch.log_softmax(lg64, -1).numpy()
        a32 = torch.log_softmax(o32.logits(inp["memory"][b], inp["out_lens"][b], pre), -1).double().numpy()
        scale = float((lg64 - lg64.mean(-1, keepdim=True)).abs().max())
        floor = np.abs(a32 - a64).max() / scale
        err = np.abs(gold[b] - a64).max() / scale
        print(f"{name} utterance {b}: reference step vs float64 {err:.2e}, float32 restatement vs float64 {floor:.2e}")
        assert floor < nm.F32_BUDGET / 2
        assert err <= nm.FLOOR_FACTOR * floor, (err, floor)


def test_search_on_a_hand_computable_case():
    """V = 3 (tokens 0, 1, sos = eos = 2), all weights zero except the output bias: every row's log-probabilities are
    lp = log_softmax(bias) whatever its prefix.  bias = (1, 0, 0.5): lp0 > lp2 (eos) > lp1.  Beam 2, three steps:
      step 1  row 0 offers (0, lp0), (eos, lp2)                       -> [0] live at lp0; [] ended at lp2
      step 2  [0] offers (0, 2 lp0), (eos, lp0 + lp2); [] offers lp2  -> lp2 > 2 lp0 > lp0 + lp2: [] ended first, [0, 0] live
      step 3  [] offers lp2; [0, 0] offers (0, 3 lp0), (eos, ..)      -> [] ended at lp2; [0, 0, 0] cut at max_steps"""
    V = 3
    sd = dc.decoder_state_dict(5, V, 256, 1, 0)
    for k in sd:
        if not k.endswith(("norm1.weight", "norm2.weight", "norm3.weight", "after_norm.weight")):
            sd[k] = np.zeros_like(sd[k])
    bias = np.array([1.0, 0.0, 0.5])
    sd["decoder.left_decoder.output_layer.bias"] = bias.astype(np.float32)
    lp = bias - np.log(np.exp(bias).sum())
    assert lp[2] > 2 * lp[0] > lp[0] + lp[2]
    o = DecoderOracle(sd, V, 1, 0)
    r = so.search(o, np.ones((4, dc.D), np.float32), 3, 2, 3)
    assert r["tokens"] == [[], [0, 0, 0]] and r["ended"].tolist() == [1, 0] and r["steps"] == 3
    np.testing.assert_allclose(r["scores"], [lp[2], 3 * lp[0]], rtol=0, atol=1e-12)
    assert r["trace_parent"].tolist() == [[0, 0], [1, 0], [0, 1]]
    assert r["trace_token"].tolist() == [[0, 2], [2, 0], [2, 0]]
    np.testing.assert_allclose(r["trace_score"], [[lp[0], lp[2]], [lp[2], 2 * lp[0]], [lp[2], 3 * lp[0]]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["token_logp"], [[lp[2], 0, 0, 0], [lp[0]] * 3 + [0]], rtol=0, atol=1e-12)
    assert so.final_from_trace(r["trace_parent"], r["trace_token"], 3, 2, V - 1) == r["tokens"]
    # beam 1 is a greedy search; with a large eos bias the empty hypothesis ends it at step 1 and nothing runs after
    sd["decoder.left_decoder.output_layer.bias"] = np.array([0.0, 0.0, 5.0], np.float32)
    r = so.search(DecoderOracle(sd, V, 1, 0), np.ones((4, dc.D), np.float32), 3, 1, 4)
    assert r["tokens"] == [[]] and r["ended"].tolist() == [1] and r["steps"] == 1
    assert (r["trace_parent"][1:] == -1).all() and (r["trace_token"][1:] == -1).all() and not r["trace_score"][1:].any()


def ends_of(res):
    """what a case's float64 search shows about endings"""
    kinds = set()
    for r in res:
        e = r["ended"].astype(bool)
        if any(e[k] and not r["tokens"][k] for k in range(len(e))):
            kinds.add("first")
        if e.any() and not e.all():
            kinds.add("mixed")
        if e.all():
            kinds.add("all")
        if not e.any():
            kinds.add("never")
    return kinds


@pytest.mark.parametrize("name", list(ac.EXACT_CASES))
def test_exact_class_admission(name):
    case = ac.EXACT_CASES[name]
    assert 1 <= case["N"] <= 4
    r64 = run(name, case, record_gaps=True)
    r32 = run(name, case, torch.float32)
    for b, r in enumerate(r64):
        tol = ac.score_tol(case, r["scale"])
        print(f"{name} utterance {b}: smallest gap {r['min_gap']:.3e} = {r['min_gap'] / tol:.1f} x tol {tol:.3e}")
        assert r["min_gap"] >= ac.EXACT_FACTOR * tol, (b, r["min_gap"], tol)
    assert same_hypotheses(r64, r32)
    assert case["ends"] in ends_of(r64), (case["ends"], ends_of(r64))
    if case["ends"] == "all":
        assert all(r["ended"].all() and r["steps"] < case["P"] for r in r64)
    if case["ends"] == "never":
        assert all(not r["ended"].any() and r["steps"] == case["P"] for r in r64)


def test_exact_class_covers_every_kind_of_ending():
    assert len(ac.EXACT_CASES) >= 6
    assert {c["ends"] for c in ac.EXACT_CASES.values()} == {"first", "mixed", "all", "never"}
    assert {c["N"] for c in ac.EXACT_CASES.values()} == {1, 2, 3, 4}


@pytest.mark.parametrize("name", list(ac.TIE_CASES))
def test_tie_cases_tie_exactly_and_nowhere_else(name):
    """the pair's log-probabilities are equal bit for bit in float64 and in float32, the pair leads, the lower id / the
    lower k * N + j goes first, and every OTHER gap is EXACT_FACTOR x the tolerance wide, so that the device must return
    the float64 search's hypotheses here too"""
    case = ac.TIE_CASES[name]
    a, b = ac.TIE_PAIR
    inp = ac.inputs(case)
    for dtype in (torch.float64, torch.float32):
        lg = oracle(case, dtype).logits(inp["memory"][0], inp["out_lens"][0], [a])
        assert bool((lg[:, a] == lg[:, b]).all())
    r64 = run(name, case, record_gaps=True, ignore_exact_ties=True)
    assert same_hypotheses(r64, run(name, case, torch.float32))
    for r in r64:
        assert r["min_gap"] >= ac.EXACT_FACTOR * ac.score_tol(case, r["scale"]), r["min_gap"]
        assert r["trace_token"][0, :2].tolist() == [a, b] and r["trace_score"][0, 0] == r["trace_score"][0, 1]
        if case["tie"] == "rows":  # step 2: four tied candidates over two parents; (0, 0) and (0, 1) go first
            assert r["trace_score"][1, 0] == r["trace_score"][1, 1]
            assert r["trace_parent"][1, :2].tolist() == [0, 0] and r["trace_token"][1, :2].tolist() == [a, b]
            if case["N"] >= 3:
                assert r["trace_parent"][1, 2] == 1 and r["trace_token"][1, 2] == a


# mutation -> the cases that must see it, and by which check: "exact" (the hypotheses differ from the float64 search's on a
# case of the exact class or a tie case) or "replay" (the mutated search's own trace fails the replay against float64)
MUTATION_SEEN_BY = {
    "ancestry_not_rewritten": ("exact", ("mixed_n2_a", "all_n3", "all_n4")),
    "ended_offers_n": ("replay", ("first_n2", "first_n3", "all_n4")),
    "no_eos_term": ("replay", ("first_n2", "all_n3", "all_n4")),
    "higher_id_on_tie": ("exact", ("tie_columns",)),
    "higher_index_on_tie": ("exact", ("tie_rows", "tie_rows_n3")),
    "key_count_off_by_one": ("replay", ("mixed_n2_a", "all_n3", "never_n2")),
    "frame_past_out_lens": ("replay", ("short_all_n3",)),
}
# the exact class runs with every frame valid; the last mutation needs frames behind out_lens
SHORT_CASES = {"short_all_n3": dict(ac.EXACT_CASES["all_n3"], out_lens=[9, 12])}


def _case(name):
    for table in (ac.EXACT_CASES, ac.TIE_CASES, SHORT_CASES):
        if name in table:
            return table[name]
    raise KeyError(name)


@pytest.mark.parametrize("mut", list(MUTATION_SEEN_BY))
def test_every_mutation_is_seen(mut):
    how, names = MUTATION_SEEN_BY[mut]
    assert set(MUTATION_SEEN_BY) == set(so.SEARCH_MUTATIONS) | set(so.DECODER_MUTATIONS)
    seen = []
    for name in names:
        case = _case(name)
        inp = ac.inputs(case)
        kw = dict(mut=mut) if mut in so.SEARCH_MUTATIONS else dict(dec_mut=so.DECODER_MUTATIONS[mut])
        bad = run(name, case, **kw)
        if how == "exact":
            seen.append(not same_hypotheses(run(name, case), bad))
            continue
        o64 = oracle(case)
        hit = False
        for b, r in enumerate(bad):
            rep = so.replay(o64, inp["memory"][b], inp["out_lens"][b], case["N"], r["trace_parent"], r["trace_token"],
                            r["trace_score"], lambda scale: ac.score_tol(case, scale))
            hit |= bool(rep["problems"])
        seen.append(hit)
    print(mut, how, dict(zip(names, seen)))
    assert all(seen), dict(zip(names, seen))


@pytest.mark.parametrize("name", ["first_n3", "mixed_n2_a", "all_n4"])
def test_replay_passes_the_clean_searches(name):
    """float64's own trace is clean at zero tolerance scale, the float32 oracle's within the tolerance"""
    case = ac.EXACT_CASES[name]
    inp = ac.inputs(case)
    o64 = oracle(case)
    for dtype in (torch.float64, torch.float32):
        for b, r in enumerate(run(name, case, dtype)):
            rep = so.replay(o64, inp["memory"][b], inp["out_lens"][b], case["N"], r["trace_parent"], r["trace_token"],
                            r["trace_score"], lambda scale: ac.score_tol(case, scale))
            assert not rep["problems"], rep["problems"]
            assert rep["hyps"] == r["tokens"] and rep["steps"] == r["steps"]
            assert rep["worst"] <= (1e-9 if dtype == torch.float64 else 0.5), rep["worst"]
