"""ppasr_rescore at the tile edges of its kernels and on trained-like weights, against the float64 restatement of the
reference's attention decoder (tests/decoder_oracle.py).  The cases are constructed, not drawn (decoder_cases.EDGE_CASES:
cross-attention key counts around the 8 key slices and the 64-key tile, a right decoder deeper than the left, the FFN
widths 256 / 768 / 4096, vocabularies and forced target columns at the output layer's wave and tile edges, row groups that
are empty, end on a tile or pass k_dec_score's block, exact ties) or leave the random initialisation in one respect
(decoder_cases.TRAINED_CASES: off-centre LayerNorm rows, near one-hot attention, logits of +-100).  tests/
test_rescore_oracle_cpu.py shows on the CPU that each case has a clear winner or an exact tie and that a kernel wrong at
its edge would leave the tolerance by >= 5 x.  Beside parity: out-of-range key counts, bit-exact reordering of hypotheses
and utterances, the two input clamps, guard bytes around the workspace and every output, a non-default stream.

Edge cases are held to numerics.F32_BUDGET (2e-5) in all three comparisons of decoder_cases.errors; trained-like cases to
numerics.tol(F32_BUDGET, e32) with e32 of the float32 oracle computed here.

First MI355X run, worst (logits, log-probabilities, scores) per group: keys 7.2e-7 4.7e-7 1.0e-7; blocks 6.1e-7 5.9e-7
1.2e-7; units 5.8e-7 4.1e-7 1.1e-7; vocab 9.1e-7 1.8e-6 6.1e-7; rows 6.7e-7 5.6e-7 3.2e-7; tie 5.3e-7 5.9e-7 1.2e-7;
reorder 7.6e-7 8.7e-7 1.6e-7.  Trained-like, worst error / tolerance: offset_16 0.22, offset_64 0.34, sharp_4 0.11, sharp_8
0.24, wide_12 0.03, wide_16 0.03 (levels: offset 16 / 64, q and k x 4 / x 8, output layer x 12 / x 16).  Every permutation,
tie, clamp, guard and stream comparison was bit-exact; no kernel had to change (NOTES.md section 31)."""
import numpy as np
import pytest
import torch

import decoder_cases as dc
import numerics as nm
import poison
from decoder_oracle import DecoderOracle

pytestmark = pytest.mark.gpu

BUDGET = nm.F32_BUDGET  # logits, log-probabilities and scores alike, as tests/test_rescore_gpu.py
OUT_KEYS = ("att", "r_att", "total", "best", "token_logp", "logits")
_memo = nm.Memo()


def conf(case):
    c = dict(attention_heads=dc.HEADS, linear_units=case["units"], num_blocks=case["blocks"][0],
             r_num_blocks=case["blocks"][1], dropout_rate=0.1, positional_dropout_rate=0.1,
             self_attention_dropout_rate=0.0, src_attention_dropout_rate=0.0)
    if "max_len" in case:
        c["max_len"] = case["max_len"]
    return c


def rescorer(name):
    """one per set of weights: cases that differ in their inputs only share it"""
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    case = dc.ALL_EDGE_CASES[name]
    key = ("gpu", case["seed"], case["V"], case["units"], case["blocks"], case.get("trained"), case.get("max_len"))
    return _memo.get(key, lambda: AttentionRescorer(dc.weights(case), case["V"], conf(case)))


def oracle_run(name, dtype):
    def go():
        case = dc.ALL_EDGE_CASES[name]
        inp = dc.edge_inputs(case)
        o = DecoderOracle(dc.weights(case), case["V"], *case["blocks"], heads=dc.HEADS, dtype=dtype)
        return o.rescore(inp["memory"], inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"], case["ctc_weight"],
                         case["reverse_weight"])
    return _memo.get(("ref", name, dtype), go)


def to_np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def call(name, inp=None, memory=None, **kw):
    """the library on the case's inputs (or `inp`), NaN behind out_lens, both taps -> numpy"""
    case = dc.ALL_EDGE_CASES[name]
    inp = dc.edge_inputs(case) if inp is None else inp
    memory = dc.poison_memory(inp) if memory is None else memory
    return to_np(rescorer(name).rescore(memory, inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"],
                                        case["ctc_weight"], case["reverse_weight"], return_token_logp=True,
                                        return_logits=True, **kw))


def same_bytes(a, b, keys=OUT_KEYS):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def check_conventions(case, inp, got):
    absent = inp["lens"] < 0
    assert np.array_equal(np.isneginf(got["total"]), absent)
    assert np.isfinite(got["total"][~absent]).all()
    assert not got["att"][absent].any() and not got["r_att"][absent].any()
    assert not got["token_logp"][absent].any() and not got["logits"][absent].any()
    for b in range(case["B"]):
        if absent[b].all():
            assert got["best"][b] == 0


@pytest.mark.parametrize("name", list(dc.EDGE_CASES))
def test_edge_parity_with_float64(name):
    case = dc.EDGE_CASES[name]
    inp = dc.edge_inputs(case)
    ref = oracle_run(name, torch.float64)
    got = call(name, inp)
    e_lg, e_lp, e_sc = dc.errors(case, got, ref)
    print(f"[edges] {case['group']} {name}: logits {e_lg:.2e}  token_logp {e_lp:.2e}  scores {e_sc:.2e}")
    assert e_lg <= BUDGET and e_lp <= BUDGET and e_sc <= BUDGET, (e_lg, e_lp, e_sc)
    check_conventions(case, inp, got)
    # fair: test_every_edge_case_has_a_clear_winner_or_an_exact_tie (a tie case: the lower duplicate)
    assert np.array_equal(got["best"], dc.expected_best(case, ref))
    if case["reverse_weight"] == 1.0:  # total ignores att
        fin = np.isfinite(got["total"])
        want = (got["r_att"] - case["ctc_weight"] * inp["ctc_scores"])[fin]
        # 0 x att + r_att is exact; the sum with the CTC term rounds once, or not at all where it is fused
        assert (np.abs(got["total"][fin] - want) <= np.spacing(np.abs(want))).all()
        assert got["att"][fin].all()
    if (inp["lens"] < 0).all():  # nothing exists at all
        assert not got["best"].any() and not got["token_logp"].any() and not got["logits"].any()


@pytest.mark.parametrize("name", list(dc.TRAINED_CASES))
def test_trained_like_parity_with_float64(name):
    case = dc.TRAINED_CASES[name]
    inp = dc.edge_inputs(case)
    ref = oracle_run(name, torch.float64)
    e32 = dc.errors(case, oracle_run(name, torch.float32), ref)  # the float32 oracle on this very case
    tols = [nm.tol(nm.F32_BUDGET, e) for e in e32]
    got = call(name, inp)
    assert np.isfinite(got["logits"]).all() and np.isfinite(got["token_logp"]).all()
    errs = dc.errors(case, got, ref)
    print(f"[trained] {name}: " + "  ".join(f"{what} {e:.2e} / tol {t:.2e} = {e / t:.2f}"
                                             for what, e, t in zip(("logits", "token_logp", "scores"), errs, tols)))
    assert all(e <= t for e, t in zip(errs, tols)), (errs, tols)
    check_conventions(case, inp, got)
    assert np.array_equal(got["best"], dc.expected_best(case, ref))


def test_out_of_range_key_counts():
    """out_lens = 0: cross-attention attends to nothing, as the oracle's masked softmax; out_lens above Tp means Tp"""
    name = "keys_b10_t129"
    case = dc.EDGE_CASES[name]
    inp = dc.edge_inputs(case)
    ref, got = oracle_run(name, torch.float64), call(name, inp)
    b0 = list(case["out_lens"]).index(0)
    assert np.isnan(dc.poison_memory(inp)[b0]).all()  # every frame of that utterance is NaN: none may be read
    e0 = nm.utt_rel(got["logits"][b0].reshape(1, -1, case["V"]), ref["logits"][b0].reshape(1, -1, case["V"]))
    print(f"[edges] out_lens = 0: logits {e0:.2e}")
    assert np.abs(ref["logits"][b0]).max() > 1.0 and e0 <= BUDGET
    b, value = case["over"]
    assert case["out_lens"][b] == case["Tp"] < value
    over = dict(inp, out_lens=inp["out_lens"].copy())
    over["out_lens"][b] = value
    same_bytes(call(name, over, memory=dc.poison_memory(inp)), got)


def _permuted(inp, out, perm):
    """hypotheses of utterance b reordered by perm[b]: inputs and the outputs that must come of them"""
    rows = np.arange(len(perm))[:, None]
    inp2 = dict(inp, tokens=np.ascontiguousarray(inp["tokens"][rows, perm]), lens=inp["lens"][rows, perm],
                ctc_scores=inp["ctc_scores"][rows, perm])
    want = {k: np.ascontiguousarray(out[k][rows, perm]) for k in OUT_KEYS if k != "best"}
    want["best"] = np.array([list(p).index(int(k)) for p, k in zip(perm, out["best"])], np.int32)
    return inp2, want


def test_reordering_hypotheses_and_utterances_is_bit_exact():
    """every packed row goes through the same arithmetic whatever its place in its tile and whatever else the call holds"""
    name = "reorder_b3_n5"
    case = dc.EDGE_CASES[name]
    inp = dc.edge_inputs(case)
    got = call(name, inp)
    perm = np.array([[4, 2, 0, 3, 1], [1, 0, 4, 2, 3], [3, 4, 1, 0, 2]])
    assert all(sorted(p) == list(range(case["nbest"])) for p in perm)
    inp2, want = _permuted(inp, got, perm)
    assert not np.array_equal(inp2["lens"], inp["lens"])
    same_bytes(call(name, inp2), want)
    # utterances: memory and out_lens move along
    order = np.array([2, 0, 1])
    inp3 = {k: np.ascontiguousarray(v[order]) for k, v in inp.items()}
    same_bytes(call(name, inp3), {k: np.ascontiguousarray(got[k][order]) for k in OUT_KEYS})
    # both at once
    inp4 = {k: np.ascontiguousarray(v[order]) for k, v in inp2.items()}
    same_bytes(call(name, inp4), {k: np.ascontiguousarray(want[k][order]) for k in OUT_KEYS})


@pytest.mark.parametrize("name", [n for n, c in dc.EDGE_CASES.items() if "tie" in c])
def test_exact_ties_pick_the_lower_index(name):
    case = dc.EDGE_CASES[name]
    i, j = case["tie"]
    got = call(name)
    for k in ("att", "r_att", "total", "token_logp", "logits"):
        assert got[k][:, i].tobytes() == got[k][:, j].tobytes(), k
    assert np.isfinite(got["total"][:, i]).all() and (got["total"].argmax(1) == i).all()
    assert np.array_equal(got["best"], np.full(case["B"], i, np.int32))


def test_clamps_of_lens_and_token_ids():
    """lens above max_tokens count as max_tokens; token ids outside [0, V - 1] as the nearer end (include/ppasr_hip.h)"""
    name = "vocab_33"
    case = dc.EDGE_CASES[name]
    inp = dc.edge_inputs(case)
    mt, V = case["L"] - 1, case["V"]
    assert (inp["lens"][:, 0] == mt).all()
    got = call(name, inp)
    long = dict(inp, lens=inp["lens"].copy())
    long["lens"][0, 0], long["lens"][1, 0] = mt + 1, 1000
    same_bytes(call(name, long), got)
    lo_hi = dict(inp, tokens=inp["tokens"].copy())
    lo_hi["tokens"][0, 0, 2], lo_hi["tokens"][0, 0, mt - 1], lo_hi["tokens"][1, 0, 0] = 0, V - 1, V - 1
    out = dict(inp, tokens=lo_hi["tokens"].copy())
    out["tokens"][0, 0, 2], out["tokens"][0, 0, mt - 1], out["tokens"][1, 0, 0] = -5, V + 9, V + 9
    clamped = call(name, lo_hi)
    assert clamped["total"].tobytes() != got["total"].tobytes()  # (the replaced tokens do take part)
    same_bytes(call(name, out), clamped)


GUARD = 256


def _embedded(nbytes, dev):
    """-> (the whole buffer, its middle `nbytes`): GUARD bytes of poison on both sides"""
    whole = poison.fill(torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=dev), poison.BYTES["a5"])
    return whole, whole[GUARD:GUARD + nbytes]


@pytest.mark.parametrize("name", ["vocab_257", "rows_absent_u3"])
def test_nothing_is_written_outside_the_workspace_and_the_outputs(name):
    case = dc.EDGE_CASES[name]
    r = rescorer(name)
    B, nbest, L, V = case["B"], case["nbest"], case["L"], case["V"]
    need = int(r.lib.ppasr_rescorer_workspace_bytes(r._h, B, case["Tp"], nbest, L - 1))
    assert need > 0
    shapes = dict(att=((B, nbest), torch.float64), r_att=((B, nbest), torch.float64), total=((B, nbest), torch.float64),
                  best=((B,), torch.int32), token_logp=((B, nbest, 2, L), torch.float32),
                  logits=((B, nbest, 2, L, V), torch.float32))
    wholes, out = {}, {}
    wholes["workspace"], ws = _embedded(need, r.device)
    assert ws.numel() == need
    for k, (shape, dt) in shapes.items():
        n = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
        wholes[k], mid = _embedded(n, r.device)
        out[k] = mid.view(dt).reshape(shape)
    got = call(name, workspace=ws, out=out)
    torch.cuda.synchronize()
    for k, whole in wholes.items():
        g = torch.cat([whole[:GUARD], whole[-GUARD:]])
        assert bool((g == poison.BYTES["a5"]).all()), f"{k}: guard bytes changed"
    same_bytes(got, call(name))


def test_a_non_default_stream_gives_the_same_bytes():
    name = "rows_32_and_64"
    got = call(name)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        on_s = call(name)
    s.synchronize()
    same_bytes(on_s, got)
