"""ppasr_rescore against the float64 restatement of the reference's attention decoder (tests/decoder_oracle.py, itself
held to the reference's own decoder by tests/test_rescore_oracle_cpu.py) over the case table of tests/decoder_cases.py:
the decoders' logits (tap), the summed per-position log-probabilities, the sequence scores and `best`; independence of
what workspace and outputs held; the refusals that need a rescorer handle."""
import numpy as np
import pytest
import torch

import decoder_cases as dc
import numerics as nm
import poison
from decoder_oracle import DecoderOracle

pytestmark = pytest.mark.gpu

# Budgets of the three comparisons (decoder_cases.errors): logits per utterance (utt_rel), log-probabilities over the
# utterance's logit scale, scores over L x that scale.  All start from, and stay at, the budget of every fp32 transformer
# route: the first MI355X run over the whole table printed worst cases of 7.8e-7 (logits), 7.1e-7 (log-probabilities) and
# 2.6e-7 (scores), so nothing had to be widened.
LOGIT_BUDGET = nm.F32_BUDGET
LOGP_BUDGET = nm.F32_BUDGET
SCORE_BUDGET = nm.F32_BUDGET

_memo = nm.Memo()


def conf(case):
    return dict(attention_heads=dc.HEADS, linear_units=case["units"], num_blocks=case["blocks"][0],
                r_num_blocks=case["blocks"][1], dropout_rate=0.1, positional_dropout_rate=0.1,
                self_attention_dropout_rate=0.0, src_attention_dropout_rate=0.0)


def rescorer(name):
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    case = dc.CASES[name]
    return _memo.get(("gpu", name), lambda: AttentionRescorer(dc.weights(case), case["V"], conf(case)))


def ref64(name):
    def go():
        case = dc.CASES[name]
        inp = dc.inputs(case)
        o = DecoderOracle(dc.weights(case), case["V"], *case["blocks"], heads=dc.HEADS, dtype=torch.float64)
        return o.rescore(inp["memory"], inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"], case["ctc_weight"],
                         case["reverse_weight"])
    return _memo.get(("ref", name), go)


def to_np(res):
    return {("logits" if k == "logits" else k): v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", list(dc.CASES))
def test_parity_with_float64(name):
    case = dc.CASES[name]
    inp = dc.inputs(case)
    ref = ref64(name)
    memory = dc.poison_memory(inp)  # NaN behind out_lens: cross-attention must not see it
    got = to_np(rescorer(name).rescore(memory, inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"],
                                       case["ctc_weight"], case["reverse_weight"], return_token_logp=True,
                                       return_logits=True))
    e_lg, e_lp, e_sc = dc.errors(case, got, ref)
    print(f"{name}: logits {e_lg:.2e}  token_logp {e_lp:.2e}  scores {e_sc:.2e}")
    assert e_lg <= LOGIT_BUDGET and e_lp <= LOGP_BUDGET and e_sc <= SCORE_BUDGET, (e_lg, e_lp, e_sc)
    absent = inp["lens"] < 0
    assert np.array_equal(np.isneginf(got["total"]), absent)
    assert not got["att"][absent].any() and not got["r_att"][absent].any()
    if case["reverse_weight"] == 0:
        assert not got["r_att"].any() and not got["token_logp"][:, :, 1].any()
    assert np.array_equal(got["best"], ref["best"])  # (fair: test_every_case_has_a_clear_winner)
    # without the taps: the same scores, bit for bit
    plain = to_np(rescorer(name).rescore(memory, inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"],
                                         case["ctc_weight"], case["reverse_weight"]))
    for k in ("att", "r_att", "total", "best"):
        assert plain[k].tobytes() == got[k].tobytes(), k


def test_the_row_limit_itself():
    """256 rows per hypothesis (255 tokens), the most the kernels take: four key tiles in the self-attention, its last
    thread, the last row of the positional rows in use"""
    from ppasr_amd.decoders.attention_rescoring import MAX_ROWS, AttentionRescorer
    case = dict(seed=21, V=67, L=MAX_ROWS, nbest=2, B=1, Tp=33, blocks=(1, 1), units=1024, reverse_weight=0.3, short=True,
                ctc_weight=0.5)
    inp = dc.inputs(case)
    assert inp["lens"].max() == MAX_ROWS - 1
    ref = DecoderOracle(dc.weights(case), case["V"], *case["blocks"], heads=dc.HEADS, dtype=torch.float64).rescore(
        inp["memory"], inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"], 0.5, 0.3)
    got = to_np(AttentionRescorer(dc.weights(case), case["V"], conf(case)).rescore(
        dc.poison_memory(inp), inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"], 0.5, 0.3,
        return_token_logp=True, return_logits=True))
    e_lg, e_lp, e_sc = dc.errors(case, got, ref)
    print(f"256 rows: logits {e_lg:.2e}  token_logp {e_lp:.2e}  scores {e_sc:.2e}")
    assert e_lg <= LOGIT_BUDGET and e_lp <= LOGP_BUDGET and e_sc <= SCORE_BUDGET, (e_lg, e_lp, e_sc)


def test_out_lens_null_means_every_frame():
    name = "v67_l17_n3_b3_t33"
    case, inp = dc.CASES[name], dc.inputs(dc.CASES[name])
    r = rescorer(name)
    full = np.full(case["B"], case["Tp"], np.int32)
    a = to_np(r.rescore(inp["memory"], None, inp["tokens"], inp["lens"], inp["ctc_scores"], 0.5, 0.3))
    b = to_np(r.rescore(inp["memory"], full, inp["tokens"], inp["lens"], inp["ctc_scores"], 0.5, 0.3))
    assert a["total"].tobytes() == b["total"].tobytes()


@pytest.mark.parametrize("name", ["v67_l17_n3_b3_t33", "v4233_l33_n10_b1_t100", "v67_l64_n3_b1_t100"])
def test_results_do_not_depend_on_buffer_contents(name):
    """workspace and every output buffer pre-filled with NaN bytes and with large finite values: byte-identical results"""
    case, inp = dc.CASES[name], dc.inputs(dc.CASES[name])
    r = rescorer(name)
    B, nbest, L, V = case["B"], case["nbest"], case["L"], case["V"]
    need = int(r.lib.ppasr_rescorer_workspace_bytes(r._h, B, case["Tp"], nbest, L - 1))
    assert need > 0
    runs = []
    for pat in ("ff", "7f"):
        ws = poison.fill(torch.empty(need, dtype=torch.uint8, device=r.device), poison.BYTES[pat])
        out = dict(att=torch.empty(B, nbest, dtype=torch.float64, device=r.device),
                   r_att=torch.empty(B, nbest, dtype=torch.float64, device=r.device),
                   total=torch.empty(B, nbest, dtype=torch.float64, device=r.device),
                   best=torch.empty(B, dtype=torch.int32, device=r.device),
                   token_logp=torch.empty(B, nbest, 2, L, dtype=torch.float32, device=r.device),
                   logits=torch.empty(B, nbest, 2, L, V, dtype=torch.float32, device=r.device))
        for t in out.values():
            poison.fill(t, poison.BYTES[pat])
        res = r.rescore(dc.poison_memory(inp), inp["out_lens"], inp["tokens"], inp["lens"], inp["ctc_scores"],
                        case["ctc_weight"], case["reverse_weight"], return_token_logp=True, return_logits=True,
                        workspace=ws, out=out)
        runs.append({k: v.cpu().numpy().tobytes() for k, v in res.items()})
    for k in runs[0]:
        assert runs[0][k] == runs[1][k], k


def test_refusals_leave_the_outputs_untouched():
    from ppasr_amd import _lib
    name = "v67_l64_n3_b1_t100"  # blocks (1, 0): no right decoder
    case, inp = dc.CASES[name], dc.inputs(dc.CASES[name])
    r = rescorer(name)
    B, nbest = case["B"], case["nbest"]

    def outs():
        return dict(att=torch.full((B, nbest), 7.0, dtype=torch.float64, device=r.device),
                    r_att=torch.full((B, nbest), 7.0, dtype=torch.float64, device=r.device),
                    total=torch.full((B, nbest), 7.0, dtype=torch.float64, device=r.device),
                    best=torch.full((B,), 7, dtype=torch.int32, device=r.device))

    def refused(status, tokens=inp["tokens"], rw=0.0, workspace=None):
        o = outs()
        with pytest.raises(_lib.PPASRHipError) as e:
            r.rescore(inp["memory"], inp["out_lens"], tokens, inp["lens"], inp["ctc_scores"], 0.5, rw, out=o,
                      workspace=workspace)
        assert e.value.status == status, e.value
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in o.values())

    refused(_lib.PPASR_EINVAL, rw=0.3)  # reverse_weight > 0 without right blocks
    refused(_lib.PPASR_EUNSUPPORTED, tokens=np.zeros((B, nbest, 256), np.int32))  # 257 rows per hypothesis
    refused(_lib.PPASR_ENOSPACE, workspace=torch.empty(1024, dtype=torch.uint8, device=r.device))
    assert r.lib.ppasr_rescorer_workspace_bytes(r._h, B, case["Tp"], nbest, 255) > 0  # 256 rows are built
    # max_tokens + 1 above the positional table
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    small = AttentionRescorer(dc.weights(case), case["V"], dict(conf(case), max_len=32))
    o = outs()
    with pytest.raises(_lib.PPASRHipError) as e:
        small.rescore(inp["memory"], None, inp["tokens"], inp["lens"], inp["ctc_scores"], 0.5, 0.0, out=o)
    assert e.value.status == _lib.PPASR_EUNSUPPORTED


def test_missing_weight_is_named():
    from ppasr_amd import _lib
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    case = dc.CASES["v67_l2_n3_b1_t31"]
    sd = dc.weights(case)
    del sd["decoder.right_decoder.decoders.1.src_attn.linear_k.bias"]
    with pytest.raises(_lib.PPASRHipError, match="decoder.right_decoder.decoders.1.src_attn.linear_k.bias") as e:
        AttentionRescorer(sd, case["V"], conf(case))
    assert e.value.status == _lib.PPASR_EMISSING
