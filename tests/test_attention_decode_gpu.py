"""ppasr_attention_decode against the float64 restatement (tests/attention_search_oracle.py, held to the reference's own
forward_one_step by tests/test_attention_search_oracle_cpu.py):

  replay       every case, none excluded: the device's trace is a top-N of the float64 candidates at every step, up to the
               score tolerance (attention_search_cases.score_tol = F32_BUDGET x (max_steps + 1) x logit scale)
  final        token_logp of the final hypotheses against the float64 teacher-forced log-probabilities of those same
               hypotheses (this sees any wrong cache slot), scores against their sum, tokens / lens against the trace
  rescoring    the same hypotheses through ppasr_rescore (ctc_weight 0, reverse_weight 0) on the device
  exact class  tokens, lens, order, ended and steps_run equal the float64 search (EXACT_CASES, TIE_CASES)
  buffers      workspace and outputs pre-filled with NaN bytes and with large finite values; with and without the taps

Budgets: all three comparisons start from, and stay at, F32_BUDGET, the budget of every fp32 transformer route.  The
first MI355X run over every case printed worst cases of 3.8e-3 x the tolerance in the replay, 5.0e-7 (token_logp
over the logit scale), 7.9e-8 (scores) and 3.4e-7 (against ppasr_rescore), so nothing had to be widened."""
import numpy as np
import pytest
import torch

import attention_search_cases as ac
import attention_search_oracle as so
import decoder_cases as dc
import numerics as nm
import poison
from decoder_oracle import DecoderOracle

pytestmark = pytest.mark.gpu

LOGP_BUDGET = nm.F32_BUDGET
SCORE_BUDGET = nm.F32_BUDGET

ALL_CASES = dict(ac.CASES, **ac.EXACT_CASES, **ac.TIE_CASES)
_memo = nm.Memo()


def rescorer(name, case=None, **conf_kw):
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    case = case or ALL_CASES[name]
    return _memo.get(("gpu", name), lambda: AttentionRescorer(ac.case_weights(case), case["V"], ac.conf(case, **conf_kw)))


def oracle64(name, case=None):
    case = case or ALL_CASES[name]
    return _memo.get(("o64", name), lambda: DecoderOracle(ac.case_weights(case), case["V"], *case["blocks"], heads=dc.HEADS,
                                                           dtype=torch.float64))


def poisoned(inp):
    """NaN behind out_lens: cross-attention must not see it"""
    m = inp["memory"].copy()
    for b, n in enumerate(inp["out_lens"]):
        m[b, int(n):] = np.nan
    return m


def decode(name, case=None, taps=True, **kw):
    case = case or ALL_CASES[name]
    inp = ac.inputs(case)
    res = rescorer(name, case).decode(poisoned(inp), inp["out_lens"], case["N"], case["P"], return_token_logp=taps,
                                      return_trace=taps, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def device(name):
    return _memo.get(("dev", name), lambda: decode(name))


def check_replay_and_final(name, case, got, o64, inp):
    """-> (worst replay violation / tol, worst token_logp error / scale, worst score error / (L x scale))"""
    B, N, P, V = case["B"], case["N"], case["P"], case["V"]
    w_rep = w_lp = w_sc = 0.0
    steps_max = 0
    for b in range(B):
        rep = so.replay(o64, inp["memory"][b], inp["out_lens"][b], N, got["trace_parent"][:, b], got["trace_token"][:, b],
                        got["trace_score"][:, b], lambda scale: ac.score_tol(case, scale))
        assert not rep["problems"], (name, b, rep["problems"])
        w_rep = max(w_rep, rep["worst"])
        steps_max = max(steps_max, rep["steps"])
        # the outputs spell the trace's hypotheses
        hyps = so.final_from_trace(got["trace_parent"][:, b], got["trace_token"][:, b], rep["steps"], N, V - 1)
        assert hyps == rep["hyps"]
        for k in range(N):
            n = len(hyps[k])
            assert got["lens"][b, k] == n
            assert got["tokens"][b, k, :n].tolist() == hyps[k] and (got["tokens"][b, k, n:] == -1).all()
            assert got["ended"][b, k] == rep["ended"][k]
            # the float64 teacher-forced log-probabilities of that same hypothesis
            lp64, lg64 = o64.token_logp(inp["memory"][b], inp["out_lens"][b], hyps[k])
            lp64 = lp64.numpy()
            m = n + 1 if got["ended"][b, k] else n  # the eos term only when the row ended
            scale = max(float((lg64 - lg64.mean(-1, keepdim=True)).abs().max()), 1e-30)
            tl = got["token_logp"][b, k]
            assert not tl[m:].any()
            w_lp = max(w_lp, float(np.abs(tl[:m] - lp64[:m]).max() / scale) if m else 0.0)
            w_sc = max(w_sc, abs(got["scores"][b, k] - lp64[:m].sum()) / ((P + 1) * max(scale, 1.0)))
            assert got["scores"][b, k] == pytest.approx(tl[:m].astype(np.float64).sum(), abs=1e-9)
        assert (np.diff(got["scores"][b]) <= 0).all()  # best first
    assert got["steps_run"][0] == steps_max
    return w_rep, w_lp, w_sc


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_replay_and_final_hypotheses(name):
    case = ALL_CASES[name]
    w_rep, w_lp, w_sc = check_replay_and_final(name, case, device(name), oracle64(name), ac.inputs(case))
    print(f"{name}: replay {w_rep:.2e} x tol  token_logp {w_lp:.2e}  scores {w_sc:.2e}  steps_run {device(name)['steps_run'][0]}")
    assert w_rep <= 1.0 and w_lp <= LOGP_BUDGET and w_sc <= SCORE_BUDGET, (w_rep, w_lp, w_sc)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_cross_check_against_rescoring(name):
    """the device's hypotheses through ppasr_rescore with ctc_weight = 0 and reverse_weight = 0: `att` is the score without
    an oracle in between (for a hypothesis cut at max_steps, rescoring adds the eos term the search never took)"""
    case = ALL_CASES[name]
    inp, got = ac.inputs(case), device(name)
    B, N, P = case["B"], case["N"], case["P"]
    res = rescorer(name).rescore(poisoned(inp), inp["out_lens"], np.maximum(got["tokens"], 0), got["lens"],
                                 np.zeros((B, N)), 0.0, 0.0, return_token_logp=True)
    tl = res["token_logp"].cpu().numpy()[:, :, 0]
    o64, worst = oracle64(name), 0.0
    for b in range(B):
        for k in range(N):
            lg = o64.logits(inp["memory"][b], inp["out_lens"][b], got["tokens"][b, k, :got["lens"][b, k]].tolist())
            scale = max(float((lg - lg.mean(-1, keepdim=True)).abs().max()), 1.0)
            m = got["lens"][b, k] + (1 if got["ended"][b, k] else 0)
            worst = max(worst, float(np.abs(tl[b, k, :m] - got["token_logp"][b, k, :m]).max() / scale) if m else 0.0)
    print(f"{name}: search vs rescoring token_logp {worst:.2e}")
    assert worst <= LOGP_BUDGET, worst


@pytest.mark.parametrize("name", list(ac.EXACT_CASES) + list(ac.TIE_CASES))
def test_exact_class_equals_the_float64_search(name):
    case = ALL_CASES[name]
    inp, got, o64 = ac.inputs(case), device(name), oracle64(name)
    steps = 0
    for b in range(case["B"]):
        ref = so.search(o64, inp["memory"][b], inp["out_lens"][b], case["N"], case["P"])
        steps = max(steps, ref["steps"])
        for k in range(case["N"]):
            n = len(ref["tokens"][k])
            assert got["lens"][b, k] == n and got["tokens"][b, k, :n].tolist() == ref["tokens"][k], (b, k)
        assert np.array_equal(got["ended"][b], ref["ended"])
        assert np.array_equal(got["trace_parent"][:, b], ref["trace_parent"])
        assert np.array_equal(got["trace_token"][:, b], ref["trace_token"])
    assert got["steps_run"][0] == steps


def test_out_lens_null_means_every_frame():
    name = "v67_n3_b2_t33_p12"
    case, inp = ALL_CASES[name], ac.inputs(ALL_CASES[name])
    r = rescorer(name)
    full = np.full(case["B"], case["Tp"], np.int32)
    a = r.decode(inp["memory"], None, case["N"], case["P"], return_token_logp=True)
    b = r.decode(inp["memory"], full, case["N"], case["P"], return_token_logp=True)
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("name", ["v67_n3_b2_t33_p12", "v4233_n10_b2_t33_p8", "v67_n4_b9_t17_p20", "all_n4"])
def test_results_do_not_depend_on_buffer_contents_or_taps(name):
    """workspace and every output pre-filled with NaN bytes and with large finite values: byte-identical results; the
    same bytes without the taps"""
    case = ALL_CASES[name]
    r = rescorer(name)
    B, N, P = case["B"], case["N"], case["P"]
    need = r.decode_workspace_bytes(B, case["Tp"], N, P)
    assert need > 0
    runs = []
    for pat in ("ff", "7f"):
        ws = poison.fill(torch.empty(need, dtype=torch.uint8, device=r.device), poison.BYTES[pat])
        e = lambda shape, dt: poison.fill(torch.empty(shape, dtype=dt, device=r.device), poison.BYTES[pat])
        out = dict(tokens=e((B, N, P), torch.int32), lens=e((B, N), torch.int32), scores=e((B, N), torch.float64),
                   ended=e((B, N), torch.int32), steps_run=e((1,), torch.int32), token_logp=e((B, N, P + 1), torch.float32),
                   trace_parent=e((P, B, N), torch.int32), trace_token=e((P, B, N), torch.int32),
                   trace_score=e((P, B, N), torch.float64))
        runs.append({k: v.tobytes() for k, v in decode(name, workspace=ws, out=out).items()})
    ref = {k: v.tobytes() for k, v in device(name).items()}
    for k in ref:
        assert runs[0][k] == runs[1][k] == ref[k], k
    plain = decode(name, taps=False)
    assert set(plain) == {"tokens", "lens", "scores", "ended", "steps_run"}
    for k in plain:
        assert plain[k].tobytes() == ref[k], k
