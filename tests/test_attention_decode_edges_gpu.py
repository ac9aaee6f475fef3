"""ppasr_attention_decode on the edges of its kernels (attention_search_cases.EDGE_CASES: prefix lengths across the
self-attention's key chunk and at the row limit, cross-attention key counts, dense row tiles, the widest beam, vocabulary
tiles with forced winners, decoder depth, FFN width), every case through the replay and the final-hypothesis checks of
tests/test_attention_decode_gpu.py at the same budgets; an utterance that finishes many steps before another; every
refusal.  Exact ties and hypotheses cut at max_steps are cases of tests/test_attention_decode_gpu.py (TIE_CASES, never_*).

The first MI355X run printed worst cases of 9.5e-3 x the tolerance in the replay, 5.3e-7 (token_logp) and 2.0e-7
(scores): inside F32_BUDGET, nothing widened."""
import pytest
import torch

import attention_search_cases as ac
import test_attention_decode_gpu as tad

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(ac.EDGE_CASES))
def test_edge_case(name):
    case = ac.EDGE_CASES[name]
    got = tad.decode(name, case)
    w_rep, w_lp, w_sc = tad.check_replay_and_final(name, case, got, tad.oracle64(name, case), ac.inputs(case))
    print(f"{name}: replay {w_rep:.2e} x tol  token_logp {w_lp:.2e}  scores {w_sc:.2e}  steps_run {got['steps_run'][0]}")
    assert w_rep <= 1.0 and w_lp <= tad.LOGP_BUDGET and w_sc <= tad.SCORE_BUDGET, (w_rep, w_lp, w_sc)
    if name.startswith("steps_"):  # eos suppressed: every row is cut at max_steps, full length
        assert got["steps_run"][0] == case["P"] and not got["ended"].any() and (got["lens"] == case["P"]).all()
    if "force" in case:  # the forced columns are what the first step's candidates are made of
        first = set(got["trace_token"][0, 0].tolist())
        assert first <= set(case["force"]), (first, case["force"])


def test_edge_table_covers_the_grid():
    cs = ac.EDGE_CASES
    assert {c["P"] for n, c in cs.items() if n.startswith("steps_")} == {63, 64, 65, 129, 255}
    assert cs["keys_b8_t129"]["out_lens"] == [1, 7, 8, 9, 63, 64, 65, 129]
    assert {c["B"] * c["N"] for n, c in cs.items() if n.startswith("rows_")} == {31, 32, 33, 64, 65}
    assert {c["N"] for c in list(cs.values()) + list(ac.CASES.values())} >= {1, 10, 32}
    assert {c["V"] for n, c in cs.items() if n.startswith("vocab_")} == {2, 33, 256, 257, 4233}
    assert set(cs["vocab_4233"]["force"]) == {0, 31, 32, 255, 256, 4231, 4232}
    assert {c["blocks"] for c in list(cs.values()) + list(ac.CASES.values())} >= {(1, 0), (3, 3), (6, 2)}
    assert {c["units"] for c in cs.values()} >= {256, 768, 4096}


def test_an_utterance_that_finished_early_stays_as_it_was():
    """mixed_n2_early: utterance 0 is done at step 3, utterance 1 runs all 12 steps.  Utterance 0's outputs equal, byte for
    byte, those of a call that holds it alone, and nothing is traced for it after its last step."""
    name = "mixed_n2_early"
    case, inp = ac.EXACT_CASES[name], ac.inputs(ac.EXACT_CASES[name])
    both = tad.device(name)
    alone = tad.rescorer(name).decode(inp["memory"][:1], inp["out_lens"][:1], case["N"], case["P"], return_token_logp=True,
                                      return_trace=True)
    alone = {k: v.cpu().numpy() for k, v in alone.items()}
    done = int(alone["steps_run"][0])
    assert done < both["steps_run"][0] == case["P"] and alone["ended"].all()
    for k in ("tokens", "lens", "scores", "ended", "token_logp"):
        assert both[k][:1].tobytes() == alone[k].tobytes(), k
    for k in ("trace_parent", "trace_token", "trace_score"):
        assert both[k][:, :1].tobytes() == alone[k].tobytes(), k
        assert (both[k][done:, 0] == (0 if k == "trace_score" else -1)).all()


def test_refusals_leave_the_outputs_untouched():
    from ppasr_amd import _lib
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    name = "v67_n3_b2_t33_p12"
    case, inp = ac.CASES[name], ac.inputs(ac.CASES[name])
    r = tad.rescorer(name)
    B = case["B"]

    def refused(status, N=3, P=12, workspace=None, rescorer=r):
        out = dict(tokens=torch.full((B, N, P), 7, dtype=torch.int32, device=r.device),
                   lens=torch.full((B, N), 7, dtype=torch.int32, device=r.device),
                   scores=torch.full((B, N), 7.0, dtype=torch.float64, device=r.device),
                   ended=torch.full((B, N), 7, dtype=torch.int32, device=r.device),
                   steps_run=torch.full((1,), 7, dtype=torch.int32, device=r.device))
        if workspace is None:  # (a shape the library refuses has no workspace size)
            workspace = torch.empty(1 << 20, dtype=torch.uint8, device=r.device)
        with pytest.raises(_lib.PPASRHipError) as e:
            rescorer.decode(inp["memory"], inp["out_lens"], N, P, out=out, workspace=workspace)
        assert e.value.status == status, e.value
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in out.values())

    refused(_lib.PPASR_EINVAL, N=0)
    refused(_lib.PPASR_EINVAL, N=68)  # beam_size > V = 67
    refused(_lib.PPASR_EINVAL, P=0)
    refused(_lib.PPASR_EUNSUPPORTED, N=33)  # <= V, above the 32 the selection takes
    refused(_lib.PPASR_EUNSUPPORTED, P=256)  # 257 rows
    refused(_lib.PPASR_ENOSPACE, workspace=torch.empty(1024, dtype=torch.uint8, device=r.device))
    assert r.decode_workspace_bytes(B, case["Tp"], 32, 255) > 0  # the limits themselves are built
    assert r.decode_workspace_bytes(B, case["Tp"], 33, 12) == 0 and r.decode_workspace_bytes(B, case["Tp"], 3, 256) == 0
    small = AttentionRescorer(ac.weights(case), case["V"], ac.conf(case, max_len=12))
    refused(_lib.PPASR_EUNSUPPORTED, P=12, rescorer=small)  # max_steps + 1 above the positional table
    assert small.default_max_steps(33) == 11
