"""ppasr_attention_decode does all its work on the caller's stream (tests/stream_gate.py, both modes, one small case), and
one rescorer decodes on two streams at once (a workspace per stream)."""
import pytest
import torch

import attention_search_cases as ac
import numerics as nm
import stream_gate as sg
import test_attention_decode_gpu as tad

pytestmark = pytest.mark.gpu
CASE = "v67_n3_b2_t33_p12"
MEMO = nm.Memo()


def _inputs(seed_shift):
    case = ac.CASES[CASE]
    inp = ac.inputs(dict(case, seed=case["seed"] + seed_shift))
    return [torch.from_numpy(inp["memory"]), torch.from_numpy(inp["out_lens"])]


@pytest.mark.parametrize("mode", sg.MODES)
def test_attention_decode_is_ordered_on_the_callers_stream(mode):
    case = ac.CASES[CASE]

    def run(ctx):
        r = tad.rescorer(CASE)
        ins = [ctx.input(a, b) for a, b in zip(_inputs(0), _inputs(1))]
        return dict(ctx.call(lambda: r.decode(*ins, case["N"], case["P"], return_token_logp=True, return_trace=True), ins))

    sg.check("attention_decode " + CASE, run, mode, MEMO)


def test_one_rescorer_decodes_on_two_streams():
    case = ac.CASES[CASE]
    a, b = ([t.cuda() for t in _inputs(s)] for s in (0, 1))
    go = lambda ins: lambda r: dict(r.decode(*ins, case["N"], case["P"], return_token_logp=True, return_trace=True))
    sg.check_two_streams("two streams attention_decode", lambda: tad.rescorer(CASE), go(a), go(b))
