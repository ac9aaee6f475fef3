"""The attention decoder's label-smoothing loss on the device (ppasr_rescorer_loss: k_dec_output<true> and k_dec_loss of
csrc/rescore_kernels.hip) against DecoderOracle.logits (float64) and the KL restatement of tests/loss_oracle.py, over the
rescoring tests' case tables with hypothesis 0 of every utterance as its label.

Tolerance (tests/test_loss_oracle_cpu.py admits it): |att_kl - ref| <= F32_BUDGET x rows x max(logit scale, 1), the
sequence-score tolerance of tests/decoder_cases.py.
"""
import numpy as np
import pytest
import torch

import decoder_cases as dc
import loss_oracle as lo
import numerics as nm
import poison
from decoder_oracle import DecoderOracle
from ppasr_amd import _lib

pytestmark = pytest.mark.gpu
_memo = nm.Memo()
EDGE_NAMES = ["vocab_3", "vocab_32", "vocab_33", "vocab_256", "vocab_257", "vocab_512", "blocks_1_3", "rows_absent_u0",
              "rows_l17_maxlen17", "keys_b10_t129"]  # FORCED_COLUMNS at every vocabulary edge; V = 257 sits just above a tile
ALL = dict(dc.CASES, **{n: dc.EDGE_CASES[n] for n in EDGE_NAMES})
NAMES = [n for n in ALL if not (ALL[n]["V"] == 4233 and ALL[n]["L"] > 33)]  # (the float64 oracle of the longest V = 4233 cases is slow)
WORST = {"err": 0.0}


def conf(case):
    c = dict(attention_heads=dc.HEADS, linear_units=case["units"], num_blocks=case["blocks"][0], r_num_blocks=case["blocks"][1])
    if "max_len" in case:
        c["max_len"] = case["max_len"]
    return c


def rescorer(name):
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    case = ALL[name]
    key = ("gpu", case["seed"], case["V"], case["units"], case["blocks"], case.get("max_len"))
    return _memo.get(key, lambda: AttentionRescorer(dc.weights(case), case["V"], conf(case)))


def label_inputs(name):
    """hypothesis 0 of every utterance as its label"""
    case = ALL[name]
    inp = dc.case_inputs(case)
    return dict(memory=inp["memory"], out_lens=inp["out_lens"], labels=np.ascontiguousarray(inp["tokens"][:, 0]),
                label_lens=np.ascontiguousarray(inp["lens"][:, 0]))


def ref_logits(name):
    """float64 logits per utterance and direction: [B][2] of [L_b + 1, V] (None where there is no row)"""
    def go():
        case, inp = ALL[name], label_inputs(name)
        o = DecoderOracle(dc.weights(case), case["V"], *case["blocks"], heads=dc.HEADS, dtype=torch.float64)
        out = []
        for b in range(case["B"]):
            n = int(inp["label_lens"][b])
            if n < 0:
                out.append((None, None))
                continue
            tok = inp["labels"][b, :n].tolist()
            lg = [o.logits(torch.as_tensor(inp["memory"][b]).double(), int(inp["out_lens"][b]), tok, right=r).numpy()
                  if (not r or case["blocks"][1] > 0) else None for r in (False, True)]
            out.append(tuple(lg))
        return out
    return _memo.get(("ref", name), go)


def to_np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def call(name, lsm, rw=None, **kw):
    case, inp = ALL[name], label_inputs(name)
    rw = case["reverse_weight"] if rw is None else rw
    return to_np(rescorer(name).loss(dc.poison_memory(inp), inp["out_lens"], inp["labels"], inp["label_lens"], lsm, rw, **kw))


@pytest.mark.parametrize("lsm", [0.0, 0.1])
@pytest.mark.parametrize("name", NAMES)
def test_sums_against_float64(name, lsm):
    case, inp = ALL[name], label_inputs(name)
    ref = ref_logits(name)
    got = call(name, lsm)
    for b in range(case["B"]):
        n = int(inp["label_lens"][b])
        if n < 0:
            assert got["rows"][b] == 0 and got["att_kl"][b] == 0.0 and got["r_att_kl"][b] == 0.0
            continue
        tok = inp["labels"][b, :n].tolist()
        assert got["rows"][b] == n + 1
        for key, right in (("att_kl", False), ("r_att_kl", True)):
            if right and case["reverse_weight"] == 0:
                assert got[key][b] == 0.0
                continue
            x = ref[b][int(right)]
            want, rows = lo.att_kl(x, tok, lsm, reverse=right)
            tol = nm.F32_BUDGET * rows * max(float(np.abs(x - x.mean(-1, keepdims=True)).max()), 1.0)
            err = abs(got[key][b] - want)
            WORST["err"] = max(WORST["err"], err / tol)
            print(f"[att_loss] {name} lsm={lsm} b={b} {key}: got {got[key][b]:.9g} ref64 {want:.9g} err {err:.2e} tol {tol:.2e} "
                  f"| worst err / tol so far {WORST['err']:.3f}")
            assert err <= tol, (name, b, key, got[key][b], want, tol)


@pytest.mark.parametrize("name", ["v67_l17_n3_b3_t33", "v4233_l16_n1_b3_t33", "vocab_257", "rows_absent_u0"])
def test_without_smoothing_it_is_the_rescorer_score_bit_for_bit(name):
    case, inp = ALL[name], label_inputs(name)
    r = rescorer(name)
    mem = dc.poison_memory(inp)
    rs = lambda: to_np(r.rescore(mem, inp["out_lens"], inp["labels"][:, None], inp["label_lens"][:, None],
                                 np.zeros((case["B"], 1)), 0.5, case["reverse_weight"], return_token_logp=True))
    before = rs()
    got = call(name, 0.0)
    after = rs()  # a loss call in between leaves ppasr_rescore's bytes alone
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert np.array_equal(got["att_kl"], -before["att"][:, 0]) and np.array_equal(got["r_att_kl"], -before["r_att"][:, 0])
    assert got["att_kl"][inp["label_lens"] >= 0].all()
    assert np.array_equal(call(name, 0.1)["rows"], got["rows"])


def test_refusals():
    name = "rows_l17_maxlen17"  # max_len 17: 16 tokens + eos fit, 17 do not
    case, inp = ALL[name], label_inputs(name)
    r = rescorer(name)
    B, Tp = case["B"], case["Tp"]

    def status(fn):
        with pytest.raises(_lib.PPASRHipError) as e:
            fn()
        return e.value.status

    ok = lambda lsm=0.1, rw=0.3, labels=inp["labels"]: r.loss(inp["memory"], inp["out_lens"], labels, inp["label_lens"], lsm, rw)
    ok()
    for lsm in (-0.1, 1.0, 1.5, float("nan")):
        assert status(lambda: ok(lsm=lsm)) == _lib.PPASR_EINVAL
    assert status(lambda: ok(rw=1.5)) == _lib.PPASR_EINVAL
    assert status(lambda: ok(labels=np.ones((B, 17), np.int32))) == _lib.PPASR_EUNSUPPORTED  # max_len
    left_only = rescorer("v67_l1_n1_b1_t1")
    one = label_inputs("v67_l1_n1_b1_t1")
    args = (one["memory"], one["out_lens"], one["labels"], one["label_lens"])
    left_only.loss(*args, 0.1, 0.0)
    assert status(lambda: left_only.loss(*args, 0.1, 0.3)) == _lib.PPASR_EINVAL  # no right decoder
    assert status(lambda: left_only.loss(one["memory"], None, np.ones((1, 256), np.int32), one["label_lens"], 0.1, 0.0)) \
        == _lib.PPASR_EUNSUPPORTED  # 255 tokens at the most
    need = int(r.lib.ppasr_rescorer_loss_workspace_bytes(r._h, B, Tp, 16))
    assert need > int(r.lib.ppasr_rescorer_workspace_bytes(r._h, B, Tp, 1, 16)) > 0
    small = torch.empty(need - 64, dtype=torch.uint8, device=r.device)
    assert status(lambda: r.loss(inp["memory"], inp["out_lens"], inp["labels"], inp["label_lens"], 0.1, 0.3, workspace=small)) \
        == _lib.PPASR_ENOSPACE
    torch.cuda.synchronize()


@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_no_result_depends_on_buffer_contents(pattern, monkeypatch):
    names = ["v67_l17_n3_b3_t33", "vocab_257"]
    other = "v67_l65_n10_b3_t31"

    def go(s):
        owners = [rescorer(n) for n in names]
        if s.pattern == "zero":
            for r in owners:
                r._ws.clear()
        outs = {}
        for n, r in zip(names, owners):
            case, inp = ALL[n], label_inputs(n)
            if s.stale:  # what a rescoring call of another shape leaves in the same workspace
                oc, oi = ALL[other], dc.case_inputs(ALL[other])
                if r is owners[0]:
                    r.rescore(oi["memory"], oi["out_lens"], oi["tokens"], oi["lens"], oi["ctc_scores"], 0.5, oc["reverse_weight"])
                else:
                    r.loss(inp["memory"], None, inp["labels"][:, :3], np.minimum(inp["label_lens"], 3), 0.3, 0.3)
            s.scratch(r)
            out = r.loss(dc.poison_memory(inp), inp["out_lens"], inp["labels"], inp["label_lens"], 0.1, case["reverse_weight"])
            s.observe(r, n)
            torch.cuda.synchronize()
            outs.update({f"{n}/{k}": v for k, v in out.items()})
        return outs, owners

    poison.check("att_loss", go, pattern, monkeypatch, _memo)
