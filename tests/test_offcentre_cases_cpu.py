"""The off-centre and saturated cases of tests/offcentre_cases.py, on the CPU oracles (no GPU):
- each case reaches the conditioning it states (median |row mean| / row std at its LayerNorms, or the largest
  |pre-activation|), measured on the float64 oracle run;
- each case is admitted by the rule of tests/numerics.py: tol = max(family budget, 4 x e32) with e32 the fp32 oracle against
  the float64 oracle on that case, computed here; tol <= 1e-3;
- each mutation moves the float64 oracle by at least MARGIN x tol: a LayerNorm with fp32 one-pass statistics and the
  DeepSpeech2 wavefront's fold on the raw row (off-centre cases), a sigmoid written e / (1 + e) (saturated cases, NaN);
- the fold with a per-row pivot, the arithmetic k_lstm_wave uses, stays inside tol.
Every figure is printed."""
import math

import numpy as np
import pytest
import torch

import numerics as nm
import offcentre_cases as oc
from ppasr_amd.utils.synth import synth_features

MEMO = nm.Memo()
MARGIN = 5.0
# feature frames per utterance: T' = 32 / 16 output frames (4x / 8x front ends), 40 for the `linear` model, 14 for DeepSpeech2
LENS = {"linear": [40, 31, 12], "deepspeech2": [60, 41]}
LENS_DEFAULT = [131, 100, 47]


def _family(case):
    return oc.MODELS[case.model][0]


def _inputs(case):
    fam = _family(case)
    lens = LENS["linear"] if case.model == "linear" else LENS.get(fam, LENS_DEFAULT)
    return synth_features(len(lens), max(lens), lens=lens, seed=sum(lens))


def _lens_out(case):
    x, lens = _inputs(case)
    if case.model == "linear":
        return [int(n) for n in lens]
    return [((int(n) - 1) // 2 - 1) // 2 for n in lens]


def _run(case, oracle):
    x, lens = _inputs(case)
    if _family(case) == "deepspeech2":
        p = oracle.forward(x, lens)[0]
        return p
    return oracle.get_encoder_out(x, lens, return_logits=True)[1]


def _oracle(case, dtype=torch.float64):
    fam, _, _, kw, _ = oc.MODELS[case.model]
    o64 = nm.oracle64(fam, case.sd(), **kw)
    return o64 if dtype == torch.float64 else o64.__class__(case.sd(), dtype=dtype, **kw)


def _ref(case):
    """-> (float64 output, conditioning record)"""
    def make():
        oracle = _oracle(case)
        with oc.conditioning(oracle, _lens_out(case)) as rec:
            out = _run(case, oracle)
        return out, rec
    return MEMO.get(("ref", case.name), make)


def _err(case, out):
    ref = _ref(case)[0]
    if not bool(torch.isfinite(out).all()):
        return float("inf")  # (the metrics take maxima, which drop NaN)
    n = _lens_out(case)
    # (the Efficient-Conformer's stride layer halves the rows once more)
    n = [min(ref.shape[1], math.ceil(v / 2)) for v in n] if case.model == "efficient_conformer" else n
    if _family(case) == "deepspeech2":
        e = max(nm.utt_rel(out, ref, n), nm.logprob_err(out, torch.log(ref), n))
    else:
        e = max(nm.utt_rel(out, ref, n), nm.logprob_err(torch.softmax(out.to(torch.float64), -1), ref, n))
    return e if np.isfinite(e) else float("inf")


def _budget(case):
    return nm.F32_BUDGET_DS2 if _family(case) == "deepspeech2" else nm.F32_BUDGET


def _e32(case):
    return MEMO.get(("e32", case.name), lambda: _err(case, _run(case, _oracle(case, torch.float32))))


def _tol(case):
    return nm.tol(_budget(case), _e32(case))


CASES = oc.ALL_CASES


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_reaches_its_stated_conditioning(case):
    out, rec = _ref(case)
    assert bool(torch.isfinite(out).all()), case
    got, names = oc.reached(case, rec)
    print(f"{case}: {case.kind} level {got:.1f} (stated {case.level:g}) over {len(names)} LayerNorms; "
          + " ".join(f"{k.replace('encoder.', '')}={v:.0f}" for k, v in sorted(rec["ln"].items())))
    assert got >= case.level, (case, got, rec)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_is_admitted(case):
    e32, tol = _e32(case), _tol(case)
    print(f"{case}: e32 {e32:.2e} tol {tol:.2e} (budget {_budget(case):.0e})")
    assert e32 <= tol / nm.FLOOR_FACTOR
    assert tol <= nm.TOL_CAP, (case, e32, tol)


def _mutations(case):
    if case.kind == "saturated":
        return ["sigmoid_exp_ratio"]
    return ["ln_one_pass"] + (["ds2_wave_fold"] if _family(case) == "deepspeech2" else [])


@pytest.mark.parametrize("case,mutation", [(c, m) for c in CASES for m in _mutations(c)], ids=repr)
def test_tolerance_catches_the_mutation(case, mutation):
    oracle = _oracle(case)
    getattr(oc, mutation)(oracle)
    e, tol = _err(case, _run(case, oracle)), _tol(case)
    print(f"{case} / {mutation}: {e:.2e} = {e / tol:.1f} x tol ({tol:.2e})")
    assert e >= MARGIN * tol, (case, mutation, e, tol)


@pytest.mark.parametrize("case", [c for c in CASES if _family(c) == "deepspeech2" and c.kind == "offcentre"], ids=repr)
def test_pivoted_fold_stays_inside_the_tolerance(case):
    oracle = _oracle(case)
    oc.ds2_wave_fold(oracle, pivot=True)
    e, tol = _err(case, _run(case, oracle)), _tol(case)
    print(f"{case} / pivoted fold: {e:.2e} = {e / tol:.2f} x tol ({tol:.2e})")
    assert e < tol, (case, e, tol)
