"""The loss oracle (tests/loss_oracle.py) against independent sources, and the admission of its tolerance: runs without a
GPU.

* the float64 forward sum agrees to 1e-10 relative with torch.nn.functional.ctc_loss in float64 on the whole case table,
  and with a brute-force sum over all labelings for T <= 6;
* the closed form of the label-smoothing KL agrees with the dense t (log t - logp);
* tolerance of the CTC value: |got - ref64| / max(|ref64|, 1) <= numerics.tol(F32_BUDGET, e32), e32 the float32 numpy walk's
  error on that very case; the float32 walk itself sits below a tenth of the budget, and every listed bug exceeds the
  tolerance by >= 5 x on at least one case;
* tolerance of the attention sums: F32_BUDGET x rows x max(logit scale, 1), the sequence-score tolerance of
  tests/decoder_cases.py (each row's log-probabilities within budget x scale); every listed bug exceeds it by >= 5 x.
"""
import numpy as np
import pytest
import torch

import loss_oracle as lo
import numerics as nm

ADMIT = 5.0
TABLE = lo.case_table()


def torch_ctc64(probs, tokens, T):
    e = torch.from_numpy(lo.emissions(probs[:T], np.float64))[:, None, :]
    tgt = torch.tensor([tokens], dtype=torch.long).reshape(1, len(tokens))
    return float(torch.nn.functional.ctc_loss(e, tgt, torch.tensor([T]), torch.tensor([len(tokens)]), blank=0,
                                              reduction="none", zero_infinity=False)[0])


@pytest.mark.parametrize("i", range(len(TABLE)))
def test_float64_forward_sum_agrees_with_torch_ctc_loss(i):
    name, probs, tokens, T = TABLE[i]
    mine, st = lo.ctc_nll(probs, tokens, T)
    ref = torch_ctc64(probs, tokens, T)
    print(f"[loss-oracle] {name}: mine {mine:.9f} torch {ref:.9f}")
    assert st == lo.OK and abs(mine - ref) <= 1e-10 * max(abs(ref), 1.0)


def test_float64_forward_sum_agrees_with_brute_force():
    rng = np.random.default_rng(3)
    for T, tokens, V in [(1, [], 3), (1, [2], 3), (3, [1, 1], 3), (4, [1, 2], 4), (5, [2, 2, 1], 3), (6, [1, 2, 1], 3), (6, [], 3),
                         (6, [1, 1, 1], 3)]:
        p = lo.softmax_table(rng, T, V, blank_boost=1.0)
        mine, st = lo.ctc_nll(p, tokens)
        ref = lo.brute_force_nll(p, tokens)
        assert st == lo.OK and abs(mine - ref) <= 1e-10 * max(abs(ref), 1.0), (T, tokens, mine, ref)
    assert lo.ctc_nll(p, [1, 1, 1, 1])[1] == lo.INFEASIBLE and lo.brute_force_nll(p, [1, 1, 1, 1]) == np.inf


def test_statuses_and_the_empty_utterance():
    p = lo.softmax_table(np.random.default_rng(4), 5, 6)
    assert lo.ctc_nll(p, [], 0) == (0.0, lo.OK)
    assert lo.ctc_nll(p, [1], 0) == (np.inf, lo.INFEASIBLE)
    assert lo.ctc_nll(p, [1, 1, 1], 4) == (np.inf, lo.INFEASIBLE) and lo.ctc_nll(p, [1, 1, 1], 5)[1] == lo.OK
    for bad in ([6], [-1], [0], [1, 0, 2]):
        assert lo.ctc_nll(p, bad) == (np.inf, lo.BAD_INPUT)
    assert lo.ctc_nll(p, [1, 2], max_tokens=1) == (np.inf, lo.BAD_INPUT)
    z = np.zeros((3, 4), np.float32)  # every probability 0: clamped to FLT_MIN, finite
    nll, st = lo.ctc_nll(z, [1])
    assert st == lo.OK and np.isfinite(nll) and nll > 3 * 87.0 - 3


def test_float32_walk_sits_below_a_tenth_of_the_budget():
    worst = 0.0
    for name, probs, tokens, T in TABLE:
        ref, _ = lo.ctc_nll(probs, tokens, T)
        e32 = lo.rel_err(lo.ctc_nll(probs, tokens, T, dtype=np.float32)[0], ref)
        print(f"[loss-oracle] {name}: float32 walk {e32:.2e}")
        worst = max(worst, e32)
    assert worst < nm.F32_BUDGET / 10, worst


@pytest.mark.parametrize("bug", lo.CTC_BUGS)
def test_every_ctc_bug_leaves_the_tolerance(bug):
    best = 0.0
    for name, probs, tokens, T in TABLE:
        ref, _ = lo.ctc_nll(probs, tokens, T)
        tol = nm.tol(nm.F32_BUDGET, lo.rel_err(lo.ctc_nll(probs, tokens, T, dtype=np.float32)[0], ref))
        assert tol <= nm.TOL_CAP
        best = max(best, lo.rel_err(lo.ctc_nll(probs, tokens, T, bug=bug)[0], ref) / tol)
    print(f"[loss-oracle] {bug}: {best:.1f} x tolerance")
    assert best >= ADMIT, (bug, best)


# ---- label smoothing ------------------------------------------------------------------------------------------------------
def att_cases():
    rng = np.random.default_rng(5)
    out = []
    for V, L in [(67, 8), (257, 5), (4233, 16), (3, 2)]:
        x = rng.standard_normal((L + 1, V)) * 3.0
        out.append((V, rng.integers(1, max(V - 1, 2), L).tolist(), x))
    return out


@pytest.mark.parametrize("lsm", [0.0, 0.1, 0.5])
def test_closed_form_agrees_with_the_dense_kl(lsm):
    for V, label, x in att_cases():
        tg = lo.targets_of(label, V)
        a, b = lo.kl_rows(x, tg, lsm), lo.kl_rows_dense(x, tg, lsm)
        assert np.abs(a - b).max() <= 1e-10 * max(np.abs(b).max(), 1.0), (V, lsm)
        if lsm == 0.0:  # the plain negative log-likelihood
            logp = lo._logsoftmax(x)[np.arange(len(tg)), tg]
            assert np.abs(a + logp).max() <= 1e-12 * np.abs(logp).max()


def att_tol(x, rows):
    scale = float(np.abs(x - x.mean(-1, keepdims=True)).max())
    return nm.F32_BUDGET * rows * max(scale, 1.0)


@pytest.mark.parametrize("bug", lo.ATT_BUGS)
def test_every_attention_bug_leaves_the_tolerance(bug):
    best = 0.0
    for V, label, x in att_cases():
        for reverse in (False, True):
            ref, rows = lo.att_kl(x, label, 0.1, reverse)
            got, _ = lo.att_kl(x, label, 0.1, reverse, bug=bug)
            best = max(best, abs(got - ref) / att_tol(x, rows))
    print(f"[loss-oracle] {bug}: {best:.1f} x tolerance")
    assert best >= ADMIT, (bug, best)


def test_the_model_combination_and_its_bug():
    nll = np.array([3.0, 40.0, 7.5])
    kl, rkl, rows = np.array([10.0, 30.0, 5.0]), np.array([12.0, 28.0, 6.0]), np.array([4, 9, 2])
    r = lo.combine(nll, kl, rkl, rows, 0.3, 0.3)
    att = 0.7 * kl.sum() / 3 + 0.3 * rkl.sum() / 3
    assert abs(r["loss_ctc"] - nll.sum() / 3) < 1e-12 and abs(r["loss_att"] - att) < 1e-12
    assert abs(r["loss"] - (0.3 * nll.sum() / 3 + 0.7 * att)) < 1e-12
    n = lo.combine(nll, kl, rkl, rows, 0.3, 0.3, length_normalized_loss=True)
    assert abs(n["loss_att"] - (0.7 * kl.sum() / 15 + 0.3 * rkl.sum() / 15)) < 1e-12
    assert lo.combine(nll, None, None, None, 1.0) == dict(loss=nll.sum() / 3, loss_att=None, loss_ctc=nll.sum() / 3)
    assert lo.combine(None, kl, rkl, rows, 0.0)["loss_ctc"] is None
    assert lo.combine(np.array([1.0, np.inf]), None, None, None, 1.0)["loss"] == np.inf  # an infeasible utterance shows
    bad = lo.combine(nll, kl, rkl, rows, 0.3, 0.3, bug="div_B_dropped")
    assert lo.rel_err(bad["loss"], r["loss"]) >= ADMIT * nm.F32_BUDGET
    assert set(lo.BUGS) == set(lo.CTC_BUGS + lo.ATT_BUGS + lo.MODEL_BUGS)


# ---- the reference's own forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lo.MODEL_CASES))
def test_the_oracle_pipeline_reproduces_the_reference_forward(name):
    """tests/golden/ref_loss.npz (1.3 KiB; tests/golden/make_loss_goldens.py): ConformerModel.forward of the reference in
    float32 against the float64 pipeline, at the tolerances the GPU tests use"""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_loss.npz"))
    want, pieces = lo.model_pipeline64(name)
    tols = lo.model_tolerances(name, pieces)
    for k in ("loss", "loss_att", "loss_ctc"):
        ref = float(gold[f"{name}/{k}"])
        print(f"[loss-oracle] {name} {k}: reference {ref:.7f} pipeline64 {want[k]:.7f} tol {tols[k]:.2e}")
        assert abs(ref - want[k]) <= tols[k], (name, k, ref, want[k], tols[k])
