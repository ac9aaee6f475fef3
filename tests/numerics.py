"""Shared numerics of the encoder tests (a plain module, imported by the test files): the float64 oracles, the
per-utterance error metrics and the fp32 error budgets every default-arithmetic comparison is held to.

The budgets were set from measurement, not borrowed from an acceptance bar (NOTES.md section 2.2): from the worst error
the MI355X route matrix (tests/test_fp64_routes_gpu.py) printed against the float64 oracle, rounded up to 1 / 2 / 5 x
10^k.  tests/test_numerics_budget_cpu.py pins them from the other side: the fp32 oracle sits below a
tenth of each budget, every constant is <= 1e-4, and each mutation of a fixed list of realistic kernel bugs exceeds its
family's budget by at least 5x.

Off-centre and saturated checkpoints (tests/offcentre_cases.py) are ill-conditioned on purpose: exact fp32 arithmetic
itself leaves the budget there.  Their tolerance is `tol(budget, e32)` below: the family budget, or four times the error
of the fp32 oracle against the float64 oracle on that very case when that is larger.  e32 is computed when the test runs,
never taken from the library under test; a case is admitted only while tol <= TOL_CAP and every mutation stays >= 5x
above it (tests/test_offcentre_cases_cpu.py)."""
import numpy as np
import torch

# Transformer families (Conformer, Efficient-Conformer, Squeezeformer), encoder logits, probabilities and stream caches.
# Measured worst case on the MI355X against the float64 oracle (tests/test_fp64_routes_gpu.py): batched routes 2.1e-6
# (every family, row threshold, route knob and attention edge), Conformer chunks 4.1e-6, Conformer session groups
# 5.6e-6, Squeezeformer chunks 9.6e-6; fp32 oracle vs float64 oracle on CPU <= 1.3e-6.  Not 10x the worst case: the
# smallest mutation of tests/test_numerics_budget_cpu.py (one Squeezeformer FFN hidden unit dropped, 1.2e-4) must stay
# >= 5x above the budget, and 2e-5 is the largest round value that keeps it there.
F32_BUDGET = 2e-5
# DeepSpeech2 (LSTM / GRU recurrences): probabilities and final states.  Measured worst case on the MI355X against the
# float64 oracle: 5.1e-6 (bidirectional LSTM, B = 3); fp32 oracle vs float64 oracle on CPU: 1.5e-6.
F32_BUDGET_DS2 = 5e-5
# every fp32 budget of this module; none may exceed 1e-4 (tests/test_numerics_budget_cpu.py)
BUDGETS = {"F32_BUDGET": F32_BUDGET, "F32_BUDGET_DS2": F32_BUDGET_DS2}

# Ill-conditioned cases: the largest ratio of a measured MI355X error to the fp32 oracle's floor recorded above is
# 5.1e-6 / 1.5e-6 = 3.4 (DeepSpeech2), rounded up.
FLOOR_FACTOR = 4.0
TOL_CAP = 1e-3  # a case whose tolerance would pass this is not admitted


def tol(budget, e32):
    """tolerance of one off-centre / saturated case: max(family budget, FLOOR_FACTOR x the fp32 oracle's error on it)"""
    return max(budget, FLOOR_FACTOR * e32)


# log-probabilities below this are compared clipped: fp32 probabilities end at ~1e-38 (e^-87)
LOG_FLOOR = -80.0


def oracle64(family, sd, **kw):
    """The family's oracle built in float64 (family: conformer / efficient_conformer / squeezeformer / deepspeech2;
    kw: the oracle's own constructor arguments)."""
    if family == "conformer":
        from oracle.conformer_oracle import ConformerOracle as cls
    elif family == "efficient_conformer":
        from oracle.efficient_conformer_oracle import EfficientConformerOracle as cls
    elif family == "squeezeformer":
        from oracle.squeezeformer_oracle import SqueezeformerOracle as cls
    elif family == "deepspeech2":
        from oracle.deepspeech2_oracle import DeepSpeech2Oracle as cls
    else:
        raise ValueError(family)
    return cls(sd, dtype=torch.float64, **kw)


class Memo:
    """Per-module cache of oracles and their outputs: one float64 run per (fixture, input), shared across the
    parametrisations that only change the route."""

    def __init__(self):
        self._d = {}

    def get(self, key, fn):
        if key not in self._d:
            self._d[key] = fn()
        return self._d[key]


def _np64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu()
        return a.to(torch.float64).numpy()
    return np.asarray(a, np.float64)


def _rows(lens_out, B, T):
    if lens_out is None:
        return [T] * B
    return [min(int(n), T) for n in (lens_out.cpu().numpy() if isinstance(lens_out, torch.Tensor) else lens_out)]


def rel(a, b):
    """max |a - b| / max |b| in float64 over two arrays of EQUAL shape: a comparison that would go through a broadcast
    (a [1, c, V] tensor against a [c, V] one) is an error of the test, not a pass."""
    a, b = _np64(a), _np64(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def utt_rel(got, ref, lens_out=None):
    """Worst utterance of max |got - ref| / max |ref| over that utterance's rows ([B, T, ...]; lens_out: valid rows per
    utterance, None = all T).  Per utterance, so that a short low-magnitude utterance cannot hide behind a long one."""
    g, r = _np64(got), _np64(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    if g.ndim == 2:
        g, r = g[None], r[None]
    worst = 0.0
    for b, n in enumerate(_rows(lens_out, g.shape[0], g.shape[1])):
        if n <= 0:
            continue
        d = np.abs(g[b, :n] - r[b, :n]).max()
        worst = max(worst, float(d / max(np.abs(r[b, :n]).max(), 1e-30)))
    return worst


def _logsoftmax64(ref):
    r = _np64(ref)
    m = r.max(-1, keepdims=True)
    return r - m - np.log(np.exp(r - m).sum(-1, keepdims=True))


def logprob_err(probs, ref_logits, lens_out=None):
    """Probabilities in log space against the float64 log_softmax of the reference logits (or log-probabilities: the
    log_softmax of those is themselves), valid frames only; worst utterance of max |log p - log p_ref| divided by that
    utterance's logit scale (max |logit - mean over the vocabulary|: probabilities fix the logits only up to a shift per
    frame).  Both sides are clipped at LOG_FLOOR, below the fp32 range.  Unlike an absolute comparison of probabilities
    this sees the tiny probabilities the beam search ranks."""
    lp_ref = _logsoftmax64(ref_logits)
    p = _np64(probs)
    assert p.shape == lp_ref.shape, (p.shape, lp_ref.shape)
    if p.ndim == 2:
        p, lp_ref = p[None], lp_ref[None]
    lp = np.log(np.maximum(p, np.exp(LOG_FLOOR)))
    worst = 0.0
    for b, n in enumerate(_rows(lens_out, p.shape[0], p.shape[1])):
        if n <= 0:
            continue
        r = lp_ref[b, :n]
        scale = max(float(np.abs(r - r.mean(-1, keepdims=True)).max()), 1e-30)
        d = np.abs(lp[b, :n] - np.maximum(r, LOG_FLOOR)).max()
        worst = max(worst, float(d / scale))
    return worst


def frame_ids_ok(got_logits, ref_logits, budget, lens_out=None):
    """Greedy ids frame by frame: equal to the float64 oracle's wherever its top-2 margin exceeds 2 x budget x the
    utterance's max |logit| (what the budget allows the two sides to move); on a near-tie frame the id may differ only
    to the reference's runner-up (the rule of tests/test_ref_pin_gpu.py).  -> (ok, number of near-tie frames)."""
    g, r = _np64(got_logits), _np64(ref_logits)
    if g.ndim == 2:
        g, r = g[None], r[None]
    near_n = 0
    for b, n in enumerate(_rows(lens_out, g.shape[0], g.shape[1])):
        if n <= 0:
            continue
        gb, rb = g[b, :n], r[b, :n]
        top2 = np.sort(rb, -1)[:, -2:]
        near = (top2[:, 1] - top2[:, 0]) <= 2 * budget * np.abs(rb).max()
        near_n += int(near.sum())
        gid, rid = gb.argmax(-1), rb.argmax(-1)
        if not np.array_equal(gid[~near], rid[~near]):
            return False, near_n
        for f in np.nonzero(near & (gid != rid))[0]:
            if gid[f] not in np.argsort(rb[f])[-2:]:
                return False, near_n
    return True, near_n


def collapse(ids, blank=0):
    """CTC collapse of one utterance's frame ids (repeats merged, blanks dropped)."""
    ids = np.asarray(ids)
    if ids.size == 0:
        return ids
    keep = np.concatenate([[True], ids[1:] != ids[:-1]]) & (ids != blank)
    return ids[keep]
