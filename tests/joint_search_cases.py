"""Case tables of the CTC-joint attention search tests.  A case is an attention_search_cases case (decoder and memory from
its seed) plus a CTC table made from the same seed (`table`: "random", "peaked" on `transcripts`, "extreme"), `w` =
ctc_weight and `blank`.

CASES        replay cases: every edge of csrc/attn_decode_joint.hip at the smallest shape that reaches it
EXACT_CASES  beams of 1 to 3 (rows that end at different steps, that all end, that never end) whose smallest float64 gap over all steps -- at the beam cut and between kept neighbours -- is at
             least EXACT_FACTOR x the score tolerance, and on which the float32 search returns the float64 search's tokens,
             order and flags (tests/test_ctc_prefix_oracle_cpu.py asserts both, so nothing is skipped at run time)
DEMO         a first_* decoder of attention_search_cases (the empty hypothesis wins at step 1) with a table peaked on a
             3-token transcript with a repeated token

TOLERANCE.  Psi is a log-sum over alignments; every finite Psi, rn and rb is a sum of T emissions, so it lies in [-S, 0]
with S = sum over the valid frames of max_v |x[t][v]| (PrefixScorer.S), and its fp32 error is rounding relative to partial
sums of that size: it scales with S, that is with the number of summed terms.
    psi_tol   = numerics.tol(F32_BUDGET, e32) x max(S, 1)
    score_tol = attention_search_cases.score_tol + w x (2 x psi_tol + (P + 1) x 2^-23 x max(S, 1))
e32 is the float32 restatement's own error, max |Psi32 - Psi64| / max(S, 1) over every Psi(g.v) of every live row the
float64 search of the case visits, measured on the CPU and recorded per case in FLOORS
(tests/test_ctc_prefix_oracle_cpu.py measures it again and holds the record to it).  The score's CTC share telescopes to
w x Psi(final hypothesis), one Psi error, plus the rounding of P + 1 differences and products; 2 x psi_tol covers the
candidate's own Psi(g.v) on top.  A case whose numerics.tol(F32_BUDGET, e32) would pass TOL_CAP is not admitted."""
import numpy as np

import attention_search_cases as ac
import numerics as nm
from align_oracle import FLT_MIN

EXACT_FACTOR = ac.EXACT_FACTOR
W = 0.5


def _j(seed, V=67, N=2, B=1, Tp=9, P=4, blocks=(1, 0), units=256, eos_bias=0.0, out_lens=None, table="random", w=W, blank=0,
       **kw):
    return ac._c(seed, V, N, B, Tp, P, blocks, units, eos_bias, out_lens, table=table, w=w, blank=blank, **kw)


FRAME_COUNTS = (63, 64, 65, 129)  # around the 64-frame chunk of k_aj_psi, k_aj_update and k_aj_init
CASES = {
    "v67_n3_b2_t33_p12": dict(ac.CASES["v67_n3_b2_t33_p12"], table="random", w=W, blank=0),
    # T = 0, 1, 2 and Tp in one batch: nothing but eos at T = 0, infeasible extensions (L + 1 + repeats > T) at 1 and 2
    "lens_0_1_2_tp": _j(301, N=3, B=4, Tp=5, P=5, out_lens=[0, 1, 2, 5], eos_bias=-2.0),
    "frames_b4_t129": _j(302, N=2, B=4, Tp=129, P=4, out_lens=list(FRAME_COUNTS), eos_bias=-4.0),
    "vocab_2": _j(303, V=2, N=2, P=3, eos_bias=-1.0),  # no token but blank and eos: one finite candidate, one row at -inf
    "vocab_33": _j(304, V=33, N=3, P=3),
    "vocab_256": _j(305, V=256, N=4, P=3), "vocab_257": _j(306, V=257, N=4, P=3, blank=256 - 1),
    "vocab_4233": _j(307, V=4233, N=4, P=3, blank=4231),
    "beam_1": _j(308, N=1, B=3, P=6, eos_bias=-2.0),
    "beam_32": _j(309, N=32, B=2, eos_bias=3.0),
    "rows_31": _j(311, N=1, B=31, Tp=5, P=3), "rows_32": _j(312, N=2, B=16, Tp=5, P=3),
    "rows_33": _j(313, N=3, B=11, Tp=5, P=3), "rows_65": _j(314, N=5, B=13, Tp=5, P=3),
    # adjacent repeats, with exactly the frames the transcript needs (every other extension is infeasible) and with two more
    "repeats_tight": _j(321, N=3, B=2, Tp=8, P=7, table="peaked", transcripts=[[5, 5, 9, 9, 9], [7, 7, 7]], out_lens=[8, 5],
                        eos_bias=-2.0, peak=1.0),
    "repeats_loose": _j(322, N=3, B=2, Tp=10, P=7, table="peaked", transcripts=[[5, 5, 9, 9, 9], [7, 7, 7]], out_lens=[10, 7],
                        eos_bias=-2.0, peak=0.99999),
    # saturated rows with zeros, denormals and FLT_MIN; where phi of [5] peaks the candidate 9 has FLT_MIN, and where 9 has
    # 1.0 phi lies e^-87 below its peak; utterance 1 is a table of zeros
    "extreme": _j(331, N=3, B=2, Tp=9, P=6, table="extreme", eos_bias=-2.0),
}

# float32 floors e32 (see the module docstring), as the CPU scan printed them, rounded up to three digits.  All lie below
# F32_BUDGET / FLOOR_FACTOR = 5e-6, so every case's unit is F32_BUDGET itself.
FLOORS = {
    "v67_n3_b2_t33_p12": 5.33e-08,
    "lens_0_1_2_tp": 5.12e-08,
    "frames_b4_t129": 1.02e-07,
    "vocab_2": 4.92e-08,
    "vocab_33": 2.84e-08,
    "vocab_256": 5.67e-08,
    "vocab_257": 4.36e-08,
    "vocab_4233": 6.12e-08,
    "beam_1": 4.05e-08,
    "beam_32": 6.69e-08,
    "rows_31": 5.32e-08,
    "rows_32": 4.65e-08,
    "rows_33": 4.95e-08,
    "rows_65": 4.86e-08,
    "repeats_tight": 4.42e-08,
    "repeats_loose": 7.84e-08,
    "extreme": 7.18e-08,
    "n1_mixed": 1.52e-07,
    "n1_never": 1.08e-07,
    "n2_mixed": 1.36e-07,
    "n2_all": 1.30e-07,
    "n2_mixed_eos4": 1.64e-07,
    "n3_mixed": 1.34e-07,
    "n3_all": 1.01e-07,
    "n3_never": 1.91e-07,
    "demo": 3.26e-08,
}


def _x(seed, N, eos_bias, peak=0.9, **kw):
    return _j(seed, N=N, B=2, Tp=17, P=12, eos_bias=eos_bias, out_lens=[17, 12], table="peaked", peak=peak, **kw)


# Chosen by a seed scan on the CPU (seeds 400 .. 415 per row of settings: beams 1, 2, 3 at eos_bias 0 and 4, tables peaked
# at 0.9 on seeded transcripts of 2 to 5 tokens, 17 and 12 valid frames).  Beside each case: the smallest gap over the
# tolerance the scan printed.
EXACT_CASES = {
    "n1_mixed": _x(414, 1, 0.0),     # 40.8
    "n1_never": _x(410, 1, 0.0),     # 15.7
    "n2_mixed": _x(409, 2, 0.0),     # 7.6
    "n2_all": _x(412, 2, 0.0),       # 9.1
    "n2_mixed_eos4": _x(402, 2, 4.0),  # 19.3
    "n3_mixed": _x(404, 3, 0.0),     # 4.2
    "n3_all": _x(404, 3, 4.0),       # 6.5
    "n3_never": _x(411, 3, 0.0),     # 5.1
}

# decoder of attention_search_cases.EXACT_CASES["first_n2"]; the table is peaked on [5, 5, 9]
DEMO = dict(ac.EXACT_CASES["first_n2"], B=1, Tp=12, P=6, out_lens=[12], table="peaked", transcripts=[[5, 5, 9]], peak=1.0,
            w=W, blank=0)
DEMO_TRANSCRIPT = [5, 5, 9]


def _peaked(rng, Tp, T, V, blank, transcript, peak):
    """frames t < T: `peak` on an alignment of the transcript (a blank between equal neighbours, the spare frames as
    further frames of a unit, spread from the seed), the rest shared equally"""
    need = len(transcript) + sum(1 for i in range(1, len(transcript)) if transcript[i] == transcript[i - 1])
    assert T >= need
    units = []
    for i, c in enumerate(transcript):
        if i and transcript[i - 1] == c:
            units.append(blank)
        units.append(c)
    path = list(units)
    for _ in range(T - need):  # a spare frame repeats the frame before it (a leading one is blank): the collapse stays
        i = int(rng.integers(0, len(path) + 1))
        path.insert(i, path[i - 1] if i > 0 else blank)
    p = np.full((Tp, V), (1.0 - peak) / (V - 1))
    for t, c in enumerate(path):
        p[t, c] = peak
    p[T:] = 1.0 / V
    return p


def _extreme(rng, Tp, V, blank):
    p = np.zeros((2, Tp, V))
    for t, c in enumerate([5, blank, 7, 9, 9, blank, 9, blank, blank][:Tp]):
        p[0, t, c] = 1.0
    p[0, ::2, 11] = 1e-40  # denormals
    p[0, 1::2, 12] = float(FLT_MIN)
    p[0, 4, 13] = 1e-30
    return p  # utterance 1: every emission is log FLT_MIN


def transcripts(case):
    """the transcripts a "peaked" table is peaked on: the case's own, or 2 to 5 tokens per utterance from its seed (a token
    repeats its neighbour with probability 0.3)"""
    if case.get("transcripts") is not None:
        return case["transcripts"]
    rng = np.random.default_rng(8500 + case["seed"])
    out = []
    for _ in range(case["B"]):
        t = []
        for _ in range(int(rng.integers(2, 6))):
            t.append(t[-1] if t and rng.random() < 0.3 else int(rng.integers(1, case["V"] - 1)))
        out.append(t)
    return out


def table(case):
    """-> probs [B, Tp, V] f32"""
    rng = np.random.default_rng(8000 + case["seed"])
    B, Tp, V, blank = case["B"], case["Tp"], case["V"], case["blank"]
    lens = case["out_lens"] if case["out_lens"] is not None else [Tp] * B
    if case["table"] == "random":
        lg = 3.0 * rng.standard_normal((B, Tp, V))
        lg[..., blank] += 2.0
        e = np.exp(lg - lg.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
    elif case["table"] == "peaked":
        p = np.stack([_peaked(rng, Tp, min(max(int(lens[b]), 0), Tp), V, blank, transcripts(case)[b], case["peak"])
                      for b in range(B)])
    elif case["table"] == "extreme":
        assert B == 2
        p = _extreme(rng, Tp, V, blank)
    else:
        raise ValueError(case["table"])
    return np.ascontiguousarray(p, np.float32)


def unit(name_or_floor):
    """numerics.tol(F32_BUDGET, e32) of a case: the tolerance of one Psi in units of max(S, 1)"""
    e32 = FLOORS[name_or_floor] if isinstance(name_or_floor, str) else float(name_or_floor)
    u = nm.tol(nm.F32_BUDGET, e32)
    assert u <= nm.TOL_CAP, (name_or_floor, u)
    return u


def psi_tol(S, u):
    return u * max(S, 1.0)


def score_tol(case, scale, S, u):
    return ac.score_tol(case, scale) + case["w"] * (2.0 * psi_tol(S, u) + (case["P"] + 1) * 2.0 ** -23 * max(S, 1.0))
