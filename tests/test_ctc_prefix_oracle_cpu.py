"""The float64 yardsticks of the CTC-joint attention search, checked on the CPU: the prefix scorer
(tests/ctc_prefix_oracle.py) against the enumeration of every path, the search (tests/joint_search_oracle.py) against its
named bugs, the admission of the exact class and of the float32 floors (tests/joint_search_cases.py), the demonstration
case, and the replay on the oracle's own traces."""
import itertools

import numpy as np
import pytest
import torch

import attention_search_cases as ac
import attention_search_oracle as so
import ctc_prefix_oracle as cp
import decoder_cases as dc
import joint_search_cases as jc
import joint_search_oracle as jo
import loss_oracle as lo
import numerics as nm
from decoder_oracle import DecoderOracle

ALL = dict(jc.CASES, **jc.EXACT_CASES, demo=jc.DEMO)
_memo = nm.Memo()


def oracle(name, dtype=torch.float64):
    case = ALL[name]
    return _memo.get(("o", name, dtype), lambda: DecoderOracle(ac.case_weights(case), case["V"], *case["blocks"],
                                                                heads=dc.HEADS, dtype=dtype))


def run(name, f64=True, mut=None, w=None):
    """the search of every utterance of a case -> list of search() results (gaps recorded)"""
    case = ALL[name]

    def go():
        inp, tab = ac.inputs(case), jc.table(case)
        o = oracle(name, torch.float64 if f64 else torch.float32)
        return [jo.search(o, inp["memory"][b], inp["out_lens"][b], tab[b], case["blank"], case["w"] if w is None else w,
                          case["N"], case["P"], dtype=np.float64 if f64 else np.float32, mut=mut, record_gaps=True)
                for b in range(case["B"])]
    return _memo.get(("run", name, f64, mut, w), go)


def measured_floor(name):
    case = ALL[name]
    inp, tab = ac.inputs(case), jc.table(case)
    return max(jo.floor_e32(tab[b], inp["out_lens"][b], case["blank"], r["psi_seen"]) for b, r in enumerate(run(name)))


# ---- the restatement against the enumeration of every path ------------------------------------------------------------------
V_ENUM = 4  # blank 0, tokens 1 .. 3; the scorer gets one more column, its eos, so that every column of the table is a token


def _tiny(T, seed=0):
    rng = np.random.default_rng(seed + T)
    p = rng.random((T, V_ENUM)).astype(np.float32)
    if T:
        p[0, 2] = 0.0  # a zero: clamped to FLT_MIN on both sides
        p /= p.sum(1, keepdims=True)
    return p, np.concatenate([p, np.zeros((T, 1), np.float32)], 1)


def _prefixes():
    return [g for L in range(4) for g in itertools.product(range(1, V_ENUM), repeat=L)]


@pytest.mark.parametrize("T", [0, 1, 2, 3, 5])
def test_restatement_equals_path_enumeration(T):
    """exp Psi(g) is the probability that the collapsed transcript starts with g, Psi(g.eos) = log P_ctc(g) = -ctc_nll(g),
    exp Psi(g) = P_ctc(g) + sum_{c != blank} exp Psi(g.c), and Psi(g.c) <= Psi(g).  The recurrence takes the frames behind
    the prefix's end to sum to 1; the fp32 table's rows do so up to 2^-24 each, hence the T x 2^-23 allowed."""
    p, padded = _tiny(T)
    ps = cp.PrefixScorer(padded, None, 0)
    slack = T * 2.0 ** -23 + 1e-12
    worst = 0.0
    for g in _prefixes():
        st = ps.state_of(g)
        psi, ref = float(st.psi), cp.prefix_logprob_enum(p, g)
        assert np.isfinite(psi) == np.isfinite(ref), (g, psi, ref)
        if np.isfinite(ref):
            worst = max(worst, abs(psi - ref))
        pc = ps.psi_all(st)
        assert pc[0] == -np.inf  # blank
        nll, status = lo.ctc_nll(padded, list(g))
        eos = float(pc[V_ENUM])
        if status == lo.OK:
            assert abs(eos + float(nll)) <= 1e-9 * max(1.0, abs(float(nll))), (g, eos, nll)
            assert abs(eos - cp.prefix_logprob_enum(p, g, exact=True)) <= 1e-9 * max(1.0, abs(eos))
        else:
            assert eos == -np.inf
        assert (pc <= psi + slack).all(), g
        if np.isfinite(psi):
            with np.errstate(divide="ignore"):
                total = np.log(np.exp(eos) + sum(np.exp(float(pc[c])) for c in range(1, V_ENUM)))
            assert abs(total - psi) <= slack * max(1.0, abs(psi)), (g, total, psi)
    print(f"T {T}: worst |Psi - enumeration| {worst:.2e}")
    assert worst <= slack


@pytest.mark.parametrize("T", [0, 1, 2, 3, 5])
def test_float32_restatement_stays_close(T):
    _, padded = _tiny(T)
    p64, p32 = cp.PrefixScorer(padded, None, 0), cp.PrefixScorer(padded, None, 0, np.float32)
    for g in _prefixes():
        a, b = p64.psi_all(p64.state_of(g)), p32.psi_all(p32.state_of(g)).astype(np.float64)
        assert np.array_equal(np.isfinite(a), np.isfinite(b))
        ok = np.isfinite(a)
        assert (np.abs(a[ok] - b[ok]) <= nm.F32_BUDGET / 10 * max(p64.S, 1.0)).all()


def test_out_len_clamps_and_hides_the_frames_behind_it():
    p = np.random.default_rng(3).random((6, 5)).astype(np.float32)
    q = p.copy()
    q[4:] = np.nan
    for out_len, T in ((-3, 0), (0, 0), (4, 4), (6, 6), (9, 6), (None, 6)):
        assert cp.PrefixScorer(p, out_len).T == T
    a, b = cp.PrefixScorer(p, 4), cp.PrefixScorer(q, 4)
    assert np.array_equal(a.psi_all(a.state_of([1, 1, 2])), b.psi_all(b.state_of([1, 1, 2])))


# ---- the named bugs ------------------------------------------------------------------------------------------------------------
BUG_CASES = ("demo", "repeats_tight", "repeats_loose", "lens_0_1_2_tp", "v67_n3_b2_t33_p12", "n2_all")


def _differs(name, a, b):
    case = ALL[name]
    for ra, rb in zip(a, b):
        if ra["tokens"] != rb["tokens"] or not np.array_equal(ra["ended"], rb["ended"]):
            return True
        tol = jc.score_tol(case, ra["scale"], ra["S"], jc.unit(name))
        fin = np.isfinite(ra["scores"])
        if not np.array_equal(fin, np.isfinite(rb["scores"])) or (np.abs(ra["scores"][fin] - rb["scores"][fin]) > tol).any():
            return True
    return False


@pytest.mark.parametrize("bug", cp.BUGS)
def test_every_named_bug_changes_a_committed_case(bug):
    seen = [name for name in BUG_CASES if _differs(name, run(name), run(name, mut=bug))]
    print(f"{bug}: seen by {seen}")
    assert seen, bug


# ---- admission: floors, the exact class, the demonstration case --------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL))
def test_recorded_floor_is_the_measured_one(name):
    fl = measured_floor(name)
    rec = jc.FLOORS[name]
    print(f"{name}: float32 floor {fl:.2e} (recorded {rec:.1e}), unit {jc.unit(name):.1e}, S {max(r['S'] for r in run(name)):.0f}")
    assert fl <= rec <= 1.12 * fl + 1e-12, (fl, rec)
    assert jc.unit(name) <= nm.TOL_CAP


@pytest.mark.parametrize("name", list(jc.EXACT_CASES) + ["demo"])
def test_exact_class_admission(name):
    r64, r32 = run(name), run(name, f64=False)
    margin = min(r["min_gap"] / jc.score_tol(ALL[name], r["scale"], r["S"], jc.unit(name)) for r in r64)
    print(f"{name}: smallest gap / tolerance {margin:.1f}")
    assert margin >= jc.EXACT_FACTOR, margin
    for a, b in zip(r64, r32):
        assert a["tokens"] == b["tokens"] and np.array_equal(a["ended"], b["ended"]) and a["steps"] == b["steps"]
        assert np.array_equal(a["trace_parent"], b["trace_parent"]) and np.array_equal(a["trace_token"], b["trace_token"])


def test_exact_class_covers_the_beams_and_the_endings():
    kinds = {}
    for name in jc.EXACT_CASES:
        for r in run(name):
            n = int(r["ended"].sum())
            kinds.setdefault(ALL[name]["N"], set()).add("all" if n == len(r["ended"]) else "never" if n == 0 else "mixed")
    assert set(kinds) == {1, 2, 3} and all(k >= {"all", "never"} for k in kinds.values()), kinds
    assert "mixed" in kinds[2] | kinds[3]


def test_demonstration_case():
    """the attention decoder alone returns the empty hypothesis; with ctc_weight 0.5 and a table peaked on [5, 5, 9] the
    search returns that transcript, repeated token included"""
    case = jc.DEMO
    inp = ac.inputs(case)
    plain = so.search(oracle("demo"), inp["memory"][0], inp["out_lens"][0], case["N"], case["P"])
    assert plain["tokens"][0] == [] and plain["ended"][0] == 1
    joint = run("demo")[0]
    assert joint["tokens"][0] == jc.DEMO_TRANSCRIPT == jc.transcripts(case)[0] and joint["ended"][0] == 1
    assert jc.DEMO_TRANSCRIPT[0] == jc.DEMO_TRANSCRIPT[1]


# ---- the replay on the oracle's own traces -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n2_mixed", "n3_all", "lens_0_1_2_tp", "vocab_2", "repeats_tight", "extreme", "demo"])
def test_replay_passes_the_clean_searches_and_sees_a_bug(name):
    case = ALL[name]
    inp, tab = ac.inputs(case), jc.table(case)
    u = jc.unit(name)
    for f64 in (True, False):
        for b, r in enumerate(run(name, f64=f64)):
            rep = jo.replay(oracle(name), inp["memory"][b], inp["out_lens"][b], tab[b], case["blank"], case["w"], case["N"],
                            r["trace_parent"], r["trace_token"], r["trace_score"], r["trace_ctc"],
                            lambda scale: jc.score_tol(case, scale, r["S"], u), jc.psi_tol(r["S"], u))
            assert not rep["problems"], (name, f64, b, rep["problems"])
            assert rep["steps"] == r["steps"] and rep["hyps"] == r["tokens"]
            assert rep["worst"] <= (1e-9 if f64 else 1.0) and rep["worst_psi"] <= (1e-9 if f64 else 1.0)
    bad = [r for r in run(name, mut="psi_g_not_subtracted")]
    probs = []
    for b, r in enumerate(bad):
        rep = jo.replay(oracle(name), inp["memory"][b], inp["out_lens"][b], tab[b], case["blank"], case["w"], case["N"],
                        r["trace_parent"], r["trace_token"], r["trace_score"], r["trace_ctc"],
                        lambda scale: jc.score_tol(case, scale, r["S"], u), jc.psi_tol(r["S"], u))
        probs += rep["problems"]
    if name != "vocab_2":  # (its one candidate per step is eos at Psi(empty) = 0: the bug changes nothing there)
        assert probs, name


def test_case_table_covers_the_grid():
    cs = jc.CASES
    assert cs["lens_0_1_2_tp"]["out_lens"] == [0, 1, 2, cs["lens_0_1_2_tp"]["Tp"]]
    assert cs["frames_b4_t129"]["out_lens"] == [63, 64, 65, 129]
    assert {c["V"] for n, c in cs.items() if n.startswith("vocab_")} == {2, 33, 256, 257, 4233}
    assert all(c["Tp"] <= 9 for n, c in cs.items() if n.startswith("vocab_"))
    assert {c["N"] for c in cs.values()} >= {1, 32}
    assert {c["B"] * c["N"] for n, c in cs.items() if n.startswith("rows_")} == {31, 32, 33, 65}
    # adjacent repeats are in the hypotheses the float64 search returns, and an infeasible extension is met on the way
    assert run("repeats_tight")[0]["tokens"][0] == [5, 5, 9, 9, 9] and run("repeats_tight")[1]["tokens"][0] == [7, 7, 7]
    assert any(r["trace_parent"][:r["steps"]].min() == -1 for n in ("repeats_tight", "lens_0_1_2_tp", "vocab_2") for r in run(n))
    # the extreme table: the hypothesis [5] is extended by 9 from terms that all lie e^-87 below phi's peak
    ext = run("extreme")[0]
    assert ext["tokens"][0][:1] == [5] and 9 in ext["tokens"][0]
    assert ext["psi_seen"][(5, 9)] < -86.0
