"""tests/ctc_beam_oracle64.py is right, every named case of tests/ctc_beam_cases.py is admitted as its table says, and the
tables catch every mutation of ctc_beam_oracle64.BUGS -- all on the CPU, so that tests/test_ctc_beam_edges_gpu.py can hold
the kernel to the oracle without skipping anything at run time.

* EXHAUSTIVE: the float64 search equals path enumeration over all V^T labelings to 1e-10, in scores and in order, and
  every finite prefix's score equals loss_oracle.ctc_nll of that prefix (a second float64 yardstick); the rows at minus
  infinity are exactly the infeasible prefixes (L + repeats > T).
* EXACT, EDGES: the float64 search equals the C oracle (oracle/ctc_beam_search_oracle.c, float32): tokens and order over
  the finite rows the case checks, scores within the case's tolerance.  This is what pins the C oracle.
* admission (ctc_beam_cases.admission) of every case, and its float32 floor held to the record in FLOORS.
* every mutation changes the checked rows of the case BUG_CASES names for it, or moves a score by >= 5 tolerances."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import ctc_beam_cases as cc
import ctc_beam_oracle64 as o64
import loss_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = float(np.finfo(np.float32).max)  # the score the C oracle and the library report for a prefix at minus infinity


@pytest.fixture(scope="module")
def c_oracle():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libctc_beam_oracle.so"))
    lib.ctc_beam_oracle_decode.restype = ctypes.c_int
    return lib


def c_decode(lib, p, case, T):
    """-> [(tokens tuple, score, finite)] of the C oracle on one utterance"""
    V, nbest = case["V"], case["nbest"]
    L = max(T, 1)
    tokens = np.empty((nbest, L), np.int32)
    lens = np.empty(nbest, np.int32)
    scores = np.empty(nbest, np.float64)
    p = np.ascontiguousarray(p[:T], np.float32)
    n = lib.ctc_beam_oracle_decode(p.ctypes.data_as(ctypes.c_void_p), T, V, case["beam"], ctypes.c_double(case["cp"]),
                                   case["top_n"], case["blank"], nbest, L, tokens.ctypes.data_as(ctypes.c_void_p),
                                   lens.ctypes.data_as(ctypes.c_void_p), scores.ctypes.data_as(ctypes.c_void_p))
    return [(tuple(tokens[i, :lens[i]].tolist()), float(scores[i]), scores[i] < 0.5 * SENTINEL) for i in range(n)]


@pytest.mark.parametrize("name", list(cc.EXHAUSTIVE))
def test_oracle_equals_enumeration_and_ctc_nll(name):
    case = cc.EXHAUSTIVE[name]
    p = cc.table(case)[0]
    T, V, blank = case["T"], case["V"], case["blank"]
    rows, rep = o64.search(p, case["beam"], case["cp"], case["top_n"], blank)
    assert max(rep.n_exist) == cc.prefix_count(V, T) <= case["beam"] and rep.n_cand == [V] * T
    want = o64.ranked(o64.enumerate_paths(p, blank))
    fin = [r for r in rows if r[2]]
    assert [r[0] for r in fin] == [w[0] for w in want], name  # the same prefixes in the same order
    assert max(abs(r[1] - w[1]) for r, w in zip(fin, want)) <= 1e-10
    for tokens, score, _ in fin:
        nll, status = lo.ctc_nll(p, list(tokens), blank=blank)
        assert status == lo.OK and abs(float(nll) - score) <= 1e-10, (tokens, nll, score)
    # every finite row precedes the rows at minus infinity, and those are the infeasible prefixes, all of them
    assert [r[2] for r in rows] == [True] * len(fin) + [False] * (len(rows) - len(fin))
    inf = {r[0] for r in rows if not r[2]}
    assert all(o64.frames_needed(t) > T for t in inf) and len(inf) + len(fin) == cc.prefix_count(V, T)
    assert not rep.undecided() and rep.ties_final == 0


@pytest.mark.parametrize("name", list(cc.EXACT) + list(cc.EDGES))
def test_oracle_equals_c_oracle(name, c_oracle):
    case = cc.ALL[name]
    p = cc.table(case)
    u = cc.unit(name)
    for b in range(case["B"]):
        T = cc.frames(case, b)
        rows = cc.run(case, b, p)[0]
        ref = c_decode(c_oracle, p[b], case, T)
        n = len(rows) if case["R"] is None else case["R"]
        assert len(ref) == len(rows)
        fin = [r for r in rows[:n] if r[2]]
        assert [r[0] for r in fin] == [r[0] for r in ref[:n] if r[2]], (name, b)
        for (t64, s64, _), (_, s32, _) in zip(fin, ref):
            assert abs(s32 - s64) <= cc.score_tol(s64, u), (name, b, t64, s32, s64)
        if case["R"] is None:  # rows at minus infinity: behind the finite ones on both sides, the sentinel as score
            assert [r[2] for r in ref] == [r[2] for r in rows]
            assert all(r[1] == SENTINEL for r in ref if not r[2])


@pytest.mark.parametrize("name", list(cc.ALL))
def test_case_is_admitted_and_its_floor_is_on_record(name):
    case = cc.ALL[name]
    problems, facts = cc.admission(name, case)
    assert not problems, (name, problems)
    assert case["R"] is None or 1 <= case["R"] <= facts["R"]
    e32, record = facts["e32"], cc.FLOORS[name]
    print(f"{name}: e32 {e32:.3e} (record {record:.2e})  gap / tolerance {facts['ratio']:.1f}  R {facts['R']}")
    assert e32 <= record <= 2.0 * e32 + 1e-9, (name, e32, record)
    assert cc.unit(name) <= cc.nm.TOL_CAP


def _checked(case, rows):
    return rows if case["R"] is None else rows[:case["R"]]


@pytest.mark.parametrize("bug", list(o64.BUGS))
def test_mutation_is_caught(bug):
    name = cc.BUG_CASES[bug]
    case = cc.ALL[name]
    p = cc.table(case)
    u = cc.unit(name)
    caught = []
    for b in range(case["B"]):
        good = _checked(case, cc.run(case, b, p)[0])
        bad = _checked(case, cc.run(case, b, p, bug=bug)[0])
        if [(r[0], r[2]) for r in good] != [(r[0], r[2]) for r in bad] or any(math.isnan(r[1]) for r in bad):
            caught.append((b, "rows"))
            continue
        worst = max([abs(x[1] - y[1]) / cc.score_tol(x[1], u) for x, y in zip(good, bad) if x[2]] + [0.0])
        if worst >= 5.0:
            caught.append((b, f"{worst:.1f} tolerances"))
    print(f"{bug}: {name} {caught}")
    assert caught, (bug, name)


def test_bug_cases_name_a_case_of_the_table_they_aim_at():
    assert set(cc.BUG_CASES) == set(o64.BUGS)
    aims = {"repeat_child_from_total": "EXTREME", "blank_is_zero": "EDGES", "blank_unpruned": "EDGES", "cutoff_gt": "EDGES",
            "top_n_plus_one": "EDGES", "tie_char_desc": "TIES", "root_after_chars": "TIES", "max_for_lse": "EXACT",
            "no_flt_min": "EXTREME", "reads_past_frame_lens": "EXACT"}
    for bug, name in cc.BUG_CASES.items():
        assert name in cc.TABLES[aims[bug]], (bug, name)


def test_floors_and_tables_match():
    assert set(cc.FLOORS) == set(cc.ALL)
    assert all(0.0 <= v < cc.nm.TOL_CAP / cc.nm.FLOOR_FACTOR for v in cc.FLOORS.values())
    assert math.isclose(cc.EXACT_FACTOR, 4.0)
    for name in cc.FORMS + cc.POISON:
        assert name in cc.ALL
