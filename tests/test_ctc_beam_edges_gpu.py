"""The scorer-less CTC prefix beam search (csrc/ctc_beam.hip) against the float64 definition tests/ctc_beam_oracle64.py on
the case tables of tests/ctc_beam_cases.py (admitted on the CPU by tests/test_ctc_beam_oracle_cpu.py), through
beam_search_ids, BeamSearchDecoder and BeamSearchSessions.

EXHAUSTIVE              the enumeration's finite rows in its order, scores within the tolerance; behind them the rows at
                        minus infinity (see MINUS INFINITY below)
EXACT, EDGES (R None),  the whole n-best equals the oracle's: tokens, lengths, order; scores within
TIES                    unit x max(|score64|, 1); rows beyond the hypotheses that exist have lens -1, score 0, tokens -1
EDGES with R            the first R rows equal the oracle's (ctc_beam_cases: stable head), and the best row equals the C
                        oracle's best row
EXTREME                 no NaN, every score finite or the sentinel, tokens equal the oracle's over the checked rows, the
                        300-frame case within the scaled tolerance
Every case runs with PPASR_BEAM_FAST 1 and 0: both pass the oracle check and are byte-identical to each other.

MINUS INFINITY.  In an under-full beam upstream's trie also holds prefixes of probability zero (infeasible ones,
L + repeats > T, and children of such).  The library returns them as the C oracle does: behind every finite row, with their
tokens and lengths and the score FLT_MAX (= -(-FLT_MAX), the NUM_FLT_INF of decoder_utils.h).  Which of several such
prefixes comes first is decided by the last character only, so the test holds each of them to the SET the oracle has at
minus infinity.  In a FULL beam a cut can fall between two such prefixes of one last character (cand_1, cutoff_one_char:
one candidate per frame, beam 4); which of them stays is then container order upstream and defined nowhere, and the test
holds those rows to the oracle's last character, the sentinel and a written length.

Worst observed error on the MI355X in units of the case's tolerance (first run; NOTES.md section 40.3): EXHAUSTIVE 0.010,
EXACT 0.015, EDGES 0.024 (exact class) and 0.008 (stable head), TIES 0.002, EXTREME 0.174 on the 300-frame table and
<= 0.002 elsewhere.  Every unit is F32_BUDGET = 2e-5; nothing was widened."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ctc_beam_cases as cc
import numerics as nm
import poison

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMO = nm.Memo()
SENTINEL = float(np.finfo(np.float32).max)


class _beam_fast:
    """PPASR_BEAM_FAST is read at every call: 1 (default) = the clipped element list first, 0 = always full rows"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("PPASR_BEAM_FAST")
        os.environ["PPASR_BEAM_FAST"] = "1" if self.on else "0"

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("PPASR_BEAM_FAST", None)
        else:
            os.environ["PPASR_BEAM_FAST"] = self.old


def c_oracle_best(p, case):
    """the best row's tokens of the C oracle (oracle/ctc_beam_search_oracle.c) on one utterance"""
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libctc_beam_oracle.so"))
    lib.ctc_beam_oracle_decode.restype = ctypes.c_int
    T, V = p.shape
    L = max(T, 1)
    tokens, lens, scores = np.empty((1, L), np.int32), np.empty(1, np.int32), np.empty(1, np.float64)
    p = np.ascontiguousarray(p, np.float32)
    n = lib.ctc_beam_oracle_decode(p.ctypes.data_as(ctypes.c_void_p), T, V, case["beam"], ctypes.c_double(case["cp"]),
                                   case["top_n"], case["blank"], 1, L, tokens.ctypes.data_as(ctypes.c_void_p),
                                   lens.ctypes.data_as(ctypes.c_void_p), scores.ctypes.data_as(ctypes.c_void_p))
    assert n == 1
    return tokens[0, :lens[0]].tolist()


def _bsd():
    from ppasr_amd.decoders import beam_search_decoder as bsd
    return bsd


def device(case, p, fast=True, nbest=None):
    """one call of beam_search_ids over the whole table -> (tokens, lens, scores) as numpy arrays"""
    bsd = _bsd()
    fl = None if case["lens"] is None else np.asarray(case["lens"], np.int32)
    with _beam_fast(fast):
        tokens, lens, scores, _ = bsd.beam_search_ids(torch.from_numpy(p).cuda(), case["beam"], case["cp"], case["top_n"],
                                                      case["blank"], frame_lens=fl, nbest=nbest or case["nbest"])
        torch.cuda.synchronize()
    return tokens.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()


def both(name, case, p):
    """the case with the fast path and without it: byte-identical -> the result"""
    a, b = device(case, p, True), device(case, p, False)
    for x, y, what in zip(a, b, ("tokens", "lens", "scores")):
        assert x.tobytes() == y.tobytes(), (name, what, "PPASR_BEAM_FAST 1 and 0 differ")
    return a


def oracle(name, case, p, b):
    return MEMO.get((name, b), lambda: cc.run(case, b, p))


def check(name, case, p, got):
    """the rules of the module docstring -> worst score error in units of the tolerance"""
    tokens, lens, scores = got
    u = cc.unit(name)
    worst = 0.0
    assert not np.isnan(scores).any(), name
    for b in range(case["B"]):
        rows, rep = oracle(name, case, p, b)
        n = len(rows) if case["R"] is None else case["R"]
        inf_set = {r[0] for r in rows if not r[2]}
        for i in range(n):
            tk, s64, finite = rows[i]
            ln = int(lens[b, i])
            if finite:
                assert ln == len(tk) and tuple(tokens[b, i, :ln].tolist()) == tk, (name, b, i, tk, tokens[b, i, :max(ln, 0)])
                assert (tokens[b, i, ln:] == -1).all()
                err = abs(float(scores[b, i]) - s64) / cc.score_tol(s64, u)
                worst = max(worst, err)
                assert err <= 1.0, (name, b, i, float(scores[b, i]), s64, err)
            else:  # a prefix at minus infinity: behind every finite row, the sentinel as score
                got_tk = tuple(tokens[b, i, :max(ln, 0)].tolist())
                assert ln >= 0 and float(scores[b, i]) == SENTINEL, (name, b, i, ln, scores[b, i])
                if rep.inf_cut:  # a cut fell between prefixes at minus infinity: the last character is all that is defined
                    assert got_tk[-1:] == tk[-1:], (name, b, i, got_tk, tk)
                else:
                    assert got_tk in inf_set, (name, b, i, got_tk)
        if case["R"] is None:
            assert len({tuple(tokens[b, i, :int(lens[b, i])].tolist()) for i in range(n)}) == n  # no prefix twice
            for i in range(n, case["nbest"]):  # hypotheses that do not exist
                assert lens[b, i] == -1 and scores[b, i] == 0.0 and (tokens[b, i] == -1).all(), (name, b, i)
        else:
            ok = np.isfinite(scores[b]) & ((scores[b] < 0.5 * SENTINEL) | (scores[b] == SENTINEL))
            assert ok.all(), (name, b)
    print(f"{name}: worst score error {worst:.3f} x tolerance (unit {u:.1e})")
    return worst


@pytest.mark.parametrize("name", list(cc.EXHAUSTIVE))
def test_exhaustive(name):
    """the answer is path enumeration over all V^T labelings"""
    import ctc_beam_oracle64 as o64
    case = cc.EXHAUSTIVE[name]
    p = cc.table(case)
    tokens, lens, scores = got = both(name, case, p)
    check(name, case, p, got)
    want = o64.ranked(o64.enumerate_paths(p[0], case["blank"]))
    u = cc.unit(name)
    for i, (tk, nll) in enumerate(want):
        assert tuple(tokens[0, i, :lens[0, i]].tolist()) == tk, (name, i)
        assert abs(scores[0, i] - nll) <= cc.score_tol(nll, u)
    # behind them: every infeasible prefix, each once, at the sentinel; then rows that do not exist
    n_all = cc.prefix_count(case["V"], case["T"])
    assert (scores[0, len(want):n_all] == SENTINEL).all() and (lens[0, n_all:] == -1).all()
    assert all(o64.frames_needed(tokens[0, i, :lens[0, i]].tolist()) > case["T"] for i in range(len(want), n_all))


@pytest.mark.parametrize("name", list(cc.EXACT) + [n for n, c in cc.EDGES.items() if c["R"] is None] + list(cc.TIES))
def test_whole_nbest_equals_the_oracle(name):
    case = cc.ALL[name]
    p = cc.table(case)
    if "state_frames" in case:  # a state sized for fewer frames than the second call alone: it grows, the search is the same
        got = _chunked(case, p, case["chunks"], state_frames=case["state_frames"], growable=True)
        assert got[3].max_frames >= case["T"] and max(case["chunks"]) > case["state_frames"]
        check(name, case, p, got[:3])
        one = both(name, case, p)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(one, got[:3]))
        return
    check(name, case, p, both(name, case, p))


@pytest.mark.parametrize("name", [n for n, c in cc.EDGES.items() if c["R"] is not None])
def test_stable_head_equals_the_oracle(name):
    case = cc.EDGES[name]
    p = cc.table(case)
    tokens, lens, scores = got = both(name, case, p)
    check(name, case, p, got)
    assert tokens[0, 0, :lens[0, 0]].tolist() == c_oracle_best(p[0], case)


@pytest.mark.parametrize("name", list(cc.EXTREME))
def test_extreme_tables(name):
    case = cc.EXTREME[name]
    p = cc.table(case)
    tokens, lens, scores = got = both(name, case, p)
    check(name, case, p, got)
    assert np.isfinite(scores).all() and (lens >= 0).all()
    assert ((scores < 0.5 * SENTINEL) | (scores == SENTINEL)).all()
    if name == "all_blank":
        assert lens[0, 0] == 0 and abs(scores[0, 0]) <= 1e-6  # the empty transcript wins, at probability one
    if name == "tiny_300_frames":
        assert scores[0, 0] > 1e4


# ---- chunked, decoder objects, session pools ---------------------------------------------------------------------------
def _chunked(case, p, chunk, state_frames=None, growable=False):
    """chunk: frames per call, or the frame counts of the calls"""
    bsd = _bsd()
    B, T, _ = p.shape
    dev = torch.from_numpy(p).cuda()
    st = bsd._BeamState(B, state_frames or T, case["beam"], dev.device)
    st.growable = growable
    sizes = [chunk] * ((T + chunk - 1) // chunk) if isinstance(chunk, int) else list(chunk)
    assert sum(sizes) >= T
    lo = 0
    for n in sizes:
        tokens, lens, scores, st = bsd.beam_search_ids(dev[:, lo:lo + n].contiguous(), case["beam"], case["cp"],
                                                       case["top_n"], case["blank"], nbest=case["nbest"], state=st)
        lo += n
    torch.cuda.synchronize()
    return tokens.cpu().numpy()[:, :, :max(T, 1)], lens.cpu().numpy(), scores.cpu().numpy(), st


@pytest.mark.parametrize("name", cc.FORMS)
def test_every_form_returns_the_one_shot_bytes(name):
    """one-shot; chunks of 1, 7 and 16 frames through a _BeamState; BeamSearchDecoder(blank_id=...); a BeamSearchSessions
    pool of three sessions fed staggered"""
    bsd = _bsd()
    case = cc.ALL[name]
    p = cc.table(case)
    T, V = case["T"], case["V"]
    one = both(name, case, p)
    check(name, case, p, one)
    for chunk in (1, 7, 16):
        got = _chunked(case, p, chunk)
        for x, y, what in zip(one, got, ("tokens", "lens", "scores")):
            assert x.tobytes() == y.tobytes(), (name, chunk, what)
    best = (float(one[2][0, 0]), one[0][0, 0, :one[1][0, 0]].tolist())
    vocab = [str(i) for i in range(V)]
    dec = bsd.BeamSearchDecoder(2.2, 4.3, case["beam"], case["cp"], case["top_n"], vocab, blank_id=case["blank"],
                                max_stream_frames=8)
    for lo in range(0, T, 7):
        c = p[:, lo:lo + 7]
        score, _, ids = dec.decode_chunk(c, np.array([c.shape[1]]), return_ids=True)
    assert (score, ids) == best, (name, "BeamSearchDecoder")
    off = dec.decode_beam_search_offline(p[0], return_ids=True)
    assert (off[0], off[2]) == best
    pool = bsd.BeamSearchSessions(3, 2.2, 4.3, case["beam"], case["cp"], case["top_n"], vocab, blank_id=case["blank"],
                                  init_frames=8)
    chunks = [(lo, min(lo + 7, T)) for lo in range(0, T, 7)]
    last = {}
    for r in range(len(chunks) + 2):  # session k starts k rounds late
        ids = [k for k in range(3) if 0 <= r - k < len(chunks)]
        block = np.zeros((len(ids), 7, V), np.float32)
        ln = []
        for j, k in enumerate(ids):
            lo, hi = chunks[r - k]
            block[j, :hi - lo] = p[0, lo:hi]
            block[j, hi - lo:] = np.nan
            ln.append(hi - lo)
        for k, res in zip(ids, pool.decode_chunks(ids, block, lens=ln, return_ids=True)):
            last[k] = (res[0], res[2])
    assert not pool.status().any()
    assert all(last[k] == best for k in range(3)), (name, last, best)


# ---- buffer contents ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("name", cc.POISON)
def test_results_do_not_depend_on_buffer_contents(name, pattern, monkeypatch):
    bsd = _bsd()
    case = cc.ALL[name]
    p = torch.from_numpy(cc.table(case)).cuda()
    B, T, V = p.shape

    def run(s):
        if s.pattern == "zero":
            bsd._scratch.clear()
        st = bsd._BeamState(B, T, case["beam"], p.device)
        args = (case["beam"], case["cp"], case["top_n"], case["blank"])
        if s.stale:
            bsd.beam_search_ids(p.flip(1).contiguous(), *args, nbest=case["nbest"], state=st)
            st.fresh, st.frames = True, 0
            s.scratch([st.buf, bsd])
        else:
            s.scratch(bsd)
        tokens, lens, scores, st = bsd.beam_search_ids(p, *args, nbest=case["nbest"], state=st)
        torch.cuda.synchronize()
        return {"tokens": tokens, "lens": lens, "scores": scores}, [st.buf, bsd]

    poison.check(f"beam edges {name}", run, pattern, monkeypatch, MEMO)
    hl = _lib().load()
    scratch = int(hl.ppasr_ctc_beam_scratch_bytes(B, T, V, case["beam"], case["cp"], case["top_n"]))
    if name == "vocab_4233_unpruned_n10":  # wide records AND the element list in HBM scratch
        assert scratch >= B * T * (2 + 2 * V) * 4 + 4 * case["beam"] * (1 + V)
    elif name == "cand_129":  # wide records, the list in LDS
        assert 0 < scratch < B * T * (2 + 2 * 129) * 4 + 4096
    else:
        assert scratch == 0


def _lib():
    from ppasr_amd import _lib
    return _lib


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_at_the_edges_of_the_accepted_range():
    """each returns the status capi_decode.hip names and leaves poisoned outputs untouched"""
    lib = _lib()
    hl = lib.load()
    T, nb = 2, 4
    p = torch.full((1, T, 16384), 1.0 / 16384, dtype=torch.float32, device="cuda")
    st = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")

    def refused(status, V=67, beam=4, blank=0, nbest=nb, top_n=40):
        tk = torch.full((1, nb, T), 7, dtype=torch.int32, device="cuda")
        ln = torch.full((1, nb), 7, dtype=torch.int32, device="cuda")
        sc = torch.full((1, nb), 7.0, dtype=torch.float64, device="cuda")
        rc = hl.ppasr_ctc_beam_search(p.data_ptr(), None, 1, T, V, beam, ctypes.c_double(0.99), top_n, blank, nbest, T,
                                      tk.data_ptr(), ln.data_ptr(), sc.data_ptr(), st.data_ptr(), st.numel(), 1, None)
        torch.cuda.synchronize()
        assert rc == status, (rc, status, V, beam, blank, nbest, top_n)
        assert bool((tk == 7).all()) and bool((ln == 7).all()) and bool((sc == 7.0).all())

    refused(lib.PPASR_EUNSUPPORTED, V=1)
    refused(lib.PPASR_EUNSUPPORTED, V=16384)
    refused(lib.PPASR_EUNSUPPORTED, beam=0, nbest=1)
    refused(lib.PPASR_EUNSUPPORTED, beam=513)
    refused(lib.PPASR_EINVAL, blank=-1)
    refused(lib.PPASR_EINVAL, blank=67)
    refused(lib.PPASR_EINVAL, nbest=5)  # nbest > beam
    refused(lib.PPASR_EINVAL, nbest=0)
    refused(lib.PPASR_EINVAL, top_n=0)
    # the limits themselves are served (EDGES: vocab_2, vocab_16383, beam_1, beam_512, blank_0, blank_66, nbest = beam)
    with pytest.raises(lib.PPASRHipError) as e:
        _bsd().beam_search_ids(p[:, :, :67].contiguous(), 4, 0.99, 40, 67)
    assert e.value.status == lib.PPASR_EINVAL


# ---- coverage ----------------------------------------------------------------------------------------------------------
def test_edge_table_covers_the_grid():
    E = cc.EDGES
    base = [c for n, c in E.items() if n.startswith("beam_")]
    assert {c["beam"] for c in base} == set(cc.BEAMS) == {1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 511, 512}
    cand = [c for n, c in E.items() if n.startswith("cand_")]
    assert {c["top_n"] for c in cand} == set(cc.CANDS) == {1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129}
    assert all(c["cp"] == cc.JUST_UNDER_1 < 1.0 and c["V"] > c["top_n"] for c in cand)
    for name, c in cc.ALL.items():  # the candidate counts are what the case names say, in every frame
        if name.startswith(("cand_", "list_", "elems_")):
            rep = oracle(name, c, cc.table(c), 0)[1]
            assert set(rep.n_cand) == {c["top_n"]}, (name, set(rep.n_cand))
    assert {c["beam"] * (1 + c["top_n"]) for n, c in E.items() if n.startswith("list_")} == {126, 128, 129, 130}
    elems = {c["beam"] * (1 + c["top_n"]): c["beam"] for n, c in E.items() if n.startswith("elems_")}
    assert set(elems) == {903, 1024, 1032, 1280} and min(elems.values()) > 128
    assert {c["V"] for n, c in E.items() if n.startswith("vocab_")} == set(cc.VOCABS) == {2, 3, 63, 64, 65, 4233, 16383}
    assert {c["blank"] for n, c in E.items() if n.startswith("blank_") and c["V"] == 67} == {0, 1, 67 // 2, 65, 66}
    assert E["blank_4232_v4233"]["blank"] == 4233 - 1 and E["blank_4232_v4233"]["top_n"] == 40
    assert E["top_n_above_v"]["top_n"] > E["top_n_above_v"]["V"] and E["top_n_above_v"]["cp"] < 1.0
    assert set(oracle("cutoff_one_char", E["cutoff_one_char"], cc.table(E["cutoff_one_char"]), 0)[1].n_cand) == {1}
    q = E["cutoff_met_exactly"]
    assert q["cp"] == 0.75 and sorted(cc.table(q)[0, 0].tolist())[-3:] == [0.25, 0.25, 0.5]
    assert set(oracle("cutoff_met_exactly", q, cc.table(q), 0)[1].n_cand) == {2}
    lens = E["lens_0_1_2_t"]
    assert lens["lens"] == [0, 1, 2, lens["T"]]
    assert np.isnan(cc.table(lens)[0]).all() and np.isnan(cc.table(lens)[2, 2:]).all()
    assert E["no_frames"]["T"] == 0
    assert E["nbest_1"]["nbest"] == 1 < E["nbest_1"]["beam"]
    assert all(c["nbest"] == c["beam"] for n, c in E.items() if n != "nbest_1")
    grows = E["state_grows"]
    assert grows["state_frames"] < max(grows["chunks"]) and sum(grows["chunks"]) == grows["T"]
    # the stable head begins at beam 128: every smaller beam is held to the whole n-best
    assert all(c["R"] is None for n, c in E.items() if n.startswith("beam_") and c["beam"] < 128)
    assert all(c["T"] <= 8 and c["B"] == 1 for c in E.values() if c["V"] == 16383 or c["beam"] >= 511)


def _forms(kernels):
    names = [k.split("(")[0].replace("void ", "").replace("ppasr::", "").strip() for k in kernels]
    threads = {int(m.group(1)) for k in names for m in [re.match(r"k_ctc_beam<\s*(\d+)", k)] if m}
    return names, threads


def test_the_cases_launch_every_form_of_the_kernel():
    """k_ctc_beam at 512, 768 and 1024 threads, both prune kernels, and the element list in HBM scratch"""
    lib = _lib()
    seen, threads = set(), set()
    expect = {"blank_66": 512, "elems_1024": 512, "elems_1032": 768, "beam_512": 768, "cand_129": 1024,
              "vocab_4233_unpruned_n10": 1024}
    for name, bt in expect.items():
        case = cc.ALL[name]
        p = cc.table(case)
        with lib.kernel_profile() as kp:
            device(case, p)
        names, th = _forms(kp.kernels)
        print(name, sorted(names))
        assert th == {bt}, (name, th, names)
        wide = any(k.startswith("k_ctc_prune_wide") for k in names)
        assert wide == (bt == 1024) and any(k.startswith("k_ctc_prune<") for k in names) == (not wide), (name, names)
        seen |= set(names)
        threads |= th
    assert threads == {512, 768, 1024}
    c = cc.ALL["vocab_4233_unpruned_n10"]
    need = int(lib.load().ppasr_ctc_beam_scratch_bytes(1, c["T"], c["V"], c["beam"], c["cp"], c["top_n"]))
    assert need >= c["T"] * (2 + 2 * c["V"]) * 4 + 4 * c["beam"] * (1 + c["V"])  # records + the list of one frame
