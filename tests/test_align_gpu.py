"""CTC forced alignment on the device (ppasr_ctc_align, csrc/ctc_align.hip) against the numpy oracle of
tests/align_oracle.py.

Boundaries of the kernel, each covered one below, at and one above:
  * tokens: a lane owns 4 (blank, token) pairs, so the final blank moves to the next lane at every multiple of 4
    (3, 4, 5 and 7, 8, 9 here; 251, 252, 253 at the far end), the gather and the per-token epilogue stride over 64 tokens
    (63, 64, 65; 127, 128, 129), and 255 tokens fill the wave (254, 255);
  * frames: emission rows are loaded 4 frames ahead (T = 1 .. 6), the back-pointer walk stages 64 frames at a time starting
    at frame 1 (T = 64, 65, 66 and 128, 129, 130), and the per-frame epilogue strides over 64 frames (63, 64, 65).

Tolerance (derived, not measured): the kernel makes one fp32 add per frame and one logf per emission, each rounding to
2^-24 relative; over T frames that is at most (T + 2) 2^-24 of the sum of |log p| along the path, doubled:
tol = 2 (T + 2) 2^-24 sum_t |log p_t| along the float64 optimum.
"""
import numpy as np
import pytest
import torch

import align_oracle as ao
import numerics as nm
import poison
from ppasr_amd import _lib
from ppasr_amd.decoders import ctc_alignment as ca

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
V = 50
OUT_NAMES = ("frame_token", "begin", "end", "peak", "conf", "score", "status")
T_LIST = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 66, 128, 129, 130, 257]
L_LIST = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 251, 252, 253, 254, 255]


# ---- inputs ------------------------------------------------------------------------------------------------------------
def softmax_table(rng, T, V, scale=3.0, blank_boost=4.0):
    """random softmax rows; the blank logit is raised on about half the frames"""
    z = rng.normal(size=(T, V)) * scale
    z[:, 0] += blank_boost * (rng.random(T) < 0.5)
    p = np.exp(z - z.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def random_tokens(rng, L, T, V, repeats=True):
    """L non-blank ids that fit into T frames, with adjacent repeats where there is room for their blanks"""
    tok = rng.integers(1, V, size=L).tolist()
    if repeats:
        for i in range(1, L):
            if rng.random() < 0.2:
                tok[i] = tok[i - 1]
    i = 1
    while ao.frames_needed(tok) > T:  # undo repeats from the left until it fits
        while tok[i] != tok[i - 1]:
            i += 1
        tok[i] = tok[i] % (V - 1) + 1
        if i + 1 < L and tok[i + 1] == tok[i]:
            tok[i + 1] = tok[i + 1] % (V - 1) + 1
    return tok


def pack_tokens(token_lists, max_tokens=None, pad=-1):
    mt = max([len(t) for t in token_lists] + [0]) if max_tokens is None else max_tokens
    tk = np.full((len(token_lists), mt), pad, np.int32)
    for b, t in enumerate(token_lists):
        tk[b, :min(len(t), mt)] = t[:mt]
    return tk, np.asarray([len(t) for t in token_lists], np.int32)


def run(probs, token_lists, frame_lens=None, blank=0, max_tokens=None, n_tokens=None):
    tk, nt = pack_tokens(token_lists, max_tokens)
    out = ca.ctc_align_ids(torch.as_tensor(probs), tk, nt if n_tokens is None else np.asarray(n_tokens, np.int32),
                           None if frame_lens is None else np.asarray(frame_lens, np.int32), blank)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def derived(probs, ft, tokens, mt):
    """begin / end / peak / conf as the definition reads them off a path and the table"""
    begin, end, peak = (np.full(mt, -1, np.int32) for _ in range(3))
    conf = np.zeros(mt, np.float32)
    for l, tok in enumerate(tokens):
        at = np.nonzero(ft == l)[0]
        begin[l], end[l] = at[0], at[-1] + 1
        col = probs[at[0]:at[-1] + 1, tok]
        peak[l], conf[l] = at[0] + int(np.argmax(col)), col.max()
    return begin, end, peak, conf


def check_utterance(got, b, probs, tokens, T, exact_path=None, label=""):
    """validity, optimality within the derived tolerance, and the per-token outputs against the returned path"""
    ref = MEMO.get(("ref", label, b), lambda: ao.align(probs, tokens, T))
    assert ref["status"] == ao.OK
    assert got["status"][b] == 0, (label, b, got["status"][b])
    ft = got["frame_token"][b]
    mine = ao.path_score64(probs, ft, tokens, T)  # (raises if the path is not an alignment of the tokens)
    tol = ao.tolerance(T, ref["abs_log"])
    opt = float(ref["score"])
    print(f"[align] {label} b={b} T={T} L={len(tokens)} optimum64={opt:.9g} path64={mine:.9g} score32={got['score'][b]:.9g} "
          f"tol={tol:.3g} same_path={bool((ft == ref['frame_token']).all())}")
    assert mine >= opt - tol, (label, b, mine, opt, tol)
    assert abs(float(got["score"][b]) - opt) <= tol, (label, b, got["score"][b], opt, tol)
    mt = got["begin"].shape[1]
    begin, end, peak, conf = derived(probs, ft, tokens, mt)
    assert (got["begin"][b] == begin).all() and (got["end"][b] == end).all() and (got["peak"][b] == peak).all()
    assert got["conf"][b].tobytes() == conf.tobytes()
    if exact_path is not None:
        assert (ft == exact_path).all(), (label, b, ft, exact_path)


def check_empty(got, b, status):
    assert got["status"][b] == status
    assert got["score"][b] == -np.inf
    assert (got["frame_token"][b] == -1).all()
    for k in ("begin", "end", "peak"):
        assert (got[k][b] == -1).all()
    assert (got["conf"][b] == 0.0).all() and not np.signbit(got["conf"][b]).any()


# ---- optimality and validity -------------------------------------------------------------------------------------------
def optimality_batches(T):
    """B = 5 per batch, every feasible L of L_LIST at this T, ragged frame_lens and n_tokens"""
    def make():
        rng = np.random.default_rng(1000 + T)
        Ls = [L for L in L_LIST if L <= T]
        batches = []
        for i in range(0, len(Ls), 5):
            group = (Ls[i:i + 5] * 5)[:5]
            probs = np.stack([softmax_table(rng, T, V) for _ in group])
            toks, lens = [], []
            for b, L in enumerate(group):
                Tb = T if b == 0 else max(L, T - int(rng.integers(0, 4)))  # ragged, never below L
                toks.append(random_tokens(rng, L, Tb, V, repeats=Tb > L))
                lens.append(Tb)
            for b in range(5):  # rows past frame_lens must never be read: NaN
                probs[b, lens[b]:] = np.nan
            batches.append((probs, toks, lens))
        return batches
    return MEMO.get(("batches", T), make)


@pytest.mark.parametrize("T", T_LIST)
def test_optimal_and_valid(T):
    for i, (probs, toks, lens) in enumerate(optimality_batches(T)):
        got = run(probs, toks, lens)
        for b in range(5):
            check_utterance(got, b, probs[b], toks[b], lens[b], label=f"opt T={T} batch={i}")
            assert (got["begin"][b, len(toks[b]):] == -1).all() and (got["conf"][b, len(toks[b]):] == 0).all()


# ---- greedy equivalence ------------------------------------------------------------------------------------------------
def test_greedy_tokens_align_to_the_argmax_path():
    from ppasr_amd.decoders.ctc_greedy_decoder import greedy_decode_ids
    T, B = 64, 3
    tables = []
    seed = 0
    while len(tables) < B:  # the first seeds whose smallest top-2 log-margin is >= 0.01 (float64)
        p = softmax_table(np.random.default_rng(seed), T, V, scale=3.0, blank_boost=4.0)
        top2 = np.sort(np.log(p.astype(np.float64)), axis=1)[:, -2:]
        margin = float((top2[:, 1] - top2[:, 0]).min())
        print(f"[align] greedy seed={seed} margin={margin:.4f}")
        if margin >= 0.01:
            tables.append(p)
        seed += 1
        assert seed < 200
    probs = torch.from_numpy(np.stack(tables)).cuda()
    tokens, n_tokens, _, frame_argmax, _ = greedy_decode_ids(probs)
    out = ca.ctc_align_ids(probs, tokens, n_tokens)
    torch.cuda.synchronize()
    fa = frame_argmax.cpu().numpy()
    ft = out["frame_token"].cpu().numpy()
    assert (out["status"].cpu().numpy() == 0).all()
    for b in range(B):
        want, idx = np.full(T, -1, np.int32), -1
        for t in range(T):
            if fa[b, t] != 0:
                if t == 0 or fa[b, t] != fa[b, t - 1]:
                    idx += 1
                want[t] = idx
        assert idx + 1 == int(n_tokens[b])
        assert (ft[b] == want).all(), (b, ft[b], want)


# ---- planted alignments ------------------------------------------------------------------------------------------------
def planted_table(rng, labels, V):
    """each frame holds 0.85 .. 0.95 at its planted label, the rest spread over the other symbols"""
    T = len(labels)
    p = np.zeros((T, V), np.float64)
    for t, lab in enumerate(labels):
        hi = 0.85 + 0.1 * rng.random()
        p[t] = (1.0 - hi) / (V - 1)
        p[t, lab] = hi
    return p.astype(np.float32)


PLANTS = [
    # (tokens, per-frame labels; 0 = blank)
    ([7, 7, 7, 3], [7, 0, 7, 7, 0, 7, 3, 3]),                 # repeats behind single blanks; first and last frame tokens
    ([5], [5, 5, 5, 5, 5, 5, 5, 5]),                            # one token over every frame
    ([9, 4, 9], [0, 0, 9, 4, 4, 9, 0, 0]),                      # blanks at both ends, skips between different tokens
    ([2, 2], [2, 0, 2, 0, 0, 0, 0, 0]),
    ([], [0, 0, 0, 0, 0, 0, 0, 0]),
    ([11, 12, 13, 14, 15, 16, 17, 18], [11, 12, 13, 14, 15, 16, 17, 18]),  # a token per frame, no blank at all
]


def test_planted_alignments_are_recovered_exactly():
    rng = np.random.default_rng(5)
    probs = np.stack([planted_table(rng, labels, V) for _, labels in PLANTS])
    toks = [t for t, _ in PLANTS]
    got = run(probs, toks)
    for b, (tokens, labels) in enumerate(PLANTS):
        want, idx = np.full(len(labels), -1, np.int32), -1
        for t, lab in enumerate(labels):
            if lab != 0:
                if t == 0 or labels[t - 1] != lab:
                    idx += 1
                want[t] = idx
        assert (got["frame_token"][b] == want).all(), (b, got["frame_token"][b], want)
        begin, end, peak, conf = derived(probs[b], want, tokens, got["begin"].shape[1])
        assert (got["begin"][b] == begin).all() and (got["end"][b] == end).all() and (got["peak"][b] == peak).all()
        assert got["conf"][b].tobytes() == conf.tobytes()  # bit-identical to the table entry
        check_utterance(got, b, probs[b], tokens, len(labels), exact_path=want, label="planted")


# ---- exact ties --------------------------------------------------------------------------------------------------------
TIE_CASES = [(12, [1, 2, 3]), (12, [1, 1, 2, 2, 2]), (9, [3, 3, 3, 3, 3]), (12, []), (1, [2]), (12, [1, 2, 1, 2, 1, 2, 1, 2, 1]),
             (70, [1, 1] * 17 + [2])]


@pytest.mark.parametrize("V_", [4, 4233])
def test_exact_ties_give_the_canonical_path(V_):
    Tp = max(T for T, _ in TIE_CASES)
    probs = np.full((len(TIE_CASES), Tp, V_), np.float32(1.0) / np.float32(V_), np.float32)
    toks = [[t if V_ == 4 else 1000 * t + 7 for t in tokens] for _, tokens in TIE_CASES]
    lens = [T for T, _ in TIE_CASES]
    got = run(probs, toks, lens)
    for b, (T, _) in enumerate(TIE_CASES):
        ref = ao.align(probs[b], toks[b], T, max_tokens=got["begin"].shape[1])
        want = np.full(Tp, -1, np.int32)
        want[:T] = ao.left_packed(toks[b], T)
        assert (ref["frame_token"] == want).all()
        assert got["status"][b] == 0
        assert (got["frame_token"][b] == want).all(), (b, got["frame_token"][b], want)
        for k in ("begin", "end", "peak"):
            assert (got[k][b] == ref[k]).all(), (k, b)
        assert got["conf"][b].tobytes() == ref["conf"].tobytes()
        assert abs(float(got["score"][b]) - float(ref["score"])) <= ao.tolerance(T, ref["abs_log"])


# ---- range -------------------------------------------------------------------------------------------------------------
SPECIALS = [0.0, 1e-40, float(ao.FLT_MIN), 1.0]


def test_zero_denormal_flt_min_and_one_on_and_off_the_optimum():
    rng = np.random.default_rng(9)
    # (a) on the optimum: T = frames needed, so the path is forced; its entries cycle through the specials and 0.3
    tight = [3, 3, 8, 9, 9, 9, 2, 4, 4, 6, 7, 1]
    ft_tight = ao.left_packed(tight, ao.frames_needed(tight))
    Ta = len(ft_tight)
    pa = softmax_table(rng, Ta, V)
    for t in range(Ta):
        pa[t, 0 if ft_tight[t] < 0 else tight[ft_tight[t]]] = (SPECIALS + [0.3])[t % 5]
    # (b) off the optimum: a planted path with room to move; the other entries of its tokens' columns and of the blank column
    # cycle through 0, a denormal and FLT_MIN, and 1.0 sits on a symbol that is none of the tokens
    tokens_b = [5, 5, 6, 7, 5]
    labels_b = [0, 5, 5, 0, 5, 6, 6, 7, 0, 0, 5, 0, 0, 0, 0, 0]
    assert len(labels_b) == Ta
    pb = planted_table(rng, labels_b, V)
    k = 0
    for t in range(Ta):
        for col in (0, 5, 6, 7):
            if col != labels_b[t]:
                pb[t, col] = SPECIALS[k % 3]
                k += 1
        pb[t, 20] = 1.0
    probs = np.stack([pa, pb])
    got = run(probs, [tight, tokens_b])
    for b, tokens in enumerate([tight, tokens_b]):
        ref = ao.align(probs[b], tokens)
        assert np.isfinite(ref["score"])
        check_utterance(got, b, probs[b], tokens, Ta, exact_path=ref["frame_token"], label="range")
    assert (got["frame_token"][0] == ft_tight).all()


# ---- infeasible and bad input in a mixed batch -------------------------------------------------------------------------
def test_infeasible_and_bad_input_leave_their_neighbours_alone():
    rng = np.random.default_rng(11)
    T = 20
    good = [random_tokens(rng, L, Tg, V) for L, Tg in ((6, T), (0, T), (11, 17), (3, T))]
    probs_good = np.stack([softmax_table(rng, T, V) for _ in good])
    lens_good = [T, 0, 17, T]  # (frame_lens = 0 with no tokens: feasible, writes nothing)
    good[1] = []
    rep = [4, 4, 4, 9]                     # needs 4 + 2 = 6 frames
    extra = softmax_table(rng, T, V)
    # batch: good0, infeasible (T = L + repeats - 1), good1, id == V, good2, id < 0, blank as a token, good3, n_tokens > max_tokens
    order = [("g", 0), ("x", rep, 5, None), ("g", 1), ("x", [3, V, 5], T, None), ("g", 2), ("x", [3, -1], T, None),
             ("x", [3, 0, 5], T, None), ("g", 3), ("x", [1, 2], T, 12)]
    probs, toks, lens, nt = [], [], [], []
    for o in order:
        if o[0] == "g":
            probs.append(probs_good[o[1]]), toks.append(good[o[1]]), lens.append(lens_good[o[1]])
            nt.append(len(good[o[1]]))
        else:
            probs.append(extra), toks.append(o[1]), lens.append(o[2]), nt.append(len(o[1]) if o[3] is None else o[3])
    mt = 11
    mixed = run(np.stack(probs), toks, lens, max_tokens=mt, n_tokens=nt)
    alone = run(probs_good, good, lens_good, max_tokens=mt)
    want_status = [0, 1, 0, 2, 0, 2, 2, 0, 2]
    assert mixed["status"].tolist() == want_status
    for b, st in enumerate(want_status):
        if st:
            check_empty(mixed, b, st)
    for g, b in enumerate([0, 2, 4, 7]):
        for k in OUT_NAMES:
            assert mixed[k][b].tobytes() == alone[k][g].tobytes(), (k, b)
        if lens_good[g]:
            check_utterance(alone, g, probs_good[g], good[g], lens_good[g], label="mixed")
    assert alone["score"][1] == 0.0 and (alone["frame_token"][1] == -1).all()
    # the rule at its edge: one frame more and the same transcript aligns
    assert run(extra[None], [rep], [6])["status"][0] == 0


def test_max_tokens_zero_and_no_frames():
    rng = np.random.default_rng(12)
    probs = np.stack([softmax_table(rng, 9, V) for _ in range(3)])
    got = run(probs, [[], [], []], [9, 4, 0])
    assert got["begin"].shape == (3, 0) and got["status"].tolist() == [0, 0, 0]
    assert (got["frame_token"] == -1).all()
    for b, T in enumerate([9, 4, 0]):
        want = float(ao.emissions(probs[b, :T])[:, 0].sum())
        assert abs(float(got["score"][b]) - want) <= ao.tolerance(T, abs(want)) + 0.0
    # Tp = 0: a valid call that writes status and score only
    got = run(np.zeros((2, 0, V), np.float32), [[], [3]], None)
    assert got["status"].tolist() == [0, 1] and got["score"][0] == 0.0 and got["score"][1] == -np.inf
    assert (got["begin"][1] == -1).all()


def test_unwanted_outputs_may_be_null():
    probs, toks, lens = optimality_batches(7)[0]
    full = run(probs, toks, lens)
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    p = torch.from_numpy(probs).to(dev)
    tk_np, nt_np = pack_tokens(toks)
    tk, nt, fl = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (tk_np, nt_np, np.asarray(lens, np.int32)))
    B, T, _ = probs.shape
    mt = tk.shape[1]
    ft = torch.empty(B, T, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    need = lib.ppasr_ctc_align_workspace_bytes(B, T, mt)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.ppasr_ctc_align(p.data_ptr(), fl.data_ptr(), B, T, V, 0, tk.data_ptr(), nt.data_ptr(), mt, ft.data_ptr(),
                                   None, None, None, None, score.data_ptr(), status.data_ptr(), ws.data_ptr(), need,
                                   torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert ft.cpu().numpy().tobytes() == full["frame_token"].tobytes()
    assert score.cpu().numpy().tobytes() == full["score"].tobytes() and (status.cpu().numpy() == full["status"]).all()
    # the device-side refusals of the wrapper's arguments
    rc = lib.ppasr_ctc_align(p.data_ptr(), None, B, T, V, 0, tk.data_ptr(), nt.data_ptr(), mt, ft.data_ptr(), None, None, None,
                             None, score.data_ptr(), status.data_ptr(), ws.data_ptr(), need - 1, None)
    assert rc == _lib.PPASR_EINVAL


# ---- buffer contents ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_no_result_depends_on_buffer_contents(pattern, monkeypatch):
    batches = optimality_batches(64) + optimality_batches(7)
    other = optimality_batches(130)[-1]

    def go(s):
        if s.pattern == "zero":
            ca.scratch._ws.clear()  # the clean reference starts without kept scratch, like a fresh process
        if s.stale:
            tk, nt = pack_tokens(other[1])
            ca.ctc_align_ids(torch.as_tensor(other[0]), tk, nt, np.asarray(other[2], np.int32))
        outs = {}
        for i, (probs, toks, lens) in enumerate(batches):
            s.scratch(ca.scratch)
            tk, nt = pack_tokens(toks)
            out = ca.ctc_align_ids(torch.as_tensor(probs), tk, nt, np.asarray(lens, np.int32))
            s.observe(ca.scratch, f"batch {i}")
            torch.cuda.synchronize()
            outs.update({f"{i}/{k}": out[k] for k in OUT_NAMES})
        return outs, ca.scratch

    poison.check("ctc_align", go, pattern, monkeypatch, MEMO)


# ---- the shipped vocabulary width --------------------------------------------------------------------------------------
def test_full_vocabulary():
    Vf, B, T, L = 4233, 2, 64, 40
    rng = np.random.default_rng(21)
    probs = np.stack([softmax_table(rng, T, Vf) for _ in range(B)])
    toks = [random_tokens(rng, L, T, Vf) for _ in range(B)]
    toks[1][-1] = Vf - 1  # the last column of the table
    if toks[1][-2] == Vf - 1:
        toks[1][-2] = Vf - 2
    got = run(probs, toks)
    for b in range(B):
        check_utterance(got, b, probs[b], toks[b], T, label="full-vocabulary")
