"""numpy oracle of CTC forced alignment (a plain module, imported by the test files, like tests/numerics.py).

The definition is the one in the header comment of ppasr_amd/csrc/ctc_align.hip, restated here without looking at how
the kernel walks it: states 0 .. 2L (even = blank, odd 2l+1 = token l), emission log(max(p, FLT_MIN)), transitions stay /
step / skip (skip only into a token state whose label differs from the token two states back), start in state 0 or 1,
end in 2L or 2L-1.  Ties: the first of stay, step, skip that attains the maximum; at the end 2L unless 2L-1 is strictly
better.  ``dtype`` selects the precision of the walk (float64: the optimum the tests hold the kernel to; float32: the
kernel's own arithmetic, one add per frame).

``path_score64`` is independent of the walk: it checks that a returned per-frame path is a CTC alignment of the tokens
and prices it in float64.  ``brute_force`` enumerates every labeling (tiny cases only).
"""
import itertools

import numpy as np

FLT_MIN = np.float32(np.finfo(np.float32).tiny)
OK, INFEASIBLE, BAD_INPUT = 0, 1, 2


def emissions(probs, dtype=np.float64):
    """log(max(p, FLT_MIN)) of an fp32 table, in ``dtype``.  A denormal clamps to FLT_MIN whatever the flush mode."""
    p = np.asarray(probs, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(p >= FLT_MIN, p, FLT_MIN)  # (NaN rows past frame_lens are never read; they map to FLT_MIN here)
    return np.log(c.astype(dtype))


def frames_needed(tokens):
    tokens = [int(x) for x in tokens]
    return len(tokens) + sum(1 for i in range(1, len(tokens)) if tokens[i] == tokens[i - 1])


def align(probs, tokens, T=None, blank=0, dtype=np.float64, max_tokens=None):
    """probs [Tp, V], tokens (list of ids), T valid frames (None: all) -> dict(status, score, frame_token [Tp], begin,
    end, peak [max_tokens] (int32, -1 padded), conf [max_tokens] f32, states [T], abs_log (float64 sum of |log p| along the
    path: what the tests' tolerance is made of))."""
    probs = np.asarray(probs, np.float32)
    Tp, V = probs.shape
    T = Tp if T is None else min(max(int(T), 0), Tp)
    tokens = [int(x) for x in tokens]
    L = len(tokens)
    mt = L if max_tokens is None else max_tokens
    out = dict(status=OK, score=dtype(-np.inf), frame_token=np.full(Tp, -1, np.int32), begin=np.full(mt, -1, np.int32),
               end=np.full(mt, -1, np.int32), peak=np.full(mt, -1, np.int32), conf=np.zeros(mt, np.float32),
               states=np.zeros(0, np.int64), abs_log=0.0)
    if L > mt or any(t < 0 or t >= V or t == blank for t in tokens):
        out["status"] = BAD_INPUT
        return out
    if T < frames_needed(tokens):
        out["status"] = INFEASIBLE
        return out
    if T == 0:
        out["score"] = dtype(0.0)
        return out
    S = 2 * L + 1
    labels = np.full(S, blank, np.int64)
    labels[1::2] = tokens
    skip_ok = np.zeros(S, bool)
    for s in range(3, S, 2):
        skip_ok[s] = labels[s] != labels[s - 2]
    e = emissions(probs[:T], dtype)[:, labels]  # [T, S]
    ninf = dtype(-np.inf)
    a = np.full(S, ninf, dtype)
    a[0] = e[0, 0]
    if L > 0:
        a[1] = e[0, 1]
    bp = np.zeros((T, S), np.int8)
    for t in range(1, T):
        best = a.copy()
        choice = np.zeros(S, np.int8)
        step = np.concatenate([[ninf], a[:-1]]).astype(dtype)
        m = step > best
        best[m], choice[m] = step[m], 1
        skip = np.concatenate([[ninf, ninf], a[:-2]]).astype(dtype)[:S]
        m = skip_ok & (skip > best)
        best[m], choice[m] = skip[m], 2
        bp[t] = choice
        a = (best + e[t]).astype(dtype)
    s = S - 1
    if L > 0 and a[S - 2] > a[S - 1]:
        s = S - 2
    out["score"] = a[s]
    states = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    assert states[0] in (0, 1)
    out["states"] = states
    ft = np.where(states % 2 == 1, states // 2, -1).astype(np.int32)
    out["frame_token"][:T] = ft
    e64 = emissions(probs[:T], np.float64)
    out["abs_log"] = float(np.abs(e64[np.arange(T), labels[states]]).sum())
    for l in range(L):
        at = np.nonzero(ft == l)[0]
        out["begin"][l], out["end"][l] = at[0], at[-1] + 1
        col = probs[at[0]:at[-1] + 1, tokens[l]]
        out["peak"][l] = at[0] + int(np.argmax(col))  # (argmax: the first that attains it)
        out["conf"][l] = col.max()
    return out


def path_score64(probs, frame_token, tokens, T=None, blank=0):
    """Checks that ``frame_token`` [Tp] is a CTC alignment of ``tokens`` over the first T frames -- monotone (token indices
    never fall and rise by one at a time, from 0 to L-1), collapsing to the tokens (two adjacent equal tokens are separated
    by a blank frame), blank (-1) at and past T -- and returns its log-probability in float64.  AssertionError otherwise."""
    probs = np.asarray(probs, np.float32)
    ft = np.asarray(frame_token, np.int64)
    Tp, V = probs.shape
    T = Tp if T is None else int(T)
    tokens = [int(x) for x in tokens]
    L = len(tokens)
    assert ft.shape == (Tp,), ft.shape
    assert (ft[T:] == -1).all(), "a token past frame_lens"
    assert ((ft[:T] >= -1) & (ft[:T] < L)).all(), "token index out of range"
    last, prev = -1, -1  # last token index seen; previous frame's entry
    for t in range(T):
        f = int(ft[t])
        if f >= 0:
            assert f == last or f == last + 1, f"frame {t}: token {f} after token {last}"
            if f == last + 1 and f > 0 and tokens[f] == tokens[f - 1]:
                assert prev == -1, f"frame {t}: repeated token {f} without a blank before it"
            last = f
        prev = f
    assert last == L - 1, f"path ends at token {last} of {L}"
    e = emissions(probs[:T], np.float64)
    labels = np.where(ft[:T] >= 0, np.asarray(tokens + [blank], np.int64)[ft[:T]], blank)
    return float(e[np.arange(T), labels].sum()) if T else 0.0


def collapse(labeling, blank=0):
    out, prev = [], None
    for x in labeling:
        if x != prev and x != blank:
            out.append(int(x))
        prev = x
    return out


def brute_force(probs, tokens, blank=0):
    """max over all V^T labelings that collapse to ``tokens`` of their float64 log-probability; None if there is none."""
    probs = np.asarray(probs, np.float32)
    T, V = probs.shape
    e = emissions(probs, np.float64)
    tokens = [int(x) for x in tokens]
    best = None
    for lab in itertools.product(range(V), repeat=T):
        if collapse(lab, blank) == tokens:
            s = float(sum(e[t, lab[t]] for t in range(T)))
            if best is None or s > best:
                best = s
    return best


def left_packed(tokens, T):
    """The canonical path on a table of exact ties: every token at its earliest frame, blanks only where a repeat needs
    one, then trailing blanks.  -> frame_token [T]."""
    ft = []
    for i, tok in enumerate(tokens):
        if i and tok == tokens[i - 1]:
            ft.append(-1)
        ft.append(i)
    assert len(ft) <= T
    return np.asarray(ft + [-1] * (T - len(ft)), np.int32)


def tolerance(T, abs_log):
    """2 (T + 2) 2^-24 sum |log p|: one rounding per add and per logf along the path, doubled."""
    return 2.0 * (T + 2) * 2.0 ** -24 * abs_log
