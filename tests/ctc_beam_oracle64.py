"""The CTC prefix beam search of csrc/ctc_beam.hip (scorer-less form) as a definition: a search over a dict of token
tuples in numpy / plain Python.  No trie, no slots, no element lists -- nothing shaped like the kernel or like
oracle/ctc_beam_search_oracle.c, which this module pins (tests/test_ctc_beam_oracle_cpu.py: equal to path enumeration over
all V^T labelings and to loss_oracle.ctc_nll on the EXHAUSTIVE cases, equal to the C oracle on the drawn ones).

``dtype``: float64 is the yardstick the tests hold the kernel to, float32 the floor (the same search in the kernel's
number format, with the C oracle's log(exp(x - m) + exp(y - m)) + m).

EMISSION.   log(p + FLT_MIN), the sum taken in double, the logarithm in double, then rounded to ``dtype``.
PRUNING.    The characters of a frame sorted by probability descending, then id ascending (the key order of
            k_ctc_prune); cumulative sum in double in that order; the list stops after the character with which
            cum >= cutoff_prob or n >= cutoff_top_n.  cutoff_prob >= 1: no pruning at all, every character is a
            candidate whatever cutoff_top_n says (upstream get_pruned_log_probs).
BLANK.      Per frame and per prefix g of the beam with (b, nb) = log mass of the alignments of g that end in blank /
            in its last character, score = lse(b, nb):
              blank c          b'(g)    (+)= lp(c) + score(g)        -- only in frames where blank survives the pruning
              c == last(g)     nb'(g)   (+)= lp(c) + nb(g)           -- a repeat extends the prefix's own non-blank mass
                               nb'(g+c) (+)= lp(c) + b(g)            -- the child on the same character: blank mass alone
              c != last(g)     nb'(g+c) (+)= lp(c) + score(g)
            A prefix of the beam that receives nothing in a frame stays, at minus infinity; a child is created even where
            its mass is minus infinity (c == last(g) with b(g) = -inf), as upstream's get_path_trie does.
SELECTION.  After every frame, when at least ``beam`` prefixes exist, the first ``beam`` in prefix_compare order: score
            descending, then last character ascending, the root's character (-1) below every id.  A tie this rule does
            not decide (equal score AND equal last character) is not resolved silently: it is reported
            (``undecided_cut``, ``undecided_final``); this module then orders by the token tuple, which no
            implementation promises.
RESULT.     -log P, the n-best in prefix_compare order.  Hypotheses at minus infinity are kept, behind every finite one,
            with score +inf and ``finite=False``; they are not dropped.
FRAMES.     Rows at t >= T (``frame_lens[b]``) are never read.

Beside the rows ``search`` returns the facts a case is admitted by (Report): the smallest RELATIVE score gap
(s_hi - s_lo) / max(|s_hi|, |s_lo|, 1) at a beam cut, between kept neighbours and in the final n-best (exact ties are not
gaps: they are counted, and flagged when prefix_compare leaves them undecided), and whether two equal probabilities
straddled a pruning cut.

BUGS: named mutations of the definition (``bug=``), each a realistic mistake of a kernel; the CPU test shows that the case
tables catch every one of them."""
import math
from dataclasses import dataclass, field

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
NINF = -math.inf

BUGS = ("repeat_child_from_total", "blank_is_zero", "blank_unpruned", "cutoff_gt", "top_n_plus_one", "tie_char_desc",
        "root_after_chars", "max_for_lse", "no_flt_min", "reads_past_frame_lens")


@dataclass
class Report:
    gap_cut: float = math.inf      # smallest relative gap between the last kept and the first dropped prefix, all frames
    gap_kept: float = math.inf     # ... between neighbours inside the kept beam, all frames
    gap_final: float = math.inf    # ... between neighbours of the final n-best (and the row behind it)
    ties_cut: int = 0              # exact score ties at a cut that the last character decided
    ties_kept: int = 0             # exact score ties between kept neighbours (decided or not: the SET does not depend on it)
    ties_final: int = 0            # exact score ties in the final n-best that the last character decided
    undecided_cut: bool = False    # equal score and equal last character across a cut
    undecided_final: bool = False  # ... between returned rows
    prune_equal: bool = False      # two equal probabilities straddled a pruning cut
    inf_cut: bool = False          # a cut fell between two prefixes at minus infinity (which of them stays is not defined)
    n_cand: list = field(default_factory=list)   # candidates per frame
    n_exist: list = field(default_factory=list)  # prefixes that existed before each cut

    def smallest_gap(self):
        return min(self.gap_cut, self.gap_kept, self.gap_final)

    def undecided(self):
        return self.undecided_cut or self.undecided_final


def _lse64(x, y):
    if x == NINF:
        return y
    if y == NINF:
        return x
    m, d = (x, y - x) if x > y else (y, x - y)
    return m + math.log1p(math.exp(d))


def _lse32(x, y):
    f = np.float32
    if x == NINF:
        return y
    if y == NINF:
        return x
    m = x if x > y else y
    return f(f(np.log(f(f(np.exp(f(x - m))) + f(np.exp(f(y - m)))))) + m)


def _max(x, y):
    return x if x > y else y


def relgap(hi, lo):
    return (hi - lo) / max(abs(hi), abs(lo), 1.0)


def prune(row, cutoff_prob, cutoff_top_n, dtype=np.float64, bug=None):
    """one frame's candidates -> ([(character, log(p + FLT_MIN) in dtype)], equal pair at the cut?)"""
    row = np.asarray(row, np.float32)
    V = row.shape[0]
    order = np.argsort(-row.astype(np.float64), kind="stable")  # probability descending, id ascending
    n = V
    if cutoff_prob < 1.0:
        top_n = cutoff_top_n + (1 if bug == "top_n_plus_one" else 0)
        cum, n = 0.0, 0
        for c in order:
            cum += float(row[c])
            n += 1
            if (cum > cutoff_prob if bug == "cutoff_gt" else cum >= cutoff_prob) or n >= top_n:
                break
    equal = bool(n < V and row[order[n - 1]] == row[order[n]])
    out = []
    with np.errstate(divide="ignore"):
        for c in order[:n]:
            p = float(row[c])
            lp = (math.log(p) if p > 0.0 else NINF) if bug == "no_flt_min" else math.log(p + FLT_MIN)
            out.append((int(c), lp if dtype == np.float64 else np.float32(lp)))
    return out, equal


def _sort_key(item, V, bug):
    pre, _, _, sc = item
    ch = pre[-1] if pre else (V if bug == "root_after_chars" else -1)
    return (-sc, -ch if bug == "tie_char_desc" else ch, pre)


def _pair(a, b, V, bug):
    """two neighbours in sorted order -> ("gap", relative gap) | ("tie", decided?) | ("inf", None)"""
    sa, sb = float(a[3]), float(b[3])
    if sb == NINF:
        return ("inf", sa == NINF)
    if sa == sb:
        return ("tie", _sort_key(a, V, bug)[1] != _sort_key(b, V, bug)[1])
    return ("gap", relgap(sa, sb))


def search(probs, beam, cutoff_prob=1.0, cutoff_top_n=40, blank=0, T=None, nbest=None, dtype=np.float64, bug=None,
           near=None):
    """probs [Tp, V] f32, T valid frames (None: all) -> (rows, Report); rows = the first ``nbest`` (None: beam) of
    [(tokens tuple, -log P as a Python float (+inf at minus infinity), finite)] in prefix_compare order.

    near = ("keep" | "drop", u): the stable-head probe.  At every cut, "keep" also keeps every prefix whose score lies
    within u x max(|score|, 1) of the last kept one, "drop" also drops every kept prefix within that distance of the first
    dropped one: the two ends of what an implementation with errors of that size may do at that cut.  ("keep" stops at
    2 x beam prefixes: on tables full of exact ties the kept set would otherwise grow with every frame.)"""
    assert bug is None or bug in BUGS, bug
    assert dtype in (np.float64, np.float32)
    probs = np.asarray(probs, np.float32)
    Tp, V = probs.shape
    T = Tp if T is None else min(max(int(T), 0), Tp)
    if bug == "reads_past_frame_lens":
        T = min(T + 1, Tp)
    f64 = dtype == np.float64
    lse = _max if bug == "max_for_lse" else (_lse64 if f64 else _lse32)
    zero = 0.0 if f64 else np.float32(0.0)
    blank_eff = 0 if bug == "blank_is_zero" else blank
    nbest = beam if nbest is None else nbest
    rep = Report()
    cur = [((), zero, NINF, zero)]  # (prefix, b, nb, score), in prefix_compare order
    for t in range(T):
        cand, equal = prune(probs[t], cutoff_prob, cutoff_top_n, dtype, bug)
        rep.prune_equal |= equal
        rep.n_cand.append(len(cand))
        new = {pre: [NINF, NINF] for pre, _, _, _ in cur}
        if bug == "blank_unpruned" and all(c != blank_eff for c, _ in cand):
            lp = math.log(float(probs[t, blank_eff]) + FLT_MIN)
            cand = cand + [(blank_eff, lp if f64 else np.float32(lp))]
        for c, lp in cand:
            if lp == NINF:
                continue
            if c == blank_eff:
                for pre, b, nb, sc in cur:
                    if sc != NINF:
                        e = new[pre]
                        e[0] = lse(e[0], lp + sc)
                continue
            for pre, b, nb, sc in cur:
                last = pre[-1] if pre else -1
                child = pre + (c,)
                e = new.get(child)
                if e is None:
                    e = new[child] = [NINF, NINF]
                if c == last:
                    if nb != NINF:
                        own = new[pre]
                        own[1] = lse(own[1], lp + nb)
                    src = sc if bug == "repeat_child_from_total" else b
                    if src != NINF:
                        e[1] = lse(e[1], lp + src)
                elif sc != NINF:
                    e[1] = lse(e[1], lp + sc)
        items = [(pre, b, nb, lse(b, nb)) for pre, (b, nb) in new.items()]
        items.sort(key=lambda it: _sort_key(it, V, bug))
        rep.n_exist.append(len(items))
        k = len(items)
        if len(items) >= beam:
            k = beam
            if len(items) > beam:
                kind, val = _pair(items[beam - 1], items[beam], V, bug)
                if kind == "gap":
                    rep.gap_cut = min(rep.gap_cut, val)
                elif kind == "tie":
                    rep.ties_cut += 1
                    rep.undecided_cut |= not val
                elif val:
                    rep.inf_cut = True
                if near is not None:
                    mode, u = near
                    if mode == "keep":
                        s = float(items[beam - 1][3])
                        while (k < min(len(items), 2 * beam) and items[k][3] != NINF
                               and s - float(items[k][3]) <= u * max(abs(s), 1.0)):
                            k += 1
                    else:
                        s = float(items[beam][3])
                        while k > 1 and s != NINF and float(items[k - 1][3]) - s <= u * max(abs(s), 1.0):
                            k -= 1
        cur = items[:k]
        for a, b_ in zip(cur, cur[1:]):
            kind, val = _pair(a, b_, V, bug)
            if kind == "gap":
                rep.gap_kept = min(rep.gap_kept, val)
            elif kind == "tie":
                rep.ties_kept += 1
    cur = cur[:max(beam, 1)] if near is None else cur
    for a, b_ in zip(cur[:nbest], cur[1:nbest + 1]):
        kind, val = _pair(a, b_, V, bug)
        if kind == "gap":
            rep.gap_final = min(rep.gap_final, val)
        elif kind == "tie":
            rep.ties_final += 1
            rep.undecided_final |= not val
    rows = [(pre, -float(sc) if sc != NINF else math.inf, sc != NINF) for pre, _, _, sc in cur[:nbest]]
    return rows, rep


def collapse(labels, blank):
    out, prev = [], None
    for c in labels:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return tuple(out)


def enumerate_paths(probs, blank, T=None):
    """{token tuple: -log of the float64 sum over all V^T labelings that collapse to it}, every factor p + FLT_MIN.
    A token sequence that no labeling of T frames collapses to (L + repeats > T) is absent: it is at minus infinity."""
    import itertools
    probs = np.asarray(probs, np.float32)
    Tp, V = probs.shape
    T = Tp if T is None else T
    p = probs[:T].astype(np.float64) + FLT_MIN
    total = {}
    for lab in itertools.product(range(V), repeat=T):
        w = 1.0
        for t, c in enumerate(lab):
            w *= p[t, c]
        key = collapse(lab, blank)
        total[key] = total.get(key, 0.0) + w
    return {k: -math.log(v) for k, v in total.items() if v > 0.0}


def ranked(nll_by_tokens):
    """enumeration in prefix_compare order: [(tokens, nll)]; asserts that no tie is left undecided"""
    rows = sorted(nll_by_tokens.items(), key=lambda kv: (kv[1], kv[0][-1] if kv[0] else -1, kv[0]))
    for (ta, a), (tb, b) in zip(rows, rows[1:]):
        assert a != b or (ta[-1] if ta else -1) != (tb[-1] if tb else -1), (ta, tb)
    return rows


def frames_needed(tokens):
    return len(tokens) + sum(1 for i in range(1, len(tokens)) if tokens[i] == tokens[i - 1])
