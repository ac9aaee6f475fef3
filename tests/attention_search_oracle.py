"""Plain restatement of the attention beam search (WeNet's `attention` decode mode) over DecoderOracle.logits, one
utterance at a time, with exactly the semantics of the header comment of ppasr_amd/csrc/attn_decode.hip:

    N rows; sos = eos = V - 1; s[0] = 0, s[k > 0] = -inf
    step: a live row offers its N largest log-probabilities (lower id first on equal values), an ended row offers
          (eos, s[k]) once, a row at -inf nothing; the N best candidates (lower k * N + j first on equal scores) are the
          new rows; the search of an utterance stops when all its rows ended or after max_steps

The decoder is causal, so the last row of the teacher-forced logits over [sos] + hyp is the incremental step.  The step is
computed in the oracle's dtype (float64: the yardstick; float32: the floor), scores are summed in float64 either way.

`mut` names one deliberate bug of the search (SEARCH_MUTATIONS); two more bugs are the decoder's own
(DECODER_MUTATIONS, passed to DecoderOracle): the step's key count off by one and a frame past out_lens visible.

`replay` holds a device trace to the float64 decoder WITHOUT demanding the same hypotheses: it rebuilds the beam of step
i - 1 from the trace and checks that the device's selection at step i is a top-N of the float64 candidates up to `tol`."""
import numpy as np
import torch

SEARCH_MUTATIONS = ("ancestry_not_rewritten", "ended_offers_n", "no_eos_term", "higher_id_on_tie", "higher_index_on_tie")
DECODER_MUTATIONS = {"key_count_off_by_one": "causal_no_diagonal", "frame_past_out_lens": "one_frame_past_out_lens"}


class StepCache:
    """log-probabilities of the next token after a prefix, memoised by prefix (one decoder run per distinct prefix)"""

    def __init__(self, oracle, memory, out_len):
        self.o, self.memory, self.out_len = oracle, memory, int(out_len)
        self._d = {}
        self.scale = 0.0  # max |logit - row mean| seen: the scale a log-probability error is measured in

    def logp(self, prefix):
        key = tuple(int(t) for t in prefix)
        if key not in self._d:
            lg = self.o.logits(self.memory, self.out_len, list(key))[-1]
            self.scale = max(self.scale, float((lg - lg.mean()).abs().max()))
            self._d[key] = torch.log_softmax(lg, -1).double().numpy()
        return self._d[key]


def _order(values, higher_index_first=False):
    """indices by larger value first; equal values: lower index first (the mutation: higher index first)"""
    v = np.asarray(values, np.float64)
    idx = np.arange(v.size)
    return np.lexsort((-idx if higher_index_first else idx, -v))


def search(oracle, memory, out_len, beam_size, max_steps, mut=None, record_gaps=False, ignore_exact_ties=False):
    """-> dict(tokens: list of N lists, scores [N] f64, ended [N] i32, steps: steps this utterance ran,
    trace_parent / trace_token [max_steps, N] i32 (-1 where nothing happened), trace_score [max_steps, N] f64 (0.0 there),
    token_logp [N, max_steps + 1] f64, scale, and with record_gaps: min_gap, the smallest score difference over all steps
    between neighbours of the N + 1 best candidates (the cut and the order of the kept rows; ignore_exact_ties: gaps of
    exactly 0, which a tie case has on purpose, are left out))"""
    assert mut is None or mut in SEARCH_MUTATIONS, mut
    N, P, V = int(beam_size), int(max_steps), oracle.V
    eos = V - 1
    hi_id, hi = mut == "higher_id_on_tie", mut == "higher_index_on_tie"  # the two tie rules: vocabulary, candidates
    sc = StepCache(oracle, memory, out_len)
    hyp = [[] for _ in range(N)]
    lps = [[] for _ in range(N)]
    s = np.full(N, -np.inf)
    s[0] = 0.0
    ended = np.zeros(N, bool)
    tp = np.full((P, N), -1, np.int32)
    tt = np.full((P, N), -1, np.int32)
    ts = np.zeros((P, N))
    steps, min_gap = 0, np.inf
    for i in range(1, P + 1):
        if ended.all():
            break
        cand = []  # (score, k * N + j, k, token, summand)
        every = []  # scores of EVERY candidate a full-vocabulary search would see (for the gaps)
        for k in range(N):
            if ended[k]:
                for j in range(N if mut == "ended_offers_n" else 1):
                    cand.append((s[k], k * N + j, k, eos, 0.0))
                every.append(s[k])
            elif np.isfinite(s[k]):
                lp = sc.logp(hyp[k])
                top = _order(lp, hi_id)[:N]
                for j, v in enumerate(top):
                    add = 0.0 if (mut == "no_eos_term" and v == eos) else float(lp[v])
                    cand.append((s[k] + add, k * N + j, k, int(v), float(lp[v])))
                every.extend((s[k] + lp).tolist())
        order = _order([c[0] for c in cand], hi)  # cand is in k * N + j order already
        if record_gaps and len(every) > 1:
            e = np.sort(np.asarray(every))[::-1][:N + 1]
            g = e[:-1] - e[1:]
            g = g[g > 0] if ignore_exact_ties else g
            min_gap = min(min_gap, float(np.min(g)) if g.size else np.inf)
        new_hyp, new_lps, new_s, new_e = [], [], np.full(N, -np.inf), np.zeros(N, bool)
        for rank, ci in enumerate(order[:N]):
            val, _, k, tok, lp = cand[ci]
            src = rank if mut == "ancestry_not_rewritten" else k
            if ended[k]:
                new_hyp.append(list(hyp[src]))
                new_lps.append(list(lps[src]))
            else:
                new_hyp.append(list(hyp[src]) + ([] if tok == eos else [tok]))
                new_lps.append(list(lps[src]) + [lp])
            new_s[rank] = val
            new_e[rank] = ended[k] or tok == eos
            tp[i - 1, rank], tt[i - 1, rank], ts[i - 1, rank] = k, tok, val
        while len(new_hyp) < N:
            new_hyp.append([])
            new_lps.append([])
        hyp, lps, s, ended = new_hyp, new_lps, new_s, new_e
        steps = i
    tlp = np.zeros((N, P + 1))
    for k in range(N):
        tlp[k, :len(lps[k])] = lps[k]
    out = dict(tokens=hyp, scores=s, ended=ended.astype(np.int32), steps=steps, trace_parent=tp, trace_token=tt,
               trace_score=ts, token_logp=tlp, scale=sc.scale)
    if record_gaps:
        out["min_gap"] = min_gap
    return out


def replay(oracle64, memory, out_len, beam_size, trace_parent, trace_token, trace_score, tol_of):
    """One utterance's device trace ([steps, N] each) against the float64 decoder.  tol_of(scale) -> the score tolerance
    for the logit scale seen so far.  Rebuilds the beam of step i - 1 from the trace, computes the float64 candidates of
    step i from it and checks, up to tol:
      * every kept candidate scores at least the float64 N-th best - tol
      * every candidate above the N-th best + tol is kept
      * kept neighbours are out of order by at most tol
      * the traced score lies within tol of the float64 score of the same candidate
    and exactly: parents are rows of the old beam that offer something, an ended parent is carried over as (eos, its
    score), no candidate is kept twice, and nothing is traced once every row has ended.
    -> dict(problems: list of str, worst: largest violation / tol seen (<= 1 when clean), steps, hyps, ended, scores64)"""
    N, V = int(beam_size), oracle64.V
    eos = V - 1
    sc = StepCache(oracle64, memory, out_len)
    tp, tt, ts = np.asarray(trace_parent), np.asarray(trace_token), np.asarray(trace_score, np.float64)
    hyp = [[] for _ in range(N)]
    s64 = np.full(N, -np.inf)
    s64[0] = 0.0
    ended = np.zeros(N, bool)
    problems, worst, steps = [], 0.0, 0
    for i in range(1, tp.shape[0] + 1):
        if ended.all():
            if (tp[i - 1:] != -1).any() or (tt[i - 1:] != -1).any() or (ts[i - 1:] != 0).any():
                problems.append(f"step {i}: traced after every row had ended")
            break
        cands = {}  # (k, token) -> float64 score
        for k in range(N):
            if ended[k]:
                cands[(k, eos)] = s64[k]
            elif np.isfinite(s64[k]):
                lp = sc.logp(hyp[k])
                for v in range(V):
                    cands[(k, v)] = s64[k] + float(lp[v])
        tol = tol_of(sc.scale)
        vals = np.sort(np.asarray(list(cands.values())))[::-1]
        nth = vals[min(N, vals.size) - 1]
        kept = [(int(tp[i - 1, r]), int(tt[i - 1, r])) for r in range(N)]
        if len(set(kept)) != N:
            problems.append(f"step {i}: a candidate kept twice {kept}")
        bad = [c for c in kept if c not in cands]
        if bad:
            problems.append(f"step {i}: kept {bad} which the old beam does not offer")
            break
        k64 = np.asarray([cands[c] for c in kept])
        worst = max(worst, float((nth - k64).max() / tol), float(np.abs(ts[i - 1] - k64).max() / tol),
                    float((k64[1:] - k64[:-1]).max() / tol) if N > 1 else 0.0)
        if (k64 < nth - tol).any():
            problems.append(f"step {i}: kept a candidate {float((nth - k64).max()):.3e} below the N-th best (tol {tol:.3e})")
        missed = [c for c, v in cands.items() if v > nth + tol and c not in kept]
        if missed:
            problems.append(f"step {i}: not kept although above the N-th best + tol: {missed[:4]}")
        if N > 1 and (k64[1:] > k64[:-1] + tol).any():
            problems.append(f"step {i}: kept rows out of order by {float((k64[1:] - k64[:-1]).max()):.3e}")
        if (np.abs(ts[i - 1] - k64) > tol).any():
            problems.append(f"step {i}: traced score off by {float(np.abs(ts[i - 1] - k64).max()):.3e} (tol {tol:.3e})")
        new_hyp, new_e = [], np.zeros(N, bool)
        for r, (k, tok) in enumerate(kept):
            new_hyp.append(list(hyp[k]) + ([] if (ended[k] or tok == eos) else [tok]))
            new_e[r] = ended[k] or tok == eos
        hyp, s64, ended = new_hyp, k64, new_e
        steps = i
    return dict(problems=problems, worst=worst, steps=steps, hyps=hyp, ended=ended.astype(np.int32), scores64=s64,
                scale=sc.scale)


def final_from_trace(trace_parent, trace_token, steps, beam_size, eos):
    """the hypotheses the back-pointers of one utterance spell: -> list of N token lists"""
    out = []
    for k in range(beam_size):
        cur, toks = k, []
        for i in range(steps, 0, -1):
            tok = int(trace_token[i - 1, cur])
            if tok != eos:
                toks.append(tok)
            cur = int(trace_parent[i - 1, cur])
        out.append(toks[::-1])
    return out
