"""Plain restatement of the CTC-joint attention beam search, one utterance at a time, with exactly the semantics of the
header comment of ppasr_amd/csrc/attn_decode_joint.hip: the search of tests/attention_search_oracle.py with

    comb[v] = logp_att[v] + ctc_weight * (Psi(g.v) - Psi(g))        (tests/ctc_prefix_oracle.py)

in place of logp_att[v]; a live row offers its N largest FINITE entries, so a row may offer, and the utterance may keep,
fewer than N candidates (the remaining rows are at -inf, not ended, with an empty hypothesis and no trace entry).

The decoder step and the CTC recurrences are computed in ``dtype`` (float64: the yardstick; float32: the floor, comb
formed in float32 as the kernel forms it), scores are summed in float64 either way.  ``mut`` names one deliberate bug
(ctc_prefix_oracle.BUGS).

``replay`` is attention_search_oracle.replay extended with the CTC term: it rebuilds the beam of step i - 1 from a device
trace and checks that the device's selection at step i is a top-N of the float64 candidates up to ``tol``, and that
trace_ctc is Psi of the traced hypotheses."""
import numpy as np

import ctc_prefix_oracle as cp
from attention_search_oracle import StepCache, _order


def _comb(lp, psi_c, psi_g, w, dtype, mut=None):
    """[V] comb in ``dtype``; -inf where the CTC term is"""
    dt = dtype
    with np.errstate(invalid="ignore"):
        d = psi_c.astype(dt) if mut == "psi_g_not_subtracted" else (psi_c.astype(dt) - dt(psi_g)).astype(dt)
        return (lp.astype(dt) + (dt(w) * d).astype(dt)).astype(dt).astype(np.float64)


def search(oracle, memory, out_len, probs, blank, ctc_weight, beam_size, max_steps, dtype=np.float64, mut=None,
           record_gaps=False):
    """-> dict(tokens: list of N lists, scores [N] f64, ended [N] i32, steps, trace_parent / trace_token [max_steps, N] i32
    (-1 where nothing happened), trace_score [max_steps, N] f64 and trace_ctc [max_steps, N] (0.0 there), scale (of the
    decoder's logits), S (the bound of every finite |Psi|: the sum over the valid frames of max_v |x[t][v]|), psi_seen: every
    finite Psi(g.v) computed, keyed by hypothesis tuple, and with record_gaps: min_gap as in attention_search_oracle)"""
    assert mut is None or mut in cp.BUGS, mut
    assert ctc_weight > 0
    N, P, V = int(beam_size), int(max_steps), oracle.V
    eos = V - 1
    ps = cp.PrefixScorer(probs, out_len, blank, dtype, mut)
    sc = StepCache(oracle, memory, out_len)
    st = [ps.empty() for _ in range(N)]
    s = np.full(N, -np.inf)
    s[0] = 0.0
    ended = np.zeros(N, bool)
    psi_row = [dtype(0.0)] * N
    tp = np.full((P, N), -1, np.int32)
    tt = np.full((P, N), -1, np.int32)
    ts = np.zeros((P, N))
    tc = np.zeros((P, N))
    psi_seen = {}
    steps, min_gap = 0, np.inf
    for i in range(1, P + 1):
        if not (~ended & np.isfinite(s)).any():  # no live row
            break
        cand, every = [], []  # (score, k * N + j, k, token, Psi of the new hypothesis)
        for k in range(N):
            if ended[k]:
                cand.append((s[k], k * N, k, eos, psi_row[k]))
                every.append(s[k])
            elif np.isfinite(s[k]):
                psi_c = ps.psi_all(st[k])
                for v in np.nonzero(np.isfinite(psi_c))[0]:
                    psi_seen[tuple(st[k].tokens) + (int(v),)] = float(psi_c[v])
                comb = _comb(sc.logp(st[k].tokens), psi_c, psi_row[k], ctc_weight, dtype, mut)
                top = [v for v in _order(comb)[:N] if np.isfinite(comb[v])]
                for j, v in enumerate(top):
                    cand.append((s[k] + float(comb[v]), k * N + j, k, int(v), psi_c[v]))
                every.extend((s[k] + comb[np.isfinite(comb)]).tolist())
        order = _order([c[0] for c in cand])
        if record_gaps and len(every) > 1:
            e = np.sort(np.asarray(every))[::-1][:N + 1]
            min_gap = min(min_gap, float(np.min(e[:-1] - e[1:])))
        new_st, new_s, new_e, new_psi = [], np.full(N, -np.inf), np.zeros(N, bool), []
        for rank, ci in enumerate(order[:N]):
            val, _, k, tok, psi = cand[ci]
            if ended[k] or tok == eos:
                new_st.append(st[k])
            else:
                new_st.append(ps.extend(st[k], tok, psi))
            new_psi.append(psi)
            new_s[rank] = val
            new_e[rank] = ended[k] or tok == eos
            tp[i - 1, rank], tt[i - 1, rank], ts[i - 1, rank], tc[i - 1, rank] = k, tok, val, float(psi)
        while len(new_st) < N:
            new_st.append(ps.empty())
            new_psi.append(dtype(0.0))
        st, s, ended, psi_row = new_st, new_s, new_e, new_psi
        steps = i
    out = dict(tokens=[list(x.tokens) if np.isfinite(v) else [] for x, v in zip(st, s)], scores=s,
               ended=ended.astype(np.int32), steps=steps, trace_parent=tp, trace_token=tt, trace_score=ts, trace_ctc=tc,
               scale=sc.scale, S=ps.S, psi_seen=psi_seen)
    if record_gaps:
        out["min_gap"] = min_gap
    return out


def replay(oracle64, memory, out_len, probs, blank, ctc_weight, beam_size, trace_parent, trace_token, trace_score, trace_ctc,
           tol_of, psi_tol):
    """One utterance's device trace ([steps, N] each) against the float64 decoder and the float64 prefix scorer.
    tol_of(scale) -> the score tolerance for the logit scale seen so far; psi_tol: the tolerance of one Psi.  The checks of
    attention_search_oracle.replay, with: a row kept only where a finite candidate exists (exactly min(N, finite
    candidates) rows are kept, the first ones), every kept candidate finite in float64, and trace_ctc within psi_tol of the
    float64 Psi of the new row's hypothesis.
    -> dict(problems, worst (violation / tol), worst_psi (|trace_ctc - Psi64| / psi_tol), steps, hyps, ended, scores64)"""
    N, V = int(beam_size), oracle64.V
    eos = V - 1
    ps = cp.PrefixScorer(probs, out_len, blank, np.float64)
    sc = StepCache(oracle64, memory, out_len)
    tp, tt = np.asarray(trace_parent), np.asarray(trace_token)
    ts, tc = np.asarray(trace_score, np.float64), np.asarray(trace_ctc, np.float64)
    st = [ps.empty() for _ in range(N)]
    s64 = np.full(N, -np.inf)
    s64[0] = 0.0
    ended = np.zeros(N, bool)
    problems, worst, worst_psi, steps = [], 0.0, 0.0, 0
    for i in range(1, tp.shape[0] + 1):
        if not (~ended & np.isfinite(s64)).any():
            if (tp[i - 1:] != -1).any() or (tt[i - 1:] != -1).any() or (ts[i - 1:] != 0).any() or (tc[i - 1:] != 0).any():
                problems.append(f"step {i}: traced after the last live row")
            break
        cands = {}  # (k, token) -> (float64 score, Psi of the new hypothesis)
        for k in range(N):
            if ended[k]:
                cands[(k, eos)] = (s64[k], st[k].psi)
            elif np.isfinite(s64[k]):
                psi_c = ps.psi_all(st[k])
                comb = _comb(sc.logp(st[k].tokens), psi_c, st[k].psi, ctc_weight, np.float64)
                for v in np.nonzero(np.isfinite(comb))[0]:
                    cands[(k, int(v))] = (s64[k] + float(comb[v]), psi_c[v])
        tol = tol_of(sc.scale)
        vals = np.sort(np.asarray([c[0] for c in cands.values()]))[::-1]
        n_keep = min(N, vals.size)
        nth = vals[n_keep - 1]
        rows = [r for r in range(N) if tp[i - 1, r] != -1]
        if rows != list(range(n_keep)):
            problems.append(f"step {i}: rows {rows} traced, {n_keep} finite candidates")
            break
        if (tt[i - 1, n_keep:] != -1).any() or (ts[i - 1, n_keep:] != 0).any() or (tc[i - 1, n_keep:] != 0).any():
            problems.append(f"step {i}: a row at -inf has trace entries")
        kept = [(int(tp[i - 1, r]), int(tt[i - 1, r])) for r in rows]
        if len(set(kept)) != n_keep:
            problems.append(f"step {i}: a candidate kept twice {kept}")
        bad = [c for c in kept if c not in cands]
        if bad:
            problems.append(f"step {i}: kept {bad} which the old beam does not offer (or only at -inf)")
            break
        k64 = np.asarray([cands[c][0] for c in kept])
        p64 = np.asarray([float(cands[c][1]) for c in kept])
        worst = max(worst, float((nth - k64).max() / tol), float(np.abs(ts[i - 1, :n_keep] - k64).max() / tol),
                    float((k64[1:] - k64[:-1]).max() / tol) if n_keep > 1 else 0.0)
        worst_psi = max(worst_psi, float(np.abs(tc[i - 1, :n_keep] - p64).max() / psi_tol))
        if (k64 < nth - tol).any():
            problems.append(f"step {i}: kept a candidate {float((nth - k64).max()):.3e} below the N-th best (tol {tol:.3e})")
        missed = [c for c, v in cands.items() if v[0] > nth + tol and c not in kept]
        if missed:
            problems.append(f"step {i}: not kept although above the N-th best + tol: {missed[:4]}")
        if n_keep > 1 and (k64[1:] > k64[:-1] + tol).any():
            problems.append(f"step {i}: kept rows out of order by {float((k64[1:] - k64[:-1]).max()):.3e}")
        if (np.abs(ts[i - 1, :n_keep] - k64) > tol).any():
            problems.append(f"step {i}: traced score off by {float(np.abs(ts[i - 1, :n_keep] - k64).max()):.3e} (tol {tol:.3e})")
        if (np.abs(tc[i - 1, :n_keep] - p64) > psi_tol).any():
            problems.append(f"step {i}: trace_ctc off by {float(np.abs(tc[i - 1, :n_keep] - p64).max()):.3e} (tol {psi_tol:.3e})")
        new_st, new_e, new_s = [], np.zeros(N, bool), np.full(N, -np.inf)
        for r, (k, tok) in enumerate(kept):
            new_st.append(st[k] if (ended[k] or tok == eos) else ps.extend(st[k], tok, cands[(k, tok)][1]))
            if not ended[k] and tok == eos:  # the ended hypothesis carries Psi(g.eos)
                new_st[-1] = cp.State(st[k].tokens, st[k].rn, st[k].rb, cands[(k, tok)][1])
            new_e[r] = ended[k] or tok == eos
            new_s[r] = k64[r]
        while len(new_st) < N:
            new_st.append(ps.empty())
        st, s64, ended = new_st, new_s, new_e
        steps = i
    hyps = [list(x.tokens) if np.isfinite(v) else [] for x, v in zip(st, s64)]
    return dict(problems=problems, worst=worst, worst_psi=worst_psi, steps=steps, hyps=hyps, ended=ended.astype(np.int32),
                scores64=s64, scale=sc.scale, S=ps.S)


def floor_e32(probs, out_len, blank, psi_seen):
    """the float32 restatement's own error on what a float64 search visited: max |Psi32 - Psi64| / max(S, 1) over every
    finite Psi(g.v) in ``psi_seen`` (search()'s), each recomputed from the empty hypothesis in float32"""
    ps32 = cp.PrefixScorer(probs, out_len, blank, np.float32)
    parents = {}
    for h, v in psi_seen.items():
        parents.setdefault(h[:-1], []).append((h[-1], v))
    worst = 0.0
    for g, items in parents.items():
        psi = ps32.psi_all(ps32.state_of(g)).astype(np.float64)
        for c, v in items:
            worst = max(worst, abs(float(psi[c]) - v)) if np.isfinite(psi[c]) else np.inf
    return worst / max(ps32.S, 1.0)
