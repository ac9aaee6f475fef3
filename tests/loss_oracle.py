"""numpy oracle of the loss half of evaluation (a plain module, imported by the test files, like tests/align_oracle.py).

* ``ctc_nll``: the forward sum of the definition in the header comment of ppasr_amd/csrc/ctc_loss.hip, restated without
  looking at how the kernel walks it: states 0 .. 2L (even = blank, odd 2l+1 = token l), emission log(max(p, FLT_MIN)),
  transitions stay / step / skip (skip only into a token state whose label differs from the token two states back),
  start in state 0 or 1, end in 2L or 2L-1, log-sum over the predecessors.  ``dtype``: float64 is the yardstick the
  tests hold the kernel to, float32 the floor (the same walk in the kernel's number format).
* ``brute_force_nll``: the sum over every labeling that collapses to the tokens (tiny cases only).
* ``kl_rows``: the label-smoothing KL of loss/label_smoothing_loss.py:68-91 of the reference from float64 logits, in the
  closed form of include/ppasr_hip.h; ``kl_rows_dense`` is the dense t * (log t - logp) it must agree with.
* ``att_kl``: the per-utterance sums over the L + 1 target rows (tokens, then eos) of one decoder direction.
* ``combine``: ConformerModel.forward's combination (conformer/model.py:98-109, 129-143; loss/ctc.py:29-50).
* ``BUGS``: deliberate mistakes, by name; every one must move some case of the table past the tolerance by 5x (the
  admission rule of tests/test_loss_oracle_cpu.py).
"""
import itertools

import numpy as np

from align_oracle import BAD_INPUT, FLT_MIN, INFEASIBLE, OK, collapse, emissions, frames_needed

CTC_BUGS = ("skip_between_equal_tokens", "skip_into_blank", "end_state_2L_only", "start_state_0_only", "max_for_sum",
            "one_frame_past_frame_lens")
ATT_BUGS = ("padded_columns_in_X", "V_for_V_minus_1", "eos_row_dropped", "right_decoder_forward_label")
MODEL_BUGS = ("div_B_dropped",)
BUGS = CTC_BUGS + ATT_BUGS + MODEL_BUGS


def ctc_nll(probs, tokens, T=None, blank=0, dtype=np.float64, max_tokens=None, bug=None):
    """probs [Tp, V] f32, tokens (list of ids), T valid frames (None: all; clamped to [0, Tp]) -> (nll, status); nll is
    +inf for status 1 (infeasible) and 2 (bad input), 0 for L = 0 with T = 0."""
    assert bug is None or bug in CTC_BUGS, bug
    probs = np.asarray(probs, np.float32)
    Tp, V = probs.shape
    T = Tp if T is None else min(max(int(T), 0), Tp)
    tokens = [int(x) for x in tokens]
    L = len(tokens)
    if (max_tokens is not None and L > max_tokens) or any(t < 0 or t >= V or t == blank for t in tokens):
        return dtype(np.inf), BAD_INPUT
    if T < frames_needed(tokens):
        return dtype(np.inf), INFEASIBLE
    if T == 0:
        return dtype(0.0), OK
    if bug == "one_frame_past_frame_lens":
        T = min(T + 1, Tp)
    S = 2 * L + 1
    labels = np.full(S, blank, np.int64)
    labels[1::2] = tokens
    skip_ok = np.zeros(S, bool)
    for s in range(2, S):
        if s % 2 == 1:
            skip_ok[s] = labels[s] != labels[s - 2] or bug == "skip_between_equal_tokens"
        else:
            skip_ok[s] = bug == "skip_into_blank"
    e = emissions(probs[:T], dtype)[:, labels]  # [T, S]
    ninf = dtype(-np.inf)
    a = np.full(S, ninf, dtype)
    a[0] = e[0, 0]
    if L > 0 and bug != "start_state_0_only":
        a[1] = e[0, 1]
    reduce = np.maximum.reduce if bug == "max_for_sum" else np.logaddexp.reduce
    for t in range(1, T):
        step = np.concatenate([[ninf], a[:-1]]).astype(dtype)
        skip = np.where(skip_ok, np.concatenate([[ninf, ninf], a[:-2]])[:S], ninf).astype(dtype)
        with np.errstate(invalid="ignore"):
            a = (reduce(np.stack([a, step, skip]), axis=0).astype(dtype) + e[t]).astype(dtype)
    ends = [a[S - 1]] + ([a[S - 2]] if L > 0 and bug != "end_state_2L_only" else [])
    return dtype(-reduce(np.asarray(ends, dtype))), OK


def brute_force_nll(probs, tokens, blank=0):
    """-log of the float64 sum over all V^T labelings that collapse to ``tokens`` (+inf if there is none)."""
    probs = np.asarray(probs, np.float32)
    T, V = probs.shape
    p = np.exp(emissions(probs, np.float64))
    tokens = [int(x) for x in tokens]
    total = 0.0
    for lab in itertools.product(range(V), repeat=T):
        if collapse(lab, blank) == tokens:
            total += float(np.prod([p[t, lab[t]] for t in range(T)]))
    return -np.log(total) if total > 0 else np.inf


# ---- label smoothing ------------------------------------------------------------------------------------------------------
def _logsoftmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def kl_rows_dense(logits, targets, lsm):
    """label_smoothing_loss.py:68-91 row by row: true_dist = lsm / (V - 1) off the target and 1 - lsm on it; KLDivLoss
    (reduction none) of log_softmax against it, a zero target contributing zero.  logits [R, V] float64 -> [R]."""
    logits = np.asarray(logits, np.float64)
    R, V = logits.shape
    t = np.full((R, V), lsm / (V - 1), np.float64)
    t[np.arange(R), np.asarray(targets, np.int64)] = 1.0 - lsm
    logp = _logsoftmax(logits)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(t > 0, t * (np.log(t) - logp), 0.0)
    return term.sum(1)


def kl_rows(logits, targets, lsm, bug=None, Vp=None):
    """The closed form: c ln c + s ln(s / (V - 1)) - c (x_y - lse) - s / (V - 1) (X - x_y - (V - 1) lse), 0 ln 0 = 0."""
    x = np.asarray(logits, np.float64)
    R, V = x.shape
    y = np.asarray(targets, np.int64)
    m = x.max(1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(1))
    xy = x[np.arange(R), y]
    X = x.sum(1)
    n = V - 1
    if bug == "V_for_V_minus_1":
        n = V
    if bug == "padded_columns_in_X":  # the zero logits of the padded columns counted as columns of the row
        n = (V + 255) // 256 * 256 - 1 if Vp is None else Vp - 1
    s, c = float(lsm), 1.0 - float(lsm)
    k0 = (c * np.log(c) if c > 0 else 0.0) + (s * np.log(s / n) if s > 0 else 0.0)
    return k0 - c * (xy - lse) - (s / n) * (X - xy - n * lse)


def targets_of(label, V, reverse=False):
    """the L + 1 target ids of one direction: the label (reversed for the right decoder), then eos = V - 1"""
    label = [int(t) for t in label]
    return (label[::-1] if reverse else label) + [V - 1]


def att_kl(logits, label, lsm, reverse=False, bug=None):
    """logits [>= L + 1, V] float64 of one (utterance, direction), teacher-forced over ``label`` (already reversed inside
    the decoder for the right one) -> (sum of the row KL terms over the L + 1 target rows, row count)."""
    x = np.asarray(logits, np.float64)
    V = x.shape[1]
    tg = targets_of(label, V, reverse and bug != "right_decoder_forward_label")
    rows = len(tg) - (1 if bug == "eos_row_dropped" else 0)
    kl = kl_rows(x[:rows], tg[:rows], lsm, bug=bug)
    total = 0.0
    for v in kl:  # in row order
        total += float(v)
    return total, len(tg)


def combine(ctc_nll_b, att_kl_b, r_att_kl_b, rows_b, ctc_weight, reverse_weight=0.0, length_normalized_loss=False,
            bug=None):
    """-> dict(loss, loss_att, loss_ctc) from the per-utterance pieces (None for a branch that does not run)."""
    B = len(ctc_nll_b) if ctc_nll_b is not None else len(att_kl_b)
    div = 1.0 if bug == "div_B_dropped" else float(B)
    loss_ctc = loss_att = None
    if ctc_weight != 0.0:
        loss_ctc = float(np.sum(np.asarray(ctc_nll_b, np.float64)) / div)
    if ctc_weight != 1.0:
        denom = float(np.sum(rows_b)) if length_normalized_loss else div
        la = float(np.sum(att_kl_b)) / denom
        ra = float(np.sum(r_att_kl_b)) / denom if reverse_weight > 0 else 0.0
        loss_att = la * (1.0 - reverse_weight) + ra * reverse_weight
    if loss_ctc is None:
        loss = loss_att
    elif loss_att is None:
        loss = loss_ctc
    else:
        loss = ctc_weight * loss_ctc + (1.0 - ctc_weight) * loss_att
    return dict(loss=loss, loss_att=loss_att, loss_ctc=loss_ctc)


def rel_err(got, ref):
    """|got - ref64| / max(|ref64|, 1); 0 when both are the same infinity"""
    got, ref = float(got), float(ref)
    if np.isinf(ref) or np.isinf(got):
        return 0.0 if got == ref else np.inf
    return abs(got - ref) / max(abs(ref), 1.0)


# ---- the two tiny checkpoints of tests/golden/ref_loss.npz ---------------------------------------------------------------
# (non-streaming: the reference's forward draws a random chunk size for a streaming model, even in eval())
MODEL_CASES = {
    "bi_lsm": dict(V=120, num_blocks=2, sd_seed=3, dec_seed=78, units=256, blocks=(1, 1), x_spec=(3, 131, [131, 100, 60], 9),
                   labels=[[5, 9, 9, 17, 3, 40, 118], [8, 8, 21, 2], [7]],
                   conf=dict(ctc_weight=0.3, lsm_weight=0.1, reverse_weight=0.3, length_normalized_loss=False)),
    "left_norm": dict(V=67, num_blocks=2, sd_seed=4, dec_seed=79, units=256, blocks=(2, 0), x_spec=(2, 99, [99, 70], 10),
                      labels=[[1, 1, 65, 30], [12, 13, 14, 15, 16, 16]],
                      conf=dict(ctc_weight=0.5, lsm_weight=0.0, reverse_weight=0.0, length_normalized_loss=True)),
}


def model_case(name):
    """-> dict(sd, x, lens, labels [B, U] -1 padded, label_lens) of a case of MODEL_CASES, all from its seeds"""
    import decoder_cases as dc
    from ppasr_amd.utils.synth import conformer_state_dict, synth_features
    c = MODEL_CASES[name]
    sd = conformer_state_dict(vocab_size=c["V"], num_blocks=c["num_blocks"], seed=c["sd_seed"], perturb_norm=True)
    sd.update(dc.decoder_state_dict(c["dec_seed"], c["V"], c["units"], *c["blocks"]))
    B, T, lens, seed = c["x_spec"]
    x, lens = synth_features(B, T, lens=lens, seed=seed)
    U = max(len(l) for l in c["labels"])
    labels = np.full((B, U), -1, np.int64)
    for b, l in enumerate(c["labels"]):
        labels[b, :len(l)] = l
    return dict(sd=sd, x=x, lens=lens, labels=labels, label_lens=np.asarray([len(l) for l in c["labels"]], np.int64))


def model_pipeline64(name, case=None):
    """The float64 pipeline of a case of MODEL_CASES: oracle.conformer_oracle (float64, non-causal) -> tests/decoder_oracle.py
    (float64) -> the two losses and their combination.  -> (dict(loss, loss_att, loss_ctc), per-utterance pieces with
    the tolerances of tests/test_model_loss_gpu.py)."""
    import torch
    from decoder_oracle import DecoderOracle
    from oracle.conformer_oracle import ConformerOracle
    c = MODEL_CASES[name]
    m = model_case(name) if case is None else case
    V, conf = c["V"], c["conf"]
    o = ConformerOracle(m["sd"], num_blocks=c["num_blocks"], causal=False, dtype=torch.float64)
    with torch.no_grad():
        enc, masks = o.encoder_forward(m["x"], m["lens"])
        logits = o.ctc_logits(enc)
        probs = torch.softmax(logits, dim=2).numpy()
    frames = masks.squeeze(1).sum(1).numpy()
    dec = DecoderOracle(m["sd"], V, *c["blocks"], heads=4, dtype=torch.float64)
    budget = 2e-5  # numerics.F32_BUDGET
    pieces = []
    for b in range(len(c["labels"])):
        T, tok = int(frames[b]), c["labels"][b]
        nll, st = ctc_nll(probs[b].astype(np.float32), tok, T)
        assert st == OK
        lg = logits[b, :T].numpy()
        ctc_tol = T * budget * float(np.abs(lg - lg.mean(-1, keepdims=True)).max()) + budget * max(abs(nll), 1.0)
        kls, scale = [0.0, 0.0], 1.0
        for right in ((False, True) if conf["reverse_weight"] > 0 else (False,)):
            xl = dec.logits(enc[b].numpy(), T, tok, right=right).numpy()
            kls[int(right)] = att_kl(xl, tok, conf["lsm_weight"], reverse=right)[0]
            scale = max(scale, float(np.abs(xl - xl.mean(-1, keepdims=True)).max()))
        rows = len(tok) + 1
        pieces.append(dict(nll=float(nll), ctc_tol=ctc_tol, kl=kls[0], r_kl=kls[1], att_tol=2 * budget * rows * scale, rows=rows,
                           frames=T))
    total = combine([p["nll"] for p in pieces], [p["kl"] for p in pieces], [p["r_kl"] for p in pieces],
                    [p["rows"] for p in pieces], conf["ctc_weight"], conf["reverse_weight"], conf["length_normalized_loss"])
    return total, pieces


def model_tolerances(name, pieces):
    """absolute tolerances of (loss, loss_att, loss_ctc) from the per-utterance ones, through the linear combination"""
    conf = MODEL_CASES[name]["conf"]
    B = len(pieces)
    denom = sum(p["rows"] for p in pieces) if conf["length_normalized_loss"] else B
    t_ctc = sum(p["ctc_tol"] for p in pieces) / B
    t_att = sum(p["att_tol"] for p in pieces) / denom
    return dict(loss=conf["ctc_weight"] * t_ctc + (1 - conf["ctc_weight"]) * t_att, loss_att=t_att, loss_ctc=t_ctc)


# ---- the case table of the CTC value ---------------------------------------------------------------------------------------
def softmax_table(rng, T, V, scale=3.0, blank_boost=4.0):
    """random softmax rows; the blank logit is raised on about half the frames"""
    z = rng.normal(size=(T, V)) * scale
    z[:, 0] += blank_boost * (rng.random(T) < 0.5)
    p = np.exp(z - z.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def random_tokens(rng, L, T, V, repeat_p=0.2):
    """L non-blank ids with adjacent repeats, as many as fit into T frames"""
    tok = rng.integers(1, V, size=L).tolist()
    for i in range(1, L):
        if rng.random() < repeat_p:
            tok[i] = tok[i - 1]
    for i in range(1, L):  # undo repeats from the left until it fits
        if frames_needed(tok) <= T:
            break
        if tok[i] == tok[i - 1]:
            tok[i] = tok[i] % (V - 1) + 1
            if i + 1 < L and tok[i + 1] == tok[i]:
                tok[i + 1] = tok[i + 1] % (V - 1) + 1
    assert frames_needed(tok) <= T
    return tok


def case_table():
    """[(name, probs [Tp, V], tokens, T)]: small enough for the CPU tests, with every feature a listed bug needs (equal
    neighbours, tight fits, endings in a token, starts in a token, rows past frame_lens)."""
    rng = np.random.default_rng(2024)
    cases = []
    for T, L, V in [(1, 0, 5), (1, 1, 5), (2, 1, 5), (3, 2, 7), (6, 3, 7), (12, 5, 20), (17, 8, 50), (33, 16, 50), (64, 40, 50),
                    (65, 20, 50), (129, 64, 50), (250, 127, 4233)]:
        p = softmax_table(rng, T + 3, V)
        cases.append((f"random T={T} L={L} V={V}", p, random_tokens(rng, L, T, V), T))
    p = softmax_table(rng, 12, 9)
    cases.append(("all equal", p, [4] * 6, 12))            # needs 11 frames: every skip is forbidden
    cases.append(("alternating", p, [3, 5] * 5, 12))
    cases.append(("fills T", p, [1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4], 12))  # a token per frame: starts and ends in a token
    cases.append(("equal pairs", softmax_table(rng, 20, 9, blank_boost=0.0), [2, 2, 6, 6, 6, 1, 1], 18))
    return cases
