"""CTC negative log-likelihood on the device (ppasr_ctc_loss, csrc/ctc_loss.hip) against the float64 forward sum of
tests/loss_oracle.py.

Tolerance (tests/test_loss_oracle_cpu.py admits it): |got - ref64| / max(|ref64|, 1) <= numerics.tol(F32_BUDGET, e32), with e32
the float32 numpy walk's error on that very utterance, computed here.

Boundaries of the kernel: emission rows are loaded 16 frames ahead (T = 1, 2, 3, 15 .. 18, 33, 64, 65, 129, 257); a lane owns 4
(blank, token) pairs (L = 3, 4, 5; 252 .. 255), the gather strides over 64 tokens (63, 64, 65; 127, 128, 129) and 255 tokens
fill the wave.

First MI355X run: largest error 9.4e-7 relative (T = 255, L = 127), where the float32 numpy walk has the same 9.4e-7; every
batch-independence and poison comparison bit-exact (NOTES.md section 34).
"""
import numpy as np
import pytest
import torch

import align_oracle as ao
import loss_oracle as lo
import numerics as nm
import poison
from ppasr_amd import _lib
from ppasr_amd.decoders import ctc_alignment as ca
from ppasr_amd.model_utils import loss as ml

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
V = 50
T_LIST = [1, 2, 3, 15, 16, 17, 18, 33, 64, 65, 129, 257]
L_LIST = [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 252, 253, 254, 255]
WORST = {"err": 0.0, "e32": 0.0}


def pack(token_lists, max_tokens=None):
    mt = max([len(t) for t in token_lists] + [0]) if max_tokens is None else max_tokens
    tk = np.full((len(token_lists), mt), -1, np.int32)
    for b, t in enumerate(token_lists):
        tk[b, :min(len(t), mt)] = t[:mt]
    return tk, np.asarray([len(t) for t in token_lists], np.int32)


def run(probs, token_lists, frame_lens=None, blank=0, max_tokens=None, n_tokens=None):
    tk, nt = pack(token_lists, max_tokens)
    out = ml.ctc_nll(torch.as_tensor(probs), tk, nt if n_tokens is None else np.asarray(n_tokens, np.int32),
                     None if frame_lens is None else np.asarray(frame_lens, np.int32), blank)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(got, b, probs, tokens, T, label):
    """status 0 and the value within the tolerance of this very utterance"""
    ref, e32 = MEMO.get(("ref", label, b), lambda: (lo.ctc_nll(probs, tokens, T)[0], lo.ctc_nll(probs, tokens, T, dtype=np.float32)[0]))
    e32 = lo.rel_err(e32, ref)
    tol = nm.tol(nm.F32_BUDGET, e32)
    err = lo.rel_err(got["nll"][b], ref)
    WORST["err"], WORST["e32"] = max(WORST["err"], err), max(WORST["e32"], e32)
    print(f"[ctc_loss] {label} b={b} T={T} L={len(tokens)} ref64={ref:.9g} got={got['nll'][b]:.9g} err={err:.2e} e32={e32:.2e} "
          f"tol={tol:.2e} | worst so far err={WORST['err']:.2e} e32={WORST['e32']:.2e}")
    assert got["status"][b] == 0, (label, b, got["status"][b])
    assert np.isfinite(got["nll"][b]) and err <= tol, (label, b, got["nll"][b], ref, err, tol)


def batches(T):
    """B = 5 per batch, every feasible L of L_LIST at this T, ragged frame_lens; rows past frame_lens are NaN"""
    def make():
        rng = np.random.default_rng(3000 + T)
        Ls = [L for L in L_LIST if L <= T]
        out = []
        for i in range(0, len(Ls), 5):
            group = (Ls[i:i + 5] * 5)[:5]
            probs = np.stack([lo.softmax_table(rng, T, V) for _ in group])
            toks, lens = [], []
            for b, L in enumerate(group):
                Tb = T if b == 0 else max(L, T - int(rng.integers(0, 4)))
                toks.append(lo.random_tokens(rng, L, Tb, V, repeat_p=0.2 if Tb > L else 0.0))
                lens.append(Tb)
                probs[b, Tb:] = np.nan
            out.append((probs, toks, lens))
        return out
    return MEMO.get(("batches", T), make)


@pytest.mark.parametrize("T", T_LIST)
def test_value_against_float64(T):
    for i, (probs, toks, lens) in enumerate(batches(T)):
        got = run(probs, toks, lens)
        for b in range(5):
            check(got, b, probs[b], toks[b], lens[b], f"T={T} batch={i}")


def test_equal_alternating_and_exactly_filling_labels():
    rng = np.random.default_rng(31)
    T = 40
    toks = [[7] * 20, [7] * 10, [3, 9] * 20, [3, 9] * 8, list(rng.integers(1, V, T)), [5] * 1]
    for i in range(1, T):  # a token per frame needs distinct neighbours
        if toks[4][i] == toks[4][i - 1]:
            toks[4][i] = toks[4][i] % (V - 1) + 1
    lens = [39, T, T, 17, T, 1]
    assert [ao.frames_needed(t) for t in toks] == [39, 19, 40, 16, 40, 1]  # 0, 2 and 4 fill their frames exactly
    probs = np.stack([lo.softmax_table(rng, T, V) for _ in toks])
    got = run(probs, toks, lens)
    for b in range(len(toks)):
        check(got, b, probs[b], toks[b], lens[b], "labels")


SPECIALS = [0.0, 1e-40, float(ao.FLT_MIN), 1.0]


def test_zero_denormal_flt_min_and_one_on_and_off_the_label():
    rng = np.random.default_rng(32)
    # (a) on the label: T = frames needed, one alignment only; its entries cycle through the specials and 0.3
    tight = [3, 3, 8, 9, 9, 9, 2, 4, 4, 6, 7, 1]
    ft = ao.left_packed(tight, ao.frames_needed(tight))
    Ta = len(ft)
    pa = lo.softmax_table(rng, Ta, V)
    for t in range(Ta):
        pa[t, 0 if ft[t] < 0 else tight[ft[t]]] = (SPECIALS + [0.3])[t % 5]
    # (b) off the label's best path: the label's columns and the blank hold specials except along one planted path, and
    # 1.0 sits on a symbol that is none of the tokens
    tokens_b = [5, 5, 6, 7, 5]
    labels_b = [0, 5, 5, 0, 5, 6, 6, 7, 0, 0, 5, 0, 0, 0, 0, 0]
    assert len(labels_b) == Ta
    pb = lo.softmax_table(rng, Ta, V)
    k = 0
    for t in range(Ta):
        for col in (0, 5, 6, 7):
            pb[t, col] = 0.9 if col == labels_b[t] else SPECIALS[k % 3]
            k += col != labels_b[t]
        pb[t, 20] = 1.0
    # (c) a table of zeros: every emission is log FLT_MIN
    pc = np.zeros((Ta, V), np.float32)
    probs = np.stack([pa, pb, pc])
    got = run(probs, [tight, tokens_b, [1, 2, 3]])
    for b, tokens in enumerate([tight, tokens_b, [1, 2, 3]]):
        check(got, b, probs[b], tokens, Ta, "range")
    forced = float(-ao.emissions(pa)[np.arange(Ta), [0 if f < 0 else tight[f] for f in ft]].sum())
    assert abs(got["nll"][0] - forced) <= 2e-5 * forced  # (a) has one alignment: the sum is that path


def test_infeasible_and_bad_input_leave_their_neighbours_alone():
    rng = np.random.default_rng(33)
    T = 20
    specs = [(6, T), (0, 0), (11, 17), (3, T)]
    good = [lo.random_tokens(rng, L, Tg, V) if L else [] for L, Tg in specs]
    lens_good = [Tg for _, Tg in specs]
    probs_good = np.stack([lo.softmax_table(rng, T, V) for _ in good])
    rep = [4, 4, 4, 9]  # needs 6 frames
    extra = lo.softmax_table(rng, T, V)
    order = [("g", 0), ("x", rep, 5, None), ("g", 1), ("x", [3, V, 5], T, None), ("g", 2), ("x", [3, -1], T, None),
             ("x", [3, 0, 5], T, None), ("g", 3), ("x", [1, 2], T, 12), ("x", [1, 2], T, -1)]
    probs, toks, lens, nt = [], [], [], []
    for o in order:
        if o[0] == "g":
            probs.append(probs_good[o[1]]), toks.append(good[o[1]]), lens.append(lens_good[o[1]]), nt.append(len(good[o[1]]))
        else:
            probs.append(extra), toks.append(o[1]), lens.append(o[2]), nt.append(len(o[1]) if o[3] is None else o[3])
    mt = 11
    mixed = run(np.stack(probs), toks, lens, max_tokens=mt, n_tokens=nt)
    want = [0, 1, 0, 2, 0, 2, 2, 0, 2, 2]
    assert mixed["status"].tolist() == want
    assert all(mixed["nll"][b] == np.inf for b, st in enumerate(want) if st)
    together = run(probs_good, good, lens_good, max_tokens=mt)
    for g, b in enumerate([0, 2, 4, 7]):
        solo = run(probs_good[g:g + 1], [good[g]], [lens_good[g]], max_tokens=mt)
        for k in ("nll", "status"):
            assert mixed[k][b].tobytes() == solo[k][0].tobytes() == together[k][g].tobytes(), (k, b)
        if lens_good[g]:
            check(solo, 0, probs_good[g], good[g], lens_good[g], f"mixed {g}")
    assert together["nll"][1] == 0.0 and together["status"][1] == 0  # L = 0 with T = 0
    again = run(np.stack(probs), toks, lens, max_tokens=mt, n_tokens=nt)
    assert again["nll"].tobytes() == mixed["nll"].tobytes()  # the same bits on any two calls
    assert run(extra[None], [rep], [6])["status"][0] == 0  # one frame more and the same transcript fits


def test_max_tokens_zero_no_frames_and_refusals():
    rng = np.random.default_rng(34)
    probs = np.stack([lo.softmax_table(rng, 9, V) for _ in range(3)])
    got = run(probs, [[], [], []], [9, 4, 0])
    assert got["status"].tolist() == [0, 0, 0] and got["nll"][2] == 0.0
    for b, T in enumerate([9, 4]):
        check(got, b, probs[b], [], T, "max_tokens=0")
    got = run(np.zeros((2, 0, V), np.float32), [[], [3]], None)  # Tp = 0: a valid call
    assert got["status"].tolist() == [0, 1] and got["nll"][0] == 0.0 and got["nll"][1] == np.inf
    with pytest.raises(_lib.PPASRHipError) as e:
        run(probs, [[1] * 256, [], []])
    assert e.value.status == _lib.PPASR_EUNSUPPORTED
    lib = _lib.load()
    assert lib.ppasr_ctc_loss_workspace_bytes(1, 4, 256) == 0 and lib.ppasr_ctc_loss_workspace_bytes(0, 4, 3) == 0
    p = torch.from_numpy(probs).cuda()
    tk, nt = (torch.from_numpy(a).cuda() for a in pack([[1], [2], [3]]))
    nll = torch.empty(3, dtype=torch.float32, device="cuda")
    st = torch.empty(3, dtype=torch.int32, device="cuda")
    need = lib.ppasr_ctc_loss_workspace_bytes(3, 9, 1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    args = lambda **kw: [kw.get("p", p.data_ptr()), None, 3, 9, kw.get("V", V), kw.get("blank", 0), tk.data_ptr(), nt.data_ptr(), 1,
                         kw.get("nll", nll.data_ptr()), st.data_ptr(), ws.data_ptr(), kw.get("need", need), None]
    assert lib.ppasr_ctc_loss(*args()) == _lib.PPASR_OK
    for kw in (dict(need=need - 1), dict(p=None), dict(nll=None), dict(blank=V), dict(blank=-1), dict(V=1)):
        assert lib.ppasr_ctc_loss(*args(**kw)) == _lib.PPASR_EINVAL, kw
    torch.cuda.synchronize()


def test_full_vocabulary():
    Vf, B, T, L = 4233, 2, 64, 40
    rng = np.random.default_rng(35)
    probs = np.stack([lo.softmax_table(rng, T, Vf) for _ in range(B)])
    toks = [lo.random_tokens(rng, L, T, Vf) for _ in range(B)]
    toks[1][-1] = Vf - 1  # the last column of the table
    if toks[1][-2] == Vf - 1:
        toks[1][-2] = Vf - 2
    got = run(probs, toks)
    for b in range(B):
        check(got, b, probs[b], toks[b], T, "full-vocabulary")


def test_the_sum_contains_the_best_path():
    """nll <= -score of ppasr_ctc_align on the same input, plus the two tolerances"""
    for probs, toks, lens in batches(65) + batches(17):
        got = run(probs, toks, lens)
        tk, nt = pack(toks)
        al = ca.ctc_align_ids(torch.as_tensor(probs), tk, nt, np.asarray(lens, np.int32))
        score = al["score"].cpu().numpy()
        assert (al["status"].cpu().numpy() == 0).all()
        for b in range(len(toks)):
            ref = ao.align(probs[b], toks[b], lens[b])
            slack = ao.tolerance(lens[b], ref["abs_log"]) + nm.F32_BUDGET * max(abs(float(score[b])), 1.0)
            assert got["nll"][b] <= -score[b] + slack, (b, got["nll"][b], -score[b], slack)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_no_result_depends_on_buffer_contents(pattern, monkeypatch):
    cases = batches(64) + batches(17)
    other = batches(129)[-1]

    def go(s):
        if s.pattern == "zero":
            ml.scratch._ws.clear()  # the clean reference starts without kept scratch, like a fresh process
        if s.stale:
            tk, nt = pack(other[1])
            ml.ctc_nll(torch.as_tensor(other[0]), tk, nt, np.asarray(other[2], np.int32))
        outs = {}
        for i, (probs, toks, lens) in enumerate(cases):
            s.scratch(ml.scratch)
            tk, nt = pack(toks)
            out = ml.ctc_nll(torch.as_tensor(probs), tk, nt, np.asarray(lens, np.int32))
            s.observe(ml.scratch, f"batch {i}")
            torch.cuda.synchronize()
            outs.update({f"{i}/{k}": out[k] for k in ("nll", "status")})
        return outs, ml.scratch

    poison.check("ctc_loss", go, pattern, monkeypatch, MEMO)
