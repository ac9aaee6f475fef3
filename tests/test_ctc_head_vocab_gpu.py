"""The CTC head at vocabulary edges, on exact ties and at extreme logits (csrc/ctc_head_kernels.hip), through the model
classes only.

Vocabulary matrix (head_cases.VOCABS): both sides of a tile (32), of a wave's second tile (256), of the row softmax's
register forms (2048 -> <8>, 5120 -> <20>, above: <0>) and of 256 tiles (8193: a split head capped at 32 slices makes a
second pass); V = 2 and 33 leave slices and waves without a tile.  Every V runs unsplit (set_ffn_split(0): the library
takes no 1), split (8) and with the automatic choice, with the logits tap (k_ctc_head<true> + k_softmax_row_wg) and without
(k_ctc_head<false>, the greedy route); which kernels ran is read back (kernel_profile) and asserted.  The other call sites
-- stream chunks, Squeezeformer, Efficient-Conformer, the general layer route's dense head and DeepSpeech2's, the fp16 x3
head -- run at V = 33 / 257 / 2049 / 5121.

Against the float64 oracle (numerics.oracle64): utt_rel of the logits, logprob_err of the probabilities and frame_maxprob
under the same log-space rule, all below the family's budget; frame_ids_ok; exact output shapes; everything finite.
Against itself: frame_argmax equals numpy's first-index argmax of the array the route ranks (its own logits on the fused
head, its own probabilities where k_frame_argmax ranks those) on EVERY row, the greedy tokens are the collapse of those
ids and the score is the float64 mean of frame_maxprob over the non-blank frames x 100.

Tie sets (head_cases.tie_sets, one model each): the planted columns' logits are bit-equal, they are the row maximum of
every frame and the head names the lowest of them -- unsplit, split, on a stream chunk and in the fp16 x3 mode.
tests/test_ctc_head_cases_cpu.py shows that these sets tell a spoilt tie rule at any of the four merge stages from the
right one.  A row that ties as a whole gives id 0 and 1 / V everywhere; heads scaled x8 / x32 (several hundred nats) keep
the budgets, saturate frame_maxprob to exactly 1, underflow to exact zeros and keep the rows' sums as close to 1 as the
fp32 softmax of the CPU does.

Every case prints its worst error as `[head] ...`; NOTES.md section 2.2 carries the table."""
import numpy as np
import pytest
import torch

import head_cases as hc
import numerics as nm
from ppasr_amd import _lib

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
WORST = {}  # group -> (worst error / budget, error, what)

# (B, T'): M = B T' = 1, 33, 31, 32 output rows (M % 32 = 1, 31, 0 and a single row)
SHAPES = [(1, 1), (3, 11), (1, 31), (2, 16)]
SITE_VOCABS = (33, 257, 2049, 5121)


def _budget(family):
    return nm.F32_BUDGET_DS2 if family == "deepspeech2" else nm.F32_BUDGET


def _note(group, err, budget, what):
    if err / budget >= WORST.get(group, (-1.0,))[0]:
        WORST[group] = (err / budget, err, what)
    w = WORST[group]
    print(f"[head] {group}: {what}: {err:.2e} (group worst {w[1]:.2e} = {w[0]:.2f} x budget)")


def _base_sd(family, V):
    return MEMO.get(("sd", family, V), lambda: hc.head_sd(family, V))


def _base_model(family, V):
    return MEMO.get(("model", family, V), lambda: hc.make_model(family, _base_sd(family, V)))


def _ref_logits(family, sd, x, lens, key):
    """float64 logits of `sd` ([B, T', V]; DeepSpeech2: log-probabilities, and the valid output lengths with them)"""
    def run():
        o = nm.oracle64(hc.oracle_family(family), sd, **hc.oracle_kw(family))
        if family == "deepspeech2":
            p, rl, _, _ = o.forward(x, lens)
            return torch.log(p), rl
        return o.get_encoder_out(x, lens, return_logits=True)[1], None
    return MEMO.get(("ref", family) + key, run)


def _unified(ref, cols):
    """float64 logits of a model with a planted set.  The set's members are ONE number (same weights, same bias), but a
    CPU matmul may run the last columns of an odd width through another code path and round them apart in the last bit
    (seen: 3.6e-15 .. 1.4e-14 at logits of 30 .. 80, only on sets that reach into the last columns, and not on every
    CPU).  numerics.frame_ids_ok would read that as an order among the members, so the set carries the value of its lowest
    column; the difference this removes is printed."""
    off = max(float((ref[..., c] - ref[..., min(cols)]).abs().max()) for c in cols)
    if off:
        assert off <= 8 * 2.0 ** -52 * float(ref.abs().max()), (cols, off)  # last bits, nothing else
        print(f"[head] NOTE float64 oracle: planted columns {list(cols)} differ by {off:.1e} among themselves; unified")
        ref = ref.clone()
        for c in cols:
            ref[..., c] = ref[..., min(cols)]
    return ref


def _tie_ref(family, sd, x, lens, key, cols):
    ref, rl = _ref_logits(family, sd, x, lens, key)
    return _unified(ref, cols), rl


def _boost(family, V, x, lens, key):
    """twice the float64 oracle's max |logit| of the unedited model on this input (DeepSpeech2: |log-probability|, which
    bounds the spread of its logits)"""
    return 2.0 * float(_ref_logits(family, _base_sd(family, V), x, lens, ("base", V) + key)[0].abs().max())


def _ran(kernels):
    return {k.split("(")[0].replace("void ", "").replace("ppasr::", "").strip() for k in kernels}


def _softmax_form(V):
    return "k_softmax_row_wg<8>" if V <= 2048 else "k_softmax_row_wg<20>" if V <= 5120 else "k_softmax_row_wg<0>"


def _log_softmax64(ref):
    r = ref.detach().cpu().to(torch.float64).numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    m = r.max(-1, keepdims=True)
    return r - m - np.log(np.exp(r - m).sum(-1, keepdims=True))


def _maxprob_err(fp, ref_logits, lens_out=None):
    """frame_maxprob against exp(max - logsumexp) of the float64 logits, by the rule of numerics.logprob_err: in log
    space, clipped at LOG_FLOOR, worst utterance of the largest difference over that utterance's logit scale"""
    lp = _log_softmax64(ref_logits)
    got = np.log(np.maximum(fp.detach().cpu().to(torch.float64).numpy(), np.exp(nm.LOG_FLOOR)))
    worst = 0.0
    for b in range(lp.shape[0]):
        n = lp.shape[1] if lens_out is None else min(int(lens_out[b]), lp.shape[1])
        if n <= 0:
            continue
        r = lp[b, :n]
        scale = max(float(np.abs(r - r.mean(-1, keepdims=True)).max()), 1e-30)
        worst = max(worst, float(np.abs(got[b, :n] - np.maximum(r.max(-1), nm.LOG_FLOOR)).max() / scale))
    return worst


def _check_greedy(tokens, n_tok, score, fa, fp, what, lens_out=None):
    """tokens = collapse of the frame ids, score = float64 mean of frame_maxprob over the non-blank frames x 100"""
    fa, fp = fa.cpu().numpy(), fp.cpu().numpy()
    for b in range(fa.shape[0]):
        n = fa.shape[1] if lens_out is None else int(lens_out[b])
        ids = fa[b, :n]
        assert np.array_equal(tokens[b, :int(n_tok[b])].cpu().numpy(), nm.collapse(ids)), (what, b)
        assert bool((tokens[b, int(n_tok[b]):] == -1).all()), (what, b)
        nb = fp[b, :n][ids != 0].astype(np.float64)
        want = float(nb.mean()) * 100 if nb.size else 0.0
        assert abs(float(score[b]) - want) <= 1e-9 * max(1.0, want), (what, b, float(score[b]), want)


def _frames(model, x, lens, tap):
    """ppasr_encode with the frame outputs: tap = True -> (probs, logits, frame_argmax, frame_maxprob), the head with the
    logits tap and the row softmax behind it; False -> (frame_argmax, frame_maxprob), the call encode_greedy makes"""
    sp, ln = model._prep(x, lens)
    B, T, _ = sp.shape
    Tp = model.out_frames(T)
    fa = torch.full((B, Tp), -7, dtype=torch.int32, device=model.device)
    fp = torch.full((B, Tp), -7.0, dtype=torch.float32, device=model.device)
    if not tap:
        with torch.cuda.device(model.device):
            model._encode(sp, ln, fa=fa, fp=fp)
        return fa, fp
    probs = torch.full((B, Tp, model.vocab_size), -7.0, dtype=torch.float32, device=model.device)
    logits = torch.full_like(probs, -7.0)
    with torch.cuda.device(model.device):
        model._encode(sp, ln, probs=probs, logits=logits, fa=fa, fp=fp)
    return probs, logits, fa, fp


def _check_encode(family, model, x, lens, ref, what, group, ranks="logits", tie=None, uniform=False, expect=(), forbid=()):
    """one input through get_encoder_out(return_logits=True), encode_greedy and the two frame forms of ppasr_encode;
    every assertion of the module docstring -> (logits, probs, frame_maxprob) as numpy arrays.  ranks: the array the route's
    argmax reads ("logits": the fused head; "probs": k_frame_argmax behind the dense head).  tie: planted columns."""
    budget = _budget(family)
    V = model.vocab_size
    with _lib.kernel_profile() as kp:
        probs, logits = model.get_encoder_out(x, lens, return_logits=True)
        tokens, n_tok, score = model.encode_greedy(x, lens)
        fa0, fp0 = _frames(model, x, lens, tap=False)
        probs1, logits1, fa1, fp1 = _frames(model, x, lens, tap=True)
        torch.cuda.synchronize()
    ran = _ran(kp.kernels)
    for k in expect:
        assert k in ran, (what, k, sorted(ran))
    for k in forbid:
        assert k not in ran, (what, k, sorted(ran))
    B, Tp = ref.shape[0], ref.shape[1]
    assert tuple(logits.shape) == tuple(probs.shape) == (B, Tp, V) == tuple(ref.shape), (what, logits.shape, ref.shape)
    assert tuple(fa0.shape) == (B, Tp)
    for t in (probs, logits, probs1, logits1, fp0, fp1):
        assert bool(torch.isfinite(t).all()), what
    assert torch.equal(logits, logits1) and torch.equal(probs, probs1), what  # the same launches, with or without frames
    lg, pr = logits.cpu().numpy(), probs.cpu().numpy()
    # ---- the planted set (before the comparisons that a broken set would only blur)
    if tie is not None:
        same = all(np.array_equal(lg[..., c], lg[..., tie[0]]) for c in tie[1:])
        if ranks == "logits":
            assert same, (what, "planted columns differ", tie,
                          [float(np.abs(lg[..., c] - lg[..., tie[0]]).max()) for c in tie[1:]])
        assert bool((lg[..., tie[0]] == lg.max(-1)).all()), (what, "planted set is not the row maximum")
        if same and (ranks == "logits" or all(np.array_equal(pr[..., c], pr[..., tie[0]]) for c in tie[1:])):
            assert bool((fa0.cpu().numpy() == min(tie)).all()) and bool((fa1.cpu().numpy() == min(tie)).all()), \
                (what, tie, np.unique(fa0.cpu().numpy()))
        else:  # (a dense head may order K differently per column block: the argmax(own output) assertion above stands)
            print(f"[head] FINDING {family} V={V} {what}: the planted columns {tie} are not bit-equal on this route")
    # ---- against float64
    e_l = nm.utt_rel(logits, ref)
    ok, near = nm.frame_ids_ok(logits, ref, budget)
    errs = [e_l, _maxprob_err(fp0, ref), _maxprob_err(fp1, ref)] if not uniform else [e_l]
    if not uniform:
        errs.append(nm.logprob_err(probs, ref))
    _note(group, max(errs), budget, f"{family} V={V} {what} near-ties {near}")
    assert max(errs) < budget, (what, errs)
    assert ok, what
    # ---- against itself: the ids of EVERY row are numpy's first-index argmax of what the route ranks
    own = (lg if ranks == "logits" else pr).argmax(-1)
    assert np.array_equal(fa0.cpu().numpy(), own), (what, "greedy form", np.nonzero(fa0.cpu().numpy() != own))
    assert np.array_equal(fa1.cpu().numpy(), own), (what, "tap form", np.nonzero(fa1.cpu().numpy() != own))
    if ranks == "probs":
        assert np.array_equal(fp1.cpu().numpy(), pr.max(-1)), what
    _check_greedy(tokens, n_tok, score, fa0, fp0, what)
    return lg, pr, fp0.cpu().numpy()


class _Split:
    """set_ffn_split(mode) for one block, the default afterwards"""

    def __init__(self, model, mode):
        self.model, self.mode = model, mode

    def __enter__(self):
        self.model.set_ffn_split(self.mode)

    def __exit__(self, *exc):
        self.model.set_ffn_split(-1)
        return False


def _head_kernels(V, split, h3=False):
    """-> (kernels that must have run, kernels that must not) on the fused Conformer head"""
    head = "k_ctc_head_h3" if h3 else "k_ctc_head"
    expect = [head + "<true>", head + "<false>", _softmax_form(V)]
    other = [f for f in ("k_softmax_row_wg<8>", "k_softmax_row_wg<20>", "k_softmax_row_wg<0>") if f != _softmax_form(V)]
    other += ["k_frame_argmax", ("k_ctc_head" if h3 else "k_ctc_head_h3") + "<true>"]
    if split == 0:
        return expect, other + ["k_ctc_merge"]
    return expect + ["k_ctc_merge"], other  # (8, and the automatic choice: these cases have at most 4 row blocks)


# ---- the vocabulary matrix on the fused Conformer head ---------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 8, -1])
@pytest.mark.parametrize("V", hc.VOCABS)
def test_vocabulary_matrix(V, split):
    model = _base_model("conformer", V)
    expect, forbid = _head_kernels(V, split)
    with _Split(model, split):
        for B, Tp in SHAPES:
            x, lens = hc.inputs("conformer", B, Tp, 100 + Tp)
            ref, _ = _ref_logits("conformer", _base_sd("conformer", V), x, lens, ("base", V, B, Tp))
            ny = 1 if split == 0 else hc.split_slices(V, B * Tp)
            _check_encode("conformer", model, x, lens, ref, f"split={split} ({ny} slices) B={B} T'={Tp}", "vocabulary matrix",
                          expect=expect, forbid=forbid)


# ---- the other call sites ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["squeezeformer", "efficient_conformer"])
@pytest.mark.parametrize("V", SITE_VOCABS)
def test_other_fused_families(family, V):
    model = _base_model(family, V)
    for B, Tp in [(3, 11), (1, 31)]:
        x, lens = hc.inputs(family, B, Tp, 200 + Tp)
        ref, _ = _ref_logits(family, _base_sd(family, V), x, lens, ("base", V, B, Tp))
        assert ref.shape[1] == Tp
        _check_encode(family, model, x, lens, ref, f"B={B} T'={Tp}", f"{family} batched",
                      expect=["k_ctc_head<true>", "k_ctc_head<false>", _softmax_form(V)], forbid=["k_frame_argmax"])


@pytest.mark.parametrize("V", SITE_VOCABS)
def test_general_route_dense_head(V):
    """width 512: the vocabulary padded to 256 columns, the dense layer, then k_softmax_row_wg + k_frame_argmax"""
    model = _base_model("general", V)
    with pytest.raises(_lib.PPASRHipError) as e:
        model.set_gemm_mode("f16x3")
    assert e.value.status == _lib.PPASR_EUNSUPPORTED
    for B, Tp in [(3, 11), (1, 31)]:
        x, lens = hc.inputs("general", B, Tp, 300 + Tp)
        ref, _ = _ref_logits("general", _base_sd("general", V), x, lens, ("base", V, B, Tp))
        _check_encode("general", model, x, lens, ref, f"B={B} T'={Tp}", "general route", ranks="probs",
                      expect=["k_frame_argmax", _softmax_form(V)],
                      forbid=["k_ctc_head<true>", "k_ctc_head<false>", "k_ctc_merge"])


def _check_ds2(model, sd, x, lens, key, what, tie=None):
    from ppasr_amd.decoders.ctc_greedy_decoder import greedy_decode_ids
    V = model.vocab_size
    ref, rl = _ref_logits("deepspeech2", sd, x, lens, key)
    with _lib.kernel_profile() as kp:
        probs = model.get_encoder_out(x, lens)
        tokens, n_tok, score, fa, fp = greedy_decode_ids(probs)
        torch.cuda.synchronize()
    ran = _ran(kp.kernels)
    assert _softmax_form(V) in ran and "k_frame_argmax" in ran, sorted(ran)
    assert tuple(probs.shape) == tuple(ref.shape) and probs.shape[2] == V
    assert bool(torch.isfinite(probs).all()) and bool((probs >= 0).all())
    errs = [nm.utt_rel(probs, torch.exp(ref), rl), nm.logprob_err(probs, ref, rl), _maxprob_err(fp, ref, rl)]
    _note("deepspeech2", max(errs), nm.F32_BUDGET_DS2, f"V={V} {what}")
    assert max(errs) < nm.F32_BUDGET_DS2, (what, errs)
    assert nm.frame_ids_ok(torch.log(probs.cpu()), ref, nm.F32_BUDGET_DS2, rl)[0], what
    pr = probs.cpu().numpy()
    assert np.array_equal(fa.cpu().numpy(), pr.argmax(-1)) and np.array_equal(fp.cpu().numpy(), pr.max(-1)), what
    _check_greedy(tokens, n_tok, score, fa, fp, what)
    if tie is not None:
        valid = [(b, t) for b in range(pr.shape[0]) for t in range(min(int(rl[b]), pr.shape[1]))]
        rows = np.array([pr[b, t] for b, t in valid])
        assert bool((rows[:, tie[0]] == rows.max(-1)).all()), (what, "planted set is not the row maximum")
        if all(np.array_equal(rows[:, c], rows[:, tie[0]]) for c in tie[1:]):
            assert bool((np.array([fa.cpu().numpy()[b, t] for b, t in valid]) == min(tie)).all()), (what, tie)
        else:
            print(f"[head] FINDING deepspeech2 V={V} {what}: the planted columns {tie} are not bit-equal on this route")


@pytest.mark.parametrize("V", SITE_VOCABS)
def test_deepspeech2_dense_head(V):
    model = _base_model("deepspeech2", V)
    for B, Tp in [(3, 11), (1, 31)]:
        x, lens = hc.inputs("deepspeech2", B, Tp, 400 + Tp)
        _check_ds2(model, _base_sd("deepspeech2", V), x, lens, ("base", V, B, Tp), f"B={B} T'={Tp}")


def _chunk_refs(sd, x, windows, required=32):
    o = nm.oracle64("conformer", sd, **hc.oracle_kw("conformer"))
    refs, att, cnn, offset = [], None, None, 0
    for a, b in windows:
        with torch.no_grad():
            xs, att, cnn = o.forward_chunk(x[:, a:b], offset, required, att, cnn)
            refs.append(o.ctc_logits(xs))
        offset += refs[-1].shape[1]
    return refs


CHUNK_WINDOWS = [(0, 163), (160, 227)]  # 40 output frames (two row blocks), then 16 (one row block: the wide slice rule)


def _check_chunks(model, sd, key, what, group, tie=None):
    """a stream handle fed CHUNK_WINDOWS with frame outputs; the chunk route returns no logits, so the ids are held to the
    probabilities: the id's probability is the row maximum, and where that maximum is unique the id is its column"""
    V = model.vocab_size
    x, _ = hc.synth_features(1, CHUNK_WINDOWS[-1][1], seed=77)
    refs = MEMO.get(("chunks",) + key, lambda: _chunk_refs(sd, x, CHUNK_WINDOWS))
    if tie is not None:
        refs = [_unified(r, tie) for r in refs]
    stream = model.new_stream()
    for (a, b), ref in zip(CHUNK_WINDOWS, refs):
        with _lib.kernel_profile() as kp:
            probs, fa, fp = stream.encode_chunk(x[:, a:b], 32, want_frames=True)
            torch.cuda.synchronize()
        ran = _ran(kp.kernels)
        c = ref.shape[1]
        slices = min((hc.n_tiles(V) + 7) // 8, 32) if c <= 32 else 8
        assert "k_ctc_head<true>" in ran and _softmax_form(V) in ran, sorted(ran)
        assert ("k_ctc_merge" in ran) == (slices > 1), (what, c, slices, sorted(ran))
        assert tuple(probs.shape) == (1, c, V) == tuple(ref.shape) and tuple(fa.shape) == (1, c), (what, probs.shape)
        assert bool(torch.isfinite(probs).all()) and bool((probs >= 0).all()) and bool(torch.isfinite(fp).all())
        errs = [nm.utt_rel(probs, torch.softmax(ref, -1)), nm.logprob_err(probs, ref), _maxprob_err(fp, ref)]
        _note(group, max(errs), nm.F32_BUDGET, f"V={V} {what} chunk of {c} frames ({slices} slices)")
        assert max(errs) < nm.F32_BUDGET, (what, c, errs)
        assert nm.frame_ids_ok(torch.log(probs.cpu().double().clamp_min(1e-300)), ref, nm.F32_BUDGET)[0], (what, c)
        pr, ids = probs.cpu().numpy()[0], fa.cpu().numpy()[0]
        top = pr.max(-1)
        assert np.array_equal(pr[np.arange(c), ids], top), (what, c)
        unique = (pr == top[:, None]).sum(-1) == 1
        assert np.array_equal(ids[unique], pr.argmax(-1)[unique]), (what, c)
        if tie is not None:
            for col in tie[1:]:
                assert np.array_equal(pr[:, col], pr[:, tie[0]]), (what, c, col)
            assert bool((pr[:, tie[0]] == top).all()) and bool((ids == min(tie)).all()), (what, c, tie, np.unique(ids))


@pytest.mark.parametrize("V", SITE_VOCABS)
def test_conformer_stream_chunks(V):
    _check_chunks(_base_model("conformer", V), _base_sd("conformer", V), ("base", V), "stream", "conformer chunks")


# ---- the fp16 x3 head ---------------------------------------------------------------------------------------------------
class _F16x3:
    """the handle in the fp16 x3 mode with the head covered; no guard event may be counted inside"""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.model.set_gemm_mode("f16x3")
        assert "head" in self.model.gemm_coverage(), self.model.gemm_coverage()
        self.before = self.model.gemm_guard_stats()

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                assert self.model.gemm_guard_stats() == self.before, (self.before, self.model.gemm_guard_stats())
        finally:
            self.model.set_gemm_mode("f32")
        return False


@pytest.mark.parametrize("split", [0, 8])
@pytest.mark.parametrize("V", [33, 257, 5121])
def test_f16x3_head(V, split):
    """k_ctc_head_h3: the mode's bound is fp32's own budget with no guard event (tests/test_fp64_routes_gpu.py)"""
    model = _base_model("conformer", V)
    expect, forbid = _head_kernels(V, split, h3=True)
    with _Split(model, split), _F16x3(model):
        for B, Tp in [(3, 11), (1, 31), (2, 16)]:
            x, lens = hc.inputs("conformer", B, Tp, 100 + Tp)
            ref, _ = _ref_logits("conformer", _base_sd("conformer", V), x, lens, ("base", V, B, Tp))
            _check_encode("conformer", model, x, lens, ref, f"f16x3 split={split} B={B} T'={Tp}", "fp16 x3 head",
                          expect=expect, forbid=forbid)


# ---- tie sets -------------------------------------------------------------------------------------------------------------
TIE_ROWS = 33  # B = 3, T' = 11


def _tie_cases(vocabs):
    out = []
    for V in vocabs:
        sets = dict(hc.tie_sets(V, 1))
        sets.update(hc.tie_sets(V, hc.split_slices(V, TIE_ROWS)))
        out += [(V, name, tuple(cols)) for name, cols in sorted(sets.items())]
    return out


@pytest.mark.parametrize("V,name,cols", _tie_cases(hc.TIE_VOCABS), ids=lambda v: str(v) if not isinstance(v, tuple) else "set")
def test_tie_sets_on_the_fused_head(V, name, cols):
    """one model per set: unsplit, split, fp16 x3 (both) and the chunk route"""
    x, lens = hc.inputs("conformer", 3, 11, 111)
    boost = _boost("conformer", V, x, lens, (3, 11))
    sd = hc.plant_tie(_base_sd("conformer", V), "conformer", list(cols), boost)
    model = hc.make_model("conformer", sd)
    ref, _ = _tie_ref("conformer", sd, x, lens, ("tie", V, name), cols)
    own = [hc.owner(c, V, hc.split_slices(V, TIE_ROWS)) for c in cols]
    print(f"[head] tie set V={V} {name}: columns {list(cols)} boost {boost:.1f} owners (slice, wave, pass, half, register) {own}")
    for split in (0, 8):
        with _Split(model, split):
            _check_encode("conformer", model, x, lens, ref, f"tie {name} split={split}", "tie sets", tie=list(cols),
                          expect=_head_kernels(V, split)[0], forbid=_head_kernels(V, split)[1])
            with _F16x3(model):
                _check_encode("conformer", model, x, lens, ref, f"tie {name} f16x3 split={split}", "tie sets, fp16 x3",
                              tie=list(cols), expect=_head_kernels(V, split, h3=True)[0])
    _check_chunks(model, sd, ("tie", V, name), f"tie {name}", "tie sets, chunks", tie=list(cols))


@pytest.mark.parametrize("V,name,cols", _tie_cases((257,)), ids=lambda v: str(v) if not isinstance(v, tuple) else "set")
@pytest.mark.parametrize("family", ["general", "deepspeech2"])
def test_tie_sets_on_the_dense_heads(family, V, name, cols):
    x, lens = hc.inputs(family, 3, 11, 112)
    boost = _boost(family, V, x, lens, (3, 11, "dense"))
    sd = hc.plant_tie(_base_sd(family, V), family, list(cols), boost)
    model = hc.make_model(family, sd)
    if family == "deepspeech2":
        _check_ds2(model, sd, x, lens, ("tie", V, name), f"tie {name}", tie=list(cols))
    else:
        ref, _ = _tie_ref(family, sd, x, lens, ("tie", V, name), cols)
        _check_encode(family, model, x, lens, ref, f"tie {name}", "tie sets, general route", ranks="probs", tie=list(cols),
                      expect=["k_frame_argmax"])


# ---- a row that ties as a whole -----------------------------------------------------------------------------------------
def _ulps(a, want):
    a = np.asarray(a, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - np.float32(want).view(np.int32).astype(np.int64)).max()


@pytest.mark.parametrize("V", [2, 33, 257, 5121, 8193])
def test_whole_row_tie(V):
    """ctc_lo = 0: every frame a V-way tie -> id 0, every probability and frame_maxprob 1 / V (2 ulp), nothing decoded"""
    sd = hc.uniform_head(_base_sd("conformer", V), "conformer")
    model = hc.make_model("conformer", sd)
    x, lens = hc.inputs("conformer", 3, 11, 113)
    ref = torch.zeros(3, 11, V, dtype=torch.float64)
    for split in (0, 8):
        with _Split(model, split):
            lg, pr, fp = _check_encode("conformer", model, x, lens, ref, f"uniform split={split}", "whole-row tie", uniform=True,
                                       expect=_head_kernels(V, split)[0])
            tokens, n_tok, score = model.encode_greedy(x, lens)
            probs_c, fa_c, fp_c = model.new_stream().encode_chunk(x[:1, :67], 32, want_frames=True)
        assert not lg.any()
        u = max(_ulps(pr, 1.0 / V), _ulps(fp, 1.0 / V), _ulps(probs_c.cpu().numpy(), 1.0 / V), _ulps(fp_c.cpu().numpy(), 1.0 / V))
        print(f"[head] whole-row tie V={V} split={split}: probabilities and frame_maxprob within {u} ulp of 1 / V")
        assert u <= 2, (V, split, u)
        assert not fa_c.cpu().numpy().any()
        assert not n_tok.cpu().numpy().any() and bool((tokens == -1).all()) and not score.cpu().numpy().any()


# ---- scaled heads ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [8, 32])
@pytest.mark.parametrize("V", [257, 5121])
def test_scaled_heads(V, factor):
    sd = hc.scaled_head(_base_sd("conformer", V), "conformer", factor)
    model = hc.make_model("conformer", sd)
    x, lens = hc.inputs("conformer", 3, 11, 114)
    ref, _ = _ref_logits("conformer", sd, x, lens, ("scaled", V, factor))
    lp = _log_softmax64(ref)
    top2 = np.sort(ref.numpy(), -1)[..., -2:]
    saturated = (top2[..., 1] - top2[..., 0]) > 104.0
    for split in (0, 8):
        with _Split(model, split):
            lg, pr, fp = _check_encode("conformer", model, x, lens, ref, f"x{factor} split={split}", f"scaled heads x{factor}",
                                       expect=_head_kernels(V, split)[0], forbid=_head_kernels(V, split)[1])
        assert bool((fp[saturated] == 1.0).all()) and bool((pr.max(-1)[saturated] == 1.0).all()), (V, factor, split)
        assert bool((pr >= 0).all()) and bool((fp > 0).all())
        # below the smallest fp32 denormal (e^-103.3) by more than the budget moves a logit: an exact zero
        gone = lp < -105.0
        assert not pr[gone].any(), (V, factor, split)
        # the rows' sums, in float64, against the fp32 softmax of the same logits on the CPU
        cpu = torch.softmax(torch.from_numpy(lg), -1).numpy()
        dev_gpu = np.abs(pr.astype(np.float64).sum(-1) - 1.0).max()
        dev_cpu = np.abs(cpu.astype(np.float64).sum(-1) - 1.0).max()
        print(f"[head] scaled x{factor} V={V} split={split}: max |logit| {np.abs(lg).max():.0f}, saturated frames "
              f"{int(saturated.sum())} of {saturated.size}, exact zeros {int((pr == 0).sum())} (required {int(gone.sum())}), "
              f"row sums off by {dev_gpu:.2e} (CPU fp32 softmax {dev_cpu:.2e})")
        assert dev_gpu <= 4 * dev_cpu, (V, factor, split, dev_gpu, dev_cpu)
