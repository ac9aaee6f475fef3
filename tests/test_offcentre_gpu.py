"""Every encoder route against the float64 oracle on off-centre and saturated checkpoints (tests/offcentre_cases.py): rows
whose |mean| is tens to hundreds of their standard deviation at the LayerNorms, swish / GLU / gate pre-activations past the
fp32 range of exp.  The randomly initialised checkpoints of every other test are centred and run every activation in its
linear range, so they cannot tell a two-pass LayerNorm from a one-pass one.

Per case: utt_rel, logprob_err and frame_ids_ok per utterance at tol(case) = max(family budget, 4 x e32(case)), capped
at numerics.TOL_CAP (e32 = the fp32 oracle against the float64 oracle on the case's own inputs, computed here), every output
finite, final states / stream caches where the route has them; the measured error is printed.

DeepSpeech2: the wavefront route (k_lstm_wave, unidirectional B >= 4 and every session group) applies the previous layer's
LayerNorm through a fold on the raw row; the controls (B = 1 persistent and per-step, B = 3, bidirectional) normalise
with the two-pass k_ln_wide.  kernel_profile pins which of them ran.  With the fold on the unshifted row (before the
per-row pivot, csrc/ds2_kernels.hip) the wavefront cases measured 8 - 32 x tol on the MI355X; figures in NOTES.md section 24."""
import os

import numpy as np
import pytest
import torch

import numerics as nm
import offcentre_cases as oc
from ppasr_amd import _lib
from ppasr_amd.utils.synth import synth_features

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()


def _focus(case):
    """one case's model, oracles and references at a time (H = 1024 .. 2048 stacks in float64 are hundreds of MB each)"""
    if MEMO.get("focus", lambda: case.name) != case.name:
        MEMO._d.clear()
        MEMO.get("focus", lambda: case.name)


def _model(case):
    _focus(case)
    return MEMO.get(("model", case.name), lambda: oc.make_model(case.model, case.sd()))


def _oracle(case, dtype=torch.float64):
    _focus(case)

    def make():
        fam, _, _, kw, _ = oc.MODELS[case.model]
        o64 = nm.oracle64(fam, case.sd(), **kw)
        return o64 if dtype == torch.float64 else o64.__class__(case.sd(), dtype=dtype, **kw)
    return MEMO.get(("oracle", case.name, dtype), make)


def _tol(budget, e32):
    """numerics.tol on this machine's e32, never wider than numerics.TOL_CAP: the fp32 oracle's floor on an ill-conditioned
    case moves by a factor of 2 - 3 with the CPU's summation order (threads, vector width); where it passes the cap, the
    case is held to the cap"""
    return min(nm.tol(budget, e32), nm.TOL_CAP)


def _finite(*tensors):
    for t in tensors:
        if t is not None:
            assert bool(torch.isfinite(torch.as_tensor(t)).all())


# ---- DeepSpeech2 -------------------------------------------------------------------------------------------------------
def _ds2_ref(case, key, x, lens, calls):
    """float64 and fp32 oracle over `calls` chained calls on x split along time -> ([(probs, lens, h, c)] float64, e32)"""
    def make():
        o64, o32 = _oracle(case), _oracle(case, torch.float32)
        T = x.shape[1] // calls
        refs, e32 = [], 0.0
        s64 = s32 = (None, None)
        for i in range(calls):
            chunk = x[:, i * T:(i + 1) * T]
            r64 = o64.forward(chunk, lens, *s64)
            r32 = o32.forward(chunk, lens, *s32)
            s64, s32 = (r64[2], r64[3]), (r32[2], r32[3])
            e32 = max(e32, _ds2_errs(case, r32, r64))
            refs.append(r64)
        return refs, e32
    return MEMO.get(("ds2ref", case.name, key), make)


def _ds2_errs(case, got, ref):
    """worst of probs (utt_rel, logprob_err), final h and (LSTM) final c against one float64 call"""
    probs, _, h, c = got
    rp, rl, rh, rc = ref
    errs = [nm.utt_rel(probs, rp, rl), nm.logprob_err(probs, torch.log(rp), rl), nm.utt_rel(h, rh)]
    if rc is not None and c is not None and not oc.MODELS[case.model][3]["use_gru"]:
        errs.append(nm.utt_rel(c, rc))
    return max(errs)


def _ds2_lens(B, T, seed):
    """the first utterance full, the others down to 13 feature frames = 2 output frames (an utterance of ONE output frame is
    not admitted: after a single step the off-centre LSTM's rows are at their narrowest and the fp32 oracle itself is
    3e-4 off there, tol > numerics.TOL_CAP)"""
    if B == 1:
        return [T]
    rng = np.random.Generator(np.random.PCG64(seed))
    return [T] + sorted((int(v) for v in rng.integers(13, T + 1, size=B - 1)), reverse=True)


def _ds2_check(case, B, T, calls, wave, what, env=None):
    """`calls` chained get_encoder_out_chunk calls of B ragged utterances, T feature frames each"""
    model = _model(case)
    lens = _ds2_lens(B, T, 7 * B + T)
    x, lens = synth_features(B, calls * T, lens=lens, seed=B + T)
    refs, e32 = _ds2_ref(case, (B, T, calls), x, lens, calls)
    tol = _tol(nm.F32_BUDGET_DS2, e32)
    old = os.environ.get("PPASR_DS2_PERSIST")
    if env is not None:
        os.environ["PPASR_DS2_PERSIST"] = env
    try:
        h = c = None
        worst = 0.0
        with _lib.kernel_profile() as kp:
            for i, ref in enumerate(refs):
                probs, out_lens, h, c = model.get_encoder_out_chunk(x[:, i * T:(i + 1) * T], lens, h, c)
                torch.cuda.synchronize()
                _finite(probs, h, c)
                assert out_lens.cpu().tolist() == ref[1].tolist()
                e = _ds2_errs(case, (probs, out_lens, h, c), ref)
                worst = max(worst, e)
                ok = nm.frame_ids_ok(torch.log(probs.cpu()), torch.log(ref[0]), tol, ref[1])[0]
                print(f"[offcentre] {case} {what} call {i}: {e:.2e} (tol {tol:.2e}, e32 {e32:.2e}) ids {'ok' if ok else 'DIFFER'}")
                assert e < tol, (case, what, i, e, tol)
                assert ok, (case, what, i)
    finally:
        if env is not None:
            if old is None:
                del os.environ["PPASR_DS2_PERSIST"]
            else:
                os.environ["PPASR_DS2_PERSIST"] = old
    ran = sorted(k for k in kp.kernels if "k_lstm_wave" in k)
    assert bool(ran) == wave, (case, what, sorted(kp.kernels))
    return worst, kp.kernels


DS2_MAIN = oc.CASES["ds2_lstm"] + oc.CASES["ds2_gru"]
DS2_L2 = oc.DS2_VARIANTS["ds2_lstm_l2"] + oc.DS2_VARIANTS["ds2_gru_l2"]


@pytest.mark.parametrize("case", DS2_MAIN, ids=repr)
def test_ds2_wavefront_two_chained_calls(case):
    """B = 6, L = 3, H = 1024, 2 x 60 feature frames (T' = 14 each), ragged: the fold runs in layers 1 and 2; the second
    call starts from the first one's final states"""
    _ds2_check(case, 6, 60, 2, True, "wave B=6")


@pytest.mark.parametrize("B", [40, 70])
@pytest.mark.parametrize("case", DS2_L2, ids=repr)
def test_ds2_wavefront_row_tiles(case, B):
    """B = 40: two 32-row tiles in one workgroup, the second partly filled; B = 70: a second workgroup along the batch
    (L = 2, 30 feature frames: T' = 6)"""
    _ds2_check(case, B, 30, 1, True, f"wave B={B}")


@pytest.mark.parametrize("case", oc.DS2_VARIANTS["ds2_lstm_h2048"], ids=repr)
def test_ds2_wavefront_h2048(case):
    _ds2_check(case, 6, 30, 1, True, "wave H=2048 B=6")


@pytest.mark.parametrize("case", DS2_MAIN, ids=repr)
def test_ds2_controls_single_utterance(case):
    """B = 1: the persistent recurrence, then the per-step kernels (PPASR_DS2_PERSIST=0); both normalise with k_ln_wide"""
    _, k1 = _ds2_check(case, 1, 60, 2, False, "persistent B=1")
    _, k0 = _ds2_check(case, 1, 60, 2, False, "per-step B=1", env="0")
    assert any("k_lstm_persist" in k for k in k1), sorted(k1)
    assert not any("k_lstm_persist" in k for k in k0), sorted(k0)
    assert any("k_ln_wide" in k for k in k0) and any("k_ln_wide" in k for k in k1)


@pytest.mark.parametrize("case", DS2_MAIN, ids=repr)
def test_ds2_controls_three_utterances(case):
    """B = 3: below the wavefront's threshold, the matrix-core step kernel per layer and time step"""
    _, k = _ds2_check(case, 3, 60, 2, False, "per-step B=3")
    assert any("k_lstm_step_mfma" in n for n in k), sorted(k)


@pytest.mark.parametrize("case", oc.DS2_VARIANTS["ds2_lstm_bi"], ids=repr)
def test_ds2_control_bidirectional(case):
    _ds2_check(case, 2, 60, 1, False, "bidirectional B=2")


@pytest.mark.parametrize("case", DS2_MAIN, ids=repr)
def test_ds2_session_group(case):
    """3 sessions of a DeepSpeech2StreamGroup over two rounds (35 feature frames: T' = 8), the second round in another order:
    the group runs the wavefront whatever n; every session against its own chained float64 call"""
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2StreamGroup
    model, o64, o32 = _model(case), _oracle(case), _oracle(case, torch.float32)
    group = DeepSpeech2StreamGroup(model, 3)
    T, lens1 = 35, np.array([35])
    s64 = {s: (None, None) for s in range(3)}
    s32 = dict(s64)
    with _lib.kernel_profile() as kp:
        for r, order in enumerate(([0, 1, 2], [2, 0, 1])):
            x = synth_features(3, T, seed=40 + r)[0]
            _, _, probs = group.encode_chunks(order, torch.from_numpy(x).cuda(), want_probs=True)
            torch.cuda.synchronize()
            _finite(probs)
            for k, s in enumerate(order):
                r64 = o64.forward(x[k:k + 1], lens1, *s64[s])
                r32 = o32.forward(x[k:k + 1], lens1, *s32[s])
                s64[s], s32[s] = (r64[2], r64[3]), (r32[2], r32[3])
                e32 = max(nm.utt_rel(r32[0], r64[0]), nm.logprob_err(r32[0], torch.log(r64[0])))
                tol = _tol(nm.F32_BUDGET_DS2, e32)
                e = max(nm.utt_rel(probs[k:k + 1], r64[0]), nm.logprob_err(probs[k:k + 1], torch.log(r64[0])))
                print(f"[offcentre] {case} group round {r} session {s}: {e:.2e} (tol {tol:.2e}, e32 {e32:.2e})")
                assert e < tol, (case, r, s, e, tol)
                assert nm.frame_ids_ok(torch.log(probs[k:k + 1].cpu()), torch.log(r64[0]), tol)[0], (case, r, s)
    assert any("k_lstm_wave" in k for k in kp.kernels), sorted(kp.kernels)


# ---- Transformer families ----------------------------------------------------------------------------------------------
# Every kernel of csrc that contains a LayerNorm (rb_layernorm / rbt_layernorm / ln_rows_inreg of rowblock.h and
# phases_t.h, ln_row of split_route_kernels.hip, g_ln_row of capi_generic.hip), by the names the kernel profile prints.
# The _h3 forms (k_ffn_qkv_h3, k_conv_ffn_h3, k_sq_mid_h3, k_sq_tail_h3, k_ctc_head_h3, k_attn_out_glu_h3) run only in the
# fp16 x3 mode, whose range guard large offsets are meant to trip (tests/test_gemm_guard_sites_gpu.py): not listed.
LN_KERNELS = {
    "fused layer kernels": ("k_ffn_qkv", "k_out_glu", "k_attn_out_glu", "k_conv_ffn<", "k_conv_ffn_stride<"),
    "16-row / 16-wave forms": ("k_ffn_qkv_t<", "k_out_glu_t<", "k_conv_ffn_t<", "k_sq_mid_t<", "k_sq_tail_t<"),
    "split-route units": ("k_ln_qkv<", "k_ln_qkv_t<", "k_ffn_part<", "k_ffn_part_t<", "k_ffn_join", "k_ffn_half16",
                          "k_conv_pre<", "k_conv_pre_cols16"),
    "Squeezeformer": ("k_sq_oproj", "k_sq_tail<", "k_ln_rows"),
    "stream forms": ("k_conv_ffn<15, true", "k_conv_ffn<7, true"),  # <KS, STREAM = true, NEXT>: the conv history in front
    "general route": ("k_g_ln", "k_g_ffn512", "k_g_proj512<", "k_g_conv_in_group"),
    "head": ("k_ctc_head<",),
}
RESULTS = {}  # (case name, what) -> kernels launched by a checked run


def _starts(kernels, prefix):
    """kernel names as the profile prints them; `prefix` ends where the name does (k_ffn_qkv must not match k_ffn_qkv_t<)"""
    return any(k == prefix or (k.startswith(prefix) and (prefix.endswith("<") or not (k[len(prefix)].isalnum() or k[len(prefix)] == "_")))
               for k in kernels)


def _tf_inputs(case, B, Tp, seed):
    """B utterances padded to T' output frames at the 4x rate (`linear` models: T' feature frames), the first one full"""
    T = Tp if case.model == "linear" else 4 * Tp + 3
    if B == 1:
        lens = [T]
    else:
        rng = np.random.Generator(np.random.PCG64(seed))
        lens = [T] + sorted((int(v) for v in rng.integers(max(8, T // 3), T + 1, size=B - 1)), reverse=True)
    return synth_features(B, T, lens=lens, seed=seed)


def _tf_ref(case, key, x, lens):
    """-> (float64 logits, e32 of the fp32 oracle on the same input)"""
    def make():
        ref = _oracle(case).get_encoder_out(x, lens, return_logits=True)[1]
        l32 = _oracle(case, torch.float32).get_encoder_out(x, lens, return_logits=True)[1]
        e32 = max(nm.utt_rel(l32, ref), nm.logprob_err(torch.softmax(l32.to(torch.float64), -1), ref))
        return ref, e32
    return MEMO.get(("tfref", case.name, key), make)


def _tf_check(case, B, Tp, what, knob=None, lens_tp=None):
    """one batched call against float64 at tol(case) -> the kernels it launched (memoised: RESULTS)"""
    key = (case.name, what)
    if key in RESULTS:
        return RESULTS[key]
    model = _model(case)
    if lens_tp is None:
        x, lens = _tf_inputs(case, B, Tp, 11 * B + Tp)
    else:
        T = 4 * Tp + 3
        x, lens = synth_features(B, T, lens=[min(T, 4 * n) if n < Tp else T for n in lens_tp], seed=5 + Tp)
    ref, e32 = _tf_ref(case, (B, Tp, lens_tp is not None), x, lens)
    tol = _tol(nm.F32_BUDGET, e32)
    try:
        if knob:
            getattr(model, "set_" + knob[0])(knob[1])
        with _lib.kernel_profile() as kp:
            probs, logits = model.get_encoder_out(x, lens, return_logits=True)
            torch.cuda.synchronize()
    finally:
        model.set_ffn_split(-1)
        model.set_row_block(-1)
    _finite(probs, logits)
    assert tuple(logits.shape) == tuple(ref.shape), (case, what)
    e_l, e_p = nm.utt_rel(logits, ref), nm.logprob_err(probs, ref)
    ok = nm.frame_ids_ok(logits, ref, tol)[0]
    print(f"[offcentre] {case} {what}: logits {e_l:.2e} logprobs {e_p:.2e} (tol {tol:.2e}, e32 {e32:.2e}) ids {'ok' if ok else 'DIFFER'}")
    assert e_l < tol and e_p < tol, (case, what, e_l, e_p, tol)
    assert ok, (case, what)
    RESULTS[key] = set(kp.kernels)
    return RESULTS[key]


# layer rows M = B * T' from tests/test_fp64_routes_gpu.py: one 16-row block, 33 rows (the split route of few row blocks),
# 513 (past the 16-row kernels' end) and 1025 (the fused kernels); Squeezeformer / Efficient-Conformer halve them once
ROWS = [(1, 16), (3, 11), (3, 171), (5, 205)]
# the per-handle route knobs at B = 3, T' = 90: fused layer kernels whatever M, the widest split, each block form
KNOBS = [("ffn_split", 0), ("ffn_split", 8), ("row_block", 16), ("row_block", 32), ("row_block", 1032)]
FAMS3 = ("conformer", "efficient_conformer", "squeezeformer")


def _off(model):
    return [c for c in oc.CASES[model] if c.kind == "offcentre"]


@pytest.mark.parametrize("case,B,Tp", [(c, b, t) for m in FAMS3 for c in _off(m) for b, t in ROWS], ids=repr)
def test_offcentre_rows_on_route_thresholds(case, B, Tp):
    _tf_check(case, B, Tp, f"B={B} T'={Tp}")


@pytest.mark.parametrize("case,knob", [(c, k) for m in FAMS3 for c in _off(m)[-1:] for k in KNOBS], ids=repr)
def test_offcentre_route_knobs(case, knob):
    _tf_check(case, 3, 90, f"{knob[0]}={knob[1]}", knob=knob)


@pytest.mark.parametrize("case", _off("squeezeformer"), ids=repr)
def test_offcentre_squeezeformer_three_frame_utterances(case):
    """T' = 3: fewer than the 4 consecutive rows a wave of the register depthwise conv walks, so the fused route's layer
    tail takes the LDS-staged 8-wave form k_sq_tail<KS, false>"""
    k = _tf_check(case, 5, 3, "B=5 T'=3 ffn_split=0", knob=("ffn_split", 0))
    assert _starts(k, "k_sq_tail<"), sorted(k)


@pytest.mark.parametrize("case,B,Tp", [(c, b, t) for c in _off("general") for b, t in ((3, 11), (3, 171))]
                         + [(c, 3, 40) for c in _off("linear")], ids=repr)
def test_offcentre_general_route(case, B, Tp):
    """output_size = 512, 8 heads: the general layer route's row kernels (k_g_ln); input_layer = linear: the embedding's own
    LayerNorm (eps 1e-12) sees the offset"""
    k = _tf_check(case, B, Tp, f"B={B} T'={Tp}")
    assert _starts(k, "k_g_ln"), sorted(k)


@pytest.mark.parametrize("case", [c for m in FAMS3 for c in oc.CASES[m] if c.kind == "saturated"], ids=repr)
def test_saturated_activations(case):
    _tf_check(case, 3, 90, "B=3 T'=90 lens'=[90, 11, 3]", lens_tp=[90, 11, 3])


def _windows(n_frames, window=67, stride=64):
    return [(cur, min(cur + window, n_frames)) for cur in range(0, n_frames - 7 + 1, stride)]


def _chunk(oracle, chunk, offset, att, cnn):
    with torch.no_grad():
        xs, att, cnn = oracle.forward_chunk(chunk, offset, -16, att, cnn)
        return oracle.ctc_logits(xs), att, cnn


def _chunk_errs(got, g_att, g_cnn, ref, att, cnn):
    errs = [nm.utt_rel(got, torch.softmax(ref.to(torch.float64), -1)), nm.logprob_err(got, ref)]
    if g_att is not None:
        errs += [nm.utt_rel(g_att, att), nm.utt_rel(g_cnn, cnn) if cnn.numel() else 0.0]
    return max(errs)


@pytest.mark.parametrize("route", [-1, 0])
@pytest.mark.parametrize("case", [_off(m)[-1] for m in FAMS3], ids=repr)
def test_offcentre_stream_chunks(case, route):
    """one stream, four 67-frame windows: probabilities and the exported attention / conv caches of every chunk; on the
    split route a stream handle takes by default and (ppasr_set_ffn_split(h, 0)) on the fused layer kernels with the conv
    history: k_conv_ffn<KS, true, .>, the 8-wave k_sq_tail<KS>"""
    model, o64, o32 = _model(case), _oracle(case), _oracle(case, torch.float32)
    x, _ = synth_features(1, 64 * 4 + 3, seed=51)
    model.set_ffn_split(route)
    try:
        stream = model.new_stream()
        _stream_chunks(case, route, model, stream, o64, o32, x)
    finally:
        model.set_ffn_split(-1)


def _stream_chunks(case, route, model, stream, o64, o32, x):
    s64, s32, offset = (None, None), (None, None), 0
    kernels = set()
    for (a, b) in _windows(x.shape[1]):
        ref, att, cnn = _chunk(o64, x[:, a:b], offset, *s64)
        r32, a32, c32 = _chunk(o32, x[:, a:b], offset, *s32)
        s64, s32, offset = (att, cnn), (a32, c32), offset + ref.shape[1]
        e32 = _chunk_errs(torch.softmax(r32.to(torch.float64), -1), a32, c32, ref, att, cnn)
        tol = _tol(nm.F32_BUDGET, e32)
        with _lib.kernel_profile() as kp:
            got = stream.encode_chunk(x[:, a:b], -16)
            g_att, g_cnn = stream.export_caches()
            torch.cuda.synchronize()
        kernels |= set(kp.kernels)
        _finite(got, g_att, g_cnn)
        assert tuple(got.shape) == tuple(ref.shape) and tuple(g_att.shape) == tuple(att.shape), (a, b)
        e = _chunk_errs(got, g_att, g_cnn, ref, att, cnn)
        print(f"[offcentre] {case} ffn_split={route} chunk {a}: {e:.2e} (tol {tol:.2e}, e32 {e32:.2e})")
        assert e < tol, (case, route, a, e, tol)
    RESULTS[(case.name, f"stream {route}")] = kernels


def test_offcentre_conformer_session_group():
    """3 sessions of a Conformer group over four windows; the group keeps its caches on the device (no export), so they
    are checked through the chunks that read them"""
    from ppasr_amd.model_utils.conformer.model import make_stream_group
    case = _off("conformer")[-1]
    model, o64, o32 = _model(case), _oracle(case), _oracle(case, torch.float32)
    n = 3
    feats = [synth_features(1, 64 * 4 + 3, seed=60 + s)[0] for s in range(n)]
    group = make_stream_group(model, n, max_frames=256)
    s64 = [(None, None, 0)] * n
    s32 = [(None, None)] * n
    kernels = set()
    for (a, b) in _windows(feats[0].shape[1]):
        chunks = np.concatenate([f[:, a:b] for f in feats], axis=0)
        with _lib.kernel_profile() as kp:
            _, _, probs = group.encode_chunks(list(range(n)), chunks, want_probs=True)
            torch.cuda.synchronize()
        kernels |= set(kp.kernels)
        _finite(probs)
        for s in range(n):
            att, cnn, off = s64[s]
            ref, att, cnn = _chunk(o64, chunks[s:s + 1], off, att, cnn)
            r32, a32, c32 = _chunk(o32, chunks[s:s + 1], off, *s32[s])
            s64[s], s32[s] = (att, cnn, off + ref.shape[1]), (a32, c32)
            e32 = _chunk_errs(torch.softmax(r32.to(torch.float64), -1), None, None, ref, None, None)
            tol = _tol(nm.F32_BUDGET, e32)
            e = _chunk_errs(probs[s:s + 1], None, None, ref, None, None)
            print(f"[offcentre] {case} group window {a} session {s}: {e:.2e} (tol {tol:.2e}, e32 {e32:.2e})")
            assert e < tol, (case, a, s, e, tol)
    RESULTS[(case.name, "group")] = kernels


def test_every_layernorm_kernel_was_reached_by_an_offcentre_case():
    """(runs the checked cases it needs itself when they have not run yet: it does not depend on the selection)"""
    for m in FAMS3:
        for c in _off(m):
            for b, t in ROWS:
                _tf_check(c, b, t, f"B={b} T'={t}")
        for k in KNOBS:
            _tf_check(_off(m)[-1], 3, 90, f"{k[0]}={k[1]}", knob=k)
        for route in (-1, 0):
            if (_off(m)[-1].name, f"stream {route}") not in RESULTS:
                test_offcentre_stream_chunks(_off(m)[-1], route)
    for c in _off("squeezeformer"):
        _tf_check(c, 5, 3, "B=5 T'=3 ffn_split=0", knob=("ffn_split", 0))
    for c in _off("general"):
        _tf_check(c, 3, 11, "B=3 T'=11")
    if (_off("conformer")[-1].name, "group") not in RESULTS:
        test_offcentre_conformer_session_group()
    general = oc.make_model("general", _off("general")[-1].sd())
    seen = set()
    for (name, _), ks in RESULTS.items():
        if oc.find(name).kind == "offcentre":
            seen |= ks
    # the general route's session group (its conv-input LayerNorm kernel), off-centre like the rest; checked against float64
    seen |= _general_group_kernels(general, _off("general")[-1])
    missing = [k for ks in LN_KERNELS.values() for k in ks if not _starts(seen, k)]
    print("[offcentre] kernels launched by the off-centre cases:", " ".join(sorted(k.split("(")[0] for k in seen)))
    assert not missing, (missing, sorted(seen))


def _general_group_kernels(model, case):
    from ppasr_amd.model_utils.conformer.model import GeneralConformerStreamGroup
    o64, o32 = _oracle(case), _oracle(case, torch.float32)
    group = GeneralConformerStreamGroup(model, 2, max_frames=256)
    feats = [synth_features(1, 64 * 2 + 3, seed=70 + s)[0] for s in range(2)]
    s64, s32 = [(None, None, 0)] * 2, [(None, None)] * 2
    kernels = set()
    for (a, b) in _windows(feats[0].shape[1]):
        chunks = np.concatenate([f[:, a:b] for f in feats], axis=0)
        with _lib.kernel_profile() as kp:
            _, _, probs = group.encode_chunks([0, 1], chunks, want_probs=True)
            torch.cuda.synchronize()
        kernels |= set(kp.kernels)
        _finite(probs)
        for s in range(2):
            att, cnn, off = s64[s]
            ref, att, cnn = _chunk(o64, chunks[s:s + 1], off, att, cnn)
            r32, a32, c32 = _chunk(o32, chunks[s:s + 1], off, *s32[s])
            s64[s], s32[s] = (att, cnn, off + ref.shape[1]), (a32, c32)
            tol = _tol(nm.F32_BUDGET, _chunk_errs(torch.softmax(r32.to(torch.float64), -1), None, None, ref, None, None))
            e = _chunk_errs(probs[s:s + 1], None, None, ref, None, None)
            print(f"[offcentre] {case} general group window {a} session {s}: {e:.2e} (tol {tol:.2e})")
            assert e < tol, (case, a, s, e, tol)
    return kernels
