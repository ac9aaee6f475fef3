"""Every fp32 encoder route against the float64 oracle at the fp32 error budget (tests/numerics.py), production routes
without debug taps: per utterance, logits (utt_rel) and probabilities in log space (logprob_err) within F32_BUDGET, and
the greedy ids of the float64 oracle (near-ties of the reference by the margin rule of numerics.frame_ids_ok).

The matrix places the layer rows M = B * T' on both sides of the route thresholds (16 / 32 row blocks, the 16-row
kernels' end at 512, the split counts' steps at 1024 / 2048, the fused kernels past 128 row blocks at 4096) -- for the
Squeezeformer and the Efficient-Conformer also the reduced / strided rows -- turns the per-handle route knobs at fixed
inputs, puts key lengths on the attention tile widths (64 / 128 / 192 / 256 +- 1) next to utterances of 1 and 3 encoder
frames, sharpens the attention so that position and mask errors are not averaged away, and streams chunks (single
sessions and Conformer session groups) against the float64 forward_chunk.  Each case prints its worst error; the
budgets were set from those prints.

The opt-in fp16 x3 GEMM mode (ppasr_set_gemm_mode, csrc/h3.h) runs the row thresholds, the attention edges, the sharpened
attention and the stream chunks a second time (`_f16x3_leg`): wherever the handle accepts the mode, the same per-utterance
checks against the same float64 results at the same F32_BUDGET (its header puts it in fp32's class), with zero guard
events; a handle that refuses it must do so with PPASR_EUNSUPPORTED and the case says what it skipped.  That the mode's
kernels ran is checked too (kernel_profile: an _h3 / <.., true> kernel was launched, and where the coverage includes the
layers one of the LAYER kernels unless the launch took the fused 16-row layer kernels, which keep fp32 by design) and the bytes
must differ from the fp32 leg's.  The fp32 legs are unchanged."""
import numpy as np
import pytest
import torch

import numerics as nm
from ppasr_amd.utils.synth import (conformer_state_dict, deepspeech2_state_dict, efficient_conformer_state_dict,
                                   squeezeformer_state_dict, synth_features)

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()


def _sharpen(sd, n_layers, factor=2.0):
    """q / k projections (weights and biases) and the position biases scaled: attention scores x factor^2"""
    sd = dict(sd)
    for i in range(n_layers):
        p = f"encoder.encoders.{i}.self_attn"
        for k in (".linear_q.weight", ".linear_q.bias", ".linear_k.weight", ".linear_k.bias", ".pos_bias_u", ".pos_bias_v"):
            sd[p + k] = (np.asarray(sd[p + k]) * factor).astype(np.float32)
    return sd


def _spec(name):
    """-> (family, state dict, model class + encoder_conf, oracle kwargs, total time reduction)"""
    if name.startswith("conformer"):
        ks = 31 if "k31" in name else 15
        sd = conformer_state_dict(vocab_size=97, num_blocks=2, cnn_module_kernel=ks, seed=121 + ks, perturb_norm=True)
        if "sharp" in name:
            sd = _sharpen(sd, 2)
        conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=ks)
        return "conformer", sd, conf, dict(num_blocks=2, cnn_module_kernel=ks), 4
    if name.startswith("squeezeformer"):
        ks = 15 if "k15" in name else 31
        sd = squeezeformer_state_dict(vocab_size=131, num_blocks=4, cnn_module_kernel=ks, seed=131 + ks, perturb_norm=True)
        if "sharp" in name:
            sd = _sharpen(sd, 4)
        conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=4, reduce_idx=1, recover_idx=3,
                    feed_forward_expansion_factor=8, cnn_module_kernel=ks)
        return "squeezeformer", sd, conf, dict(num_blocks=4, reduce_idx=1, recover_idx=3, cnn_module_kernel=ks), 4
    sd = efficient_conformer_state_dict(vocab_size=113, num_blocks=4, seed=141, perturb_norm=True, stride_layer_idx=1,
                                        group_layer_idx=(0, 1))
    if "sharp" in name:
        sd = _sharpen(sd, 4)
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                cnn_module_norm="layer_norm",
                efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3, stride_kernel=True))
    return "efficient_conformer", sd, conf, dict(num_blocks=4, stride_layer_idx=1, group_layer_idx=(0, 1)), 8


def _model(name):
    def make():
        fam, sd, conf, _, _ = _spec(name)
        if fam == "conformer":
            from ppasr_amd.model_utils.conformer.model import ConformerModel as M
        elif fam == "squeezeformer":
            from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
        else:
            from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
        V = int(sd["ctc.ctc_lo.bias"].shape[0])
        return M(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    return MEMO.get(("model", name), make)


def _oracle(name):
    def make():
        fam, sd, _, kw, _ = _spec(name)
        return nm.oracle64(fam, sd, **kw)
    return MEMO.get(("oracle", name), make)


def _inputs(Tp, lens_tp, seed):
    """features of B = len(lens_tp) utterances padded to T' = Tp output frames (4x front end); utterance b's length
    gives lens_tp[b] valid output frames"""
    T = 4 * Tp + 3
    lens = [min(T, 4 * n) if n < Tp else T for n in lens_tp]
    return synth_features(len(lens), T, lens=lens, seed=seed)


def _ref(name, Tp, lens_tp, seed):
    x, lens = _inputs(Tp, lens_tp, seed)
    return x, lens, MEMO.get(("ref", name, Tp, tuple(lens_tp), seed),
                             lambda: _oracle(name).get_encoder_out(x, lens, return_logits=True)[1])


def _check(name, model, x, lens, ref_logits, what, skip_padding=False):
    probs, logits = model.get_encoder_out(x, lens, return_logits=True)
    tokens, n_tok, _ = model.encode_greedy(x, lens, trim_to_length=skip_padding)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == tuple(ref_logits.shape), what
    lens_out = model.valid_out_frames(lens, x.shape[1]).cpu().numpy() if skip_padding else None
    if skip_padding:
        for b, n in enumerate(lens_out):
            assert not bool(probs[b, n:].any()), (what, b)
    e_l = nm.utt_rel(logits, ref_logits, lens_out)
    e_p = nm.logprob_err(probs, ref_logits, lens_out)
    ok, near = nm.frame_ids_ok(logits, ref_logits, nm.F32_BUDGET, lens_out)
    print(f"[fp64] {name} {what}: logits {e_l:.2e} logprobs {e_p:.2e} near-ties {near}")
    assert e_l < nm.F32_BUDGET and e_p < nm.F32_BUDGET, (what, e_l, e_p)
    assert ok, what
    if near == 0:
        r = ref_logits.numpy()
        for b in range(x.shape[0]):
            n = int(lens_out[b]) if skip_padding else r.shape[1]
            assert np.array_equal(tokens[b, :int(n_tok[b])].cpu().numpy(), nm.collapse(r[b, :n].argmax(-1))), (what, b)
    return max(e_l, e_p), logits.cpu().numpy().tobytes()


def _check_both(test, name, x, lens, ref, what):
    """the fp32 leg (as before), then the same case in the fp16 x3 mode"""
    model = _model(name)
    e32, bytes32 = _check(name, model, x, lens, ref, what)
    e16 = _f16x3_leg(test, name, model, lambda label: _check(name, model, x, lens, ref, label + what), bytes32)
    _note(test, name, what, e16, e32)


WORST_F16X3 = {}  # test name -> (worst f16x3 error, the fp32 leg's error of that case, what)
# the mode's kernels by name (csrc: the _h3 kernels, and the <.., H3 = true> forms of the split route's units, whose last
# template parameter is H3); other kernels carry trailing bool parameters of their own, so the names are listed
FRONT_HEAD_H3 = ("k_conv_stage_h3", "k_embed_h3", "k_ctc_head_h3")
LAYER_H3 = ("k_ffn_qkv_h3", "k_conv_ffn_h3", "k_attn_out_glu_h3", "k_sq_mid_h3", "k_sq_tail_h3")
LAYER_H3_TRUE = ("k_ffn_part<", "k_ln_qkv<", "k_out_glu<", "k_pw1_glu_cols<", "k_conv_pre<", "k_conv_ffn_stride<")
ROWS16_FUSED = ("k_ffn_qkv_t<", "k_conv_ffn_t<", "k_sq_mid_t<", "k_sq_tail_t<")  # the layer kernels of 33 .. 128 row blocks


def _mode_kernels(names):
    """-> (the mode's kernels among `names`, its LAYER kernels among them, the fused 16-row layer kernels launched)"""
    layer = sorted(k for k in names
                   if k.startswith(LAYER_H3) or (k.startswith(LAYER_H3_TRUE) and k.rstrip().endswith("true>")))
    return sorted(k for k in names if k.startswith(FRONT_HEAD_H3)) + layer, layer, sorted(k for k in names if k.startswith(ROWS16_FUSED))


def _f16x3_leg(test, name, model, run, bytes32):
    """`run(label)` -> (worst error, output bytes) once more with the handle in the fp16 x3 mode -> its worst error (the checks
    are run's own); no guard event and no fallback may be counted, kernels of the mode must have run and the bytes must differ
    from `bytes32`, the fp32 leg's.  A refusal must be PPASR_EUNSUPPORTED."""
    from ppasr_amd import _lib
    try:
        model.set_gemm_mode("f16x3")
    except _lib.PPASRHipError as e:
        assert e.status == _lib.PPASR_EUNSUPPORTED, e
        print(f"[fp64] {name}: f16x3 refused (PPASR_EUNSUPPORTED): fp16 x3 leg skipped on every route of this case")
        return None
    try:
        cov = "+".join(sorted(model.gemm_coverage()))
        assert cov, name
        before = model.gemm_guard_stats()
        with _lib.kernel_profile() as kp:
            err, got = run(f"f16x3[{cov}] ")
            torch.cuda.synchronize()
        assert model.gemm_guard_stats() == before, (name, before, model.gemm_guard_stats())
        mode, layer, t_forms = _mode_kernels(kp.kernels)
        print(f"[fp64] {name} f16x3[{cov}]: mode kernels {len(mode)} (layer kernels {len(layer)}), 16-row layer kernels {len(t_forms)}: "
              + " ".join(k.split("(")[0] for k in layer + t_forms))
        assert mode, (name, sorted(kp.kernels))  # a route that quietly stayed in fp32 would pass every check above
        if "layers" in cov:
            assert layer or t_forms, (name, sorted(kp.kernels))
        assert got != bytes32, name
    finally:
        model.set_gemm_mode("f32")
    return err


def _note(test, name, what, e16, e32):
    if e16 is not None and e16 >= WORST_F16X3.get(test, (-1.0,))[0]:
        WORST_F16X3[test] = (e16, e32, f"{name} {what}")
    w = WORST_F16X3.get(test)
    if w:
        print(f"[fp64] {test}: worst f16x3 so far {w[0]:.2e} (fp32 leg of that case {w[1]:.2e}) at {w[2]}")


def _ragged(B, Tp, seed):
    """B utterance lengths in output frames, the first one full, the others spread below it"""
    if B == 1:
        return [Tp]
    rng = np.random.Generator(np.random.PCG64(seed))
    return [Tp] + sorted((int(v) for v in rng.integers(max(1, Tp // 3), Tp + 1, size=B - 1)), reverse=True)


# ---- row counts on the route thresholds -------------------------------------------------------------------------------
# (B, T'): M = B * T' layer rows; comments give M (and the reduced / strided rows)
ROWS_CONFORMER = [(1, 16), (1, 17), (2, 16), (3, 11), (1, 32), (4, 128), (3, 171), (4, 256), (5, 205), (8, 256), (3, 683),
                  (4, 1024), (17, 241)]
#                 16      17       32       33       32       512       513       1024      1025      2048      2049
#                 4096       4097
ROWS_HALVED = [(1, 16), (1, 17), (3, 11), (2, 512), (1, 1025), (1, 1026), (2, 1024), (1, 2050), (4, 1024)]
#              16/8     17/9     33/18    1024/512  1025/513   1026/513   2048/1024  2050/1025  4096/2048
ROWS_K31 = [(1, 16), (1, 17), (4, 128), (3, 171), (4, 256), (5, 205)]


@pytest.mark.parametrize("name,B,Tp", [("conformer", b, t) for b, t in ROWS_CONFORMER]
                         + [("conformer_k31", b, t) for b, t in ROWS_K31]
                         + [(n, b, t) for n in ("squeezeformer", "efficient") for b, t in ROWS_HALVED]
                         + [("squeezeformer_k15", b, t) for b, t in ROWS_K31])
def test_rows_on_route_thresholds(name, B, Tp):
    lens_tp = _ragged(B, Tp, B * 7919 + Tp)
    x, lens, ref = _ref(name, Tp, lens_tp, Tp + B)
    _check_both("rows_on_route_thresholds", name, x, lens, ref, f"B={B} T'={Tp} M={B * Tp}")


# ---- route knobs at fixed inputs --------------------------------------------------------------------------------------
KNOBS = ([("ffn_split", v) for v in (0, 2, 4, 8, -1)] + [("row_block", v) for v in (16, 32, 1032)]
         + [("front_fused", v) for v in (0, 1)] + [("skip_padding", "no_hint"), ("skip_padding", "hint")])


@pytest.mark.parametrize("knob,value", KNOBS)
@pytest.mark.parametrize("name", ["conformer", "squeezeformer", "efficient"])
def test_route_knobs(name, knob, value):
    model = _model(name)
    Tp, lens_tp = 83, [83, 70, 30, 1]
    x, lens, ref = _ref(name, Tp, lens_tp, 17)
    skip = knob == "skip_padding"
    try:
        if knob == "ffn_split":
            model.set_ffn_split(value)
        elif knob == "row_block":
            model.set_row_block(value)
        elif knob == "front_fused":
            model.set_front_fused(value)
        else:
            model.set_skip_padding(True)
            if value == "hint":
                model.set_lengths_hint([int(v) for v in lens])
        _check(name, model, x, lens, ref, f"{knob}={value}", skip_padding=skip)
    finally:
        model.set_ffn_split(-1)
        model.set_row_block(-1)
        model.set_front_fused(-1)
        model.set_skip_padding(False)
        model.set_lengths_hint(None)


# ---- attention edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Tp", [("conformer", t) for t in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)]
                         + [(n, t) for n in ("squeezeformer", "efficient") for t in (127, 128, 129, 256, 257, 385)])
def test_attention_key_lengths_and_tiny_utterances(name, Tp):
    """T' keys on and around the k_attention_t tile widths (halved in the reduced / strided layers), next to an
    utterance of 1 or 3 encoder frames and one a tile width long"""
    lens_tp = [Tp, 1 if Tp % 2 else 3, 64]
    x, lens, ref = _ref(name, Tp, lens_tp, 3 * Tp)
    _check_both("attention_key_lengths", name, x, lens, ref, f"T'={Tp} lens'={lens_tp}")


@pytest.mark.parametrize("name", ["conformer_sharp", "squeezeformer_sharp", "efficient_sharp"])
@pytest.mark.parametrize("B,Tp", [(3, 90), (1, 257)])
def test_sharpened_attention(name, B, Tp):
    lens_tp = [Tp, 11, 3][:B] if B > 1 else [Tp]
    x, lens, ref = _ref(name, Tp, lens_tp, 5 + Tp)
    _check_both("sharpened_attention", name, x, lens, ref, f"B={B} T'={Tp}")


# ---- streaming --------------------------------------------------------------------------------------------------------
def _windows(n_frames, window=67, stride=64):
    return [(cur, min(cur + window, n_frames)) for cur in range(0, n_frames - 7 + 1, stride)]


def _ref_chunk(oracle, chunk, offset, required, att, cnn):
    with torch.no_grad():
        xs, att, cnn = oracle.forward_chunk(chunk, offset, required, att, cnn)
        return oracle.ctc_logits(xs), att, cnn


@pytest.mark.parametrize("required", [-16, 32])
@pytest.mark.parametrize("name", ["conformer", "squeezeformer", "efficient"])
def test_stream_chunks(name, required):
    model, oracle = _model(name), _oracle(name)
    x, _ = synth_features(1, 64 * 4 + 3, seed=51)
    refs = []  # the float64 chunks, once for both legs
    att = cnn = None
    offset = 0
    for (a, b) in _windows(x.shape[1]):
        ref, att, cnn = _ref_chunk(oracle, x[:, a:b], offset, required, att, cnn)
        refs.append((a, b, ref, att, cnn))
        offset += ref.shape[1]

    def run(label):
        stream = model.new_stream()
        worst = 0.0
        outs = []
        for (a, b, ref, att, cnn) in refs:
            got = stream.encode_chunk(x[:, a:b], required)
            g_att, g_cnn = stream.export_caches()
            torch.cuda.synchronize()
            outs.append(got.cpu().numpy().tobytes())
            assert tuple(got.shape) == tuple(ref.shape) and tuple(g_att.shape) == tuple(att.shape), (a, b)
            errs = [nm.utt_rel(got, torch.softmax(ref, -1)),
                    nm.logprob_err(got, ref), nm.utt_rel(g_att, att), nm.utt_rel(g_cnn, cnn) if cnn.numel() else 0.0]
            worst = max(worst, *errs)
            assert max(errs) < nm.F32_BUDGET, (label, a, b, errs)
        print(f"[fp64] {name} {label}chunks required={required}: worst {worst:.2e}")
        return worst, b"".join(outs)

    e32, bytes32 = run("")
    e16 = _f16x3_leg("stream_chunks", name, model, run, bytes32)
    _note("stream_chunks", name, f"required={required}", e16, e32)


def test_conformer_session_group():
    from ppasr_amd.model_utils.conformer.model import make_stream_group
    model, oracle = _model("conformer"), _oracle("conformer")
    n = 3
    feats = [synth_features(1, 64 * 4 + 3, seed=60 + s)[0] for s in range(n)]
    group = make_stream_group(model, n, max_frames=256)
    state = [(None, None, 0)] * n
    worst = 0.0
    for (a, b) in _windows(feats[0].shape[1]):
        chunks = np.concatenate([f[:, a:b] for f in feats], axis=0)
        _, _, probs = group.encode_chunks(list(range(n)), chunks, want_probs=True)
        torch.cuda.synchronize()
        for s in range(n):
            att, cnn, off = state[s]
            ref, att, cnn = _ref_chunk(oracle, chunks[s:s + 1], off, -16, att, cnn)
            state[s] = (att, cnn, off + ref.shape[1])
            e = max(nm.utt_rel(probs[s:s + 1], torch.softmax(ref, -1)), nm.logprob_err(probs[s:s + 1], ref))
            worst = max(worst, e)
            assert e < nm.F32_BUDGET, (a, s, e)
    print(f"[fp64] conformer session group: worst {worst:.2e}")


# ---- DeepSpeech2 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gru", [False, True])
@pytest.mark.parametrize("streaming", [True, False])
@pytest.mark.parametrize("B", [1, 3, 6])
def test_deepspeech2(gru, streaming, B):
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
    V, L = 89, 2
    key = ("ds2", gru, streaming)
    sd = MEMO.get(key + ("sd",), lambda: deepspeech2_state_dict(vocab_size=V, num_rnn_layers=L, streaming=streaming,
                                                                 seed=211 + 2 * gru + streaming, perturb_norm=True,
                                                                 use_gru=gru))
    model = MEMO.get(key + ("model",), lambda: DeepSpeech2Model(
        80, V, streaming=streaming, encoder_conf=dict(num_rnn_layers=L, rnn_size=1024, use_gru=gru), state_dict=sd,
        device="cuda:0"))
    oracle = MEMO.get(key + ("oracle",), lambda: nm.oracle64("deepspeech2", sd, num_rnn_layers=L, rnn_size=1024,
                                                             streaming=streaming, use_gru=gru))
    T = 123
    lens = [T] + [int(v) for v in np.linspace(100, 9, B - 1)] if B > 1 else [T]
    x, lens = synth_features(B, 2 * T, lens=lens, seed=B)
    h = c = rh = rc = None
    worst = 0.0
    # two calls, the final states of the first as the initial states of the second (non-streaming: independent calls)
    for s0 in (0, T):
        chunk = x[:, s0:s0 + T]
        probs, out_lens, h, c = model.get_encoder_out_chunk(chunk, lens, h if streaming else None, c if streaming else None)
        rp, rl, rh, rc = oracle.forward(chunk, lens, rh if streaming else None, rc if streaming else None)
        torch.cuda.synchronize()
        assert out_lens.cpu().tolist() == rl.tolist()
        errs = [nm.utt_rel(probs, rp, rl), nm.logprob_err(probs, torch.log(rp), rl), nm.utt_rel(h, rh)]
        if not gru:
            errs.append(nm.utt_rel(c, rc))
        worst = max(worst, *errs)
        assert max(errs) < nm.F32_BUDGET_DS2, (s0, errs)
        assert nm.frame_ids_ok(torch.log(probs.cpu()), torch.log(rp), nm.F32_BUDGET_DS2, rl)[0], s0
    print(f"[fp64] deepspeech2 gru={gru} streaming={streaming} B={B}: worst {worst:.2e}")
