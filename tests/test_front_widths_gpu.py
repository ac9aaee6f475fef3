"""GPU: the front ends at every feature width the library accepts, against the float64 oracle at the fp32 budget
(tests/numerics.py).  Every other GPU test builds its models at input_dim = 80; the front end's index math -- conv1's row
buffer, the pair form's LDS window of conv2, the embed GEMM's K = 256 * F2 and its slices, the streaming chunk's conv2
K-split, the 6x / 8x / linear input layers, DeepSpeech2's conv tile -- depends on the width F through F1 = (F - 1) / 2
and F2 = (F1 - 1) / 2, so a stride, clamp or window bound that only happens to be right at 80 bins passes everywhere
else.

  F    F1  F2
  7     3   1   smallest conv2d width: 32 pairs per 32-row tile, one embed K chunk (most slices empty)
  12    5   2   two f2 per pair
  40   19   9   the reference's n_mfcc width, 8 kHz 40-mel width
  64   31  15
  81   40  19   even F1: conv1's last column is unused by conv2
  128  63  31   largest width: k_conv1's full row buffer, embed K = 7936
  80   39  19   control (the width of the rest of the suite)

Covered: (a) batched encodes of the three transformer families, both front-end routes, padding skipped and computed,
the front end's own output through the debug taps; (b) the 6x / 8x / linear input layers and 512 channels; (c) single
streams chunk by chunk, with chunks on both sides of the conv2 K-split's row limit; (d) session groups of every family;
(e) DeepSpeech2 batched and streaming, LSTM and GRU; (f) the opt-in fp16 x3 mode; (g) the widths create refuses; (h) the
chunk workspace, which must never shrink as the chunk grows.  Each case prints its worst error."""
import ctypes
import time

import numpy as np
import pytest
import torch

import numerics as nm
from ppasr_amd import _lib
from ppasr_amd.utils.synth import (conformer_state_dict, deepspeech2_state_dict, efficient_conformer_state_dict,
                                   squeezeformer_state_dict, synth_features)

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
WIDTHS = [7, 12, 40, 64, 81, 128, 80]
FAMILIES = ["conformer", "squeezeformer", "efficient"]


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"\n[widths] {__name__}: {time.time() - t0:.1f} s wall")


def _spec(fam, F):
    """-> (oracle family, state dict, encoder_conf, oracle kwargs): small models (1 Conformer block, 2 Squeezeformer
    blocks, 2 Efficient-Conformer blocks with the stride layer)"""
    if fam == "conformer":
        sd = conformer_state_dict(input_dim=F, vocab_size=97, num_blocks=1, seed=300 + F, perturb_norm=True)
        conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=1, cnn_module_kernel=15)
        return "conformer", sd, conf, dict(num_blocks=1, cnn_module_kernel=15)
    if fam == "squeezeformer":
        sd = squeezeformer_state_dict(input_dim=F, vocab_size=97, num_blocks=2, seed=400 + F, perturb_norm=True)
        conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=2, reduce_idx=None, recover_idx=None,
                    feed_forward_expansion_factor=8, cnn_module_kernel=31)
        return "squeezeformer", sd, conf, dict(num_blocks=2, reduce_idx=None, recover_idx=None, cnn_module_kernel=31)
    sd = efficient_conformer_state_dict(input_dim=F, vocab_size=97, num_blocks=2, seed=500 + F, perturb_norm=True,
                                        stride_layer_idx=1, group_layer_idx=(0, 1))
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15,
                cnn_module_norm="layer_norm",
                efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3, stride_kernel=True))
    return "efficient_conformer", sd, conf, dict(num_blocks=2, stride_layer_idx=1, group_layer_idx=(0, 1))


def _cls(fam):
    if fam == "conformer":
        from ppasr_amd.model_utils.conformer.model import ConformerModel as M
    elif fam == "squeezeformer":
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
    else:
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
    return M


def _model(fam, F):
    def make():
        _, sd, conf, _ = _spec(fam, F)
        return _cls(fam)(F, 97, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    return MEMO.get(("model", fam, F), make)


def _oracle(fam, F):
    def make():
        ofam, sd, _, kw = _spec(fam, F)
        return nm.oracle64(ofam, sd, **kw)
    return MEMO.get(("oracle", fam, F), make)


def _inputs(F, B, Tp, seed):
    """B utterances of F bins padded to T' = Tp output frames (4x front end): the first one full, the others ragged"""
    T = 4 * Tp + 3
    rng = np.random.default_rng(seed)
    lens_tp = [Tp] + sorted((int(v) for v in rng.integers(1, Tp + 1, size=B - 1)), reverse=True)
    lens = [min(T, 4 * n) if n < Tp else T for n in lens_tp]
    return synth_features(B, T, n_mels=F, lens=lens, seed=seed)


def _ref(fam, F, B, Tp, seed):
    x, lens = _inputs(F, B, Tp, seed)
    return x, lens, MEMO.get(("ref", fam, F, B, Tp, seed),
                             lambda: _oracle(fam, F).get_encoder_out(x, lens, return_logits=True)[1])


def _check_logits(what, probs, logits, ref, lens_out=None):
    assert tuple(logits.shape) == tuple(ref.shape), what
    assert torch.isfinite(logits).all() and torch.isfinite(probs).all(), what
    e_l = nm.utt_rel(logits, ref, lens_out)
    e_p = nm.logprob_err(probs, ref, lens_out)
    ok, near = nm.frame_ids_ok(logits, ref, nm.F32_BUDGET, lens_out)
    print(f"[widths] {what}: logits {e_l:.2e} logprobs {e_p:.2e} near-ties {near}")
    assert e_l < nm.F32_BUDGET and e_p < nm.F32_BUDGET, (what, e_l, e_p)
    assert ok, what
    return max(e_l, e_p)


# ---- (a) batched encodes ---------------------------------------------------------------------------------------------
# (B, T'): T' = 1, 2, 3, odd and even, a ragged batch; at F = 7 and 128 also B * ceil(T' / 2) = 32 and 33 output-frame
# pairs, so that a 32-row tile boundary of the pair form falls on a pair (F2 = 1) or inside one (F2 = 31)
CASES = [(1, 1), (1, 2), (1, 3), (3, 9)]
EDGE_CASES = {7: [(1, 64), (1, 66), (2, 31), (3, 22)], 128: [(1, 64), (1, 66), (2, 31), (3, 22)]}


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("F,B,Tp", [(F, b, t) for F in WIDTHS for b, t in CASES + EDGE_CASES.get(F, [])])
def test_batched_front_end_widths(fam, F, B, Tp):
    x, lens, ref = _ref(fam, F, B, Tp, seed=F * 131 + B * 17 + Tp)
    m = _model(fam, F)
    try:
        for fused in (1, 0):
            m.set_front_fused(fused)
            for skip in (False, True):
                m.set_skip_padding(skip)
                probs, logits = m.get_encoder_out(x, lens, return_logits=True)
                torch.cuda.synchronize()
                lens_out = m.valid_out_frames(lens, x.shape[1]).cpu().numpy() if skip else None
                _check_logits(f"{fam} F={F} B={B} T'={Tp} fused={fused} skip={skip}", probs, logits, ref, lens_out)
    finally:
        m.set_front_fused(-1)
        m.set_skip_padding(False)


@pytest.mark.parametrize("F", WIDTHS)
def test_front_end_output_through_debug_taps(F):
    """The front end's own output (the first M * 256 tap floats: x0 = embed(conv2(conv1(cmvn(x)))) * sqrt(d)) against the
    oracle's, so that a width bug is pinned on the front end and not on a later layer"""
    _, sd, conf, kw = _spec("conformer", F)
    m = _cls("conformer")(F, 97, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    oracle = _oracle("conformer", F)
    B, Tp = 3, 9
    x, lens = _inputs(F, B, Tp, seed=F + 1)
    M = B * Tp
    taps = m.set_debug_taps(M * 256 + 1 * (M * 256 * 5 + M * 768))
    probs, logits = m.get_encoder_out(x, lens, return_logits=True)
    torch.cuda.synchronize()
    x0 = taps[:M * 256].cpu().numpy().reshape(B, Tp, 256)
    with torch.no_grad():
        enc, _, layers = oracle.encoder_forward(x, lens, return_layers=True)
        ref_logits = oracle.ctc_logits(enc)
    e0 = nm.utt_rel(x0, layers[0])
    print(f"[widths] conformer F={F} front-end output x0: {e0:.2e}")
    assert e0 < nm.F32_BUDGET, (F, e0)
    _check_logits(f"conformer F={F} taps route", probs, logits, ref_logits)
    m.set_debug_taps(0)


# ---- (b) the other input layers and 512 channels ---------------------------------------------------------------------
GENERAL = ([("conv2d6", F, 256) for F in (11, 40, 128)] + [("conv2d8", F, 256) for F in (15, 40, 128)]
           + [("linear", F, 256) for F in (1, 7, 81, 128)] + [("conv2d", F, 512) for F in (7, 128)])


def _input_layer_model(il, F, width=256):
    """-> (model, float64 oracle): one Conformer block behind input layer `il` at F bins and `width` channels"""
    def make():
        from ppasr_amd.model_utils.conformer.model import ConformerModel
        heads, V = width // 64, 53
        sd = conformer_state_dict(input_dim=F, vocab_size=V, num_blocks=1, seed=600 + F + width, perturb_norm=True,
                                  output_size=width, attention_heads=heads, input_layer=il)
        conf = dict(output_size=width, attention_heads=heads, linear_units=2048, num_blocks=1, cnn_module_kernel=15,
                    input_layer=il)
        m = ConformerModel(F, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
        return m, nm.oracle64("conformer", sd, num_blocks=1, attention_heads=heads, cnn_module_kernel=15)
    return MEMO.get(("input_layer", il, F, width), make)


T_MIN = {"linear": 1, "conv2d": 7, "conv2d6": 11, "conv2d8": 15}


def _check_input_layer(il, F, width, B, T, lens):
    m, oracle = _input_layer_model(il, F, width)
    x, la = synth_features(B, T, n_mels=F, lens=lens, seed=F + T)
    probs, logits = m.get_encoder_out(x, la, return_logits=True)
    torch.cuda.synchronize()
    ref = oracle.get_encoder_out(x, la, return_logits=True)[1]
    _check_logits(f"{il} F={F} d={width} B={B} T={T}", probs, logits, ref)


@pytest.mark.parametrize("il,F,width", GENERAL)
def test_input_layers_and_widths(il, F, width):
    t_min = T_MIN[il]
    T = 23 if il == "linear" else 61
    for B, Tb, lens in ((3, T, [T, T // 2 + t_min, t_min]), (1, t_min, [t_min])):
        _check_input_layer(il, F, width, B, Tb, lens)


# conv2d8 at F2 = 3 (F = 15 .. 18): the embed's K-split partial sums (S = 8 tiles of M = B T' rows) go to conv2's output
# buffer, which holds B T2 F2 >= 6 M + 3 B rows of its own -- short of 8 M from T' = 4 on.  Shapes whose overflow does not
# line up row for row with the next buffer (the embed's output): T' = 7 (T = 67), 12 (T = 101), 16 (T = 131).
@pytest.mark.parametrize("F,B,T", [(15, 1, 67), (15, 2, 101), (18, 1, 67), (18, 2, 101), (16, 4, 131)])
def test_conv2d8_embed_split_scratch(F, B, T):
    _check_input_layer("conv2d8", F, 256, B, T, [T] + [T - 8 * k for k in range(1, B)])


# ---- (c) streaming chunks --------------------------------------------------------------------------------------------
# chunk lengths in feature frames.  At 128 bins the chunk's conv2 has c * F2 rows: 868 at 115 frames (c = 28, K split),
# 899 at 119 (c = 29, unsplit); at 80 bins 893 at 191 (c = 47) and 912 at 195 (c = 48).  A chunk with an odd c comes last:
# behind the stride layer the next chunk's half-rate cache would not line up (the reference fails there too).
CHUNKS = {7: [67, 67, 35, 7], 40: [67, 67, 35, 7], 128: [67, 115, 67, 119], 80: [67, 195, 191]}


def _ref_chunk(oracle, chunk, offset, required, att, cnn):
    with torch.no_grad():
        xs, att, cnn = oracle.forward_chunk(chunk, offset, required, att, cnn)
        return oracle.ctc_logits(xs), att, cnn


def _stream_against_oracle(m, oracle, F, lengths, required, what):
    x, _ = synth_features(1, sum(lengths), n_mels=F, seed=F + 71)
    stream = m.new_stream()
    att = cnn = None
    offset, a, worst = 0, 0, 0.0
    for T in lengths:
        chunk = x[:, a:a + T]
        a += T
        ref, att, cnn = _ref_chunk(oracle, chunk, offset, required, att, cnn)
        got = stream.encode_chunk(chunk, required)
        g_att, g_cnn = stream.export_caches()
        torch.cuda.synchronize()
        assert tuple(got.shape) == tuple(ref.shape) and tuple(g_att.shape) == tuple(att.shape), T
        assert torch.isfinite(got).all(), T
        errs = [nm.utt_rel(got, torch.softmax(ref, -1)), nm.logprob_err(got, ref), nm.utt_rel(g_att, att),
                nm.utt_rel(g_cnn, cnn) if cnn.numel() else 0.0]
        worst = max(worst, *errs)
        assert max(errs) < nm.F32_BUDGET, (T, errs)
        offset += ref.shape[1]
    print(f"[widths] {what} F={F} chunks {lengths} required={required}: worst {worst:.2e}")


@pytest.mark.parametrize("required", [-16, 32])
@pytest.mark.parametrize("F", [7, 40, 128, 80])
@pytest.mark.parametrize("fam", FAMILIES)
def test_stream_chunks_widths(fam, F, required):
    _stream_against_oracle(_model(fam, F), _oracle(fam, F), F, CHUNKS[F], required, fam)


@pytest.mark.parametrize("required", [-16, 32])
@pytest.mark.parametrize("il,F", [("conv2d8", 15), ("conv2d8", 18), ("conv2d8", 40), ("conv2d6", 11), ("conv2d6", 40)])
def test_input_layer_stream_chunks(il, F, required):
    """the 6x / 8x front ends chunk by chunk (conv2d8 at F2 = 3: the embed's K split into conv2's output buffer)"""
    m, oracle = _input_layer_model(il, F)
    _stream_against_oracle(m, oracle, F, [67, 131, 67, 35, T_MIN[il]], required, il)


# ---- (d) session groups ----------------------------------------------------------------------------------------------
ROUNDS = [([0, 1, 2], 67), ([2, 0], 67), ([1, 2, 0], 35)]


def _group(fam, m, n):
    if fam == "conformer":
        from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup as G
    elif fam == "squeezeformer":
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup as G
    else:
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup as G
    return G(m, n)


@pytest.mark.parametrize("F", [7, 128])
@pytest.mark.parametrize("fam", FAMILIES)
def test_session_group_widths(fam, F):
    m, oracle = _model(fam, F), _oracle(fam, F)
    group = _group(fam, m, 3)
    state = {s: (None, None, 0) for s in range(3)}
    worst = 0.0
    for r, (act, T) in enumerate(ROUNDS):
        x, _ = synth_features(len(act), T, n_mels=F, seed=F * 7 + r)
        _, _, probs = group.encode_chunks(act, x, want_probs=True)
        torch.cuda.synchronize()
        assert torch.isfinite(probs).all(), r
        for k, s in enumerate(act):
            att, cnn, off = state[s]
            ref, att, cnn = _ref_chunk(oracle, x[k:k + 1], off, -16, att, cnn)
            state[s] = (att, cnn, off + ref.shape[1])
            e = max(nm.utt_rel(probs[k:k + 1], torch.softmax(ref, -1)), nm.logprob_err(probs[k:k + 1], ref))
            worst = max(worst, e)
            assert e < nm.F32_BUDGET, (r, s, e)
            assert group.offset(s) == state[s][2], (r, s)
    print(f"[widths] {fam} F={F} session group: worst {worst:.2e}")


# ---- (e) DeepSpeech2 -------------------------------------------------------------------------------------------------
def _ds2(F, gru, streaming, L=2, V=89):
    def make():
        sd = deepspeech2_state_dict(input_dim=F, vocab_size=V, num_rnn_layers=L, streaming=streaming,
                                    seed=700 + F + 2 * gru + streaming, perturb_norm=True, use_gru=gru)
        from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
        model = DeepSpeech2Model(F, V, streaming=streaming, encoder_conf=dict(num_rnn_layers=L, rnn_size=1024, use_gru=gru),
                                 state_dict=sd, device="cuda:0")
        oracle = nm.oracle64("deepspeech2", sd, num_rnn_layers=L, rnn_size=1024, streaming=streaming, use_gru=gru)
        return model, oracle
    return MEMO.get(("ds2", F, gru, streaming), make)


@pytest.mark.parametrize("gru", [False, True])
@pytest.mark.parametrize("streaming", [True, False])
@pytest.mark.parametrize("F", [7, 40, 82])
def test_deepspeech2_widths(F, gru, streaming):
    """F = 82: F1 = 40, conv2's full tile[3][40][32]; two calls, the first one's final states starting the second"""
    model, oracle = _ds2(F, gru, streaming)
    B, T = 3, 61
    x, lens = synth_features(B, 2 * T, n_mels=F, lens=[T, 40, 9], seed=F + 3)
    h = c = rh = rc = None
    worst = 0.0
    for s0 in (0, T):
        chunk = x[:, s0:s0 + T]
        probs, out_lens, h, c = model.get_encoder_out_chunk(chunk, lens, h if streaming else None, c if streaming else None)
        rp, rl, rh, rc = oracle.forward(chunk, lens, rh if streaming else None, rc if streaming else None)
        torch.cuda.synchronize()
        assert out_lens.cpu().tolist() == rl.tolist()
        assert torch.isfinite(probs).all()
        errs = [nm.utt_rel(probs, rp, rl), nm.logprob_err(probs, torch.log(rp), rl), nm.utt_rel(h, rh)]
        if not gru:
            errs.append(nm.utt_rel(c, rc))
        worst = max(worst, *errs)
        assert max(errs) < nm.F32_BUDGET_DS2, (s0, errs)
        assert nm.frame_ids_ok(torch.log(probs.cpu()), torch.log(rp), nm.F32_BUDGET_DS2, rl)[0], s0
    print(f"[widths] deepspeech2 F={F} gru={gru} streaming={streaming}: worst {worst:.2e}")


@pytest.mark.parametrize("F", [7, 82])
def test_deepspeech2_session_group_widths(F):
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2StreamGroup
    model, oracle = _ds2(F, False, True)
    group = DeepSpeech2StreamGroup(model, 3)
    state = {s: (None, None) for s in range(3)}
    worst = 0.0
    for r, (act, T) in enumerate(ROUNDS):
        x = torch.from_numpy(synth_features(len(act), T, n_mels=F, seed=F * 5 + r)[0]).cuda()
        _, _, probs = group.encode_chunks(act, x, want_probs=True)
        torch.cuda.synchronize()
        for k, s in enumerate(act):
            rp, rl, rh, rc = oracle.forward(x[k:k + 1].cpu().double(), np.array([T]), *state[s])
            state[s] = (rh, rc)
            e = max(nm.utt_rel(probs[k:k + 1], rp), nm.logprob_err(probs[k:k + 1], torch.log(rp)))
            worst = max(worst, e)
            assert e < nm.F32_BUDGET_DS2, (r, s, e)
    print(f"[widths] deepspeech2 F={F} session group: worst {worst:.2e}")


# ---- (f) the fp16 x3 mode --------------------------------------------------------------------------------------------
TOL_F16X3 = 1e-3  # that mode's own tolerance (tests/test_ref_pin_gpu.py)


@pytest.mark.parametrize("F", [7, 128])
def test_f16x3_front_end_widths(F):
    """k_conv_stage_h3 / k_embed_h3 at K other than 80 bins'"""
    _, sd, conf, _ = _spec("conformer", F)
    m = _cls("conformer")(F, 97, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    m.set_gemm_mode("f16x3")
    assert "front" in m.gemm_coverage(), m.gemm_coverage()
    for B, Tp in ((1, 3), (3, 9), (2, 31)):
        x, lens, ref = _ref("conformer", F, B, Tp, seed=F * 131 + B * 17 + Tp)
        probs, logits = m.get_encoder_out(x, lens, return_logits=True)
        torch.cuda.synchronize()
        assert torch.isfinite(logits).all()
        e_l, e_p = nm.utt_rel(logits, ref), nm.logprob_err(probs, ref)
        print(f"[widths] f16x3 conformer F={F} B={B} T'={Tp}: logits {e_l:.2e} logprobs {e_p:.2e}")
        assert e_l < TOL_F16X3 and e_p < TOL_F16X3, (B, Tp, e_l, e_p)


# ---- (g) refused widths ----------------------------------------------------------------------------------------------
def _create_status(il, F, ds2=False):
    """status of creating a handle of input width F (the weights of an 80-bin model: every refusal comes before the
    weights are read)"""
    try:
        if ds2:
            from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
            sd = deepspeech2_state_dict(vocab_size=31, num_rnn_layers=1, rnn_size=1024, seed=9)
            DeepSpeech2Model(F, 31, streaming=True, encoder_conf=dict(num_rnn_layers=1, rnn_size=1024), state_dict=sd,
                             device="cuda:0")
        else:
            from ppasr_amd.model_utils.conformer.model import ConformerModel
            sd = conformer_state_dict(vocab_size=31, num_blocks=1, seed=9, input_layer=il)
            ConformerModel(F, 31, streaming=True, state_dict=sd, device="cuda:0",
                           encoder_conf=dict(num_blocks=1, input_layer=il))
    except _lib.PPASRHipError as e:
        return e.status
    return _lib.PPASR_OK


@pytest.mark.parametrize("il,F,status", [("conv2d", 6, _lib.PPASR_EUNSUPPORTED), ("conv2d", 129, _lib.PPASR_EUNSUPPORTED),
                                         ("ds2", 83, _lib.PPASR_EUNSUPPORTED)]
                         + [("conv2d6", F, _lib.PPASR_EINVAL) for F in (7, 8, 9, 10)]
                         + [("conv2d8", 14, _lib.PPASR_EINVAL)])
def test_refused_widths(il, F, status):
    """conv2d6 at F = 7 .. 10 (F1 = 3, 4): (F1 - 5) / 3 truncated toward zero gave F2 = 1, and the 5-wide conv read
    past the end of each conv1 row"""
    assert _create_status(il, F, ds2=il == "ds2") == status


@pytest.mark.parametrize("il,F", [("conv2d6", 11), ("conv2d8", 15), ("ds2", 82)])
def test_smallest_and_largest_accepted_widths(il, F):
    if il == "ds2":
        sd = deepspeech2_state_dict(input_dim=F, vocab_size=31, num_rnn_layers=1, rnn_size=1024, seed=9)
        from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
        DeepSpeech2Model(F, 31, streaming=True, encoder_conf=dict(num_rnn_layers=1, rnn_size=1024), state_dict=sd,
                         device="cuda:0")
    else:
        from ppasr_amd.model_utils.conformer.model import ConformerModel
        sd = conformer_state_dict(input_dim=F, vocab_size=31, num_blocks=1, seed=9, input_layer=il)
        ConformerModel(F, 31, streaming=True, state_dict=sd, device="cuda:0", encoder_conf=dict(num_blocks=1, input_layer=il))


@pytest.mark.parametrize("fam", FAMILIES + ["deepspeech2"])
def test_features_of_the_wrong_width_are_refused(fam):
    F = 40
    if fam == "deepspeech2":
        model, _ = _ds2(F, False, True)
        with pytest.raises(AssertionError):
            model.get_encoder_out(*synth_features(1, 67, n_mels=F + 1, seed=1))
        with pytest.raises(AssertionError):
            model.get_encoder_out_chunk(*synth_features(1, 67, n_mels=F - 1, seed=1))
        return
    m = _model(fam, F)
    for n_mels in (F - 1, F + 1):
        with pytest.raises(AssertionError):
            m.get_encoder_out(*synth_features(1, 67, n_mels=n_mels, seed=1))
        with pytest.raises(AssertionError):
            m.new_stream().encode_chunk(synth_features(1, 67, n_mels=n_mels, seed=1)[0])


# ---- (h) chunk workspace ---------------------------------------------------------------------------------------------
def _nondecreasing(sizes, what):
    drops = [(T, sizes[T - 1], sizes[T]) for T in sorted(sizes) if T - 1 in sizes and sizes[T] < sizes[T - 1]]
    assert not drops, (what, drops[:4])


@pytest.mark.parametrize("F", [7, 40, 80, 128])
@pytest.mark.parametrize("fam", FAMILIES)
def test_chunk_workspace_never_shrinks(fam, F):
    m = _model(fam, F)
    lib = m.lib
    sizes = {T: int(lib.ppasr_chunk_workspace_bytes(m._h, T)) for T in range(7, 261)}
    # the conv2 K-split's row limit: c * F2 = 896 (80 bins: T = 191 / 195; 128 bins: T = 115 / 119)
    F2 = ((F - 1) // 2 - 1) // 2
    rows = lambda T: ((T - 1) // 2 - 1) // 2 * F2  # conv2 rows of a T-frame chunk
    edge = [T for T in range(8, 261) if rows(T - 1) <= 896 < rows(T)]
    print(f"[widths] {fam} F={F} chunk workspace bytes around the split limit: "
          + ", ".join(f"T={T - 1}: {sizes[T - 1]}, T={T}: {sizes[T]}" for T in edge))
    _nondecreasing(sizes, (fam, F))
    for n in (1, 3, 8):
        _nondecreasing({T: int(lib.ppasr_group_chunk_workspace_bytes(m._h, n, T)) for T in range(7, 261)}, (fam, F, n))
    # one workspace sized for the longest chunk serves every shorter one (offsets from 0 again after each)
    ws = torch.empty(sizes[260], dtype=torch.uint8, device="cuda:0")
    stream = m.new_stream()
    x, _ = synth_features(1, 260, n_mels=F, seed=F)
    xd = torch.from_numpy(x).cuda()
    for T in sorted({7, 8, 11, 35, 67, 114, 115, 118, 119, 190, 191, 194, 195, 259, 260} | set(edge) | {T - 1 for T in edge}):
        stream.reset()
        c = m.out_frames(T)
        probs = torch.empty(1, c, m.vocab_size, dtype=torch.float32, device="cuda:0")
        c_out = ctypes.c_int(0)
        st = lib.ppasr_encode_chunk(stream._s, xd.data_ptr(), T, -1, probs.data_ptr(), None, None, ctypes.byref(c_out),
                                    ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert st == _lib.PPASR_OK, (T, st, lib.ppasr_last_error())
        torch.cuda.synchronize()
        assert c_out.value == c and torch.isfinite(probs).all(), T


@pytest.mark.parametrize("F", [7, 82])
def test_deepspeech2_workspace_never_shrinks(F):
    """the dense layers' K-split scratch ends at 512 stacked frames (n = 8: T = 262 / 263)"""
    model, _ = _ds2(F, False, True)
    lib = model.lib
    for n in (1, 3, 8):
        _nondecreasing({T: int(lib.ppasr_group_chunk_workspace_bytes(model._h, n, T)) for T in range(7, 301)}, (F, n))
        _nondecreasing({T: int(lib.ppasr_ds2_workspace_bytes(model._h, n, T)) for T in range(7, 301)}, (F, n, "batched"))
