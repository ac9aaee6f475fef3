"""The fused attention kernel (k_attn_out_glu, fp32) with the positional term of its scores folded into the keys:
(q + u) . k + (q + v) . p = (q + u) . (k + p) + d, d = (v - u) . p.  The QKV stage writes k + p, the kernel contracts 64
wide and starts every score from the load-time table d (csrc/conformer_kernels.h AttnArgs::dtab).

Every case forces the fused route (set_ffn_split(0)), is held to the float64 oracle at F32_BUDGET with the frame-id rule
(tests/numerics.py) and checks through the launch profile that k_attn_out_glu ran and that neither the stand-alone
plain-head attention (k_attention_t<64>) nor the fp16 x3 form did.  The Efficient-Conformer fixture's grouped layers 0 - 1
cannot take the fused kernel (it serves plain 4 x 64 heads); they run k_attention_t<192>, which the check admits for that
fixture only.  Dropping d moves the logits of these fixtures by 3e-3 .. 6e-3, 150 - 270 x the budget.

Key counts put U = keys + shift on and around the 64-key sub-block, the 128-key wave half and the 256-key block; with
B = 3 the first rows b * T' of the utterances give three different shifts (mod 8), masked keys sit at both ends, and the
32-row blocks of the producers straddle utterances (the positional row of batch row m is frame m mod T').  Each case
prints its worst error."""
import numpy as np
import pytest
import torch

import numerics as nm
from ppasr_amd import _lib
from ppasr_amd.utils.synth import conformer_state_dict, efficient_conformer_state_dict, synth_features

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
V = 64
WORST = [0.0, ""]


def _sharpen(sd, n_layers, factor=2.0):
    """q / k projections (weights and biases) and the position biases scaled: attention scores x factor^2 (the helper of
    tests/test_fp64_routes_gpu.py): with large scores d decides the softmax"""
    sd = dict(sd)
    for i in range(n_layers):
        p = f"encoder.encoders.{i}.self_attn"
        for k in (".linear_q.weight", ".linear_q.bias", ".linear_k.weight", ".linear_k.bias", ".pos_bias_u", ".pos_bias_v"):
            sd[p + k] = (np.asarray(sd[p + k]) * factor).astype(np.float32)
    return sd


def _spec(name):
    """-> (family, state dict, encoder_conf, oracle kwargs)"""
    if name.startswith("conformer"):
        sd = conformer_state_dict(vocab_size=V, num_blocks=4, seed=1234, perturb_norm=True)
        if "sharp" in name:
            sd = _sharpen(sd, 4)
        conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15)
        return "conformer", sd, conf, dict(num_blocks=4)
    # the Efficient-Conformer fixture of tests/test_fp64_routes_gpu.py: stride layer 1, grouped layers 0 - 1; layers 2 - 3 run
    # fused at half the frame rate with positional stride 2
    sd = efficient_conformer_state_dict(vocab_size=113, num_blocks=4, seed=141, perturb_norm=True, stride_layer_idx=1,
                                        group_layer_idx=(0, 1))
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                cnn_module_norm="layer_norm",
                efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3, stride_kernel=True))
    return "efficient_conformer", sd, conf, dict(num_blocks=4, stride_layer_idx=1, group_layer_idx=(0, 1))


def _model(name):
    def make():
        fam, sd, conf, _ = _spec(name)
        if fam == "conformer":
            from ppasr_amd.model_utils.conformer.model import ConformerModel as M
        else:
            from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
        return M(80, int(sd["ctc.ctc_lo.bias"].shape[0]), streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    return MEMO.get(("model", name), make)


def _ref(name, Tp, lens_tp, seed):
    """features of B = len(lens_tp) utterances padded to T' = Tp frames behind the 4x front end, utterance b with
    lens_tp[b] valid ones, and the float64 oracle's logits (computed once per fixture and input)"""
    T = 4 * Tp + 3
    x, lens = synth_features(len(lens_tp), T, lens=[min(T, 4 * n) if n < Tp else T for n in lens_tp], seed=seed)

    def run():
        fam, sd, _, kw = _spec(name)
        oracle = MEMO.get(("oracle", name), lambda: nm.oracle64(fam, sd, **kw))
        return oracle.get_encoder_out(x, lens, return_logits=True)[1]
    return x, lens, MEMO.get(("ref", name, Tp, tuple(lens_tp), seed), run)


def _lens_tp(Tp):
    return [Tp, 1 if Tp % 2 else 3, Tp // 2]


def _fused_kernels_ran(name, kernels):
    ran = {k.split("(")[0].strip() for k in kernels}
    assert "k_attn_out_glu" in ran, sorted(ran)
    assert "k_attn_out_glu_h3" not in ran, sorted(ran)
    alone = {k for k in ran if k.startswith("k_attention_t")}
    assert alone <= ({"k_attention_t<192>"} if name == "efficient" else set()), sorted(ran)


def _check(name, model, x, lens, ref_logits, what, skip_padding=False):
    """one fused run against the float64 logits -> (worst error, logits bytes)"""
    with _lib.kernel_profile() as kp:
        probs, logits = model.get_encoder_out(x, lens, return_logits=True)
        tokens, n_tok, _ = model.encode_greedy(x, lens, trim_to_length=skip_padding)
        torch.cuda.synchronize()
    _fused_kernels_ran(name, kp.kernels)
    assert tuple(logits.shape) == tuple(ref_logits.shape), what
    lens_out = model.valid_out_frames(lens, x.shape[1]).cpu().numpy() if skip_padding else None
    if skip_padding:
        for b, n in enumerate(lens_out):
            assert not bool(probs[b, n:].any()), (what, b)
    e_l = nm.utt_rel(logits, ref_logits, lens_out)
    e_p = nm.logprob_err(probs, ref_logits, lens_out)
    ok, near = nm.frame_ids_ok(logits, ref_logits, nm.F32_BUDGET, lens_out)
    if max(e_l, e_p) > WORST[0]:
        WORST[:] = [max(e_l, e_p), f"{name} {what}"]
    print(f"[fold] {name} {what}: logits {e_l:.2e} logprobs {e_p:.2e} near-ties {near}; worst so far {WORST[0]:.2e} at {WORST[1]}")
    assert e_l < nm.F32_BUDGET and e_p < nm.F32_BUDGET, (what, e_l, e_p)
    assert ok, what
    if near == 0:
        r = ref_logits.numpy()
        for b in range(x.shape[0]):
            n = int(lens_out[b]) if skip_padding else r.shape[1]
            assert np.array_equal(tokens[b, :int(n_tok[b])].cpu().numpy(), nm.collapse(r[b, :n].argmax(-1))), (what, b)
    return max(e_l, e_p), logits.cpu().numpy().tobytes()


class _Fused:
    """the handle on the fused route (ppasr_set_ffn_split(0)), the default restored afterwards"""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.model.set_ffn_split(0)
        return self.model

    def __exit__(self, *exc):
        self.model.set_ffn_split(-1)
        self.model.set_skip_padding(False)
        self.model.set_lengths_hint(None)


@pytest.mark.parametrize("Tp", [1, 7, 33, 63, 65, 127, 129, 193, 255, 257])
def test_key_count_edges(Tp):
    x, lens, ref = _ref("conformer", Tp, _lens_tp(Tp), 3 * Tp)
    with _Fused(_model("conformer")) as model:
        _check("conformer", model, x, lens, ref, f"T'={Tp} lens'={_lens_tp(Tp)}")


def test_skip_padding_with_hint():
    """the key loop stops at the last valid key; skipped row blocks write no K"""
    Tp = 129
    x, lens, ref = _ref("conformer", Tp, _lens_tp(Tp), 3 * Tp)
    with _Fused(_model("conformer")) as model:
        model.set_skip_padding(True)
        model.set_lengths_hint([int(v) for v in lens])
        _check("conformer", model, x, lens, ref, f"skip_padding+hint T'={Tp}", skip_padding=True)


@pytest.mark.parametrize("Tp", [17, 129, 257])
def test_efficient_conformer_stride_two(Tp):
    """layers 2 - 3 run fused on ceil(T' / 2) frames with positional stride 2"""
    x, lens, ref = _ref("efficient", Tp, _lens_tp(Tp), 3 * Tp)
    with _Fused(_model("efficient")) as model:
        _check("efficient", model, x, lens, ref, f"T'={Tp} lens'={_lens_tp(Tp)}")


def test_sharpened_attention():
    Tp = 90
    x, lens, ref = _ref("conformer_sharp", Tp, _lens_tp(Tp), 5 + Tp)
    with _Fused(_model("conformer_sharp")) as model:
        _check("conformer_sharp", model, x, lens, ref, f"B=3 T'={Tp}")


def test_sixteen_wave_producers():
    """the 32-row x 16-wave forms of the QKV stage (set_row_block(1032)) write k + p as well"""
    Tp = 65
    x, lens, ref = _ref("conformer", Tp, _lens_tp(Tp), 3 * Tp)
    with _Fused(_model("conformer")) as model:
        model.set_row_block(1032)
        try:
            with _lib.kernel_profile() as kp:
                _check("conformer", model, x, lens, ref, f"16-wave forms T'={Tp}")
        finally:
            model.set_row_block(-1)
    ran = {k.split("(")[0].strip() for k in kp.kernels}
    assert any(k.startswith("k_ffn_qkv_t<") for k in ran) and any(k.startswith("k_conv_ffn_t<") for k in ran), sorted(ran)


def test_second_run_is_bit_identical():
    Tp = 65
    x, lens, ref = _ref("conformer", Tp, _lens_tp(Tp), 3 * Tp)
    with _Fused(_model("conformer")) as model:
        _, first = _check("conformer", model, x, lens, ref, f"run 1 T'={Tp}")
        _, second = _check("conformer", model, x, lens, ref, f"run 2 T'={Tp}")
    assert first == second


def test_forced_split_in_between_reads_plain_keys():
    """ppasr_set_ffn_split(2) takes the two-kernel route: the QKV stage must write plain k again (the stand-alone attention
    contracts [k | p] itself), and the fused route afterwards must give its earlier bytes"""
    Tp = 129
    x, lens, ref = _ref("conformer", Tp, _lens_tp(Tp), 3 * Tp)
    with _Fused(_model("conformer")) as model:
        _, first = _check("conformer", model, x, lens, ref, f"fused T'={Tp}")
        model.set_ffn_split(2)
        with _lib.kernel_profile() as kp:
            logits = model.get_encoder_out(x, lens, return_logits=True)[1]
            torch.cuda.synchronize()
        ran = {k.split("(")[0].strip() for k in kp.kernels}
        assert "k_attention_t<64>" in ran and "k_attn_out_glu" not in ran, sorted(ran)
        e = nm.utt_rel(logits, ref)
        ok, _ = nm.frame_ids_ok(logits, ref, nm.F32_BUDGET)
        print(f"[fold] conformer forced split between fused runs T'={Tp}: logits {e:.2e}")
        assert e < nm.F32_BUDGET and ok, e
        model.set_ffn_split(0)
        _, again = _check("conformer", model, x, lens, ref, f"fused again T'={Tp}")
    assert first == again
