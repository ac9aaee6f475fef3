"""Shared cases of the off-centre / saturated-activation tests (a plain module: tests/test_offcentre_cases_cpu.py,
tests/test_offcentre_gpu.py).

A randomly initialised checkpoint (ppasr_amd/utils/synth.py) feeds every LayerNorm rows whose mean is ~0 against their
spread, and keeps every gate, swish and GLU in its linear range; a trained one does neither.  The state-dict
transformers below move a synth checkpoint off both: `offset_*` make LayerNorm rows with |row mean| >> row std,
`saturate_*` push swish / GLU / gate pre-activations past the fp32 range of exp (|x| > 88.7).  Each case states the
conditioning it is meant to reach (`level`, on the LayerNorms `where` names) and `conditioning()` measures it on a float64
oracle run, so a case that silently stopped being off-centre fails the CPU test.

The mutations restate in the float64 oracles the arithmetic a kernel might use and must not: a LayerNorm with fp32
one-pass statistics (`ln_one_pass`), the DeepSpeech2 wavefront's LayerNorm fold on the raw row (`ds2_wave_fold`) and a
sigmoid written e / (1 + e) (`sigmoid_exp_ratio`)."""
import contextlib

import numpy as np
import torch

from ppasr_amd.utils.synth import (conformer_state_dict, deepspeech2_state_dict, efficient_conformer_state_dict,
                                   squeezeformer_state_dict)

# ---- models -----------------------------------------------------------------------------------------------------------
# name -> (family of numerics.oracle64, state dict maker, encoder_conf of the model class, oracle kwargs, time reduction)
_EFF_CONF = dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3, stride_kernel=True)
DS2_V, DS2_H = 89, 1024


def _ds2(L, H, gru, seed, streaming=True):
    return ("deepspeech2",
            lambda: deepspeech2_state_dict(vocab_size=DS2_V, num_rnn_layers=L, rnn_size=H, streaming=streaming, seed=seed,
                                           perturb_norm=True, use_gru=gru),
            dict(num_rnn_layers=L, rnn_size=H, use_gru=gru),
            dict(num_rnn_layers=L, rnn_size=H, streaming=streaming, use_gru=gru), 4)


MODELS = {
    "conformer": ("conformer", lambda: conformer_state_dict(vocab_size=97, num_blocks=2, seed=321, perturb_norm=True),
                  dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15),
                  dict(num_blocks=2), 4),
    "general": ("conformer", lambda: conformer_state_dict(vocab_size=97, num_blocks=2, seed=322, perturb_norm=True,
                                                          output_size=512, attention_heads=8),
                dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=2, cnn_module_kernel=15),
                dict(num_blocks=2, attention_heads=8), 4),
    "linear": ("conformer", lambda: conformer_state_dict(vocab_size=97, num_blocks=1, seed=323, perturb_norm=True,
                                                         output_size=512, attention_heads=8, input_layer="linear"),
               dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=1, cnn_module_kernel=15,
                    input_layer="linear"),
               dict(num_blocks=1, attention_heads=8), 1),
    "efficient_conformer": ("efficient_conformer",
                            lambda: efficient_conformer_state_dict(vocab_size=113, num_blocks=4, seed=324, perturb_norm=True,
                                                                   stride_layer_idx=1, group_layer_idx=(0, 1)),
                            dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                                 cnn_module_norm="layer_norm", efficient_conf=_EFF_CONF),
                            dict(num_blocks=4, stride_layer_idx=1, group_layer_idx=(0, 1)), 8),
    "squeezeformer": ("squeezeformer",
                      lambda: squeezeformer_state_dict(vocab_size=131, num_blocks=4, seed=325, perturb_norm=True),
                      dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=4, reduce_idx=1, recover_idx=3,
                           feed_forward_expansion_factor=8, cnn_module_kernel=31),
                      dict(num_blocks=4, reduce_idx=1, recover_idx=3), 4),
    "ds2_lstm": _ds2(3, DS2_H, False, 331),
    "ds2_gru": _ds2(3, DS2_H, True, 332),
    "ds2_lstm_l2": _ds2(2, DS2_H, False, 333),
    "ds2_gru_l2": _ds2(2, DS2_H, True, 334),
    "ds2_lstm_h2048": _ds2(2, 2048, False, 335),
    "ds2_lstm_bi": _ds2(2, DS2_H, False, 336, streaming=False),
}


def make_model(model, sd, device="cuda:0"):
    """the product model class of `model` on `sd`"""
    fam, _, conf, _, _ = MODELS[model]
    V = int(sd["decoder.ctc_lo.bias" if fam == "deepspeech2" else "ctc.ctc_lo.bias"].shape[0])
    if fam == "deepspeech2":
        from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
        return DeepSpeech2Model(80, V, streaming=MODELS[model][3]["streaming"], encoder_conf=conf, state_dict=sd, device=device)
    if fam == "conformer":
        from ppasr_amd.model_utils.conformer.model import ConformerModel as M
    elif fam == "squeezeformer":
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
    else:
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
    return M(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device=device)


# ---- state-dict transformers (each returns a new dict; the arrays it changes are copies) ---------------------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def offset_embed(sd, c):
    """a constant on the bias of the embedding's projection: every row of the residual stream moves by c * sqrt(d)
    (`linear` models: the rows that enter the embedding's own LayerNorm move by c)"""
    sd = dict(sd)
    sd["encoder.embed.out.0.bias"] = _f32(np.asarray(sd["encoder.embed.out.0.bias"]) + np.float32(c))
    return sd


def offset_squeezeformer(sd, c):
    """post-LN blocks: the embedding's offset is gone after `preln`, so the constant also goes on the bias of every module
    output and every LayerNorm of every block sees an off-centre sum"""
    sd = dict(sd)
    keys = ["encoder.embed.input_proj.0.bias"] + [k for k in sd if k.startswith("encoder.encoders.") and k.endswith(
        (".w_2.bias", ".linear_out.bias", ".pointwise_conv2.bias"))]
    for k in keys:
        sd[k] = _f32(np.asarray(sd[k]) + np.float32(c))
    return sd


def saturate_transformer(sd, factor, glu_factor=None):
    """w_1 (weight and bias) of every feed-forward module and the gate half of every pointwise_conv1 scaled: swish and
    GLU pre-activations of several tens up to past the fp32 range of exp"""
    sd = dict(sd)
    for k in list(sd):
        if k.endswith((".w_1.weight", ".w_1.bias")):
            sd[k] = _f32(np.asarray(sd[k]) * np.float32(factor))
        elif k.endswith((".pointwise_conv1.weight", ".pointwise_conv1.bias")):
            a = np.array(sd[k], np.float32)
            a[a.shape[0] // 2:] *= np.float32(glu_factor or factor)  # F.glu: the second half of the channels is the gate
            sd[k] = a
    return sd


def _ds2_gates(sd, use_gru, scale, shifts):
    sd = dict(sd)
    G = 3 if use_gru else 4
    for k in list(sd):
        if ".weight_ih" in k or ".weight_hh" in k:
            sd[k] = _f32(np.asarray(sd[k]) * np.float32(scale))
        elif ".bias_ih" in k:
            a = np.array(sd[k], np.float32)
            H = a.shape[0] // G
            for g, s in enumerate(shifts):
                a[g * H:(g + 1) * H] += np.float32(s)
            sd[k] = a
    return sd


def offset_ds2(sd, use_gru, scale, shifts):
    """recurrent and input weights scaled down, gate biases shifted (LSTM: i, f, g, o; GRU: r, z, c): every unit's h sits
    near one value with a small spread, so the rows that enter the LayerNorms are off-centre"""
    return _ds2_gates(sd, use_gru, scale, shifts)


def saturate_ds2(sd, use_gru, shifts):
    """gate biases of several tens on top of the synth weights: sigmoids at 0 / 1 and past the fp32 range of exp"""
    return _ds2_gates(sd, use_gru, 1.0, shifts)


# ---- cases ------------------------------------------------------------------------------------------------------------
class Case:
    """name; model (MODELS key); kind: "offcentre" (level = median |row mean| / row std that every LayerNorm `where`
    accepts must reach) or "saturated" (level = largest |pre-activation| of a swish, GLU gate or recurrent gate);
    make(sd) -> transformed state dict"""

    def __init__(self, name, model, kind, level, make, where=None):
        self.name, self.model, self.kind, self.level, self.make, self.where = name, model, kind, level, make, where

    def sd(self):
        return self.make(MODELS[self.model][1]())

    def __repr__(self):
        return self.name


def _layer0(prefix):
    """pre-LN blocks end in norm_final, which centres the stream again: the offset reaches the five norms of block 0"""
    return prefix.startswith("encoder.encoders.0.norm_")


def _sq_norms(prefix):
    return prefix == "encoder.preln" or ".layer_norm" in prefix


def _ds2_norms(prefix):
    return prefix.startswith("encoder.layernorm_list.")


def _embed_ln(prefix):
    return prefix == "encoder.embed.out.1"


# past 88.73 = log(FLT_MAX): exp overflows in fp32.  LSTM: i, o open and f shut; GRU: r open, z shut
LSTM_SAT, GRU_SAT = (95.0, -95.0, 0.0, 95.0), (95.0, -95.0, 0.0)
# (weight scale, gate-bias shifts) of the two off-centre levels.  Levels of about 10 are not here: at |mean| / std = 4 .. 24
# (LSTM) and 9 .. 14 (GRU) the one-pass mutations moved the output by 0.4 .. 3.5 tolerances, below the margin of
# tests/test_offcentre_cases_cpu.py, so the lower level is the smallest one that cleared it with room; past the upper
# one the fp32 oracle's own error grows faster than the mutations' (LSTM 0.05 / +-6: fold 2.8 x tol; GRU 0.03: 3.8 x).
DS2_LEVELS = {False: [(85.0, 0.3, (4.0, -4.0, 2.0, 4.0)), (380.0, 0.1, (5.0, -5.0, 2.0, 5.0))],
              True: [(40.0, 0.06, (0.0, -4.0, 1.0)), (85.0, 0.08, (0.0, -4.0, 1.5))]}


def _ds2_cases(model, gru):
    tag = model.replace("ds2_", "")
    out = [Case(f"{tag}/off_{n}", model, "offcentre", level, lambda sd, sc=scale, sh=shifts: offset_ds2(sd, gru, sc, sh),
                _ds2_norms) for n, (level, scale, shifts) in zip(("lo", "hi"), DS2_LEVELS[gru])]
    out.append(Case(f"{tag}/saturated", model, "saturated", 90.0, lambda sd: saturate_ds2(sd, gru, GRU_SAT if gru else LSTM_SAT)))
    return out


# Transformer levels: an offset of about 10 standard deviations (the embedding bias + 3) moved the one-pass LayerNorm
# mutation by 0.3 .. 2 tolerances only, below the margin of tests/test_offcentre_cases_cpu.py; the lower level of each family
# is the smallest that cleared it with room, the upper one the largest tried whose tolerance stays under numerics.TOL_CAP.
CASES = {
    "conformer": [Case("conformer/off_lo", "conformer", "offcentre", 30.0, lambda sd: offset_embed(sd, 10.0), _layer0),
                  Case("conformer/off_hi", "conformer", "offcentre", 300.0, lambda sd: offset_embed(sd, 100.0), _layer0),
                  Case("conformer/saturated", "conformer", "saturated", 90.0, lambda sd: saturate_transformer(sd, 60.0))],
    "general": [Case("general/off_lo", "general", "offcentre", 75.0, lambda sd: offset_embed(sd, 20.0), _layer0),
                Case("general/off_hi", "general", "offcentre", 300.0, lambda sd: offset_embed(sd, 100.0), _layer0)],
    "linear": [Case("linear/off_lo", "linear", "offcentre", 150.0, lambda sd: offset_embed(sd, 100.0), _embed_ln),
               Case("linear/off_hi", "linear", "offcentre", 450.0, lambda sd: offset_embed(sd, 300.0), _embed_ln)],
    "efficient_conformer": [
        Case("efficient/off_lo", "efficient_conformer", "offcentre", 75.0, lambda sd: offset_embed(sd, 20.0), _layer0),
        Case("efficient/off_hi", "efficient_conformer", "offcentre", 300.0, lambda sd: offset_embed(sd, 100.0), _layer0),
        Case("efficient/saturated", "efficient_conformer", "saturated", 90.0, lambda sd: saturate_transformer(sd, 60.0))],
    "squeezeformer": [
        Case("squeezeformer/off_lo", "squeezeformer", "offcentre", 65.0, lambda sd: offset_squeezeformer(sd, 100.0), _sq_norms),
        Case("squeezeformer/off_hi", "squeezeformer", "offcentre", 160.0, lambda sd: offset_squeezeformer(sd, 250.0), _sq_norms),
        Case("squeezeformer/saturated", "squeezeformer", "saturated", 90.0, lambda sd: saturate_transformer(sd, 600.0, 60.0))],
    "ds2_lstm": _ds2_cases("ds2_lstm", False),
    "ds2_gru": _ds2_cases("ds2_gru", True),
}
# the same transforms on the other DeepSpeech2 shapes of the GPU test (two layers for the row tiles, H = 2048)
DS2_VARIANTS = {"ds2_lstm_l2": _ds2_cases("ds2_lstm_l2", False), "ds2_gru_l2": _ds2_cases("ds2_gru_l2", True),
                "ds2_lstm_h2048": _ds2_cases("ds2_lstm_h2048", False), "ds2_lstm_bi": _ds2_cases("ds2_lstm_bi", False)}
ALL_CASES = [c for cs in CASES.values() for c in cs]


def find(name):
    for cs in list(CASES.values()) + list(DS2_VARIANTS.values()):
        for c in cs:
            if c.name == name:
                return c
    raise KeyError(name)


# ---- conditioning -----------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def conditioning(oracle, lens_out=None):
    """Records on `oracle` while the block runs -> dict: "ln": {LayerNorm prefix: median |row mean| / row std over the
    valid rows}, "act": the largest |pre-activation| of a swish, a GLU gate or a recurrent gate.  lens_out: valid output
    frames per utterance at the encoder's full rate (None: all rows); a LayerNorm that sees fewer frames (time reduction,
    stride layers) is given its share of them."""
    import torch.nn.functional as F
    rec = {"ln": {}, "act": 0.0}
    orig_ln, orig_glu = oracle._ln, F.glu
    t_full = [None]

    def ln(x, prefix, eps=1e-5):
        x64 = x.detach().to(torch.float64)
        if x64.ndim == 3 and lens_out is not None:
            if t_full[0] is None:
                t_full[0] = x64.shape[1]
            f = max(1, round(t_full[0] / x64.shape[1]))
            rows = torch.cat([x64[b, :min(x64.shape[1], (int(n) + f - 1) // f)] for b, n in enumerate(lens_out)])
        else:
            rows = x64.reshape(-1, x64.shape[-1])
        if rows.shape[0]:
            ratio = rows.mean(-1).abs() / rows.std(-1, unbiased=False).clamp_min(1e-300)
            rec["ln"].setdefault(prefix, []).append(ratio)
        return orig_ln(x, prefix, eps)

    def act_rec(x):
        rec["act"] = max(rec["act"], float(x.detach().abs().max())) if x.numel() else rec["act"]

    def glu(x, dim=-1):
        act_rec(x.narrow(dim, x.shape[dim] // 2, x.shape[dim] // 2))
        return orig_glu(x, dim)

    oracle._ln = ln
    had_swish = hasattr(oracle, "_swish")
    if had_swish:
        orig_swish = oracle._swish

        def swish(x):
            act_rec(x)
            return orig_swish(x)
        oracle._swish = swish
    else:
        oracle.taps = {}
    F.glu = glu
    try:
        yield rec
    finally:
        F.glu = orig_glu
        del oracle._ln
        if had_swish:
            del oracle._swish
        else:
            rec["act"] = oracle.taps.get("gates", 0.0)
            oracle.taps = None
        rec["ln"] = {k: float(torch.cat(v).median()) for k, v in rec["ln"].items()}


def reached(case, rec):
    """-> (the conditioning the case reached, as its `level` is stated; the LayerNorms counted)"""
    if case.kind == "saturated":
        return rec["act"], []
    names = [k for k in rec["ln"] if case.where(k)]
    assert names, (case, sorted(rec["ln"]))
    return min(rec["ln"][k] for k in names), names


# ---- mutations (patches on ONE oracle instance) -------------------------------------------------------------------------
def ln_one_pass(oracle):
    """every LayerNorm with fp32 one-pass statistics: var = max(E[x^2] - E[x]^2, 0)"""
    def ln(x, prefix, eps=1e-5):
        x32 = x.to(torch.float32)
        mean = x32.mean(-1, keepdim=True)
        var = ((x32 * x32).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
        y = (x32 - mean) * torch.rsqrt(var + np.float32(eps))
        return y.to(x.dtype) * oracle.p[prefix + ".weight"] + oracle.p[prefix + ".bias"]
    oracle._ln = ln


def sigmoid_exp_ratio(oracle):
    """sigmoid(x) = e / (1 + e), e = exp(x) in fp32: inf / inf = NaN once x passes log(FLT_MAX) = 88.7 (the swish of
    the Transformer oracles, the gates of the DeepSpeech2 oracle)"""
    import torch.nn.functional as F

    def sig(x):
        e = torch.exp(x.to(torch.float32))
        return (e / (1.0 + e)).to(x.dtype)

    if hasattr(oracle, "_swish"):
        oracle._swish = lambda x: x * sig(x)
        return None
    oracle._sigmoid = sig
    return None


def ds2_wave_fold(oracle, slices=8, pivot=False):
    """The DeepSpeech2 wavefront kernel's LayerNorm fold, restated in fp32 numpy for layers >= 1 (csrc/ds2_kernels.hip
    k_lstm_wave, csrc/capi_ds2.hip ds2_create): W' = W_ih diag(gamma), s_n = its column sums and c_n = W_ih beta + b_ih
    (+ b_hh: LSTM), both summed in double and rounded; per K slice the fp32 sums of y, y^2 and y W' over the RAW row of the
    previous layer; then mean = sum / H, var = max(sumsq / H - mean^2, 0), rstd = 1 / sqrt(var + eps) and
    x W_ih^T + b = rstd * (acc - mean * s_n) + c_n.
    pivot=True: the same after a per-row pivot (the mean of the row's first four elements) is subtracted from the row --
    acc and the sums run on y - pivot and `mean` is the mean of y - pivot; the algebra is the same, exactly."""
    f32 = np.float32
    raw = {}
    orig_ln = oracle._ln
    G = 3 if oracle.use_gru else 4

    def ln(x, prefix, eps=1e-5):
        raw[int(prefix.rsplit(".", 1)[1])] = x.detach().to(torch.float64).numpy()
        return orig_ln(x, prefix, eps)

    table = {}

    def fold(l, prefix, sfx):
        y = raw[l - 1].astype(f32)                       # [B, T, H] raw rows, fp32 as the kernel holds them
        B, T, H = y.shape
        g64 = oracle.p[f"encoder.layernorm_list.{l - 1}.weight"].to(torch.float64).numpy()
        b64 = oracle.p[f"encoder.layernorm_list.{l - 1}.bias"].to(torch.float64).numpy()
        w64 = oracle.p[prefix + "weight_ih" + sfx].to(torch.float64).numpy()  # [G H, H]
        bias = oracle.p[prefix + "bias_ih" + sfx].to(torch.float64).numpy()
        if G == 4:
            bias = bias + oracle.p[prefix + "bias_hh" + sfx].to(torch.float64).numpy()
        wp = (g64.astype(f32)[None, :] * w64.astype(f32)).astype(f32)          # W' in fp32, as packed
        s_n = (w64.astype(f32).astype(np.float64) @ g64.astype(f32).astype(np.float64)).astype(f32)
        c_n = (w64.astype(f32).astype(np.float64) @ b64.astype(f32).astype(np.float64) + bias).astype(f32)
        rows = y.reshape(B * T, H)
        piv = rows[:, :4].mean(-1, dtype=f32, keepdims=True) if pivot else np.zeros((B * T, 1), f32)
        rows = (rows - piv).astype(f32)
        ks = H // slices
        ss = np.zeros(B * T, f32)
        qq = np.zeros(B * T, f32)
        acc = np.zeros((B * T, G * H), f32)
        for w in range(slices):
            r = rows[:, w * ks:(w + 1) * ks]
            ss = (ss + r.sum(-1, dtype=f32)).astype(f32)
            qq = (qq + (r * r).sum(-1, dtype=f32)).astype(f32)
            acc = (acc + r @ wp[:, w * ks:(w + 1) * ks].T).astype(f32)
        mean = (ss / f32(H)).astype(f32)
        var = np.maximum(qq / f32(H) - mean * mean, f32(0)).astype(f32)
        rstd = (f32(1) / np.sqrt(var + f32(1e-5))).astype(f32)
        vi = (rstd[:, None] * (acc - mean[:, None] * s_n[None, :]) + c_n[None, :]).astype(f32)
        # _xproj returns the input part without the bias the oracle adds itself
        return torch.from_numpy((vi.astype(np.float64) - bias[None, :]).reshape(B, T, G * H)).to(oracle.dtype)

    orig_xproj = oracle._xproj

    def xproj(x, bi, t, prefix, sfx):
        l = int(prefix.split(".")[2])
        if l == 0:
            return orig_xproj(x, bi, t, prefix, sfx)
        if l not in table:
            table[l] = fold(l, prefix, sfx)
        return table[l][bi, t]

    orig_forward = oracle.forward

    def forward(*a, **kw):
        raw.clear()
        table.clear()
        return orig_forward(*a, **kw)

    oracle._ln, oracle._xproj, oracle.forward = ln, xproj, forward
