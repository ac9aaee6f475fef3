"""The fp32 error budgets of tests/numerics.py must be low enough to catch real kernel bugs and high enough for exact fp32
arithmetic (no GPU: the oracles on the CPU).  Per family, on a small perturbed-norm fixture with a ragged batch:
- the floor: the fp32 oracle against the float64 oracle stays below a tenth of the budget;
- each mutation of a fixed list of realistic kernel bugs (a lost bias term of one head, a dropped FFN hidden unit, a
  dropped depthwise tap, a wrong LayerNorm eps, an ignored key mask, ...) moves the float64 oracle's output by at least
  5x the budget -- so a kernel with that bug fails the GPU tests held to the budget;
- no budget constant exceeds 1e-4.
Mutations change a state-dict entry or patch a method on one oracle instance; the oracle sources stay as they are."""
import functools

import numpy as np
import pytest
import torch

import numerics as nm
from ppasr_amd.utils.synth import (conformer_state_dict, deepspeech2_state_dict, efficient_conformer_state_dict,
                                   squeezeformer_state_dict, synth_features)

LENS = [333, 280, 120]
DS2_LENS = [300, 210]
MARGIN = 5.0  # each mutation must move the output by at least this many budgets


def _fixture(family):
    if family == "conformer":
        sd = conformer_state_dict(vocab_size=97, num_blocks=2, seed=21, perturb_norm=True)
        return sd, dict(num_blocks=2), 4
    if family == "squeezeformer":
        sd = squeezeformer_state_dict(vocab_size=131, num_blocks=4, seed=23, perturb_norm=True)
        return sd, dict(num_blocks=4, reduce_idx=1, recover_idx=3), 4
    if family == "efficient_conformer":
        sd = efficient_conformer_state_dict(vocab_size=113, num_blocks=4, seed=22, perturb_norm=True, stride_layer_idx=1,
                                            group_layer_idx=(0, 1))
        return sd, dict(num_blocks=4, stride_layer_idx=1, group_layer_idx=(0, 1)), 8
    sd = deepspeech2_state_dict(vocab_size=89, num_rnn_layers=2, streaming=True, seed=24)
    return sd, dict(num_rnn_layers=2, rnn_size=1024, streaming=True), 4


@functools.lru_cache(maxsize=None)
def _inputs(family):
    lens = DS2_LENS if family == "deepspeech2" else LENS
    return synth_features(len(lens), max(lens), lens=lens, seed=sum(lens))


def _run(family, oracle):
    """-> (output, reference for logprob_err): logits of the Transformer families, probabilities of DeepSpeech2."""
    x, lens = _inputs(family)
    if family == "deepspeech2":
        p = oracle.forward(x, lens)[0]
        return p, torch.log(p.to(torch.float64))
    _, logits = oracle.get_encoder_out(x, lens, return_logits=True)
    return logits, logits


@functools.lru_cache(maxsize=None)
def _ref64(family):
    sd, kw, _ = _fixture(family)
    return _run(family, nm.oracle64(family, sd, **kw))


def _valid(family, T):
    _, _, mul = _fixture(family)
    return [min(T, (ln + mul - 1) // mul) for ln in _inputs(family)[1]]


def _budget(family):
    return nm.F32_BUDGET_DS2 if family == "deepspeech2" else nm.F32_BUDGET


def _err(family, out, lens_out=None):
    ref, ref_lp = _ref64(family)
    if family == "deepspeech2":
        return max(nm.utt_rel(out, ref, lens_out), nm.logprob_err(out, ref_lp, lens_out))
    return max(nm.utt_rel(out, ref, lens_out), nm.logprob_err(torch.softmax(out.to(torch.float64), -1), ref_lp, lens_out))


FAMILIES = ["conformer", "squeezeformer", "efficient_conformer", "deepspeech2"]


def test_every_budget_is_at_most_1e_4():
    for name, v in nm.BUDGETS.items():
        assert 0 < v <= 1e-4, (name, v)


@pytest.mark.parametrize("family", FAMILIES)
def test_fp32_oracle_floor_is_below_a_tenth_of_the_budget(family):
    sd, kw, _ = _fixture(family)
    out, _ = _run(family, nm.oracle64(family, sd, **kw).__class__(sd, **kw))  # the same oracle class in float32
    e = _err(family, out)
    print(f"{family}: fp32 oracle vs float64 oracle {e:.2e} (budget {_budget(family):.0e})")
    assert e < _budget(family) / 10


# ---- mutations --------------------------------------------------------------------------------------------------------
def _sd_set(key, fn):
    def mut(sd, oracle):
        sd[key] = fn(np.array(sd[key]))
    return mut


def _zero_at(idx):
    def fn(a):
        a[idx] = 0.0
        return a
    return fn


def _ffn_unit(prefix, j):
    """one hidden unit of a feed-forward module dropped: its column of w_1 (and bias) and its row of w_2"""
    def mut(sd, oracle):
        for k, idx in ((prefix + ".w_1.weight", (slice(None), j)), (prefix + ".w_1.bias", j), (prefix + ".w_2.weight", j)):
            sd[k] = np.array(sd[k])
            sd[k][idx] = 0.0
    return mut


def _ln_eps(layer, eps):
    """LayerNorm eps of one layer's norms"""
    def mut(sd, oracle):
        if oracle is None:
            return
        orig = oracle._ln
        tag = f"encoder.encoders.{layer}."
        oracle._ln = lambda x, prefix, eps_=1e-5: orig(x, prefix, eps if prefix.startswith(tag) else eps_)
    return mut


def _no_key_mask(sd, oracle):
    """attention of every layer ignores the key mask (a ragged batch: padded keys are attended to)"""
    if oracle is None:
        return
    for name in ("_attention", "_attention_sq", "_grouped_attention"):
        if hasattr(oracle, name):
            orig = getattr(oracle, name)
            if name == "_attention":
                setattr(oracle, name, lambda x, mask, pos_emb, cache, prefix, _o=orig: _o(x, None, pos_emb, cache, prefix))
            else:
                setattr(oracle, name, lambda x, mask, pos_emb, prefix, cache=None, _o=orig: _o(x, None, pos_emb, prefix, cache))


def _time_reduce_tap(sd, oracle):
    """Squeezeformer time reduction: the pointwise conv's bias dropped"""
    sd["encoder.time_reduction_layer.pw_conv.bias"] = np.zeros_like(sd["encoder.time_reduction_layer.pw_conv.bias"])


def _recover_shift(sd, oracle):
    """Squeezeformer recover path: the upsampled rows added one frame late"""
    if oracle is None:
        return
    orig = oracle._linear

    def linear(x, prefix, bias=True):
        y = orig(x, prefix, bias)
        return torch.cat([y[:, :1], y[:, :-1]], dim=1) if prefix == "encoder.time_recover_layer" else y
    oracle._linear = linear


def _ds2_gate_bias(layer, gate, unit):
    def mut(sd, oracle):
        for k in (f"encoder.rnn.{layer}.bias_ih_l0", f"encoder.rnn.{layer}.bias_hh_l0"):
            sd[k] = np.array(sd[k])
            sd[k][gate * 1024 + unit] = 0.0
    return mut


ATT = "encoder.encoders.{}.self_attn"
CONV = "encoder.encoders.{}.conv_module.depthwise_conv.weight"
MUTATIONS = {
    "conformer": {
        "pos_bias_v_one_head": _sd_set(ATT.format(1) + ".pos_bias_v", _zero_at(2)),
        "ffn_hidden_unit": _ffn_unit("encoder.encoders.1.feed_forward", 1777),
        "depthwise_first_tap": _sd_set(CONV.format(0), _zero_at((slice(None), 0, 0))),
        "depthwise_last_tap": _sd_set(CONV.format(1), _zero_at((slice(None), 0, -1))),
        "layernorm_eps_1e-3": _ln_eps(1, 1e-3),
        "bias_linear_v": _sd_set(ATT.format(1) + ".linear_v.bias", lambda a: a * 0),
        "key_mask_ignored": _no_key_mask,
    },
    "squeezeformer": {
        "pos_bias_v_one_head": _sd_set(ATT.format(2) + ".pos_bias_v", _zero_at(1)),
        "ffn_hidden_unit": _ffn_unit("encoder.encoders.2.ffn2", 1031),
        "depthwise_first_tap": _sd_set(CONV.format(0), _zero_at((slice(None), 0, 0))),
        "depthwise_last_tap": _sd_set(CONV.format(2), _zero_at((slice(None), 0, -1))),
        "layernorm_eps_1e-3": _ln_eps(2, 1e-3),
        "bias_linear_v": _sd_set(ATT.format(2) + ".linear_v.bias", lambda a: a * 0),
        "key_mask_ignored": _no_key_mask,
        "time_reduction_bias": _time_reduce_tap,
        "recover_one_frame_late": _recover_shift,
    },
    "efficient_conformer": {
        "pos_bias_v_one_head": _sd_set(ATT.format(2) + ".pos_bias_v", _zero_at(3)),
        "ffn_hidden_unit": _ffn_unit("encoder.encoders.2.feed_forward", 5),
        "depthwise_first_tap": _sd_set(CONV.format(0), _zero_at((slice(None), 0, 0))),
        "depthwise_last_tap": _sd_set(CONV.format(3), _zero_at((slice(None), 0, -1))),
        "layernorm_eps_1e-3": _ln_eps(2, 1e-3),
        "bias_linear_v": _sd_set(ATT.format(3) + ".linear_v.bias", lambda a: a * 0),
        "key_mask_ignored": _no_key_mask,
        "stride_conv_first_tap": _sd_set(CONV.format(1), _zero_at((slice(None), 0, 0))),
        "stride_conv_last_tap": _sd_set(CONV.format(1), _zero_at((slice(None), 0, -1))),
    },
    "deepspeech2": {
        "forget_gate_bias_one_unit": _ds2_gate_bias(1, 1, 300),
        "input_gate_bias_one_unit": _ds2_gate_bias(0, 0, 17),
        "cell_gate_bias_one_unit": _ds2_gate_bias(1, 2, 640),
        "output_gate_bias_one_unit": _ds2_gate_bias(0, 3, 900),
    },
}


@pytest.mark.parametrize("family,mutation", [(f, m) for f in FAMILIES for m in MUTATIONS[f]])
def test_budget_catches_the_mutation(family, mutation):
    sd, kw, _ = _fixture(family)
    sd = dict(sd)
    mut = MUTATIONS[family][mutation]
    mut(sd, None)  # state-dict mutations act here (idempotent), method patches on the oracle built from it
    oracle = nm.oracle64(family, sd, **kw)
    mut(sd, oracle)
    out, _ = _run(family, oracle)
    e = _err(family, out, _valid(family, out.shape[1]))
    print(f"{family} / {mutation}: {e:.2e} = {e / _budget(family):.0f} x budget")
    assert e > MARGIN * _budget(family), (family, mutation, e)
