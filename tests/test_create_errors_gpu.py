"""GPU: ppasr_create's PPASR_EMISSING path, one tensor per section of the loader (csrc/weights.h and the families'
*_create), for every model family -- and that a create which follows failed ones, and one from a freshly drawn dict, give
the same bytes out.

Each model is as small as its family allows.  Per model a fixed list of tensor names; each name is tried twice: removed
from the dict, and truncated by one element along its first axis (the loader checks element counts only, so a reshape of
the same size is no error).  Exactly one tensor is wrong per create."""
import numpy as np
import pytest
import torch

from ppasr_amd import _lib
from ppasr_amd.utils import synth

pytestmark = pytest.mark.gpu
V = 37
L0, L1 = "encoder.encoders.0.", "encoder.encoders.1."


def _conformer_names(lay, ffn="feed_forward", norm="norm_mha"):
    return ["encoder.global_cmvn.mean", "encoder.embed.conv.0.weight", "encoder.embed.out.0.weight", lay + norm + ".bias",
            lay + "conv_module.norm.weight", lay + ffn + ".w_2.weight", lay + "self_attn.linear_k.bias",
            lay + "self_attn.linear_pos.weight", lay + "self_attn.pos_bias_v", lay + "conv_module.depthwise_conv.weight",
            "encoder.after_norm.weight", "ctc.ctc_lo.bias"]


def _squeezeformer_names(lay):
    return ["encoder.global_cmvn.mean", "encoder.embed.input_proj.0.weight", lay + "layer_norm1.bias",
            lay + "conv_module.norm.weight", lay + "ffn1.w_2.weight", lay + "self_attn.linear_k.bias",
            lay + "self_attn.linear_pos.weight", lay + "self_attn.pos_bias_v", lay + "conv_module.depthwise_conv.weight",
            "ctc.ctc_lo.bias", lay + "ffn1.ada_scale"]


def _model(family):
    if family == "conformer":
        from ppasr_amd.model_utils.conformer.model import ConformerModel as M
    elif family == "efficient_conformer":
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
    elif family == "squeezeformer":
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
    else:
        from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model as M
    return M


# name -> (family, state dict from scratch, encoder_conf, the tensors the walk breaks)
MODELS = {
    "conf256": ("conformer", lambda: synth.conformer_state_dict(vocab_size=V, num_blocks=1, seed=701, perturb_norm=True),
                dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=1, cnn_module_kernel=15),
                _conformer_names(L0)),
    "conf512_concat": ("conformer",
                       lambda: synth.conformer_state_dict(vocab_size=V, num_blocks=1, seed=702, perturb_norm=True, output_size=512,
                                                          attention_heads=8, concat_after=True),
                       dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=1, cnn_module_kernel=15,
                            concat_after=True),
                       _conformer_names(L0) + [L0 + "concat_linear.weight"]),
    # layers 0 and 1 with grouped attention, layer 1 the stride layer (the walk breaks that layer's tensors), layer 2 behind it
    "eff_grouped_stride": ("efficient_conformer",
                           lambda: synth.efficient_conformer_state_dict(vocab_size=V, num_blocks=3, seed=703, perturb_norm=True,
                                                                        stride_layer_idx=1, group_layer_idx=(0, 1)),
                           dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=3, cnn_module_kernel=15,
                                cnn_module_norm="layer_norm",
                                efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3,
                                                    stride_kernel=True)),
                           _conformer_names(L1)),
    "sq_flat": ("squeezeformer", lambda: synth.squeezeformer_state_dict(vocab_size=V, num_blocks=1, seed=704, perturb_norm=True),
                dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=1, reduce_idx=None, recover_idx=None,
                     feed_forward_expansion_factor=8, cnn_module_kernel=31),
                _squeezeformer_names(L0)),
    "sq_reduce": ("squeezeformer", lambda: synth.squeezeformer_state_dict(vocab_size=V, num_blocks=3, seed=705, perturb_norm=True),
                  dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=3, reduce_idx=1, recover_idx=2,
                       feed_forward_expansion_factor=8, cnn_module_kernel=31),
                  _squeezeformer_names(L1) + ["encoder.time_reduction_layer.pw_conv.weight"]),
    "ds2_lstm": ("deepspeech2", lambda: synth.deepspeech2_state_dict(vocab_size=V, num_rnn_layers=1, streaming=True, seed=706,
                                                                     perturb_norm=True),
                 dict(num_rnn_layers=1, rnn_size=1024, use_gru=False),
                 ["encoder.global_cmvn.mean", "encoder.conv.conv.0.weight", "encoder.rnn.0.weight_hh_l0",
                  "encoder.layernorm_list.0.bias", "decoder.ctc_lo.bias"]),
}


def _create(name, sd):
    family, _, conf, _ = MODELS[name]
    return _model(family)(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


def _probs(model):
    x, lens = synth.synth_features(2, 67, lens=[67, 41], seed=707)
    out = model.get_encoder_out(x, lens)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(MODELS))
def test_one_wrong_tensor_is_named_and_later_creates_are_unaffected(name):
    _, make_sd, _, names = MODELS[name]
    intact = make_sd()
    for tensor in names:
        assert tensor in intact, tensor
        broken = {"removed": {k: v for k, v in intact.items() if k != tensor},
                  "truncated": dict(intact, **{tensor: np.asarray(intact[tensor])[:-1]})}
        for how, sd in broken.items():
            with pytest.raises(_lib.PPASRHipError) as e:
                _create(name, sd)
            assert e.value.status == _lib.PPASR_EMISSING, (tensor, how, str(e.value))
            assert str(e.value).endswith(tensor), (tensor, how, str(e.value))
    after_failures = _probs(_create(name, intact))
    from_scratch = _probs(_create(name, make_sd()))
    assert after_failures.shape[0] == 2 and after_failures.shape[2] == V and np.isfinite(after_failures).all()
    assert after_failures.tobytes() == from_scratch.tobytes()
