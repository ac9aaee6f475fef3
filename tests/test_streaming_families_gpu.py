"""GPU parity of forward_chunk for the Squeezeformer and Efficient-Conformer families (device-resident caches, half-rate
layers held once) vs the oracles' restatements of squeezeformer/encoder.py:260-381 and
efficient_conformer/encoder.py:266-393, chunk by chunk with predict_stream's windowing (predict.py:277-283,306-307)."""
import pytest
import torch

from oracle.efficient_conformer_oracle import EfficientConformerOracle
from oracle.squeezeformer_oracle import SqueezeformerOracle
from ppasr_amd.utils.synth import efficient_conformer_state_dict, squeezeformer_state_dict, synth_features
from numerics import F32_BUDGET, rel

pytestmark = pytest.mark.gpu
TOL = F32_BUDGET  # fp32 error budget (tests/numerics.py)


def _windows(n_frames, window=67, stride=64):
    return [(cur, min(cur + window, n_frames)) for cur in range(0, n_frames - 7 + 1, stride)]


def _sq(sd, V, L, red, rec):
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel
    conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=L, reduce_idx=red, recover_idx=rec,
                feed_forward_expansion_factor=8, cnn_module_kernel=31)
    return SqueezeformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


def _eff(sd, V, L, stride_idx, groups):
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=L, cnn_module_kernel=15,
                cnn_module_norm="layer_norm",
                efficient_conf=dict(stride_layer_idx=[stride_idx] if stride_idx is not None else [],
                                    stride=[2] if stride_idx is not None else [], group_layer_idx=list(groups),
                                    group_size=3, stride_kernel=True))
    return EfficientConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


def _run_stream(model, oracle, x, required, frames_per_chunk):
    stream = model.new_stream()
    att = cnn = None
    offset = 0
    for (a, b) in _windows(x.shape[1]):
        chunk = x[:, a:b]
        ref, att, cnn = oracle.get_encoder_out_chunk(chunk, offset, required, att, cnn)
        got = stream.encode_chunk(chunk, required)
        torch.cuda.synchronize()
        assert tuple(got.shape) == tuple(ref.shape), (a, b)
        e = rel(got.cpu().numpy(), ref.numpy())
        assert e < TOL, (a, b, e)
        offset += ref.shape[1]
        assert stream.offset == offset and stream.cache_frames == att.shape[2]
        g_att, g_cnn = stream.export_caches()
        assert tuple(g_att.shape) == tuple(att.shape) and tuple(g_cnn.shape) == tuple(cnn.shape)
        assert rel(g_att.cpu().numpy(), att.numpy()) < TOL
        assert rel(g_cnn.cpu().numpy(), cnn.numpy()) < TOL
    return stream


@pytest.mark.parametrize("L,red,rec,required", [
    (4, 1, 3, -16),        # reduce before layer 1, recover before layer 3, unbounded history
    (4, 1, 3, 32),         # bounded cache: both rates are shifted
    (3, None, None, -16),  # no time reduction
])
def test_squeezeformer_chunks_match_oracle(L, red, rec, required):
    V = 180
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=L, seed=71, perturb_norm=True)
    x, _ = synth_features(1, 64 * 4 + 40, seed=72)
    model = _sq(sd, V, L, red, rec)
    oracle = SqueezeformerOracle(sd, num_blocks=L, reduce_idx=red, recover_idx=rec)
    stream = _run_stream(model, oracle, x, required, 16)
    # reset -> first chunk again
    first_ref, _, _ = oracle.get_encoder_out_chunk(x[:, :67], 0, required)
    stream.reset()
    again = stream.encode_chunk(x[:, :67], required)
    assert rel(again.cpu().numpy(), first_ref.numpy()) < TOL


@pytest.mark.parametrize("L,stride_idx,groups,required", [
    (4, 1, (0, 1), -16),      # grouped attention over cache + chunk (16 is not a multiple of 3), stride layer, 7-tap convs
    (4, 1, (0, 1), 32),
    (3, None, (0, 2), -16),   # grouped attention only
    (3, 0, (), -16),          # stride layer only
])
def test_efficient_conformer_chunks_match_oracle(L, stride_idx, groups, required):
    V = 180
    sd = efficient_conformer_state_dict(vocab_size=V, num_blocks=L, seed=81, perturb_norm=True, stride_layer_idx=stride_idx,
                                        group_layer_idx=groups)
    # every window must give an even number of frames: with an odd chunk the reference's own cache concat fails
    # (efficient_conformer/encoder.py:380-391, "TODO There is a bug in this code"); ours refuses the export likewise
    x, _ = synth_features(1, 64 * 3 + 67, seed=82)
    model = _eff(sd, V, L, stride_idx, groups)
    oracle = EfficientConformerOracle(sd, num_blocks=L, stride_layer_idx=stride_idx, group_layer_idx=groups)
    _run_stream(model, oracle, x, required, 8)


@pytest.mark.parametrize("family", ["squeezeformer", "efficient"])
def test_stateless_signature_and_one_giant_chunk(family):
    """get_encoder_out_chunk with explicit (host) caches, and the whole utterance as ONE chunk with empty caches equals
    get_encoder_out (inference_predictor.py:127-137)."""
    V = 150
    x, lens = synth_features(1, 403, seed=92)  # T' = 100: even, see above
    if family == "squeezeformer":
        sd = squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=91, perturb_norm=True)
        model, oracle = _sq(sd, V, 4, 1, 3), SqueezeformerOracle(sd, num_blocks=4, reduce_idx=1, recover_idx=3)
    else:
        sd = efficient_conformer_state_dict(vocab_size=V, num_blocks=4, seed=91, perturb_norm=True, stride_layer_idx=1,
                                            group_layer_idx=(0, 1))
        model = _eff(sd, V, 4, 1, (0, 1))
        oracle = EfficientConformerOracle(sd, num_blocks=4, stride_layer_idx=1, group_layer_idx=(0, 1))
    full = model.get_encoder_out(x, lens)
    one, att, cnn = model.get_encoder_out_chunk(x, 0, -1)
    torch.cuda.synchronize()
    assert rel(one.cpu().numpy(), full.cpu().numpy()) < 1e-5
    r_probs, r_att, r_cnn = oracle.get_encoder_out_chunk(x, 0, -1)
    assert tuple(att.shape) == tuple(r_att.shape)
    assert rel(att.cpu().numpy(), r_att.numpy()) < TOL and rel(cnn.cpu().numpy(), r_cnn.numpy()) < TOL
    x2, _ = synth_features(1, 67, seed=93)
    ref2, ratt2, _ = oracle.get_encoder_out_chunk(x2, r_probs.shape[1], -1, r_att, r_cnn)
    got2, att2, _ = model.get_encoder_out_chunk(x2, r_probs.shape[1], -1, r_att, r_cnn)
    torch.cuda.synchronize()
    assert rel(got2.cpu().numpy(), ref2.numpy()) < TOL
    assert tuple(att2.shape) == tuple(ratt2.shape)
