"""GPU parity: HIP Conformer path (through the C-ABI) vs the CPU oracle, stage by stage.

Tolerance: the fp32 error budget of tests/numerics.py (F32_BUDGET, set from the measured
error of the fp32 routes against a float64 oracle) on encoder logits; every intermediate
is checked to the same bound, relative to the tensor's max magnitude.  Greedy token ids must match the oracle exactly on frames whose
oracle top-1 margin exceeds the measured logit error (all frames, in practice).
"""
import numpy as np
import pytest
import torch

from oracle.conformer_oracle import ConformerOracle
from oracle.ctc_decoders_oracle import greedy_tokens
from ppasr_amd.utils.synth import conformer_state_dict, synth_features
from numerics import F32_BUDGET, rel

pytestmark = pytest.mark.gpu

TOL = F32_BUDGET  # fp32 error budget (tests/numerics.py)


def _model(sd, V, L):
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=L, cnn_module_kernel=15)
    return ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


@pytest.mark.parametrize("B,T,lens", [(3, 203, [203, 150, 67]), (1, 67, [67]), (2, 700, [700, 512])])
def test_stage_taps_match_oracle(B, T, lens):
    L, V = 2, 300
    sd = conformer_state_dict(vocab_size=V, num_blocks=L, seed=11, perturb_norm=True)
    x, lens = synth_features(B, T, lens=lens, seed=5)
    model = _model(sd, V, L)
    Tp = model.out_frames(T)
    M = B * Tp
    per_layer = M * 256 * 5 + M * 768
    taps = model.set_debug_taps(M * 256 + L * per_layer)
    probs, logits = model.get_encoder_out(x, lens, return_logits=True)
    torch.cuda.synchronize()
    taps = taps.cpu().numpy()

    oracle = ConformerOracle(sd, num_blocks=L)
    oracle.trace = {}
    with torch.no_grad():
        enc, _, layers = oracle.encoder_forward(x, lens, return_layers=True)
        ref_logits = oracle.ctc_logits(enc)
        ref_probs = torch.softmax(ref_logits, dim=2)
    tr = oracle.trace

    off = 0

    def take(n, shape):
        nonlocal off
        out = taps[off:off + n].reshape(shape)
        off += n
        return out

    errs = {}
    errs["x0"] = rel(take(M * 256, (B, Tp, 256)), layers[0].numpy())
    for i in range(L):
        p = f"encoder.encoders.{i}"
        errs[f"L{i}.x1"] = rel(take(M * 256, (B, Tp, 256)), tr[p + ".x1"].numpy())
        qkv = take(M * 768, (B, Tp, 768))
        errs[f"L{i}.q"] = rel(qkv[..., :256], tr[p + ".self_attn.q"].numpy())
        errs[f"L{i}.k"] = rel(qkv[..., 256:512], tr[p + ".self_attn.k"].numpy())
        errs[f"L{i}.v"] = rel(qkv[..., 512:], tr[p + ".self_attn.v"].numpy())
        errs[f"L{i}.ctx"] = rel(take(M * 256, (B, Tp, 256)), tr[p + ".self_attn.ctx"].numpy())
        errs[f"L{i}.x2"] = rel(take(M * 256, (B, Tp, 256)), tr[p + ".x2"].numpy())
        errs[f"L{i}.glu"] = rel(take(M * 256, (B, Tp, 256)), tr[p + ".conv_module.glu"][:, 14:, :].numpy())
        errs[f"L{i}.out"] = rel(take(M * 256, (B, Tp, 256)), layers[i + 1].numpy())
    errs["logits"] = rel(logits.cpu().numpy(), ref_logits.numpy())
    errs["probs"] = rel(probs.cpu().numpy(), ref_probs.numpy())
    print({k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad
    assert abs(float(probs.sum(-1).mean()) - 1.0) < 1e-5


@pytest.mark.parametrize("trim", [False, True])
def test_fused_greedy_tokens_match_oracle(trim):
    L, V, B, T = 3, 4233, 4, 403
    lens = [403, 300, 250, 99]
    sd = conformer_state_dict(vocab_size=V, num_blocks=L, seed=21)
    x, lens = synth_features(B, T, lens=lens, seed=9)
    model = _model(sd, V, L)
    tokens, n_tokens, score = model.encode_greedy(x, lens, trim_to_length=trim)
    torch.cuda.synchronize()
    ref_probs, ref_logits = ConformerOracle(sd, num_blocks=L).get_encoder_out(x, lens, return_logits=True)
    Tp = ref_probs.shape[1]
    for b in range(B):
        n = min(Tp, (int(lens[b]) + 3) // 4) if trim else Tp
        p = ref_probs[b, :n].numpy()
        ids, _, max_prob = greedy_tokens(p)
        got = tokens[b, : int(n_tokens[b])].cpu().numpy()
        assert np.array_equal(ids, got), (b, ids[:20], got[:20])
        assert (tokens[b, int(n_tokens[b]):] == -1).all()
        ref_score = float(np.mean(max_prob.astype(np.float64))) * 100.0 if len(max_prob) else 0.0
        assert abs(float(score[b]) - ref_score) <= 1e-3 * max(1.0, abs(ref_score)), (float(score[b]), ref_score)


@pytest.mark.parametrize("B,T,lens", [(3, 331, [331, 250, 90]), (2, 1000, [1000, 640]), (1, 135, [135]),
                                     (2, 2300, [2300, 1100])])  # T' = 574: three 256-key blocks, online softmax
def test_fused_attention_route_equals_two_kernel_route(B, T, lens):
    """Without debug taps the batched path runs attention + out-projection/GLU as ONE launch (k_attn_out_glu); with taps
    set it runs k_attention + k_out_glu.  Both must give the same logits (same arithmetic, different blocking) and match
    the oracle."""
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    from ppasr_amd.utils.synth import conformer_state_dict, synth_features
    from oracle.conformer_oracle import ConformerOracle
    L, V = 3, 260
    sd = conformer_state_dict(vocab_size=V, num_blocks=L, seed=77, perturb_norm=True)
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=L, cnn_module_kernel=15)
    x, lens = synth_features(B, T, lens=lens, seed=78)
    m = ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    _, fused = m.get_encoder_out(x, lens, return_logits=True)
    m.set_debug_taps(1 << 16)  # any tap buffer switches to the two-kernel route
    _, split = m.get_encoder_out(x, lens, return_logits=True)
    m.set_debug_taps(0)
    torch.cuda.synchronize()
    ref = ConformerOracle(sd, num_blocks=L).get_encoder_out(x, lens, return_logits=True)[1].numpy()
    f, s = fused.cpu().numpy(), split.cpu().numpy()
    scale = np.abs(ref).max()
    assert np.abs(f - s).max() / scale < 1e-5
    assert np.abs(f - ref).max() / scale < TOL


@pytest.mark.parametrize("B,T,lens,k", [(3, 331, [331, 250, 90], 15), (2, 523, [523, 300], 31), (1, 67, [67], 7)])
def test_non_streaming_model_non_causal_conv(B, T, lens, k):
    """streaming=False models use the non-causal conv module (symmetric zero padding of the depthwise conv input,
    conformer/convolution.py:50-52) and full attention: logits / greedy ids vs the oracle built with causal=False."""
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    L, V = 2, 210
    sd = conformer_state_dict(vocab_size=V, num_blocks=L, seed=123, perturb_norm=True, cnn_module_kernel=k)
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=L, cnn_module_kernel=k)
    x, lens = synth_features(B, T, lens=lens, seed=124)
    m = ConformerModel(80, V, streaming=False, encoder_conf=conf, state_dict=sd, device="cuda:0")
    probs, logits = m.get_encoder_out(x, lens, return_logits=True)
    torch.cuda.synchronize()
    oracle = ConformerOracle(sd, num_blocks=L, cnn_module_kernel=k, causal=False)
    ref_probs, ref_logits = oracle.get_encoder_out(x, lens, return_logits=True)
    assert np.abs(logits.cpu().numpy() - ref_logits.numpy()).max() / np.abs(ref_logits.numpy()).max() < TOL
    # and it differs from the causal module on the same weights (the test would be vacuous otherwise)
    causal_logits = ConformerOracle(sd, num_blocks=L, cnn_module_kernel=k, causal=True).get_encoder_out(
        x, lens, return_logits=True)[1]
    assert np.abs(causal_logits.numpy() - ref_logits.numpy()).max() > 1e-2
    tokens, n_tokens, _ = m.encode_greedy(x, lens)
    for b in range(B):
        ids, _, _ = greedy_tokens(ref_probs[b].numpy())
        assert np.array_equal(ids, tokens[b, : int(n_tokens[b])].cpu().numpy())
    with pytest.raises(Exception):
        m.new_stream()  # forward_chunk needs the causal module
