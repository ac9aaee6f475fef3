"""GPU: conv2 of Conv2dSubsampling4 in the quad form (csrc/front_fused.hip: output frames in pairs x output bins in
pairs, Winograd F(2x2, 2x2)) against the float64 oracle at the fp32 budget, for the Conformer and the Squeezeformer front
end, the one-launch and the two-launch route, padding skipped and computed.

  F    F1  F2  Q
  80   39  19  10   odd F2: the last quad's second column is dead (computed, never written)
  86   42  20  10   even F2: every column is live

T' = 1, 2, 3 and odd / even T' (the dead second frame of an odd T''s last pair); 32-row tiles that start inside a pair
(Q = 10) and, at T' = 31 / 32 (16 pairs = 160 rows = 5 tiles per utterance), exactly between two utterances; ragged
lengths."""
import numpy as np
import pytest

import numerics as nm
from ppasr_amd.utils.synth import conformer_state_dict, squeezeformer_state_dict, synth_features

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()


def _spec(fam, F):
    if fam == "conformer":
        sd = conformer_state_dict(input_dim=F, vocab_size=97, num_blocks=1, seed=600 + F, perturb_norm=True)
        conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=1, cnn_module_kernel=15)
        return sd, conf, dict(num_blocks=1, cnn_module_kernel=15)
    sd = squeezeformer_state_dict(input_dim=F, vocab_size=97, num_blocks=2, seed=700 + F, perturb_norm=True)
    conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=2, reduce_idx=None, recover_idx=None,
                feed_forward_expansion_factor=8, cnn_module_kernel=31)
    return sd, conf, dict(num_blocks=2, reduce_idx=None, recover_idx=None, cnn_module_kernel=31)


def _model(fam, F):
    def make():
        sd, conf, _ = _spec(fam, F)
        if fam == "conformer":
            from ppasr_amd.model_utils.conformer.model import ConformerModel as M
        else:
            from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
        return M(F, 97, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    return MEMO.get(("model", fam, F), make)


def _oracle(fam, F):
    def make():
        sd, _, kw = _spec(fam, F)
        return nm.oracle64(fam, sd, **kw)
    return MEMO.get(("oracle", fam, F), make)


# (B, T'): T' = 1, 2, 3, odd / even, tiles ending between utterances (T' = 31, 32), ragged batches
CASES = [(1, 1), (1, 2), (1, 3), (2, 3), (2, 31), (3, 32), (4, 61), (3, 128)]


@pytest.mark.parametrize("F", [80, 86])
@pytest.mark.parametrize("fam", ["conformer", "squeezeformer"])
@pytest.mark.parametrize("B,Tp", CASES)
def test_quad_form_front_end_against_float64(F, fam, B, Tp):
    T = 4 * Tp + 3
    rng = np.random.default_rng(B * 1000 + Tp + F)
    lens_tp = [Tp] + [int(v) for v in rng.integers(1, Tp + 1, size=B - 1)]
    lens = [min(T, 4 * n) if n < Tp else T for n in lens_tp]
    x, la = synth_features(B, T, n_mels=F, lens=lens, seed=Tp + 7 * B + F)
    ref = MEMO.get(("ref", fam, F, B, Tp), lambda: _oracle(fam, F).get_encoder_out(x, la, return_logits=True)[1])
    m = _model(fam, F)
    outs = {}
    try:
        for fused in (1, 0):
            m.set_front_fused(fused)
            for skip in (False, True):
                m.set_skip_padding(skip)
                probs, logits = m.get_encoder_out(x, la, return_logits=True)
                lens_out = m.valid_out_frames(la, x.shape[1]).cpu().numpy() if skip else None
                e = nm.utt_rel(logits, ref, lens_out)
                print(f"[quad] {fam} F={F} B={B} Tp={Tp} fused={fused} skip={skip}: logits {e:.2e}")
                assert np.isfinite(logits.cpu().numpy()).all()
                assert e < nm.F32_BUDGET, (fam, F, B, Tp, fused, skip, e)
                outs[(fused, skip)] = logits.cpu().numpy()
    finally:
        m.set_front_fused(1)
        m.set_skip_padding(False)
    # the two routes share one body: bit-identical with padding computed
    assert np.array_equal(outs[(1, False)], outs[(0, False)]), (fam, F, B, Tp)
