"""GPU: conv2 of Conv2dSubsampling4 in the pair form (csrc/front_fused.hip: output frames in pairs, Winograd F(2,2) over
time) against the float64 oracle at the fp32 budget -- odd and even T' (the dead second frame of an odd T''s last pair),
T' = 1, 2, 3, ragged lengths with padding skipped and computed, the one-launch and the two-launch route, the Conformer
and the Squeezeformer front end."""
import numpy as np
import pytest

import numerics as nm
from ppasr_amd.utils.synth import conformer_state_dict, squeezeformer_state_dict, synth_features

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()


def _spec(fam):
    if fam == "conformer":
        sd = conformer_state_dict(vocab_size=97, num_blocks=1, seed=171, perturb_norm=True)
        conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=1, cnn_module_kernel=15)
        return sd, conf, dict(num_blocks=1, cnn_module_kernel=15)
    sd = squeezeformer_state_dict(vocab_size=97, num_blocks=2, seed=172, perturb_norm=True)
    conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=2, reduce_idx=None, recover_idx=None,
                feed_forward_expansion_factor=8, cnn_module_kernel=31)
    return sd, conf, dict(num_blocks=2, reduce_idx=None, recover_idx=None, cnn_module_kernel=31)


def _model(fam):
    def make():
        sd, conf, _ = _spec(fam)
        if fam == "conformer":
            from ppasr_amd.model_utils.conformer.model import ConformerModel as M
        else:
            from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
        return M(80, 97, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    return MEMO.get(("model", fam), make)


def _oracle(fam):
    def make():
        sd, _, kw = _spec(fam)
        return nm.oracle64(fam, sd, **kw)
    return MEMO.get(("oracle", fam), make)


# (B, T'): T' = 1, 2, 3, odd / even, one utterance and ragged batches
CASES = [(1, 1), (1, 2), (1, 3), (2, 3), (1, 16), (1, 17), (3, 40), (4, 61), (5, 128), (3, 249)]


@pytest.mark.parametrize("fam", ["conformer", "squeezeformer"])
@pytest.mark.parametrize("B,Tp", CASES)
def test_pair_form_front_end_against_float64(fam, B, Tp):
    T = 4 * Tp + 3
    rng = np.random.default_rng(B * 1000 + Tp)
    lens_tp = [Tp] + [int(v) for v in rng.integers(1, Tp + 1, size=B - 1)]
    lens = [min(T, 4 * n) if n < Tp else T for n in lens_tp]
    x, la = synth_features(B, T, lens=lens, seed=Tp + 7 * B)
    ref = MEMO.get(("ref", fam, B, Tp), lambda: _oracle(fam).get_encoder_out(x, la, return_logits=True)[1])
    m = _model(fam)
    try:
        for fused in (1, 0):
            m.set_front_fused(fused)
            for skip in (False, True):
                m.set_skip_padding(skip)
                probs, logits = m.get_encoder_out(x, la, return_logits=True)
                lens_out = m.valid_out_frames(la, x.shape[1]).cpu().numpy() if skip else None
                e = nm.utt_rel(logits, ref, lens_out)
                print(f"[winograd] {fam} B={B} Tp={Tp} fused={fused} skip={skip}: logits {e:.2e}")
                assert np.isfinite(logits.cpu().numpy()).all()
                assert e < nm.F32_BUDGET, (fam, B, Tp, fused, skip, e)
    finally:
        m.set_front_fused(1)
        m.set_skip_padding(False)
