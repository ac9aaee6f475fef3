"""ppasr_set_memory_out / get_encoder_out(return_memory=True): the encoder output the attention decoder attends to, for
the three Conformer families on the small reference cases (tests/ref_cases.py), fused walks and the general layer route:
against the family's float64 oracle at the fp32 budget; the probabilities byte-identical with and without the pointer;
zero rows behind the valid frames under skip-padding; nothing written once the pointer is cleared."""
import numpy as np
import pytest
import torch

import numerics as nm
import poison
import ref_cases as rc
from ppasr_amd.utils.synth import synth_features

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
CASES = ["conf_s", "eff_s", "sq_s", "conf512"]  # fused Conformer / Efficient-Conformer / Squeezeformer walks, general route
LENS = {1: [131], 3: [131, 90, 38]}


def _model(name):
    def make():
        case = rc.SMALL[name]
        fam = case["family"]
        if fam == "conformer":
            from ppasr_amd.model_utils.conformer.model import ConformerModel as M
        elif fam == "efficient_conformer":
            from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
        else:
            from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
        return M(80, case["V"], streaming=case["streaming"], encoder_conf=rc.product_encoder_conf(case),
                 state_dict=rc.state_dict(case), device="cuda:0")
    return MEMO.get(("model", name), make)


def _oracle(name):
    def make():
        case = rc.SMALL[name]
        fam, L, kw = case["family"], case["L"], case["kw"]
        common = dict(num_blocks=L, causal=case["streaming"], attention_heads=kw.get("attention_heads", 4))
        if fam == "efficient_conformer":
            common.update(stride_layer_idx=kw["stride_layer_idx"], group_layer_idx=kw["group_layer_idx"])
        elif fam == "squeezeformer":
            common.update(reduce_idx=kw["reduce_idx"], recover_idx=kw["recover_idx"])
        return nm.oracle64(fam, rc.state_dict(case), **common)
    return MEMO.get(("oracle", name), make)


def _ref(name, B):
    def go():
        x, lens = synth_features(B, 131, lens=LENS[B], seed=700 + B)
        with torch.no_grad():
            enc, _ = _oracle(name).encoder_forward(x, lens)
        return x, lens, enc
    return MEMO.get(("ref", name, B), go)


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_memory_matches_float64_and_leaves_probs_alone(name, B, skip):
    model = _model(name)
    x, lens, enc = _ref(name, B)
    model.set_skip_padding(skip)
    try:
        plain = model.get_encoder_out(x, lens)
        probs, memory = model.get_encoder_out(x, lens, return_memory=True)
        torch.cuda.synchronize()
        assert tuple(memory.shape) == tuple(enc.shape)
        assert probs.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
        lens_out = model.valid_out_frames(lens, x.shape[1]).cpu().numpy() if skip else None
        err = nm.utt_rel(memory, enc, lens_out)
        print(f"{name} B={B} skip={skip}: memory {err:.2e}")
        assert err < nm.F32_BUDGET
        if skip:
            for b, n in enumerate(lens_out):
                assert not bool(memory[b, int(n):].any()), b
        # the pointer is cleared behind the call: a further encode writes nothing into the buffer
        poison.fill(memory, poison.BYTES["7f"])
        again = model.get_encoder_out(x, lens)
        torch.cuda.synchronize()
        assert bool((memory.view(torch.uint8) == poison.BYTES["7f"]).all())
        assert again.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    finally:
        model.set_skip_padding(False)


def test_too_small_a_buffer_is_refused():
    from ppasr_amd import _lib
    model = _model("conf_s")
    x, lens, _ = _ref("conf_s", 1)
    buf = torch.zeros(16, dtype=torch.float32, device=model.device)
    _lib.check(model.lib.ppasr_set_memory_out(model._h, buf.data_ptr(), buf.numel()))
    try:
        with pytest.raises(_lib.PPASRHipError) as e:
            model.get_encoder_out(x, lens)
        assert e.value.status == _lib.PPASR_ENOSPACE
    finally:
        _lib.check(model.lib.ppasr_set_memory_out(model._h, None, 0))


def test_final_proj_handles_refuse_it():
    """Squeezeformer with final_proj: the projection is folded into the CTC head, so the encoder's own output is never
    formed -- refused, not emulated"""
    from ppasr_amd import _lib
    model = _model("sq_fproj")
    x, lens = synth_features(1, 131, lens=[131], seed=701)
    with pytest.raises(_lib.PPASRHipError) as e:
        model.get_encoder_out(x, lens, return_memory=True)
    assert e.value.status == _lib.PPASR_EUNSUPPORTED
    assert model.get_encoder_out(x, lens).shape[0] == 1  # (the handle is left usable)
