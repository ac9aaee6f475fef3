"""Regenerate tests/golden/ref_loss.npz by running the REFERENCE's OWN ConformerModel.forward.

    python tests/golden/make_loss_goldens.py

Like make_decoder_goldens.py: `sys.path[:0] = [oracle/paddle_shim, /root/reference]`, so that
`ppasr/model_utils/conformer/model.py` (ConformerModel: encoder, BiTransformerDecoder, CTCLoss, LabelSmoothingLoss,
add_sos_eos / reverse_pad_list, the combination) imports and runs unmodified on the torch-backed shim.  For the two tiny
checkpoints of loss_oracle.MODEL_CASES (one with reverse_weight 0.3, lsm_weight 0.1, ctc_weight 0.3) the model is built
with the case's shape, the seeded synthetic state dict is loaded BY NAME, and `forward(speech, lens, text, text_lens)` is
called in eval().

The shim's two stub layers are given bodies here, since they are Paddle's ops and not the reference's:
  paddle.nn.CTCLoss   warp-ctc on unnormalised activations [T, B, V]: log_softmax, then the CTC negative log-likelihood
                      per utterance, reduction "sum" / "mean" / "none" (torch.nn.functional.ctc_loss in float64)
  paddle.nn.KLDivLoss label * (log(label) - input), zero where label <= 0; reduction "none"

Stored per case: `<name>/loss`, `<name>/loss_att`, `<name>/loss_ctc` (float64 scalars).  Inputs and weights come from the
seeds and are not stored.  Needs /root/reference, so it runs in the build container only; the .npz travels."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loss_oracle as lo  # noqa: E402


def paddle_ops(paddle, torch):
    """bodies for the shim's CTCLoss and KLDivLoss"""
    Tensor = paddle.Tensor

    class CTCLoss(paddle.nn.Layer):
        def __init__(self, blank=0, reduction="mean"):
            super().__init__()
            self.blank, self.reduction = blank, reduction

        def forward(self, log_probs, labels, input_lengths, label_lengths, norm_by_times=False):
            lp = torch.log_softmax(log_probs._t.double(), dim=2)
            tgt = labels._t.long().clamp(min=0)  # (the -1 padding behind label_lengths is never read)
            nll = torch.nn.functional.ctc_loss(lp, tgt, input_lengths._t.long(), label_lengths._t.long(), blank=self.blank,
                                               reduction="none", zero_infinity=False)
            if self.reduction == "sum":
                nll = nll.sum()
            elif self.reduction == "mean":
                nll = (nll / label_lengths._t.double()).mean()
            return Tensor(nll.to(torch.float32))

    class KLDivLoss(paddle.nn.Layer):
        def __init__(self, reduction="mean"):
            super().__init__()
            assert reduction == "none"

        def forward(self, input, label):
            x, t = input._t, label._t
            return Tensor(torch.where(t > 0, t * (torch.log(t.clamp(min=1e-300)) - x), torch.zeros_like(x)))

    paddle.nn.CTCLoss, paddle.nn.KLDivLoss = CTCLoss, KLDivLoss


def main():
    if not os.path.isdir(REFERENCE):
        raise SystemExit("needs /root/reference (build container only)")
    sys.path[:0] = [os.path.join(ROOT, "oracle", "paddle_shim"), REFERENCE]
    import paddle
    import torch
    torch.set_grad_enabled(False)
    paddle_ops(paddle, torch)
    from ppasr.model_utils.conformer.model import ConformerModel

    out = {}
    for name, c in lo.MODEL_CASES.items():
        m = lo.model_case(name)
        sd = m["sd"]
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump({"mean": sd["encoder.global_cmvn.mean"].tolist(), "istd": sd["encoder.global_cmvn.istd"].tolist()}, f)
            mean_istd = f.name
        enc = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=c["num_blocks"], dropout_rate=0.1,
                   positional_dropout_rate=0.1, attention_dropout_rate=0.1, input_layer="conv2d", normalize_before=True,
                   cnn_module_kernel=15, use_cnn_module=True, activation_type="swish", pos_enc_layer_type="rel_pos",
                   cnn_module_norm="layer_norm")
        dec = dict(attention_heads=4, linear_units=c["units"], num_blocks=c["blocks"][0], r_num_blocks=c["blocks"][1],
                   dropout_rate=0.1, positional_dropout_rate=0.1, self_attention_dropout_rate=0.1,
                   src_attention_dropout_rate=0.1)
        model = ConformerModel(input_dim=80, vocab_size=c["V"], mean_istd_path=mean_istd, streaming=False, encoder_conf=enc,
                               decoder_conf=dec, **c["conf"])
        os.unlink(mean_istd)
        own = model.state_dict()
        for k, v in sd.items():
            assert k in own, f"{name}: synthetic parameter {k} is not a name of the reference model"
            assert list(own[k].shape) == list(v.shape), f"{name}: {k} shape {v.shape} vs reference {own[k].shape}"
        missing, unexpected = model.set_state_dict(sd)
        assert not unexpected and not missing, (missing[:8], unexpected[:8])
        model.eval()
        res = model(paddle.to_tensor(m["x"]), paddle.to_tensor(m["lens"], dtype=paddle.int64),
                    paddle.to_tensor(m["labels"]), paddle.to_tensor(m["label_lens"]))
        for k in ("loss", "loss_att", "loss_ctc"):
            out[f"{name}/{k}"] = np.float64(float(res[k]))
        print(f"[ref] {name}: " + "  ".join(f"{k} {out[name + '/' + k]:.7f}" for k in ("loss", "loss_att", "loss_ctc")), flush=True)
    path = os.path.join(HERE, "ref_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote ref_loss.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
