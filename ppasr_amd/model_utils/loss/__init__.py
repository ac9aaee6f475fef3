"""The loss half of evaluation on the HIP kernels behind ``ppasr_ctc_loss`` and ``ppasr_rescorer_loss``
(include/ppasr_hip.h): what ``ConformerModel.forward`` (conformer/model.py:98-109) and ``DeepSpeech2Model.forward`` of the
reference return, forward only -- no backward pass, no dropout (evaluation runs the model in ``eval()``).

    loss     = ctc_weight * loss_ctc + (1 - ctc_weight) * loss_att
    loss_ctc = sum_b -log P_ctc(y_b | x_b) / B                                       (loss/ctc.py:29-50)
    loss_att = (1 - rw) * LS(left decoder) + rw * LS(right decoder)                  (conformer/model.py:129-143)
    LS       = sum of the target rows' KL(smoothed one-hot || softmax) / (B, or the row count)
                                                                                     (loss/label_smoothing_loss.py:68-91)

The definition of the CTC value is the header comment of csrc/ctc_loss.hip.
"""
import numpy as np
import torch

from ppasr_amd import _lib
from ppasr_amd.decoders.ctc_alignment import MAX_TOKENS, STATUS_BAD_INPUT, STATUS_INFEASIBLE, STATUS_OK, _device, _Scratch

__all__ = ["ctc_nll", "model_loss", "MAX_TOKENS", "STATUS_OK", "STATUS_INFEASIBLE", "STATUS_BAD_INPUT"]

scratch = _Scratch()


def ctc_nll(probs, labels, label_lens, frame_lens=None, blank_index=0):
    """probs [B, T, V], labels [B, max_tokens] i32 (only the first label_lens[b] of a row are read), label_lens [B] i32,
    frame_lens [B] i32 or None (all T rows) -> dict of device tensors: nll [B] f32 = -log P_ctc(label | probs), status [B]
    i32 (0 ok; 1 infeasible and 2 bad input, both with nll = +inf).  numpy or device input; asynchronous on the current
    stream."""
    lib = _lib.load()
    dev = probs.device if isinstance(probs, torch.Tensor) and probs.is_cuda else _device()
    p = torch.as_tensor(probs, dtype=torch.float32).to(dev).contiguous()
    tk = torch.as_tensor(labels, dtype=torch.int32).to(dev).contiguous()
    nt = torch.as_tensor(label_lens, dtype=torch.int32).to(dev).contiguous()
    fl = None if frame_lens is None else torch.as_tensor(frame_lens, dtype=torch.int32).to(dev).contiguous()
    B, T, V = p.shape
    assert tk.dim() == 2 and tk.shape[0] == B and nt.shape == (B,) and (fl is None or fl.shape == (B,))
    mt = tk.shape[1]
    out = dict(nll=torch.empty(B, dtype=torch.float32, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev))
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        ws = scratch.get(dev, int(lib.ppasr_ctc_loss_workspace_bytes(B, T, min(mt, MAX_TOKENS))))
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.ppasr_ctc_loss(ptr(p), ptr(fl), B, T, V, int(blank_index), ptr(tk), nt.data_ptr(), mt,
                                      out["nll"].data_ptr(), out["status"].data_ptr(), ws.data_ptr(), ws.numel(), stream))
    return out


def model_loss(model, rescorer, inputs, input_lens, labels, label_lens, ctc_weight, lsm_weight=0.0, reverse_weight=0.0,
               length_normalized_loss=False):
    """One batch of the reference's loader (inputs [B, T, F], input_lens [B], labels [B, U] padded with -1, label_lens [B])
    -> ``{"loss", "loss_att", "loss_ctc"}`` (floats; ``None`` for a branch that does not run, as ``ConformerModel.forward``)
    plus the per-utterance pieces as numpy arrays: ``ctc_nll`` [B], ``ctc_status`` [B], ``att_kl`` / ``r_att_kl`` [B]
    (float64 sums of the row KL terms), ``rows`` [B], ``frames`` [B].

    ``rescorer``: the ``AttentionRescorer`` of the same checkpoint.  ``ctc_weight = 1``, or ``rescorer=None`` with a
    DeepSpeech2 model, gives ``loss = loss_ctc``; ``rescorer=None`` with ``ctc_weight < 1`` raises ``ValueError``.  An
    infeasible utterance makes ``loss_ctc`` ``inf``, as warp-ctc does.  One encode, one read-back."""
    ctc_weight = _branches(model, rescorer, ctc_weight)
    probs, memory, frames = encode_for_loss(model, inputs, input_lens, want_memory=ctc_weight != 1.0)
    return loss_of_encoded(rescorer, probs, memory, frames, labels, label_lens, ctc_weight, lsm_weight, reverse_weight,
                           length_normalized_loss)


def _branches(model, rescorer, ctc_weight):
    """-> the ctc_weight the combination runs with (1.0 for a DeepSpeech2 model without a rescorer); ValueError for a
    combination that needs a decoder that is not there"""
    ctc_weight = float(ctc_weight)
    conformer = hasattr(model, "valid_out_frames")
    if rescorer is None and not conformer:
        ctc_weight = 1.0  # DeepSpeech2Model.forward is the CTCLoss alone
    if rescorer is None and ctc_weight != 1.0:
        raise ValueError("model_loss: ctc_weight < 1 needs the attention decoder (rescorer=None)")
    if rescorer is not None and not conformer:
        raise ValueError("model_loss: a DeepSpeech2 model has no attention decoder")
    return ctc_weight


def encode_for_loss(model, inputs, input_lens, want_memory):
    """One encode -> (probs [B, T', V], memory [B, T', D] or None, frames [B] i32: the encoder's valid output frames, the
    reference's ``encoder_mask.sum`` / ``eouts_len``)."""
    if hasattr(model, "valid_out_frames"):
        frames = model.valid_out_frames(input_lens, inputs.shape[1])
        if want_memory:
            probs, memory = model.get_encoder_out(inputs, input_lens, return_memory=True)
            return probs, memory, frames
        return model.get_encoder_out(inputs, input_lens), None, frames
    probs, frames = model.get_encoder_out_chunk(inputs, input_lens)[:2]
    return probs, None, torch.clamp(frames, max=probs.shape[1]).to(torch.int32)


def loss_of_encoded(rescorer, probs, memory, frames, labels, label_lens, ctc_weight, lsm_weight=0.0, reverse_weight=0.0,
                    length_normalized_loss=False):
    """``model_loss`` behind its encode (``evaluate`` decodes the same probabilities): two launches' worth of kernels on
    the current stream, one read-back."""
    want_att, want_ctc = ctc_weight != 1.0, ctc_weight != 0.0
    dev = probs.device
    lab = torch.as_tensor(labels, dtype=torch.int32).to(dev).contiguous()
    ll = torch.as_tensor(label_lens, dtype=torch.int32).to(dev).contiguous()
    B = lab.shape[0]
    f64 = lambda t: t.to(torch.float64)
    pack = [f64(frames)]
    if want_ctc:
        c = ctc_nll(probs, lab, ll, frames, blank_index=0)
        pack += [f64(c["nll"]), f64(c["status"])]
    if want_att:
        a = rescorer.loss(memory, frames, lab, ll, lsm_weight, reverse_weight)
        pack += [a["att_kl"], a["r_att_kl"], f64(a["rows"])]
    host = torch.stack(pack).cpu().numpy()  # (the read-back; fp32 and int32 are exact in fp64)
    out = {"loss": None, "loss_att": None, "loss_ctc": None, "frames": host[0].astype(np.int64)}
    at = 1
    if want_ctc:
        out["ctc_nll"], out["ctc_status"] = host[at], host[at + 1].astype(np.int64)
        out["loss_ctc"] = float(host[at].sum() / B)
        at += 2
    if want_att:
        out["att_kl"], out["r_att_kl"], out["rows"] = host[at], host[at + 1], host[at + 2].astype(np.int64)
        denom = float(out["rows"].sum()) if length_normalized_loss else float(B)
        rw = float(reverse_weight)
        out["loss_att"] = float(out["att_kl"].sum() / denom * (1.0 - rw) + (out["r_att_kl"].sum() / denom) * rw)
    if not want_ctc:
        out["loss"] = out["loss_att"]
    elif not want_att:
        out["loss"] = out["loss_ctc"]
    else:
        out["loss"] = ctc_weight * out["loss_ctc"] + (1.0 - ctc_weight) * out["loss_att"]
    return out
