"""Attention beam-search decoding (WeNet's ``attention`` decode mode) with the checkpoint's own left attention decoder,
on the HIP kernels behind ``ppasr_attention_decode`` and, with ``ctc_weight``, ``ppasr_attention_decode_joint``.

Unlike ``attention_rescoring`` the hypotheses are not limited to what the CTC head proposed: the search is autoregressive
and driven by the decoder itself (the reference's ``forward_one_step``, which it ships and never calls).  The semantics
are the header comment of ``csrc/attn_decode.hip``.
"""
import torch

from ppasr_amd.decoders.beam_search_decoder import _text

__all__ = ["attention_decode"]


def attention_decode(model, rescorer, memory, out_lens, vocabulary, beam_size=10, max_steps=None, return_ids=False, probs=None,
                     ctc_weight=0.0, blank_id=0):
    """memory [B, T', D] of one encode (``model.get_encoder_out(..., return_memory=True)``), out_lens [B] valid frames or
    None -> per utterance ``(score, text)`` of the best hypothesis of the beam search (its log-probability under the left
    decoder, the eos term included when it ended within ``max_steps``).  ``max_steps=None``: ``min(T', 255, max_len - 1)``.
    Every step is queued on the current stream and the result is read back once.  ``return_ids``: ``(score, text, ids)``,
    the token ids the text was made of (for ``ctc_alignment``).

    ``ctc_weight > 0`` with ``probs`` [B, T', V], the CTC table of the same encode: the CTC-joint search (WeNet's
    ``ctc_weight`` in its attention beam search; ``csrc/attn_decode_joint.hip``).  Every candidate also gets ``ctc_weight`` x
    the log-probability, under the CTC head, that the transcript starts with it, which keeps the decoder from deleting,
    repeating and ending early; the score is then ``log P_att + ctc_weight x log P_ctc`` of the hypothesis."""
    del model  # (kept in the signature for symmetry with the other decoders: the encode already happened)
    fl = None if out_lens is None else torch.as_tensor(out_lens, dtype=torch.int32)
    if ctc_weight:
        if probs is None:
            raise ValueError("attention_decode: ctc_weight > 0 needs probs, the CTC table of the same encode")
        res = rescorer.decode(memory, fl, beam_size=beam_size, max_steps=max_steps, ctc_probs=probs,
                              ctc_weight=float(ctc_weight), blank=blank_id)
    else:
        res = rescorer.decode(memory, fl, beam_size=beam_size, max_steps=max_steps)
    pack = (res["tokens"][:, 0], res["lens"][:, 0], res["scores"][:, 0])
    tk, ln, sc = [t.cpu().numpy() for t in pack]  # (the read-back)
    ids = [tk[b, :max(int(ln[b]), 0)].tolist() for b in range(tk.shape[0])]
    return [(float(sc[b]), _text(ids[b], vocabulary)) + ((ids[b],) if return_ids else ()) for b in range(tk.shape[0])]
