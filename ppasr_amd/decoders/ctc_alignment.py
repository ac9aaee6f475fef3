"""CTC forced alignment on the HIP kernels behind ``ppasr_ctc_align`` (include/ppasr_hip.h): when in the probability
table each token of a transcript sits, and how confident the model was of it there.  No reference counterpart: PPASR
returns text and a score only.

The transcript may be a decoder's own output (greedy, beam search, attention rescoring) or one the caller supplies.  The
table stays on the device; one call, one read-back.  The definition of the path (trellis, ties, feasibility) is the
header comment of csrc/ctc_align.hip.
"""
import numpy as np
import torch

from ppasr_amd import _lib

__all__ = ["ctc_align_ids", "forced_align", "align_one", "text_to_ids", "frames_needed", "MAX_TOKENS", "STATUS_OK",
           "STATUS_INFEASIBLE", "STATUS_BAD_INPUT"]

MAX_TOKENS = 255  # tokens per utterance the kernel is built for
STATUS_OK, STATUS_INFEASIBLE, STATUS_BAD_INPUT = 0, 1, 2


class _Scratch:
    """The workspace kept between calls, one tensor per (device, HIP stream)."""

    def __init__(self):
        self._ws = {}

    def get(self, dev, need):
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        return ws


scratch = _Scratch()


def _device():
    if not torch.cuda.is_available():
        raise _lib.PPASRHipError("no HIP device visible: ppasr_amd has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def frames_needed(ids):
    """Frames the shortest alignment of ``ids`` takes: one per token and one blank between two equal neighbours."""
    ids = [int(i) for i in ids]
    return len(ids) + sum(1 for i in range(1, len(ids)) if ids[i] == ids[i - 1])


def ctc_align_ids(probs, tokens, n_tokens, frame_lens=None, blank_index=0):
    """probs [B, T, V], tokens [B, max_tokens] i32 (only the first n_tokens[b] of a row are read), n_tokens [B] i32,
    frame_lens [B] i32 or None (all T rows) -> dict of device tensors: frame_token [B, T] i32, begin / end / peak
    [B, max_tokens] i32, conf [B, max_tokens] f32, score [B] f32, status [B] i32 (0 aligned, 1 infeasible, 2 bad input).
    numpy or device input; asynchronous on the current stream."""
    lib = _lib.load()
    dev = probs.device if isinstance(probs, torch.Tensor) and probs.is_cuda else _device()
    p = torch.as_tensor(probs, dtype=torch.float32).to(dev).contiguous()
    tk = torch.as_tensor(tokens, dtype=torch.int32).to(dev).contiguous()
    nt = torch.as_tensor(n_tokens, dtype=torch.int32).to(dev).contiguous()
    fl = None if frame_lens is None else torch.as_tensor(frame_lens, dtype=torch.int32).to(dev).contiguous()
    B, T, V = p.shape
    assert tk.dim() == 2 and tk.shape[0] == B and nt.shape == (B,) and (fl is None or fl.shape == (B,))
    mt = tk.shape[1]
    out = dict(frame_token=torch.empty(B, T, dtype=torch.int32, device=dev),
               begin=torch.empty(B, mt, dtype=torch.int32, device=dev), end=torch.empty(B, mt, dtype=torch.int32, device=dev),
               peak=torch.empty(B, mt, dtype=torch.int32, device=dev), conf=torch.empty(B, mt, dtype=torch.float32, device=dev),
               score=torch.empty(B, dtype=torch.float32, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev))
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        ws = scratch.get(dev, int(lib.ppasr_ctc_align_workspace_bytes(B, T, min(mt, MAX_TOKENS))))
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.ppasr_ctc_align(ptr(p), ptr(fl), B, T, V, int(blank_index), ptr(tk), nt.data_ptr(), mt,
                                       ptr(out["frame_token"]), ptr(out["begin"]), ptr(out["end"]), ptr(out["peak"]),
                                       ptr(out["conf"]), out["score"].data_ptr(), out["status"].data_ptr(), ws.data_ptr(),
                                       ws.numel(), stream))
    return out


def text_to_ids(text, vocabulary, space_token=True):
    """The ids of a transcript: at every position the longest vocabulary entry that matches (entries are single
    characters except markers such as ``<unk>``).  ``space_token``: a blank character stands for ``<space>`` when the
    vocabulary has that entry.  ValueError for a character no entry starts with."""
    index = {v: i for i, v in enumerate(vocabulary)}
    longest = max((len(v) for v in vocabulary), default=1)
    ids, at = [], 0
    while at < len(text):
        if space_token and text[at] == " " and "<space>" in index:
            ids.append(index["<space>"])
            at += 1
            continue
        for n in range(min(longest, len(text) - at), 0, -1):
            i = index.get(text[at:at + n])
            if i is not None:
                ids.append(i)
                at += n
                break
        else:
            raise ValueError(f"forced alignment: character {text[at]!r} is not in the vocabulary")
    return ids


def align_one(probs_seq, ids, blank_index=0):
    """One [T, V] table (numpy or device tensor) and the ids of its transcript -> list of ``(begin_frame, end_frame,
    conf)``, one per token; one call and one read-back.  ValueError for a bad id and for a transcript that does not fit
    into T frames; more than MAX_TOKENS ids are refused (PPASR_EUNSUPPORTED)."""
    ids = [int(i) for i in ids]
    T, V = probs_seq.shape
    if any(i < 0 or i >= V or i == blank_index for i in ids):
        raise ValueError(f"forced alignment: token ids must lie in [0, {V}) and differ from the blank ({blank_index})")
    if len(ids) > MAX_TOKENS:
        raise _lib.PPASRHipError(f"forced alignment: {len(ids)} tokens exceed the {MAX_TOKENS} the kernel is built for; "
                                 "align shorter segments", _lib.PPASR_EUNSUPPORTED)
    need = frames_needed(ids)
    if T < need:
        raise ValueError(f"forced alignment: the transcript does not fit: T = {T} frames, {need} needed "
                         f"({len(ids)} tokens, {need - len(ids)} repeats)")
    p = probs_seq if isinstance(probs_seq, torch.Tensor) else np.asarray(probs_seq, np.float32)
    n = len(ids)
    out = ctc_align_ids(torch.as_tensor(p)[None], np.asarray(ids, np.int32).reshape(1, n), np.asarray([n], np.int32), None,
                        blank_index)
    pack = torch.cat([out["begin"][0].to(torch.float64), out["end"][0].to(torch.float64), out["conf"][0].to(torch.float64),
                      out["status"].to(torch.float64)]).cpu().numpy()  # (the read-back; fp32 and int32 are exact in fp64)
    if int(pack[3 * n]) != STATUS_OK:
        raise _lib.PPASRHipError(f"forced alignment: status {int(pack[3 * n])}")
    return [(int(pack[l]), int(pack[n + l]), float(pack[2 * n + l])) for l in range(n)]


def forced_align(probs_seq, text_or_ids, vocabulary, blank_index=0):
    """One [T, V] table and its transcript (a string, split into vocabulary entries, or a list of ids) -> list of
    ``(token_str, begin_frame, end_frame, conf)``, one per token.  ValueError for a character outside the vocabulary, a
    bad id, and a transcript that does not fit into T frames (the message gives T and the frames needed)."""
    ids = text_to_ids(text_or_ids, vocabulary) if isinstance(text_or_ids, str) else [int(i) for i in text_or_ids]
    spans = align_one(probs_seq, ids, blank_index)
    return [(vocabulary[i].replace("<space>", " "), b, e, c) for i, (b, e, c) in zip(ids, spans)]
