"""CTC forced alignment on the HIP kernels behind ``ppasr_ctc_align`` (include/ppasr_hip.h): when in the probability
table each token of a transcript sits, and how confident the model was of it there.  No reference counterpart: PPASR
returns text and a score only.

The transcript may be a decoder's own output (greedy, beam search, attention rescoring) or one the caller supplies.  The
table stays on the device; one call, one read-back.  The definition of the path (trellis, ties, feasibility) is the
header comment of csrc/ctc_align.hip.
"""
import ctypes

import numpy as np
import torch

from ppasr_amd import _lib

__all__ = ["ctc_align_ids", "forced_align", "align_one", "ProbArena", "text_to_ids", "frames_needed", "MAX_TOKENS", "STATUS_OK",
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


def greedy_runs(frame_ids, frame_maxprob, blank_index=0):
    """The greedy decoder's own tokens with their frames, from what a stream already has on the host: the argmax id and the
    largest probability of every frame so far.  -> (ids, [(begin_frame, end_frame, conf)]): one entry per run of a
    non-blank id -- its first frame, one past its last, the largest probability in between.  That is the alignment of
    greedy's tokens whenever no frame is a near-tie (every frame then takes its argmax on the best path), so a greedy
    stream needs no probability table."""
    fid = np.asarray(frame_ids, np.int64).reshape(-1)
    fp = np.asarray(frame_maxprob, np.float32).reshape(-1)
    assert fid.shape == fp.shape
    if fid.size == 0:
        return [], []
    starts = np.flatnonzero(np.concatenate([[True], fid[1:] != fid[:-1]]))
    ends = np.concatenate([starts[1:], [fid.size]])
    ids, spans = [], []
    for b, e in zip(starts.tolist(), ends.tolist()):
        if fid[b] != blank_index:
            ids.append(int(fid[b]))
            spans.append((b, e, float(fp[b:e].max())))
    return ids, spans


def token_entries(ids, spans, vocabulary, frame_seconds, duration, space_as_blank=False):
    """ids and their ``(begin_frame, end_frame, conf)`` -> [{'text', 'start', 'end', 'score'}]: start = begin x the frame
    step, end = min(end x the frame step, duration).  space_as_blank: ``<space>`` reads as a blank character (greedy's text)."""
    return [{"text": vocabulary[i].replace("<space>", " ") if space_as_blank else vocabulary[i], "start": b * frame_seconds,
             "end": min(e * frame_seconds, duration), "score": c} for i, (b, e, c) in zip(ids, spans)]


class ProbArena:
    """The CTC tables of ``n_sessions`` streams on the device (``ppasr_prob_arena_*``), so that a stream can be aligned:
    one slab of ``n_pages`` pages of ``page_frames`` rows of ``V`` floats, allocated once.  ``append`` puts one round's
    rows of any number of sessions behind their last frames with one launch; ``align`` reads the emissions straight out
    of the pages, for any number of sessions in one call.  All calls on one arena go on one HIP stream."""

    def __init__(self, n_sessions, V, page_frames=16, n_pages=None, device=None):
        """n_pages None: one page per session (a caller that knows its streams' lengths passes the sum of their pages)."""
        self.n_sessions, self.V, self.page_frames = int(n_sessions), int(V), int(page_frames)
        self.n_pages = self.n_sessions if n_pages is None else int(n_pages)
        if min(self.n_sessions, self.page_frames, self.n_pages) < 1 or self.V < 2:
            raise ValueError("ProbArena: n_sessions, page_frames and n_pages must be >= 1 and V >= 2")
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        self._device = torch.device(device) if device is not None else _device()
        with torch.cuda.device(self._device):
            _lib.check(self._lib.ppasr_prob_arena_create(self.n_sessions, self.V, self.page_frames, self.n_pages, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.ppasr_prob_arena_destroy(h)
            self._h = None

    def _stream(self):
        return torch.cuda.current_stream(self._device).cuda_stream

    def _list(self, sessions, what):
        ids = [int(s) for s in sessions]
        if not ids or len(set(ids)) != len(ids) or any(not 0 <= s < self.n_sessions for s in ids):
            raise ValueError(f"ProbArena.{what}: sessions must be distinct indices in [0, {self.n_sessions})")
        return ids, (ctypes.c_int * len(ids))(*ids)

    def append(self, sessions, probs, frames=None):
        """probs [n, c, V] (device tensor or array): rows 0 .. frames[k] - 1 (None: all c) of entry k go behind session
        sessions[k]'s last frame.  One launch, no read-back.  PPASRHipError with status PPASR_ENOSPACE, and nothing
        appended for any session, when the call needs more pages than are free."""
        ids, c_ids = self._list(sessions, "append")
        p = torch.as_tensor(probs, dtype=torch.float32).to(self._device).contiguous()
        if p.dim() != 3 or int(p.shape[0]) != len(ids) or int(p.shape[2]) != self.V:
            raise ValueError(f"ProbArena.append: probs must be [{len(ids)}, c, {self.V}], got {tuple(p.shape)}")
        c = int(p.shape[1])
        c_fr = None
        if frames is not None:
            fr = [int(f) for f in frames]
            if len(fr) != len(ids) or any(not 0 <= f <= c for f in fr):
                raise ValueError("ProbArena.append: frames must hold n values in [0, c]")
            c_fr = (ctypes.c_int * len(ids))(*fr)
        with torch.cuda.device(self._device):
            _lib.check(self._lib.ppasr_prob_arena_append(self._h, c_ids, len(ids), p.data_ptr() if p.numel() else None, c,
                                                         c_fr, self._stream()))

    def reset(self, session=-1):
        """The session's pages (-1: every session's) go back to the free list."""
        if int(session) >= self.n_sessions:
            raise ValueError(f"ProbArena.reset: session {session} out of range")
        _lib.check(self._lib.ppasr_prob_arena_reset(self._h, int(session)))

    def frames(self, session):
        if not 0 <= int(session) < self.n_sessions:
            raise ValueError(f"ProbArena.frames: session {session} out of range")
        return int(self._lib.ppasr_prob_arena_frames(self._h, int(session)))

    def free_pages(self):
        return int(self._lib.ppasr_prob_arena_free_pages(self._h))

    def read(self, session):
        """-> the session's table as one dense device tensor [frames, V]."""
        T = self.frames(session)
        dense = torch.empty(T, self.V, dtype=torch.float32, device=self._device)
        with torch.cuda.device(self._device):
            _lib.check(self._lib.ppasr_prob_arena_read(self._h, int(session), dense.data_ptr() if T else None, self._stream()))
        return dense

    def read_many(self, sessions, Tp=None):
        """-> (dense [n, Tp, V], lens [n] i32) device tensors: the listed sessions' rows with zeros behind each session's
        frames, and the frame counts.  Tp None: the longest listed session.  One launch, nothing read back."""
        ids, c_ids = self._list(sessions, "read_many")
        longest = max(self.frames(s) for s in ids)
        Tp = longest if Tp is None else int(Tp)
        if Tp < longest:
            raise ValueError(f"ProbArena.read_many: Tp = {Tp} is below the longest listed session ({longest} frames)")
        dense = torch.empty(len(ids), Tp, self.V, dtype=torch.float32, device=self._device)
        lens = torch.empty(len(ids), dtype=torch.int32, device=self._device)
        with torch.cuda.device(self._device):
            _lib.check(self._lib.ppasr_prob_arena_read_many(self._h, c_ids, len(ids), Tp, dense.data_ptr() if Tp else None,
                                                            lens.data_ptr(), self._stream()))
        return dense, lens

    def align_ids(self, sessions, tokens, n_tokens, blank_index=0):
        """``ctc_align_ids`` over the listed sessions' tables: B = n, T = the longest listed session, each session's own
        frame count as its frame_lens.  Every output equals ``ctc_align_ids`` on the dense tables, bit for bit."""
        ids, c_ids = self._list(sessions, "align_ids")
        dev = self._device
        tk = torch.as_tensor(tokens, dtype=torch.int32).to(dev).contiguous()
        nt = torch.as_tensor(n_tokens, dtype=torch.int32).to(dev).contiguous()
        B, T = len(ids), max(self.frames(s) for s in ids)
        assert tk.dim() == 2 and tk.shape[0] == B and nt.shape == (B,)
        mt = tk.shape[1]
        out = dict(frame_token=torch.empty(B, T, dtype=torch.int32, device=dev),
                   begin=torch.empty(B, mt, dtype=torch.int32, device=dev), end=torch.empty(B, mt, dtype=torch.int32, device=dev),
                   peak=torch.empty(B, mt, dtype=torch.int32, device=dev), conf=torch.empty(B, mt, dtype=torch.float32, device=dev),
                   score=torch.empty(B, dtype=torch.float32, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev))
        ptr = lambda t: t.data_ptr() if t.numel() else None
        with torch.cuda.device(dev):
            ws = scratch.get(dev, int(self._lib.ppasr_ctc_align_arena_workspace_bytes(B, T, min(mt, MAX_TOKENS))))
            _lib.check(self._lib.ppasr_ctc_align_arena(self._h, c_ids, B, int(blank_index), ptr(tk), nt.data_ptr(), mt,
                                                       ptr(out["frame_token"]), ptr(out["begin"]), ptr(out["end"]),
                                                       ptr(out["peak"]), ptr(out["conf"]), out["score"].data_ptr(),
                                                       out["status"].data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def align(self, sessions, ids_per_session, blank_index=0):
        """The token ids of each listed session's transcript -> per session a list of ``(begin_frame, end_frame, conf)``,
        one per token, as ``align_one`` on the session's dense table; one call and one read-back for all of them.
        ValueError for a bad id and for a transcript that does not fit into its session's frames; more than MAX_TOKENS
        ids are refused (PPASR_EUNSUPPORTED)."""
        lists = [[int(i) for i in ids] for ids in ids_per_session]
        if len(lists) != len(list(sessions)):
            raise ValueError("ProbArena.align: one id list per session")
        for s, ids in zip(sessions, lists):
            if any(i < 0 or i >= self.V or i == blank_index for i in ids):
                raise ValueError(f"forced alignment: token ids must lie in [0, {self.V}) and differ from the blank ({blank_index})")
            if len(ids) > MAX_TOKENS:
                raise _lib.PPASRHipError(f"forced alignment: {len(ids)} tokens exceed the {MAX_TOKENS} the kernel is built "
                                         "for; align shorter segments", _lib.PPASR_EUNSUPPORTED)
            if self.frames(s) < frames_needed(ids):
                raise ValueError(f"forced alignment: the transcript does not fit: T = {self.frames(s)} frames, "
                                 f"{frames_needed(ids)} needed")
        n, mt = len(lists), max([len(ids) for ids in lists] + [0])
        tk = np.zeros((n, mt), np.int32)
        for k, ids in enumerate(lists):
            tk[k, :len(ids)] = ids
        out = self.align_ids(sessions, tk, np.asarray([len(ids) for ids in lists], np.int32), blank_index)
        pack = torch.cat([out["begin"].reshape(-1).to(torch.float64), out["end"].reshape(-1).to(torch.float64),
                          out["conf"].reshape(-1).to(torch.float64), out["status"].to(torch.float64)]).cpu().numpy()
        status = pack[3 * n * mt:]
        if (status != STATUS_OK).any():
            raise _lib.PPASRHipError(f"forced alignment: status {status.astype(int).tolist()}")
        b, e, c = (pack[j * n * mt:(j + 1) * n * mt].reshape(n, mt) for j in range(3))
        return [[(int(b[k, l]), int(e[k, l]), float(c[k, l])) for l in range(len(ids))] for k, ids in enumerate(lists)]


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
