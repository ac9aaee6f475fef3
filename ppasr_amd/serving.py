"""Many-session streaming recogniser built on session groups (``ppasr_encode_chunk_group``; per-session stream handles for
the families ``make_stream_group`` builds no group for -- a ready group, e.g. ``SqueezeformerStreamGroup``, can be passed in).

No reference counterpart: PPASR serves one stream per ``PPASRPredictor`` (``predict_stream``, predict.py:232-337, one
global predictor behind its FastAPI / GUI apps).  ``StreamPool`` keeps the per-session state machine of
``predict_stream`` (audio remainder, cached feature frames, 67-frame windows with stride 64 = 16 output frames,
greedy_decoder_chunk's running lists) for N sessions and advances every session that has a full window buffered with ONE
set of kernel launches per round.  Each session's result equals what its own ``PPASRPredictor.predict_stream`` returns
with the same decoder: ``ctc_greedy`` (the default), or ``ctc_beam_search``, where every round's CTC probabilities go to a
``BeamSearchSessions`` pool -- one beam-search launch for all sessions of the round, on the same stream as the encoder, with
no host synchronisation in between.

``timestamps=True`` adds token times to a pool (``finish(...)["timestamps"]``, ``pool.timestamps(session)``).  A beam
search's tokens are aligned against the session's probability table, which a ``ProbArena`` keeps on the device: one more
launch per round, whatever the number of sessions.  Greedy keeps no table: its tokens are the runs of the frame ids the
pool downloads anyway, which is their alignment whenever no frame is a near-tie.  Their confidences are read off the
round's table before it is dropped (``ppasr_ctc_greedy``'s per-frame stage, a fixed number of launches per round): the
head's own per-frame maximum is 1 / sum of its running statistics and may differ from the table's entry, which the
alignment copies, in the last bit."""
import numpy as np
import torch

from ppasr_amd.data_utils.featurizer import AudioFeaturizer, StreamResampler, db_gain, pcm_bytes_to_float
from ppasr_amd.model_utils.conformer.model import make_stream_group

__all__ = ["StreamPool"]

_WINDOW, _STRIDE, _CONTEXT, _KEEP = 67, 64, 7, 3  # predict.py:277-283
_DECODERS = ("ctc_greedy", "ctc_beam_search")
# keys of ctc_beam_search_decoder_conf (configs/conformer.yml); the shipped values except the language model
_BEAM_DEFAULTS = dict(alpha=2.2, beta=4.3, beam_size=300, num_processes=10, cutoff_prob=0.99, cutoff_top_n=40,
                      language_model_path=None)
# decoder="attention_rescoring": PPASRPredictor's defaults for attention_rescoring_decoder_conf
_RESCORING_DEFAULTS = dict(beam_size=10, ctc_weight=0.5, reverse_weight=0.3, cutoff_prob=0.99, cutoff_top_n=40)
_MAX_RESCORE_TOKENS = 255  # tokens per hypothesis the rescoring kernels take (attention_rescoring.MAX_ROWS - 1)


class _Session:
    def __init__(self):
        self.remained_wav = None
        self.cached_feat = None
        self.frame_ids = []    # argmax index of every output frame so far
        self.frame_probs = []  # max prob of the non-blank frames
        self.result = None
        self.sample_rate = None  # fixed by the session's first packet
        self.resampler = None    # StreamResampler of a session whose rate is not the featurizer's
        # timestamps=True only
        self.seconds = 0.0       # audio fed so far
        self.frame_maxprob = []  # greedy: largest entry of every output frame's table row so far
        self.ids = []            # beam search: token ids of the current best hypothesis
        self.overflow = False    # beam search: the session outgrew its share of the probability arena


class StreamPool:
    def __init__(self, model, vocab_list, n_sessions, preprocess_conf=None, max_seconds=200.0, blank_index=0, group=None,
                 decoder="ctc_greedy", decoder_conf=None, beam_compact=False, timestamps=False, table_seconds=30.0,
                 page_frames=16, rescorer=None, memory_seconds=30.0):
        """group: a ready session group for `model` with `n_sessions` slots (e.g. ``SqueezeformerStreamGroup``,
        ``GeneralConformerStreamGroup``); None =
        ``make_stream_group``'s choice.  decoder: "ctc_greedy" or "ctc_beam_search"; decoder_conf: keys of
        ``ctc_beam_search_decoder_conf`` (alpha, beta, beam_size, num_processes, cutoff_prob, cutoff_top_n,
        language_model_path), over the shipped values without a language model.  beam_compact: the beam-search pool
        compacts a session's prefix arena before it would grow its block (``BeamSearchSessions(compact=True)``), so that
        long streams stay in bounded memory; not a decoder_conf key, which mirror the YAML.
        timestamps: ``finish`` adds ``"timestamps": [{"text", "start", "end", "score"}, ...]`` and ``timestamps(session)``
        gives the same for the current partial text.  With beam search every session may keep ``table_seconds`` of
        probabilities in an arena of ``page_frames``-row pages (n_sessions x ceil(table_seconds x frames per second /
        page_frames) pages of page_frames x V floats, allocated once); a session that outgrows its share, or whose
        hypothesis exceeds 255 tokens, gets ``"timestamps": None`` (with ``"table_overflow": True`` in the first case)
        and keeps its text and score.  Off (the default): no arena, no extra launch, results as before.
        decoder="attention_rescoring" with rescorer=<AttentionRescorer>: WeNet's two-pass mode for streams.  While audio
        arrives the pool is a ``ctc_beam_search`` pool without a scorer (decoder_conf: beam_size, ctc_weight,
        reverse_weight, cutoff_prob, cutoff_top_n, over ``PPASRPredictor``'s rescoring defaults) whose encoder rounds
        also keep their encoder output, ``memory_seconds`` per session, in an arena of ``page_frames``-row pages of 256
        floats -- one more launch per round.  ``finish`` / ``finish_many`` then rescore the beam's n-best list over that
        memory: ``{"text", "score", "rescored": True}``, score = the total as offline ``attention_rescoring`` returns
        it.  A session that outgrew ``memory_seconds`` (``"memory_overflow": True``) or whose best hypothesis exceeds
        255 tokens keeps its CTC result with ``"rescored": False``.  Conformer models on the fused route."""
        if not isinstance(timestamps, (bool, np.bool_)):
            raise ValueError("StreamPool: timestamps must be True or False")
        if isinstance(table_seconds, (bool, np.bool_)) or not isinstance(table_seconds, (int, float, np.integer, np.floating)) \
                or not 0 < float(table_seconds) < float("inf"):
            raise ValueError("StreamPool: table_seconds must be a positive number of seconds")
        if isinstance(page_frames, (bool, np.bool_)) or not isinstance(page_frames, (int, np.integer)) or page_frames < 1:
            raise ValueError("StreamPool: page_frames must be an integer >= 1")
        rescoring = decoder == "attention_rescoring"
        if decoder not in _DECODERS and not rescoring:
            raise ValueError(f"StreamPool: unknown decoder {decoder!r} (one of {', '.join(_DECODERS)}, attention_rescoring)")
        if rescoring and rescorer is None:
            raise ValueError("StreamPool: decoder='attention_rescoring' needs rescorer=<AttentionRescorer> (the checkpoint's "
                             "attention decoder): without one a pool decodes with ctc_greedy or ctc_beam_search")
        if rescorer is not None and not rescoring:
            raise ValueError("StreamPool: rescorer applies to decoder='attention_rescoring' only")
        if isinstance(memory_seconds, (bool, np.bool_)) or not isinstance(memory_seconds, (int, float, np.integer, np.floating)) \
                or not 0 < float(memory_seconds) < float("inf"):
            raise ValueError("StreamPool: memory_seconds must be a positive number of seconds")
        if not isinstance(beam_compact, (bool, np.bool_)):
            raise ValueError("StreamPool: beam_compact must be True or False")
        if beam_compact and decoder != "ctc_beam_search":
            raise ValueError("StreamPool: beam_compact applies to decoder='ctc_beam_search' only")
        conf = dict(decoder_conf or {})
        known = _RESCORING_DEFAULTS if rescoring else _BEAM_DEFAULTS
        if rescoring and "language_model_path" in conf:
            raise ValueError("StreamPool: decoder='attention_rescoring' takes no language_model_path: the n-best list is the "
                             "plain CTC prefix beam search's, as offline")
        unknown = sorted(set(conf) - set(known))
        if unknown:
            raise ValueError(f"StreamPool: unknown decoder_conf keys {unknown} (known: {sorted(known)})")
        if conf and decoder == "ctc_greedy":
            raise ValueError("StreamPool: decoder_conf applies to decoder='ctc_beam_search' and 'attention_rescoring' only")
        if rescoring and timestamps:
            raise ValueError("StreamPool: timestamps=True is not built for decoder='attention_rescoring'")
        self.decoder = decoder
        self.model = model
        self.vocab = list(vocab_list)
        self.blank = blank_index
        if group is None:
            # (one set of launches per round for plain Conformer and streaming DeepSpeech2 handles; per-session stream
            #  handles behind the same interface for the Squeezeformer, the Efficient-Conformer and the general route)
            # (DeepSpeech2: session states that do not grow, no max_len)
            max_frames = int(max_seconds * 25) + 32
            if hasattr(model, "max_len"):
                max_frames = min(model.max_len, max_frames)
            group = make_stream_group(model, n_sessions, max_frames=max_frames)
        elif getattr(group, "model", None) is not model or int(getattr(group, "n_sessions", -1)) != int(n_sessions):
            raise ValueError("StreamPool(group=...): the group must be built for the same model and session count")
        self.group = group
        self.featurizer = AudioFeaturizer(**(preprocess_conf or {}))
        self.sessions = [_Session() for _ in range(n_sessions)]
        self.beam = None
        if decoder == "ctc_beam_search":
            from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
            self.beam = BeamSearchSessions(n_sessions, vocab_list=self.vocab, blank_id=blank_index,
                                           compact=bool(beam_compact), **{**_BEAM_DEFAULTS, **conf})
        self.with_timestamps = bool(timestamps)
        self.frame_seconds = float(getattr(model, "total_subsampling", 4)) * 0.010  # (PPASRPredictor._token_times' step)
        self.arena = None
        self.session_pages = 0  # pages a session may hold
        if self.with_timestamps and self.beam is not None:
            from ppasr_amd.decoders.ctc_alignment import ProbArena
            frames = int(np.ceil(float(table_seconds) / self.frame_seconds - 1e-6))  # (2.56 s / 0.04 s is 64 frames, not 65)
            self.session_pages = max(1, -(-frames // int(page_frames)))
            self.arena = ProbArena(n_sessions, len(self.vocab), page_frames=int(page_frames),
                                   n_pages=int(n_sessions) * self.session_pages, device=self.beam._device)
        self.rescorer = rescorer
        self.memory = None       # attention_rescoring: the sessions' encoder output, a ProbArena of 256-wide rows
        self.memory_pages = 0    # pages a session may hold there
        if rescoring:
            from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
            from ppasr_amd.decoders.ctc_alignment import ProbArena
            self.rescoring_conf = {**_RESCORING_DEFAULTS, **conf}
            rc = self.rescoring_conf
            self.beam = BeamSearchSessions(n_sessions, alpha=0.0, beta=0.0, vocab_list=self.vocab, blank_id=blank_index,
                                           beam_size=rc["beam_size"], cutoff_prob=rc["cutoff_prob"],
                                           cutoff_top_n=rc["cutoff_top_n"])
            frames = int(np.ceil(float(memory_seconds) / self.frame_seconds - 1e-6))
            self.memory_pages = max(1, -(-frames // int(page_frames)))
            self.memory = ProbArena(n_sessions, int(rescorer.d_model), page_frames=int(page_frames),
                                    n_pages=int(n_sessions) * self.memory_pages, device=self.beam._device)

    def _rate_of(self, session, sample_rate):
        """The rate of a packet for `session` (None = the featurizer's) -> (rate, the session's resampler or None: a new
        one is returned, not stored).  ValueError, before anything is modified: a rate other than the one the session's
        first packet fixed; a foreign rate without ``resample="device"`` in preprocess_conf."""
        s = self.sessions[session]
        model_rate = int(self.featurizer._sr)
        rate = model_rate if sample_rate is None else int(sample_rate)
        if s.sample_rate is not None and rate != s.sample_rate:
            raise ValueError(f"StreamPool: session {session} is fed at {s.sample_rate} Hz, not {rate} Hz: a session's rate is "
                             "fixed by its first packet (reset it for a new stream)")
        if rate == model_rate:
            return rate, None
        if self.featurizer.resample_mode != "device":
            raise ValueError(f"StreamPool: packets at {rate} Hz for a model at {model_rate} Hz need resample=\"device\" in "
                             "preprocess_conf (AudioFeaturizer(resample=\"device\")): a pool does not resample on the host")
        return rate, s.resampler if s.resampler is not None else StreamResampler(self.featurizer, rate)

    def feed(self, session, audio_data, channels=1, samp_width=2, sample_rate=None):
        """Append PCM bytes or float samples to a session's buffer (what predict_stream does with each packet).
        sample_rate: the packet's rate, None = the featurizer's.  A foreign rate (``resample="device"``) goes through the
        session's ``StreamResampler`` first; the model-rate samples that are complete then take the path below."""
        rate, resampler = self._rate_of(session, sample_rate)
        s = self.sessions[session]
        samples = (pcm_bytes_to_float(audio_data, channels, samp_width) if isinstance(audio_data, (bytes, bytearray))
                   else np.asarray(audio_data, np.float32).reshape(-1))
        s.seconds += samples.size / float(rate)
        if resampler is not None:
            samples = resampler.push(samples)
        s.sample_rate, s.resampler = rate, resampler
        self._feed_model_rate(s, samples)

    def _feed_model_rate(self, s, samples):
        s.remained_wav = samples if s.remained_wav is None else np.concatenate([s.remained_wav, samples])
        feat = self.featurizer.featurize(s.remained_wav)
        # predict_stream's buffered samples are normalised IN PLACE by the reference's featurize() (ppasr_amd/predict.py
        # explains): the remainder that stays buffered carries this call's gain
        if self.featurizer.use_db_normalization and s.remained_wav.size:
            s.remained_wav = s.remained_wav * db_gain(s.remained_wav, self.featurizer.target_db)
        if feat.shape[0] > 0:
            feat = feat[np.newaxis]
            s.cached_feat = self._joined(s.cached_feat, feat)
            hop = int(round(getattr(self.featurizer, "sample_rate", 16000) * 0.010))  # 10 ms at the featurizer's rate
            s.remained_wav = s.remained_wav[hop * feat.shape[1]:]

    def _joined(self, cached, feat):
        """cached_feat [1, T, F] + new frames [1, t, F]: numpy while a session is fed by ``feed`` alone, a device tensor
        from its first ``feed_many`` on (the same float32 values either way)."""
        if cached is None:
            return feat
        if isinstance(cached, np.ndarray) and isinstance(feat, np.ndarray):
            return np.concatenate([cached, feat], axis=1)
        dev = self.featurizer._device
        return torch.cat([torch.as_tensor(cached).to(dev), torch.as_tensor(feat).to(dev)], dim=1)

    def feed_many(self, packets, channels=1, samp_width=2, sample_rate=None):
        """``feed`` for many sessions at once: packets = {session: PCM bytes or float samples}.  sample_rate: one rate for
        all packets or {session: rate} (a session not listed: the featurizer's); the packets of one foreign rate are
        resampled by one batched launch, then everything takes the path below.  The listed sessions'
        buffers go to the device in one upload and are featurized by one set of launches
        (``AudioFeaturizer.featurize_many``); their features stay on the device (``cached_feat`` becomes a device tensor,
        ``step`` / ``finish`` cut the windows there).  Every session ends up exactly where ``feed`` would leave it.  An
        unknown or repeated session index and a refused gain raise ValueError before any session is modified."""
        ids = [int(i) for i in (packets.keys() if hasattr(packets, "keys") else [p[0] for p in packets])]
        audio = list(packets.values()) if hasattr(packets, "values") else [p[1] for p in packets]
        if len(set(ids)) != len(ids) or any(i < 0 or i >= len(self.sessions) for i in ids):
            raise ValueError(f"StreamPool.feed_many: session indices must be distinct and in 0..{len(self.sessions) - 1}")
        rates = [self._rate_of(i, sample_rate.get(i) if isinstance(sample_rate, dict) else sample_rate) for i in ids]
        new = [(pcm_bytes_to_float(a, channels, samp_width) if isinstance(a, (bytes, bytearray))
                else np.asarray(a, np.float32).reshape(-1)) for a in audio]
        seconds = [x.size / float(rate) for x, (rate, _) in zip(new, rates)]
        by_rate = {}  # foreign rate -> positions in `ids`
        for k, (rate, resampler) in enumerate(rates):
            if resampler is not None:
                by_rate.setdefault(rate, []).append(k)
        states = {}
        for rate, members in by_rate.items():
            jobs = [rates[k][1]._prepare(new[k]) for k in members]
            for k, job, out in zip(members, jobs, self.featurizer._resample_windows(rate, [j[0] for j in jobs])):
                new[k], states[k] = out, job[1]
        wavs = []
        for i, samples in zip(ids, new):
            s = self.sessions[i]
            wavs.append(samples if s.remained_wav is None else np.concatenate([s.remained_wav, samples]))
        feats, counts = self.featurizer.featurize_many(wavs)
        for k, i in enumerate(ids):  # nothing raises from here on: the sessions take their new state
            self.sessions[i].sample_rate, self.sessions[i].resampler = rates[k]
            self.sessions[i].seconds += seconds[k]
            if k in states:
                rates[k][1]._commit(states[k])
        # (the remainder's gain: on the host, as in feed)
        if self.featurizer.use_db_normalization:
            wavs = [w * db_gain(w, self.featurizer.target_db) if w.size else w for w in wavs]
        hop = int(round(getattr(self.featurizer, "sample_rate", 16000) * 0.010))
        row = 0
        for i, w, t in zip(ids, wavs, counts.tolist()):
            s = self.sessions[i]
            if t > 0:
                s.cached_feat = self._joined(s.cached_feat, feats[row:row + t].unsqueeze(0))
                w = w[hop * t:]
                row += t
            s.remained_wav = w

    def step(self):
        """Advance, as often as possible, every session that holds a full 67-frame window; -> {session: result dict}
        for the sessions that produced new output."""
        updated = {}
        while True:
            ready = [i for i, s in enumerate(self.sessions)
                     if s.cached_feat is not None and s.cached_feat.shape[1] >= _WINDOW]
            if not ready:
                break
            windows = [self.sessions[i].cached_feat[:, :_WINDOW] for i in ready]
            if all(isinstance(w, np.ndarray) for w in windows):
                chunks = np.concatenate(windows, axis=0)
            else:  # sessions fed by feed_many: the windows are cut and stacked on the device
                dev = self.featurizer._device
                chunks = torch.cat([torch.as_tensor(w).to(dev) for w in windows], dim=0)
            results = self._advance(ready, chunks)
            for k, i in enumerate(ready):
                s = self.sessions[i]
                # windows advance by the stride; predict_stream keeps `end - 3` frames once no full window is left,
                # which is the same position because the next window starts at cur + 64 = end - 3
                s.cached_feat = s.cached_feat[:, _STRIDE:]
                s.result = results[k]
                updated[i] = s.result
        return updated

    def _advance(self, ids, chunks):
        """One encoder round for the listed sessions, then their decoder step -> result dicts by list position."""
        if self.memory is not None:
            # the encoder round keeps its output (one more launch), the search is the beam-search pool's
            c = int(self.model.out_frames(int(chunks.shape[1])))
            _, _, probs = self.group.encode_chunks(ids, chunks, want_probs=True, memory_arena=self.memory,
                                                   memory_frames=self._memory_frames(ids, c))
            return [{"text": text, "score": score} for score, text in self.beam.decode_chunks(ids, probs)]
        if self.beam is not None:
            # the probabilities stay on the device: the search is queued behind the encoder on the same stream
            _, _, probs = self.group.encode_chunks(ids, chunks, want_probs=True)
            if self.arena is None:
                return [{"text": text, "score": score} for score, text in self.beam.decode_chunks(ids, probs)]
            self._keep_table(ids, probs)
            out = []
            for i, (score, text, tokens) in zip(ids, self.beam.decode_chunks(ids, probs, return_ids=True)):
                self.sessions[i].ids = tokens
                out.append({"text": text, "score": score})
            return out
        if self.with_timestamps:
            from ppasr_amd.decoders.ctc_greedy_decoder import greedy_decode_ids
            fa, fp, probs = self.group.encode_chunks(ids, chunks, want_probs=True)
            table_max = greedy_decode_ids(probs, None, self.blank)[4].cpu().numpy()  # each frame's largest table entry
        else:
            fa, fp = self.group.encode_chunks(ids, chunks)
        fa, fp = fa.cpu().numpy(), fp.cpu().numpy()
        out = []
        for k, i in enumerate(ids):
            s = self.sessions[i]
            s.frame_ids.extend(fa[k].tolist())
            s.frame_probs.extend(fp[k][fa[k] != self.blank].tolist())
            if self.with_timestamps:
                s.frame_maxprob.extend(table_max[k].tolist())
            out.append(self._result(s))
        return out

    def _keep_table(self, ids, probs):
        """The round's probabilities go behind the listed sessions' tables: one launch.  A session whose table would
        outgrow its share of the arena gives its pages back and appends nothing from then on (until ``reset``); the
        shares add up to the arena, so the others always fit."""
        c = int(probs.shape[1])
        room = self.session_pages * self.arena.page_frames
        frames = []
        for i in ids:
            s = self.sessions[i]
            if not s.overflow and self.arena.frames(i) + c > room:
                s.overflow = True
                self.arena.reset(i)
            frames.append(0 if s.overflow else c)
        self.arena.append(ids, probs, frames)

    def _memory_frames(self, ids, c):
        """Rows of this round each listed session keeps in the memory arena (``_keep_table``'s policy): a session whose
        memory would outgrow its share gives its pages back and keeps nothing from then on (until ``reset``)."""
        room = self.memory_pages * self.memory.page_frames
        frames = []
        for i in ids:
            s = self.sessions[i]
            if not s.overflow and self.memory.frames(i) + c > room:
                s.overflow = True
                self.memory.reset(i)
            frames.append(0 if s.overflow else c)
        return frames

    def finish_many(self, sessions):
        """``finish`` for many sessions of a ``decoder="attention_rescoring"`` pool: each is flushed as ``finish`` does,
        then ONE n-best read of the beam-search pool, ONE gather of the sessions' memory, ONE ``ppasr_rescore`` call with
        B = the sessions that can be rescored, and one read-back.  -> [result dict] by list position (None for a session
        that never produced output)."""
        if self.memory is None:
            raise ValueError("StreamPool.finish_many: built for decoder='attention_rescoring' (finish each session otherwise)")
        ids = [int(i) for i in sessions]
        if len(set(ids)) != len(ids) or any(i < 0 or i >= len(self.sessions) for i in ids):
            raise ValueError(f"StreamPool.finish_many: session indices must be distinct and in 0..{len(self.sessions) - 1}")
        for i in ids:
            self._flush(i)
        out = {i: (None if self.sessions[i].result is None else dict(self.sessions[i].result, rescored=False)) for i in ids}
        for i in ids:
            if out[i] is not None and self.sessions[i].overflow:
                out[i]["memory_overflow"] = True
        live = [i for i in ids if out[i] is not None and not self.sessions[i].overflow and self.memory.frames(i) > 0]
        if live:
            from ppasr_amd.decoders.beam_search_decoder import _text
            rc = self.rescoring_conf
            L = min(max(self.beam.frames(i) for i in live), _MAX_RESCORE_TOKENS)
            tokens, lens, scores = self.beam.nbest(live, rc["beam_size"], max_tokens=max(L, 1))
            memory, mlens = self.memory.read_many(live)
            res = self.rescorer.rescore(memory, mlens, tokens, lens, scores, rc["ctc_weight"], rc["reverse_weight"])
            best = res["best"].to(torch.int64)
            idx = best[:, None, None].expand(-1, 1, tokens.shape[2])
            pack = (tokens.gather(1, idx)[:, 0], lens.gather(1, best[:, None])[:, 0],
                    res["total"].gather(1, best[:, None])[:, 0], lens.max(dim=1).values)
            tk, ln, sc, longest = [t.cpu().numpy() for t in pack]  # (the read-back)
            for k, i in enumerate(live):
                if int(longest[k]) > tokens.shape[2]:  # a hypothesis beyond 255 tokens: the CTC result stays
                    continue
                out[i] = {"text": _text(tk[k, :max(int(ln[k]), 0)].tolist(), self.vocab), "score": float(sc[k]),
                          "rescored": True}
        return [out[i] for i in ids]

    def timestamps(self, session):
        """[{"text", "start", "end", "score"}, ...], one entry per token of the session's current text: start = first
        frame x the model's frame step, end = one past the last frame x the step, clipped to the audio fed so far, score
        = the token's largest probability in between.  None for a beam-search session without a table (it outgrew
        ``table_seconds``) or with more than 255 tokens.  Beam search: one alignment call and one read-back."""
        from ppasr_amd.decoders.ctc_alignment import MAX_TOKENS, greedy_runs, token_entries
        if not self.with_timestamps:
            raise ValueError("StreamPool.timestamps: the pool was built with timestamps=False")
        s = self.sessions[session]
        if self.arena is None:
            ids, spans = greedy_runs(s.frame_ids, s.frame_maxprob, self.blank)
            return token_entries(ids, spans, self.vocab, self.frame_seconds, s.seconds, space_as_blank=True)
        if s.overflow or len(s.ids) > MAX_TOKENS:
            return None
        if not s.ids:
            return []
        spans = self.arena.align([session], [s.ids], self.blank)[0]
        return token_entries(s.ids, spans, self.vocab, self.frame_seconds, s.seconds)

    def session_probs(self, session):
        """The session's probability table so far, a dense device tensor [frames, V] (beam search with timestamps=True;
        [0, V] for a session that outgrew ``table_seconds``)."""
        if self.arena is None:
            raise ValueError("StreamPool.session_probs: no table is kept (timestamps=True with decoder='ctc_beam_search')")
        return self.arena.read(session)

    def finish(self, session):
        """End of a session's audio (``predict_stream(..., is_end=True)``, predict.py:291-298): run the buffered full
        windows, then the last, shorter window if at least 7 frames (the conv front-end's context) are left.
        -> the session's final result dict (None if it never produced output); with ``timestamps=True`` a copy of it
        with ``"timestamps"`` (``timestamps(session)``) and, for a session that outgrew its table, ``"table_overflow":
        True``.  The session keeps its state until ``reset``.  A session fed at a foreign rate flushes its resampler first: the last model-rate samples, which waited
        for audio that will not come, are fed like a packet.  ``decoder="attention_rescoring"``: the flush, then the
        second pass -- ``finish_many([session])[0]``."""
        if self.memory is not None:
            return self.finish_many([session])[0]
        s = self.sessions[session]
        self._flush(session)
        if not self.with_timestamps or s.result is None:
            return s.result
        out = dict(s.result, timestamps=self.timestamps(session))
        if s.overflow:
            out["table_overflow"] = True
        return out

    def _flush(self, session):
        """The end of a session's audio: the resampler's last samples, the buffered full windows, the last shorter one."""
        s = self.sessions[session]
        if s.resampler is not None:
            rest = s.resampler.flush()
            if rest.size:
                self._feed_model_rate(s, rest)
        self.step()
        if s.cached_feat is not None and s.cached_feat.shape[1] >= _CONTEXT:
            s.result = self._advance([session], s.cached_feat)[0]
            s.cached_feat = s.cached_feat[:, s.cached_feat.shape[1] - _KEEP:]

    def _result(self, s):
        hist = np.asarray(s.frame_ids, np.int64)
        keep = np.ones(len(hist), bool)
        keep[1:] = hist[1:] != hist[:-1]
        ids = hist[keep]
        ids = ids[ids != self.blank]
        score = float(sum(s.frame_probs) / len(s.frame_probs)) * 100.0 if s.frame_probs else 0
        text = "".join(self.vocab[i] for i in ids).replace("<space>", " ")
        return {"text": text, "score": score}

    def reset(self, session):
        self.group.reset(session)
        if self.beam is not None:
            self.beam.reset(session)
        if self.arena is not None:
            self.arena.reset(session)
        if self.memory is not None:
            self.memory.reset(session)
        self.sessions[session] = _Session()
