"""Drop-in for ``ppasr/predict.py`` (``PPASRPredictor``): ``predict`` (:163-187), ``predict_stream``
(:232-337), ``reset_stream`` (:340-347), ``decode`` (:114-140) with the same arguments and return
dicts, plus token timestamps (``predict(..., timestamps=True)``, ``align``: ``decoders/ctc_alignment.py``, no reference
counterpart).  Audio -> fbank is host-side glue (``data_utils/featurizer.py``); encoder + CTC decode run in
the HIP library.  VAD (`predict_long`), punctuation and ITN are separate models outside the hot
path and are not provided (``use_pun=True`` / ``is_itn=True`` raise).
"""
import numpy as np
import torch
import yaml

from ppasr_amd.data_utils.featurizer import AudioFeaturizer, TextFeaturizer, db_gain, load_audio, pcm_bytes_to_float
from ppasr_amd.decoders.ctc_greedy_decoder import greedy_decoder, greedy_decoder_chunk
from ppasr_amd.infer_utils.inference_predictor import InferencePredictor

__all__ = ["PPASRPredictor"]

FRAME_SHIFT = 0.010  # seconds per feature frame (the Kaldi fbank / MFCC hop)


class _Cfg(dict):
    """dict_to_object (utils/utils.py:45-56): nested attribute access."""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError as e:
            raise AttributeError(k) from e
        return _Cfg(v) if isinstance(v, dict) else v

    def __setattr__(self, k, v):
        self[k] = v


class PPASRPredictor:
    def __init__(self, configs=None, model_tag=None, model_path="models/conformer_streaming_fbank/infer/",
                 use_pun=False, pun_model_dir="models/pun_models/", use_gpu=True, state_dict=None, vocab_list=None,
                 warmup=True):
        if configs is None:
            raise Exception("configs (yaml path or dict) is required: model download is unavailable offline")
        if isinstance(configs, str):
            with open(configs, "r", encoding="utf-8") as f:
                configs = yaml.load(f.read(), Loader=yaml.FullLoader)
        if use_pun:
            raise NotImplementedError("punctuation model is outside the hot path (SURVEY.md §2 row 19)")
        self.configs = _Cfg(configs)
        self.running = False
        if vocab_list is not None:
            self._text_featurizer = TextFeaturizer(vocab_list=vocab_list)
        else:
            self._text_featurizer = TextFeaturizer(vocab_filepath=self.configs.dataset_conf.dataset_vocab)
        self._audio_featurizer = AudioFeaturizer(**self.configs.preprocess_conf)
        self.remained_wav = None
        self.cached_feat = None
        self.greedy_last_max_prob_list = None
        self.greedy_last_max_index_list = None
        # predict_stream(timestamps=True): audio fed so far, greedy's per-frame max probs, the beam's best ids and table
        self._stream_seconds, self._stream_maxprob, self._stream_ids = 0.0, None, []
        self._stream_arena, self._stream_overflow = None, False
        self.beam_search_decoder = None
        if self.configs.decoder == "attention_rescoring":
            if self.configs.use_model == "deepspeech2":
                raise ValueError("decoder: attention_rescoring needs a Conformer-family model (DeepSpeech2 has no "
                                 "attention decoder)")
            # WeNet's decode defaults with the shipped reverse_weight (configs/conformer.yml)
            self._rescoring_conf = dict(beam_size=10, ctc_weight=0.5, reverse_weight=0.3, cutoff_prob=0.99, cutoff_top_n=40)
            self._rescoring_conf.update(dict(self.configs.get("attention_rescoring_decoder_conf") or {}))
        if self.configs.decoder == "attention":
            if self.configs.use_model == "deepspeech2":
                raise ValueError("decoder: attention needs a Conformer-family model (DeepSpeech2 has no attention decoder)")
            # WeNet's decode defaults (maxlen = T'); ctc_weight > 0: CTC-joint scoring inside the search
            self._attention_conf = dict(beam_size=10, max_steps=None, ctc_weight=0.0)
            self._attention_conf.update(dict(self.configs.get("attention_decoder_conf") or {}))
        if self.configs.decoder == "ctc_beam_search":
            from ppasr_amd.decoders.beam_search_decoder import BeamSearchDecoder
            self.beam_search_decoder = BeamSearchDecoder(vocab_list=self._text_featurizer.vocab_list,
                                                         **self.configs.ctc_beam_search_decoder_conf)
        self.predictor = InferencePredictor(configs=self.configs, use_model=self.configs.use_model,
                                            streaming=self.configs.streaming, model_dir=model_path, use_gpu=use_gpu,
                                            state_dict=state_dict, vocab_size=self._text_featurizer.vocab_size)
        if warmup:  # predict.py:88-89
            self.predict(audio_data=np.random.uniform(low=-2.0, high=2.0, size=(134240,)).astype(np.float32))

    def decode(self, output_data, use_pun=False, is_itn=False):
        """predict.py:114-140"""
        if use_pun or is_itn:
            raise NotImplementedError("punctuation / ITN are outside the hot path")
        if self.configs.decoder == "ctc_beam_search":
            result = self.beam_search_decoder.decode_beam_search_offline(probs_split=output_data)
        else:
            result = greedy_decoder(probs_seq=output_data, vocabulary=self._text_featurizer.vocab_list)
        return result[0], result[1]

    def predict(self, audio_data, use_pun=False, is_itn=False, sample_rate=16000, timestamps=False):
        """-> {'text': str, 'score': float}.  predict.py:163-187
        ``timestamps=True`` adds ``'timestamps': [{'text', 'start', 'end', 'score'}, ...]``, one entry per token of the
        text: ``start`` / ``end`` in seconds on the encoder's frame grid (``_token_times``), ``score`` the largest
        probability of the token inside its span."""
        samples, sr = load_audio(audio_data, sample_rate)
        feat = self._audio_featurizer.featurize(samples, sr)
        input_data = np.asarray(feat, np.float32)[np.newaxis, :]
        audio_len = np.array([input_data.shape[1]]).astype(np.int64)
        if timestamps:
            if use_pun or is_itn:
                raise NotImplementedError("punctuation / ITN are outside the hot path")
            return self._predict_timestamps(input_data, audio_len, len(samples) / float(sr))
        if self.configs.decoder == "attention_rescoring":
            if use_pun or is_itn:
                raise NotImplementedError("punctuation / ITN are outside the hot path")
            from ppasr_amd.decoders.attention_rescoring import attention_rescoring
            probs, memory = self.predictor.predict_device_memory(input_data, audio_len)
            score, text = attention_rescoring(self.predictor.model, self.predictor.rescorer, probs, memory, None,
                                              self._text_featurizer.vocab_list, **self._rescoring_conf)[0]
            return {"text": text, "score": score}
        if self.configs.decoder == "attention":
            if use_pun or is_itn:
                raise NotImplementedError("punctuation / ITN are outside the hot path")
            from ppasr_amd.decoders.attention_decoder import attention_decode
            probs, memory = self.predictor.predict_device_memory(input_data, audio_len)
            score, text = attention_decode(self.predictor.model, self.predictor.rescorer, memory, None,
                                           self._text_featurizer.vocab_list, probs=probs, **self._attention_conf)[0]
            return {"text": text, "score": score}
        probs = self.predictor.predict_device(input_data, audio_len)[0]  # stays on the device
        score, text = self.decode(output_data=probs, use_pun=use_pun, is_itn=is_itn)
        return {"text": text, "score": score}

    # ---- token timestamps (CTC forced alignment on the device, decoders/ctc_alignment.py) ----
    def _blank(self):
        return self.beam_search_decoder.blank_id if self.beam_search_decoder is not None else 0

    def _token_times(self, probs, ids, duration):
        """The Viterbi alignment of ``ids`` through ``probs`` [T', V] (device) -> one {'text', 'start', 'end', 'score'} per
        token.  start = begin x m x frame shift, end = min(end x m x frame shift, duration), with m the model's total
        subsampling: the times lie on the encoder's frame grid, and the receptive-field offset of the convolutional front
        end is not corrected."""
        from ppasr_amd.decoders.ctc_alignment import align_one
        step = self.predictor.model.total_subsampling * FRAME_SHIFT
        vocab = self._text_featurizer.vocab_list
        greedy = self.configs.decoder == "ctc_greedy"  # (the only decoder whose text shows <space> as a blank character)
        return [{"text": vocab[i].replace("<space>", " ") if greedy else vocab[i], "start": b * step,
                 "end": min(e * step, duration), "score": c}
                for i, (b, e, c) in zip(ids, align_one(probs, ids, self._blank()))]

    def _predict_timestamps(self, input_data, audio_len, duration):
        """predict() with the winning hypothesis aligned against the same device-resident table: one more call and one
        more read-back than predict()."""
        vocab = self._text_featurizer.vocab_list
        if self.configs.decoder == "attention_rescoring":
            from ppasr_amd.decoders.attention_rescoring import attention_rescoring
            probs, memory = self.predictor.predict_device_memory(input_data, audio_len)
            score, text, ids = attention_rescoring(self.predictor.model, self.predictor.rescorer, probs, memory, None, vocab,
                                                   return_ids=True, **self._rescoring_conf)[0]
            probs = probs[0]
        elif self.configs.decoder == "attention":
            from ppasr_amd.decoders.attention_decoder import attention_decode
            probs, memory = self.predictor.predict_device_memory(input_data, audio_len)
            score, text, ids = attention_decode(self.predictor.model, self.predictor.rescorer, memory, None, vocab,
                                                return_ids=True, probs=probs, **self._attention_conf)[0]
            probs = probs[0]
        else:
            probs = self.predictor.predict_device(input_data, audio_len)[0]
            if self.configs.decoder == "ctc_beam_search":
                score, text, ids = self.beam_search_decoder.decode_beam_search_offline(probs_split=probs, return_ids=True)
            else:
                score, text, ids = greedy_decoder(probs_seq=probs, vocabulary=vocab, return_ids=True)
        return {"text": text, "score": score, "timestamps": self._token_times(probs, ids, duration)}

    def align(self, audio_data, text, sample_rate=16000):
        """Forced alignment of a transcript the caller supplies: the list ``predict(..., timestamps=True)`` returns under
        ``'timestamps'``, for ``text``.  ValueError for a character that is not in the vocabulary and for a transcript
        that does not fit into the utterance's frames."""
        from ppasr_amd.decoders.ctc_alignment import text_to_ids
        samples, sr = load_audio(audio_data, sample_rate)
        feat = self._audio_featurizer.featurize(samples, sr)
        input_data = np.asarray(feat, np.float32)[np.newaxis, :]
        audio_len = np.array([input_data.shape[1]]).astype(np.int64)
        ids = text_to_ids(text, self._text_featurizer.vocab_list, space_token=self.configs.decoder == "ctc_greedy")
        probs = self.predictor.predict_device(input_data, audio_len)[0]
        return self._token_times(probs, ids, len(samples) / float(sr))

    def score(self, audio_data, text, sample_rate=16000):
        """How likely is this transcript given this audio: ``{'ctc_nll', 'att_nll', 'tokens', 'frames'}`` with
        ``ctc_nll = -log P_ctc(text | audio)`` (``model_utils/loss.ctc_nll``) and ``att_nll`` the left attention decoder's
        ``-log P(text, eos | audio)`` (``AttentionRescorer.loss`` without smoothing; ``None`` when the predictor holds no
        decoder weights, i.e. was not configured with ``decoder: attention_rescoring`` or ``attention``).  The transcript is split as in
        ``align``.  ValueError for a character that is not in the vocabulary and for a transcript that does not fit into
        the utterance's frames."""
        from ppasr_amd.decoders.ctc_alignment import frames_needed, text_to_ids
        from ppasr_amd.model_utils.loss import STATUS_OK, ctc_nll
        samples, sr = load_audio(audio_data, sample_rate)
        feat = self._audio_featurizer.featurize(samples, sr)
        input_data = np.asarray(feat, np.float32)[np.newaxis, :]
        audio_len = np.array([input_data.shape[1]]).astype(np.int64)
        ids = text_to_ids(text, self._text_featurizer.vocab_list, space_token=self.configs.decoder == "ctc_greedy")
        rescorer = self.predictor.rescorer
        if rescorer is not None:
            probs, memory = self.predictor.predict_device_memory(input_data, audio_len)
        else:
            probs, memory = self.predictor.predict_device(input_data, audio_len), None
        T, need = int(probs.shape[1]), frames_needed(ids)
        if T < need:
            raise ValueError(f"score: the transcript does not fit: T = {T} frames, {need} needed "
                             f"({len(ids)} tokens, {need - len(ids)} repeats)")
        lab = np.asarray(ids, np.int32).reshape(1, len(ids))
        n = np.asarray([len(ids)], np.int32)
        c = ctc_nll(probs, lab, n, None, self._blank())
        pack = [c["nll"].to(torch.float64), c["status"].to(torch.float64)]
        if rescorer is not None:
            pack.append(rescorer.loss(memory, None, lab, n, 0.0, 0.0)["att_kl"])
        host = torch.cat(pack).cpu().numpy()  # (the read-back)
        if int(host[1]) != STATUS_OK:
            raise ValueError(f"score: the transcript cannot be scored (status {int(host[1])})")
        return {"ctc_nll": float(host[0]), "att_nll": float(host[2]) if rescorer is not None else None, "tokens": len(ids),
                "frames": T}

    def predict_long(self, audio_data, use_pun=False, is_itn=False, sample_rate=16000, speech_timestamps=None,
                     vad_predictor=None, timestamps=False):
        """predict.py:190-229: recognise the speech segments of a long recording one by one and join the texts with
        '，'; score = mean of the segment scores (2 decimals).  The reference finds the segments with its Silero VAD
        model (``init_vad``), which is a separate model outside this path: pass the segments as ``speech_timestamps``
        (``[{'start': sample, 'end': sample}, ...]``, what ``get_speech_timestamps`` returns) or an object with that
        method as ``vad_predictor``.  ``timestamps=True``: the segments' token timestamps (``predict``), each moved by its
        segment's start, in one list under ``'timestamps'``."""
        if use_pun:
            raise NotImplementedError("punctuation is a separate model outside the hot path")
        samples, sr = load_audio(audio_data, sample_rate)
        if speech_timestamps is None:
            if vad_predictor is None:
                raise NotImplementedError("predict_long needs speech_timestamps or a vad_predictor: the Silero VAD "
                                          "model is not part of this library")
            speech_timestamps = vad_predictor.get_speech_timestamps(samples, sr)
        texts, scores, stamps = "", [], []
        for t in speech_timestamps:
            if timestamps:
                result = self.predict(audio_data=samples[t["start"]:t["end"]], use_pun=False, is_itn=is_itn, sample_rate=sr,
                                      timestamps=True)
                at = t["start"] / float(sr)
                stamps += [dict(e, start=e["start"] + at, end=e["end"] + at) for e in result["timestamps"]]
            else:
                result = self.predict(audio_data=samples[t["start"]:t["end"]], use_pun=False, is_itn=is_itn, sample_rate=sr)
            score, text = result["score"], result["text"]
            if text != "":
                texts = texts + "，" + text
            scores.append(score)
        if texts[:1] == "，":
            texts = texts[1:]
        out = {"text": texts, "score": round(sum(scores) / len(scores), 2) if scores else 0}
        if timestamps:
            out["timestamps"] = stamps
        return out

    def predict_stream(self, audio_data, is_end=False, use_pun=False, is_itn=False, channels=1, samp_width=2,
                       sample_rate=16000, timestamps=False):
        """predict.py:232-337 (same windowing constants: 16 output frames per 67-frame window, stride 64,
        3 cached feature frames, required_cache_size = -16).
        ``timestamps=True`` (every call of the stream alike) adds ``'timestamps'``, the list ``predict(...,
        timestamps=True)`` returns, for the current text: beam search keeps the stream's probabilities in a one-session
        ``ProbArena`` and aligns against it, greedy reads its own frame lists.  None (with ``'table_overflow': True``)
        once the stream outgrows the arena, and for more than 255 tokens.  Not built for DeepSpeech2, whose chunk
        probabilities reach this method on the host."""
        if not self.configs.streaming:
            raise Exception(f"不支持改该模型流式识别，当前模型：{self.configs.use_model}")
        if self.configs.decoder in ("attention_rescoring", "attention"):
            raise NotImplementedError(f"decoder: {self.configs.decoder} scores whole utterances (it attends to the encoder "
                                      "output of every frame): use predict / predict_long, or ctc_greedy / "
                                      "ctc_beam_search for predict_stream")
        if timestamps and self.configs.use_model == "deepspeech2":
            raise NotImplementedError("predict_stream(timestamps=True) is not built for DeepSpeech2 (its chunk probabilities "
                                      "come back on the host): use serving.StreamPool(timestamps=True)")
        rate = sample_rate
        if isinstance(audio_data, np.ndarray):
            samples, rate = load_audio(audio_data, sample_rate)
        elif isinstance(audio_data, bytes):
            samples = pcm_bytes_to_float(audio_data, channels, samp_width)
        else:
            raise Exception(f"不支持该数据类型，当前数据类型为：{type(audio_data)}")
        self._stream_seconds += len(samples) / float(rate)
        self.remained_wav = samples if self.remained_wav is None else np.concatenate([self.remained_wav, samples])
        x_chunk = self._audio_featurizer.featurize(self.remained_wav, sample_rate)
        x_chunk = np.asarray(x_chunk, np.float32)[np.newaxis, :]
        self.cached_feat = x_chunk if self.cached_feat is None else np.concatenate([self.cached_feat, x_chunk], axis=1)
        # The reference's featurize() normalises the AudioSegment it is given IN PLACE (audio_featurizer.py:48-50 ->
        # audio.py:287-304, `self._samples *= gain`), and here that segment is the buffered `remained_wav`: the samples
        # that stay buffered for the next call are the GAINED ones, and they are gained again with the next chunk's
        # factor.  Reproduced (found by tests/golden/ref_wav.npz: without it 12 of 13 streaming texts of the reference's
        # own test.wav differed).
        if self._audio_featurizer.use_db_normalization and self.remained_wav.size:
            self.remained_wav = self.remained_wav * db_gain(self.remained_wav, self._audio_featurizer.target_db)
        # frames consumed x hop (10 ms) at the CALLER's sample rate (the reference's constant 160 is 10 ms at 16 kHz,
        # predict.py:275).  DIVERGENCE for streams that are not 16 kHz: the reference resamples its buffered AudioSegment in
        # place (audio_featurizer.py:46-47), so from the second call on it concatenates 16 kHz remainders with raw samples
        # of the caller's rate under the caller's rate label and drops 160 samples per frame of that mixture; here the
        # buffer stays at the caller's rate (featurize() resamples a copy) and the gain above is computed on the
        # un-resampled samples.  16 kHz streams -- the only ones the reference handles consistently -- are identical.
        self.remained_wav = self.remained_wav[int(round(sample_rate * 0.010)) * x_chunk.shape[1]:]

        decoding_chunk_size, context, subsampling = 16, 7, 4
        cached_feature_num = context - subsampling
        decoding_window = (decoding_chunk_size - 1) * subsampling + context
        stride = subsampling * decoding_chunk_size
        num_frames = self.cached_feat.shape[1]
        if num_frames < decoding_window and not is_end:
            return None
        if num_frames < context:
            return None
        left_frames = context if is_end else decoding_window
        score, text, end = None, None, None
        for cur in range(0, num_frames - left_frames + 1, stride):
            end = min(cur + decoding_window, num_frames)
            x = self.cached_feat[:, cur:end, :]
            if self.configs.use_model == "deepspeech2":
                probs_np, lens = self.predictor.predict_chunk_deepspeech(x_chunk=x)
                probs = torch.from_numpy(probs_np)
            else:
                required_cache_size = decoding_chunk_size * -1
                if self.predictor._stream is None:
                    raise NotImplementedError(f"streaming of {self.configs.use_model} is not built yet")
                probs = self.predictor._stream.encode_chunk(x, required_cache_size)  # device tensor [1,c,V]
                lens = np.array([probs.shape[1]])
            if self.configs.decoder == "ctc_beam_search":
                if timestamps:
                    self._stream_keep(probs)
                    score, text, self._stream_ids = self.beam_search_decoder.decode_chunk(probs=probs, logits_lens=lens,
                                                                                          return_ids=True)
                else:
                    score, text = self.beam_search_decoder.decode_chunk(probs=probs, logits_lens=lens)
            else:
                if timestamps and self._stream_maxprob is None:
                    self._stream_maxprob = []
                score, text, self.greedy_last_max_prob_list, self.greedy_last_max_index_list = greedy_decoder_chunk(
                    probs_seq=probs[0], vocabulary=self._text_featurizer.vocab_list,
                    last_max_index_list=self.greedy_last_max_index_list,
                    last_max_prob_list=self.greedy_last_max_prob_list,
                    frame_maxprob_list=self._stream_maxprob if timestamps else None)
        self.cached_feat = self.cached_feat[:, end - cached_feature_num:, :]
        if use_pun or is_itn:
            raise NotImplementedError("punctuation / ITN are outside the hot path")
        if timestamps:
            return self._stream_timestamps({"text": text, "score": score})
        return {"text": text, "score": score}

    # ---- token timestamps of a stream ----
    def _stream_keep(self, probs):
        """One chunk's probabilities [1, c, V] (device) go behind the stream's table: a one-session arena sized for the
        model's longest stream.  A stream that outgrows it loses its table until ``reset_stream``."""
        from ppasr_amd.decoders.ctc_alignment import ProbArena
        if self._stream_arena is None:
            frames = int(getattr(self.predictor.model, "max_len", 5000))
            self._stream_arena = ProbArena(1, int(probs.shape[2]), page_frames=16, n_pages=(frames + 15) // 16,
                                           device=probs.device)
        a = self._stream_arena
        if not self._stream_overflow and a.frames(0) + int(probs.shape[1]) > a.n_pages * a.page_frames:
            self._stream_overflow = True
            a.reset(0)
        if not self._stream_overflow:
            a.append([0], probs)

    def _stream_timestamps(self, result):
        from ppasr_amd.decoders.ctc_alignment import MAX_TOKENS, greedy_runs, token_entries
        step = self.predictor.model.total_subsampling * FRAME_SHIFT
        vocab = self._text_featurizer.vocab_list
        if self.configs.decoder == "ctc_beam_search":
            ids = self._stream_ids
            if self._stream_overflow or len(ids) > MAX_TOKENS:
                result["timestamps"] = None
                if self._stream_overflow:
                    result["table_overflow"] = True
                return result
            spans = self._stream_arena.align([0], [ids], self._blank())[0] if ids else []
            result["timestamps"] = token_entries(ids, spans, vocab, step, self._stream_seconds)
        else:
            ids, spans = greedy_runs(self.greedy_last_max_prob_list, self._stream_maxprob, 0)  # (the swapped naming: ids)
            result["timestamps"] = token_entries(ids, spans, vocab, step, self._stream_seconds, space_as_blank=True)
        return result

    def reset_stream(self):
        """predict.py:340-347"""
        self.predictor.reset_stream()
        self.remained_wav = None
        self.cached_feat = None
        self.greedy_last_max_prob_list = None
        self.greedy_last_max_index_list = None
        self._stream_seconds, self._stream_maxprob, self._stream_ids = 0.0, None, []
        self._stream_overflow = False
        if self._stream_arena is not None:
            self._stream_arena.reset(0)
        if self.configs.decoder == "ctc_beam_search" and self.beam_search_decoder is not None:
            self.beam_search_decoder.reset_decoder()
