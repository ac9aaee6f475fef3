"""Feature front-end that feeds the hot path: the host-side mirror of
``ppasr/data_utils/featurizer/audio_featurizer.py`` (dB normalisation -> int16 scale -> Kaldi fbank, dither 0 at
inference, :37-67,120-138) and ``text_featurizer.py`` (vocabulary file loader).

The arithmetic runs in ``csrc/fbank.hip`` behind ``ppasr_fbank_*`` (one workgroup per frame, frame resident in LDS
from the raw samples to the 80 log-mel values); this module only loads audio and moves buffers.  There is no CPU
path: without a HIP device ``featurize`` raises.  paddleaudio is not installable offline, so the front-end is
"parity unpinned" (checked against ``oracle/fbank_oracle.py``, a float64 restatement of Kaldi's algorithm).
``feature_method='mfcc'`` is the same kernel with one more stage (``ppasr_mfcc_create``: DCT-II over the mel axis and the
cepstral lifter, Kaldi's defaults); ``'linear'`` is not built.
Audio at another rate than the model's is resampled first: on the host by default (``resample``, scipy in float64), or with
``AudioFeaturizer(resample="device")`` by ``csrc/resample.hip`` behind ``ppasr_resample_*`` -- the same filter as a
polyphase kernel, for single waveforms, packed batches (``featurize_many(sample_rates=...)``) and streams
(``StreamResampler``), which all give the same bytes.
"""
import ctypes
import io
import wave

import numpy as np
import torch

__all__ = ["AudioFeaturizer", "StreamResampler", "TextFeaturizer", "load_audio", "db_gain"]



def load_audio(audio_data, sample_rate=16000):
    """-> (float32 samples in [-1,1] mono, sample_rate).  Accepts a .wav path, a binary file object,
    wav-file bytes or a numpy array (predict.py:143-160; only PCM wav is supported without soundfile)."""
    if isinstance(audio_data, np.ndarray):
        x = audio_data
        if x.dtype.kind == "i":
            x = x.astype(np.float32) / float(2 ** (8 * x.dtype.itemsize - 1))
        return x.astype(np.float32).reshape(-1) if x.ndim == 1 else x.astype(np.float32).mean(axis=1), sample_rate
    if isinstance(audio_data, (bytes, bytearray)):
        audio_data = io.BytesIO(audio_data)
    if isinstance(audio_data, str) or hasattr(audio_data, "read"):
        with wave.open(audio_data, "rb") as w:
            sr, ch, sw, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
            raw = w.readframes(n)
        return pcm_bytes_to_float(raw, ch, sw), sr
    raise Exception(f"unsupported audio_data type: {type(audio_data)}")


def resample(samples, sample_rate, target_sample_rate):
    """``AudioSegment.resample`` (data_utils/audio.py:306-317).  The reference calls ``resampy.resample(...,
    filter='kaiser_best')``; resampy is not installable offline, so this is scipy's polyphase resampler with a Kaiser
    window (``scipy.signal.resample_poly``): the same kind of band-limited interpolation, not bit-identical to resampy.
    Host code on the audio I/O side of the path."""
    if int(sample_rate) == int(target_sample_rate):
        return np.asarray(samples, np.float32)
    from math import gcd

    from scipy.signal import resample_poly
    g = gcd(int(sample_rate), int(target_sample_rate))
    up, down = int(target_sample_rate) // g, int(sample_rate) // g
    return resample_poly(np.asarray(samples, np.float64), up, down, window=("kaiser", 14.769656459379492)).astype(np.float32)


def db_gain(samples, target_db=-20.0):
    """Gain factor of ``AudioSegment.normalize(target_db)`` (data_utils/audio.py:287-304 -> rms_db :519-530 -> gain_db
    :256-264) with the scalar types numpy 1.x gives the reference there: the mean square and its log10 in float32, ``10 *
    log10``, ``target_db - rms_db`` and the power in float64, rounded to float32 when it scales the float32 samples (the
    arithmetic of csrc/fbank.hip, pinned by tests/golden/ref_wav.npz).  Host-side: ``predict_stream`` needs it because the
    reference normalises its buffered ``remained_wav`` IN PLACE (see ppasr_amd/predict.py)."""
    x = np.asarray(samples, np.float32)
    ms = np.mean(x ** 2) if x.size else np.float32(0.0)
    rms_db = 10.0 * float(np.log10(ms)) if ms != 0 else 0.0
    check_gain_db(float(target_db) - rms_db, target_db)
    return np.float32(10.0 ** ((float(target_db) - rms_db) / 20.0))


MAX_GAIN_DB = 300.0  # AudioSegment.normalize's max_gain_db default (data_utils/audio.py:287)
CEPSTRAL_LIFTER = 22.0  # paddleaudio.compliance.kaldi.mfcc's default, which audio_featurizer.py:109-115 leaves alone


def check_gain_db(gain, target_db):
    """``AudioSegment.normalize`` refuses a gain beyond max_gain_db (audio.py:301-303): same exception type and text."""
    if gain > MAX_GAIN_DB:
        raise ValueError(f"无法将段规范化到{target_db}dB，音频增益{gain}增益已经超过max_gain_db ({MAX_GAIN_DB}dB)")


def pcm_bytes_to_float(data, channels=1, samp_width=2):
    """AudioSegment.from_pcm_bytes (data_utils/audio.py:122-139)."""
    dt = {1: np.int8, 2: np.int16, 4: np.int32}[samp_width]
    x = np.frombuffer(data, dtype=dt).astype(np.float32) / float(2 ** (8 * samp_width - 1))
    if channels > 1:
        x = x.reshape(-1, channels).mean(axis=1)
    return x


class AudioFeaturizer:
    def __init__(self, feature_method="fbank", n_mels=80, n_mfcc=40, sample_rate=16000, use_dB_normalization=True,
                 target_dB=-20, train=False, device=None, resample="host", **_ignored):
        if feature_method == "linear":
            # 161 wide: beyond what any front end takes (input_dim <= 128), and a 320-point transform of un-quantised samples
            raise NotImplementedError("feature_method='linear' is not built: its 161-wide rows fit no encoder front end here "
                                      "(input_dim <= 128); use 'fbank' or 'mfcc'")
        if feature_method not in ("fbank", "mfcc"):
            raise NotImplementedError(f"feature_method={feature_method!r} is not built: 'fbank' and 'mfcc' are")
        if feature_method == "mfcc" and not 1 <= n_mfcc <= n_mels:  # paddleaudio.compliance.kaldi.mfcc asserts this
            raise AssertionError(f"n_mfcc must be in 1 .. n_mels: {n_mfcc} vs {n_mels}")
        if resample not in ("host", "device"):
            raise ValueError(f"resample={resample!r}: 'host' (scipy on the CPU, the default) or 'device' (csrc/resample.hip)")
        self._resample = resample
        self._resamplers = {}  # foreign rate -> (ppasr_resampler_handle, its geometry); resample="device" only
        self._feature_method = feature_method
        self._n_mels = n_mels
        self._n_mfcc = n_mfcc
        self._sr = sample_rate
        self._use_db = use_dB_normalization
        self._target_db = target_dB
        self._device = torch.device(device or "cuda:0")
        self._h = None
        self._ws = None
        self._scratch = {}  # featurize_many's staging buffers (pinned host, device, workspace)
        self._uploaded = self._queued = None  # events: its last upload has left the pinned buffer / its last call has run

    def _handle(self):
        if self._h is None:
            from ppasr_amd import _lib
            if not torch.cuda.is_available():
                raise _lib.PPASRHipError("no HIP device visible: the fbank front-end has no CPU fallback")
            self._lib = _lib.load()
            h = ctypes.c_void_p()
            with torch.cuda.device(self._device):
                if self._feature_method == "mfcc":
                    _lib.check(self._lib.ppasr_mfcc_create(self._sr, self._n_mels, self._n_mfcc, 25.0, 10.0, CEPSTRAL_LIFTER,
                                                           ctypes.byref(h)))
                else:
                    _lib.check(self._lib.ppasr_fbank_create(self._sr, self._n_mels, 25.0, 10.0, ctypes.byref(h)))
                assert self._lib.ppasr_fbank_feature_dim(h) == self.feature_dim
            self._h = h
        return self._h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.ppasr_fbank_destroy(h)
            self._h = None
        for r, _ in getattr(self, "_resamplers", {}).values():
            self._lib.ppasr_resampler_destroy(r)
        self._resamplers = {}

    @property
    def resample_mode(self):
        """'host' or 'device': where audio at another rate than the featurizer's is resampled"""
        return self._resample

    def _resampler(self, sample_rate):
        """-> (handle, rate) of the device resampler sample_rate -> the featurizer's rate, built on first use.  What the
        library refuses (max(up, down) > 1024, a rate <= 0) raises ``PPASRHipError``: there is no host fallback."""
        from ppasr_amd import _lib
        rate = int(sample_rate)
        if self._resample != "device":
            raise ValueError(f"audio at {rate} Hz for a featurizer at {self._sr} Hz: this call resamples on the device only, "
                             'construct the AudioFeaturizer with resample="device"')
        got = self._resamplers.get(rate)
        if got is None:
            self._handle()  # (the library, and the refusal without a device)
            r = ctypes.c_void_p()
            with torch.cuda.device(self._device):
                _lib.check(self._lib.ppasr_resampler_create(rate, int(self._sr), ctypes.byref(r)))
            got = self._resamplers[rate] = (r, rate)
        return got

    def _foreign(self, sample_rate):
        return sample_rate is not None and int(sample_rate) != int(self._sr)

    def resample_device(self, samples, sample_rate):
        """float32 mono samples at `sample_rate` (numpy or tensor) -> the same audio at the featurizer's rate, a float32
        DEVICE tensor of ceil(n up / down) samples: uploads the raw samples and resamples them there (``resample="device"``).
        Samples already at the featurizer's rate are only uploaded."""
        from ppasr_amd import _lib
        x = torch.as_tensor(samples, dtype=torch.float32).reshape(-1).to(self._device).contiguous()
        if not self._foreign(sample_rate):
            return x
        r, rate = self._resampler(sample_rate)
        n = int(x.numel())
        n_out = int(self._lib.ppasr_resampler_out_len(rate, int(self._sr), n))
        y = torch.empty(n_out, dtype=torch.float32, device=self._device)
        with torch.cuda.device(self._device):
            cur = torch.cuda.current_stream(self._device)
            _lib.check(self._lib.ppasr_resample_compute(r, x.data_ptr(), 0, n, y.data_ptr(), 0, n_out, cur.cuda_stream))
            x.record_stream(cur)  # `x` must outlive the kernel
        return y

    def _resample_windows(self, sample_rate, windows):
        """windows = [(held samples (numpy), absolute index of the first one, absolute index of the first output wanted,
        outputs wanted)] of any streams at `sample_rate` -> their outputs (numpy float32), by one packed upload, ONE batched
        launch (``ppasr_resample_compute_batch``) and one download."""
        from ppasr_amd import _lib
        r, rate = self._resampler(sample_rate)
        n = len(windows)
        outs_n = [int(w[3]) for w in windows]
        total_in, total_out = int(sum(w[0].size for w in windows)), int(sum(outs_n))
        if n == 0 or total_out == 0:
            return [np.zeros(0, np.float32) for _ in windows]
        seg_bytes = ctypes.sizeof(_lib.ResampleSegment) * n
        host = torch.empty(seg_bytes + 4 * total_in, dtype=torch.uint8, pin_memory=True)
        table = (_lib.ResampleSegment * n).from_address(host.data_ptr())
        packed = host[seg_bytes:].view(torch.float32).numpy()
        off_in = off_out = 0
        for b, (x, in_first, out_first, n_out) in enumerate(windows):
            packed[off_in:off_in + x.size] = x
            table[b] = _lib.ResampleSegment(off_in, int(in_first), int(x.size), off_out, int(out_first), int(n_out))
            off_in += x.size
            off_out += int(n_out)
        with torch.cuda.device(self._device):
            cur = torch.cuda.current_stream(self._device)
            dev = host.to(self._device, non_blocking=True)
            y = torch.empty(total_out, dtype=torch.float32, device=self._device)
            _lib.check(self._lib.ppasr_resample_compute_batch(r, dev.data_ptr() + seg_bytes, dev.data_ptr(), n, max(outs_n),
                                                              y.data_ptr(), cur.cuda_stream))
            y = y.cpu().numpy()  # (synchronises: the pinned buffer and `dev` are free again)
        return [y[o - k:o] for o, k in zip(np.cumsum(outs_n).tolist(), outs_n)]

    @property
    def feature_dim(self):
        """audio_featurizer.py:140-154: the width of a feature row, the model's ``input_dim``"""
        return self._n_mfcc if self._feature_method == "mfcc" else self._n_mels

    @property
    def use_db_normalization(self):
        return bool(self._use_db)

    @property
    def target_db(self):
        return self._target_db

    def featurize_device(self, samples, sample_rate=None):
        """float32 mono samples in [-1, 1] (numpy or tensor) -> fbank [T, n_mels] (mfcc: [T, n_mfcc]) float32 DEVICE tensor."""
        from ppasr_amd import _lib
        sr = sample_rate or self._sr
        if sr != self._sr and self._resample == "device":  # the same step on the device: no host round trip
            samples = self.resample_device(samples, sr)
        elif sr != self._sr:  # audio_featurizer.py:46-47: up / down-sample to the model's rate first (host side)
            samples = resample(np.asarray(torch.as_tensor(samples).cpu(), np.float32).reshape(-1), sr, self._sr)
        h = self._handle()
        x = torch.as_tensor(samples, dtype=torch.float32).reshape(-1).to(self._device).contiguous()
        n = int(x.numel())
        frames = int(self._lib.ppasr_fbank_frames(h, n))
        feats = torch.empty(frames, self.feature_dim, dtype=torch.float32, device=self._device)
        if frames == 0:
            return feats
        need = int(self._lib.ppasr_fbank_workspace_bytes(h, n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self._device)
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _lib.check(self._lib.ppasr_fbank_compute(h, x.data_ptr(), n, int(bool(self._use_db)), float(self._target_db),
                                                     feats.data_ptr(), self._ws.data_ptr(), self._ws.numel(), stream))
            torch.cuda.current_stream(self._device).synchronize()  # `x` must outlive the kernel
        if self._use_db:  # the workspace's tail: [.. chunk sums .., gain, gain in dB] (csrc/fbank.hip k_gain)
            chunks = (n + 8191) // 8192
            self.last_gain, gain_db = (float(v) for v in self._ws[4 * chunks:4 * chunks + 8].view(torch.float32).cpu())
            check_gain_db(gain_db, self._target_db)
        return feats

    def featurize(self, samples, sample_rate=None):
        """float32 mono samples -> fbank [T, n_mels] (mfcc: [T, n_mfcc]) float32 (numpy), the reference's return type."""
        return self.featurize_device(samples, sample_rate).cpu().numpy()

    def _stage(self, key, nbytes, pinned=False):
        """Staging buffers of ``featurize_many``: owned by the featurizer, grow only."""
        t = self._scratch.get(key)
        if t is None or t.numel() < nbytes:
            t = (torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) if pinned
                 else torch.empty(nbytes, dtype=torch.uint8, device=self._device))
            self._scratch[key] = t
        return t

    def featurize_many(self, waveforms, padded=False, sample_rates=None):
        """A list of float32 mono waveforms (numpy or tensor) -> their fbank features on the
        device, by ONE packed upload and ONE set of launches (``ppasr_fbank_compute_batch``: three with dB normalisation,
        one without, whatever the number of waveforms).  Every waveform's rows equal ``featurize_device`` on it alone,
        byte for byte.
          padded=False: (feats [sum of frames, n_mels], frame_counts [B] int64 numpy) -- waveform b's rows follow b - 1's;
          padded=True:  (feats [B, Tmax, n_mels], lens [B] int64 tensor) -- what ``get_encoder_out`` takes; the rows
                        past a waveform's frames are zero.
        A waveform shorter than one window has no frame.  ``self.last_gains`` holds the gains ([B] float32) afterwards
        when dB normalisation is on.  (``feature_method='mfcc'``: read n_mfcc for n_mels.)
        sample_rates: None = every waveform is at the featurizer's rate; one rate for all, or one per waveform.  A foreign
        rate needs ``resample="device"`` (ValueError otherwise): the raw samples go up in the same packed upload and ONE
        batched resample launch per distinct foreign rate writes the model-rate samples into the buffer the fbank launches
        read.  With no foreign rate the call runs what it runs without the argument."""
        from ppasr_amd import _lib
        wavs = [np.asarray(w.cpu() if isinstance(w, torch.Tensor) else w, np.float32).reshape(-1) for w in waveforms]
        n = len(wavs)
        if sample_rates is None or np.ndim(sample_rates) == 0:
            rates = [int(sample_rates or self._sr)] * n
        else:
            rates = [int(r or self._sr) for r in sample_rates]
            if len(rates) != n:
                raise ValueError(f"featurize_many: {len(rates)} sample rates for {n} waveforms")
        foreign = [b for b in range(n) if rates[b] != int(self._sr)]
        if foreign and self._resample != "device":
            raise ValueError(f"featurize_many: waveforms at {sorted({rates[b] for b in foreign})} Hz for a featurizer at "
                             f'{self._sr} Hz need AudioFeaturizer(resample="device")')
        h = self._handle()
        lib, dev = self._lib, self._device
        by_rate = {}  # foreign rate -> its waveforms, in order
        for b in foreign:
            by_rate.setdefault(rates[b], []).append(b)
        resamplers = {rate: self._resampler(rate)[0] for rate in by_rate}  # (refusals before anything is staged)
        # samples at the featurizer's rate: a foreign waveform's are made on the device, behind the uploaded ones
        sizes = [int(w.size) for w in wavs]
        for b in foreign:
            sizes[b] = int(lib.ppasr_resampler_out_len(rates[b], int(self._sr), int(wavs[b].size)))
        counts = (ctypes.c_int * max(n, 1))(*sizes)
        win, shift = int(self._sr * 0.001 * 25.0), int(self._sr * 0.001 * 10.0)
        frames = np.array([0 if k < win else 1 + (k - win) // shift for k in sizes], np.int64)
        t_max = max(int(frames.max()) if n else 0, 1) if padded else 0
        total = int(sum(w.size for w in wavs))                 # uploaded samples
        made = int(sum(sizes[b] for b in foreign))             # samples the resampler writes behind them
        seg_bytes = ctypes.sizeof(_lib.FbankSegment) * n + ctypes.sizeof(_lib.ResampleSegment) * len(foreign)
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            # the pinned buffer: not before the upload that may still read it has finished
            if self._uploaded is not None:
                self._uploaded.synchronize()
            host = self._stage("host", seg_bytes + 4 * total + 4, pinned=True)
            chunks, n_frames = ctypes.c_int(0), ctypes.c_int(0)
            _lib.check(lib.ppasr_fbank_plan_batch(self._sr, 25.0, 10.0, ctypes.addressof(counts), n, t_max, host.data_ptr(),
                                                  ctypes.byref(chunks), ctypes.byref(n_frames)))
            chunks, n_frames = chunks.value, n_frames.value
            assert n_frames == int(frames.sum())
            packed = host[seg_bytes:seg_bytes + 4 * total].view(torch.float32).numpy()
            off, raw_at = 0, []
            for w in wavs:
                packed[off:off + w.size] = w
                raw_at.append(off)
                off += w.size
            if foreign:
                # the fbank table's segments: where each waveform's model-rate samples are -- its uploaded samples, or
                # its slot in the resampled region [total, total + made)
                fb = (_lib.FbankSegment * n).from_address(host.data_ptr())
                rs = (_lib.ResampleSegment * len(foreign)).from_address(host.data_ptr() + ctypes.sizeof(_lib.FbankSegment) * n)
                at, k, launches = total, 0, []
                for b in range(n):
                    fb[b].first_sample = raw_at[b]
                for rate, members in by_rate.items():
                    launches.append((rate, k, len(members), max(sizes[b] for b in members)))
                    for b in members:
                        fb[b].first_sample = at
                        rs[k] = _lib.ResampleSegment(raw_at[b], 0, int(wavs[b].size), at, 0, sizes[b])
                        at += sizes[b]
                        k += 1
            # the device buffers: a call queued on another stream may still read them
            if self._queued is not None:
                cur.wait_event(self._queued)
            stage = self._stage("stage", seg_bytes + 4 * (total + made) + 4)
            stage[:seg_bytes + 4 * total].copy_(host[:seg_bytes + 4 * total], non_blocking=True)
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(cur)
            samples_dev = stage.data_ptr() + seg_bytes
            if foreign:
                rs_dev = stage.data_ptr() + ctypes.sizeof(_lib.FbankSegment) * n
                for rate, k, count, longest in launches:
                    _lib.check(lib.ppasr_resample_compute_batch(resamplers[rate], samples_dev,
                                                                rs_dev + ctypes.sizeof(_lib.ResampleSegment) * k, count,
                                                                longest, samples_dev, cur.cuda_stream))
            ws = self._stage("ws", int(lib.ppasr_fbank_batch_workspace_bytes(n, chunks)))
            feats = (torch.empty(n, t_max, self.feature_dim, dtype=torch.float32, device=dev) if padded
                     else torch.empty(n_frames, self.feature_dim, dtype=torch.float32, device=dev))
            if padded:
                feats.zero_()  # the padding rows; the kernel writes the others
            if n:
                _lib.check(lib.ppasr_fbank_compute_batch(h, samples_dev, stage.data_ptr(), n, chunks,
                                                         n_frames, int(bool(self._use_db)), float(self._target_db),
                                                         feats.data_ptr() if feats.numel() else ws.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), cur.cuda_stream))
            self._queued = torch.cuda.Event()
            self._queued.record(cur)
            if self._use_db:  # the workspace's tail: {gain, gain in dB} per waveform
                gains = ws[4 * chunks:4 * chunks + 8 * n].view(torch.float32).cpu().numpy().reshape(n, 2)
                for b in range(n):
                    if frames[b] > 0:  # (as featurize: a waveform without a frame is not normalised)
                        check_gain_db(float(gains[b, 1]), self._target_db)
                self.last_gains = gains[:, 0].copy()
        return (feats, torch.from_numpy(frames)) if padded else (feats, frames)


class StreamResampler:
    """One stream at `sample_rate`, packet by packet -> the same stream at the featurizer's rate, on the device resampler
    (``AudioFeaturizer(resample="device")``).  The kernel is stateless and addressed by absolute stream position; this class
    keeps, on the host, the raw tail the coming outputs still read and the two absolute counters.  Everything ``push``
    returns followed by what ``flush`` returns equals ``resample_device`` of all the samples pushed, byte for byte,
    wherever the packets were cut."""

    def __init__(self, featurizer, sample_rate):
        self._f = featurizer
        self._rate = int(sample_rate)
        featurizer._resampler(self._rate)  # (ValueError without resample="device"; the library's refusals)
        self._lib = featurizer._lib
        self._tail = np.zeros(0, np.float32)  # raw samples tail_first .. n_in - 1
        self._tail_first = 0
        self._n_in = 0    # raw samples pushed so far
        self._n_out = 0   # outputs handed out so far
        self._flushed = False

    @property
    def sample_rate(self):
        return self._rate

    def _prepare(self, samples, flush=False):
        """-> (the window a launch needs: (held samples, their first absolute index, first output, outputs), the state
        after it).  Changes nothing: ``_commit`` takes the state once the outputs exist."""
        if self._flushed:
            raise ValueError("StreamResampler: the stream was flushed; make a new one for new audio")
        x = np.asarray(samples, np.float32).reshape(-1)
        held = np.concatenate([self._tail, x]) if x.size else self._tail
        n_in = self._n_in + int(x.size)
        fr = int(self._f._sr)
        done = int((self._lib.ppasr_resampler_out_len if flush else self._lib.ppasr_resampler_ready)(self._rate, fr, n_in))
        assert done >= self._n_out
        keep = min(int(self._lib.ppasr_resampler_first_needed(self._rate, fr, done)), n_in)  # the next output's first sample
        keep = max(keep, self._tail_first)
        state = (held[keep - self._tail_first:], keep, n_in, done, flush)
        return (held, self._tail_first, self._n_out, done - self._n_out), state

    def _commit(self, state):
        self._tail, self._tail_first, self._n_in, self._n_out, self._flushed = state

    def push(self, samples):
        """raw samples -> the model-rate samples that are complete now (numpy float32; possibly none)"""
        window, state = self._prepare(samples)
        out = self._f._resample_windows(self._rate, [window])[0]
        self._commit(state)
        return out

    def flush(self):
        """End of the stream: the remaining outputs up to ceil(n up / down) of everything pushed, with zeros for the samples
        that never came.  The stream takes no more audio afterwards."""
        if self._flushed:
            return np.zeros(0, np.float32)
        window, state = self._prepare(np.zeros(0, np.float32), flush=True)
        out = self._f._resample_windows(self._rate, [window])[0]
        self._commit(state)
        return out


class TextFeaturizer:
    """Vocabulary loader (text_featurizer.py:8-59): one token per line, optional tab-separated count."""

    def __init__(self, vocab_filepath=None, vocab_list=None):
        if vocab_list is None:
            with open(vocab_filepath, "r", encoding="utf-8") as f:
                vocab_list = [line.split("\t")[0].replace("\n", "") for line in f.readlines()]
        self._vocab_list = list(vocab_list)
        self._vocab_dict = {t: i for i, t in enumerate(self._vocab_list)}
        self.unk = "<unk>"

    @property
    def vocab_size(self):
        return len(self._vocab_list)

    @property
    def vocab_list(self):
        return self._vocab_list

    def featurize(self, text):
        ids = []
        for tok in list(text.strip()):
            tok = "<space>" if tok == " " else tok
            ids.append(self._vocab_dict.get(tok, self._vocab_dict.get(self.unk, 0)))
        return ids
