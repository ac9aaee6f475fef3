"""Where foreign-rate audio is resampled: host (scipy, float64, one waveform at a time -- the default) against device
(``AudioFeaturizer(resample="device")``, csrc/resample.hip).  One JSON line per section; run on one otherwise idle MI355X:

    python tools/bench_resample.py [--reps R] [--warmup W]

  featurize_many  32 waveforms of 10 s at 8 kHz and at 48 kHz -> features on the device.
                  host:   ``resample`` per waveform, then ``featurize_many`` (what the code does without the option);
                  device: ``featurize_many(sample_rates=rate)``.
                  The two variants take turns in one process, W warm-up calls first; a host clock around work that ends in a
                  device synchronise; median and 10th / 90th percentile over R calls.  Reported apart: the host resampling
                  alone, the bytes each route uploads and the time of a pinned upload of that many bytes, and the kernels'
                  own time (dispatch-attached events, ``_lib.kernel_profile``) split into resample and fbank launches.
  pool            one round of 64 sessions, a 0.64 s packet at 8 kHz each: ``feed_many(sample_rate=8000)`` against 64 x
                  ``feed(sample_rate=8000)`` (both on the device resampler; a pool has no host route), front stage only
                  (packets -> cached features; ``step`` runs outside the clock)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppasr_amd import _lib  # noqa: E402
from ppasr_amd.data_utils.featurizer import AudioFeaturizer, resample  # noqa: E402


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "p10_p90_ms": [round(float(np.percentile(ms, q)), 3) for q in (10, 90)]}


def _waves(n, seconds, rate, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(int(seconds * rate)) / float(rate)
    x = 0.1 * np.sin(2 * np.pi * (150 + 3 * np.arange(n))[:, None] * t) + 0.03 * rng.standard_normal((n, t.size))
    return [w for w in x.astype(np.float32)]


def _upload_ms(nbytes, reps):
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    ms = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dev.copy_(host, non_blocking=True)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms[2:]


def featurize_many_section(rate, reps, warmup, n=32, seconds=10.0):
    waves = _waves(n, seconds, rate, seed=rate)
    fh, fd = AudioFeaturizer(resample="host"), AudioFeaturizer(resample="device")
    t_host, t_host_resample, t_dev = [], [], []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model_rate = [resample(w, rate, 16000) for w in waves]
        t1 = time.perf_counter()
        a, _ = fh.featurize_many(model_rate)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        b, _ = fd.featurize_many(waves, sample_rates=rate)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if r >= warmup:
            t_host.append((t2 - t0) * 1e3)
            t_host_resample.append((t1 - t0) * 1e3)
            t_dev.append((t3 - t2) * 1e3)
    with _lib.kernel_profile() as kp:
        fd.featurize_many(waves, sample_rates=rate)
        torch.cuda.synchronize()
    k_rs = sum(ms for k, (ms, _) in kp.kernels.items() if "resample" in k)
    k_fb = sum(ms for k, (ms, _) in kp.kernels.items() if "resample" not in k)
    up_host, up_dev = 4 * sum(w.size for w in model_rate), 4 * sum(w.size for w in waves)
    out = {"section": "featurize_many", "rate": rate, "waveforms": n, "seconds_each": seconds, "reps": reps,
           "host": _stats(t_host), "host_resample_alone": _stats(t_host_resample), "device": _stats(t_dev),
           "ratio_host_over_device": round(float(np.median(t_host) / np.median(t_dev)), 2),
           "upload_bytes": {"host": up_host, "device": up_dev},
           "upload_alone": {"host": _stats(_upload_ms(up_host, reps)), "device": _stats(_upload_ms(up_dev, reps))},
           "device_kernels_ms": {"resample": round(k_rs, 3), "fbank": round(k_fb, 3),
                                 "launches": int(sum(c for _, c in kp.kernels.values()))},
           "max_abs_feature_difference": round(float((a - b).abs().max()), 5)}
    print(json.dumps(out), flush=True)


def pool_section(reps, warmup, n=64, packet=5120, rate=8000):
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    from ppasr_amd.serving import StreamPool
    from ppasr_amd.utils.synth import conformer_state_dict, synth_vocabulary
    V = 97
    model = ConformerModel(80, V, streaming=True, device="cuda:0",
                           encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=1,
                                             cnn_module_kernel=15),
                           state_dict=conformer_state_dict(vocab_size=V, num_blocks=1, seed=3))
    total = warmup + reps
    audio = _waves(n, 4 * packet / rate, rate, seed=64)
    conf = dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True, target_dB=-20,
                resample="device")
    pools = {k: StreamPool(model, synth_vocabulary(V), n_sessions=n, preprocess_conf=conf,
                           max_seconds=packet / rate * total + 2.0) for k in ("feed", "feed_many")}
    front = {k: [] for k in pools}
    for r in range(total):
        lo = (r % 4) * packet
        packets = {i: audio[i][lo:lo + packet] for i in range(n)}
        for k, pool in pools.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "feed":
                for i, p in packets.items():
                    pool.feed(i, p, sample_rate=rate)
            else:
                pool.feed_many(packets, sample_rate=rate)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            pool.step()
            if r >= warmup:
                front[k].append((t1 - t0) * 1e3)
    same = all(a.frame_ids == b.frame_ids for a, b in zip(pools["feed"].sessions, pools["feed_many"].sessions))
    out = {"section": "pool_front", "sessions": n, "packet_s": packet / rate, "rate": rate, "reps": reps,
           "feed": _stats(front["feed"]), "feed_many": _stats(front["feed_many"]), "same_frame_ids": bool(same),
           "ratio_feed_over_feed_many": round(float(np.median(front["feed"]) / np.median(front["feed_many"])), 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    reps, warmup = _arg("--reps", 10), _arg("--warmup", 3)
    for rate in (8000, 48000):
        featurize_many_section(rate, reps, warmup)
    pool_section(reps, warmup)
