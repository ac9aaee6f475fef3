"""The batched audio front stage in its two forms, fbank and MFCC, on the same packets in one process.

    python tools/bench_front_forms.py [--sessions 256] [--packet 10240] [--rounds 30] [--warmup 5]

N packets of `--packet` samples go through ``AudioFeaturizer.featurize_many`` (one packed upload, three launches) with
``feature_method='fbank'`` and with ``'mfcc'`` (80 mel bins, 40 coefficients), the two forms taking each round in turn.  Two
figures per form: a host clock around the call up to a device synchronise (what a serving round pays), and HIP events
around the call (upload + launches on the device); then, in a pass of its own, each kernel's own time from
dispatch-attached events.  Prints one JSON line: median [10th, 90th percentile] in ms."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppasr_amd.data_utils.featurizer import AudioFeaturizer  # noqa: E402


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    n, packet, rounds, warmup = _arg("--sessions", 256), _arg("--packet", 10240), _arg("--rounds", 30), _arg("--warmup", 5)
    rng = np.random.Generator(np.random.PCG64(0))
    wavs = [(0.1 * rng.standard_normal(packet)).astype(np.float32) for _ in range(n)]
    forms = {m: AudioFeaturizer(feature_method=m, n_mels=80, n_mfcc=40, sample_rate=16000) for m in ("fbank", "mfcc")}
    host, dev = {m: [] for m in forms}, {m: [] for m in forms}
    for r in range(warmup + rounds):
        for m, f in forms.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            f.featurize_many(wavs)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= warmup:
                host[m].append((t1 - t0) * 1e3)
                dev[m].append(e0.elapsed_time(e1))

    # the frame kernel's own time: dispatch-attached events (ppasr_kprof_*), in a pass of its own
    from ppasr_amd._lib import kernel_profile
    kern = {}
    for m, f in forms.items():
        with kernel_profile() as kp:
            for _ in range(10):
                f.featurize_many(wavs)
            torch.cuda.synchronize()
        kern[m] = {k: round(ms / c, 4) for k, (ms, c) in kp.kernels.items()}

    def stat(v):
        return [round(float(np.median(v)), 3)] + [round(float(np.percentile(v, q)), 3) for q in (10, 90)]

    print(json.dumps({"section": "front_forms", "sessions": n, "packet_s": packet / 16000.0, "rounds": rounds,
                      **{m: {"host_ms_median_p10_p90": stat(host[m]), "device_ms_median_p10_p90": stat(dev[m]),
                             "kernel_ms_mean_of_10": kern[m]} for m in forms}}))


if __name__ == "__main__":
    main()
