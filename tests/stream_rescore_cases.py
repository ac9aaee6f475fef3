"""Shared cases of the streaming attention-rescoring tests (a plain module): one small Conformer checkpoint with decoder
weights, the feature streams of five sessions cut into predict_stream's windows, and their float64 encoder output.

Sessions, fed at the group level (67-frame windows, stride 64, then the last shorter window when >= 7 frames are left):
  A 131 frames: two full windows, 32 memory frames
  B 161 frames: its last window of 33 frames gives c = 7 -- odd, not a multiple of the 4 rows a workgroup takes
  C  76 frames: its last window of 12 frames gives c = 2
  D  71 frames: its last window of exactly 7 frames gives c = 1
  E  A's features again; the first round lists it in the middle of the list with mem_frames = 0, so it keeps round 2 only
"""
import numpy as np
import torch

import decoder_cases as dc
from numerics import oracle64
from ppasr_amd.utils.synth import conformer_state_dict, synth_features

V, UNITS, BLOCKS = 67, 256, (1, 1)
ENC = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
DEC = dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0], r_num_blocks=BLOCKS[1])
WINDOW, STRIDE, CONTEXT = 67, 64, 7
FRAMES = dict(A=131, B=161, C=76, D=71)
SLOT = dict(A=0, B=1, C=2, D=3, E=4)
PAGE_FRAMES = (5, 1, 64)


def checkpoint(seed=3, dec_seed=77):
    sd = conformer_state_dict(vocab_size=V, num_blocks=2, seed=seed)
    sd.update(dc.decoder_state_dict(dec_seed, V, UNITS, *BLOCKS))
    return sd


def features():
    """name -> [1, frames, 80] float32"""
    out = {}
    for k, (name, n) in enumerate(FRAMES.items()):
        x, _ = synth_features(1, n, lens=[n], seed=21 + k)
        out[name] = np.asarray(x, np.float32)
    out["E"] = out["A"]
    return out


def windows(x):
    """the windows predict_stream cuts from a whole stream [1, n, F]"""
    n, cur, out = x.shape[1], 0, []
    while n - cur >= WINDOW:
        out.append(x[:, cur:cur + WINDOW])
        cur += STRIDE
    if n - cur >= CONTEXT:
        out.append(x[:, cur:])
    return out


def rounds(feats):
    """[(names, window index, mem_frames or None)]: the group rounds of the five sessions, in order"""
    return [(["A", "E", "B", "C", "D"], 0, [16, 0, 16, 16, 16]),
            (["A", "E", "B"], 1, None),
            (["B"], 2, None), (["C"], 1, None), (["D"], 1, None)]


def oracle_memory(sd, feats):
    """name -> float64 encoder output [frames, 256] of the whole stream, chunk by chunk through forward_chunk"""
    oracle = oracle64("conformer", sd, num_blocks=2)
    out = {}
    with torch.no_grad():
        for name in FRAMES:
            att = cnn = None
            off, rows = 0, []
            for w in windows(feats[name]):
                xs, att, cnn = oracle.forward_chunk(w, off, -1, att, cnn)
                off += xs.shape[1]
                rows.append(xs[0].numpy())
            out[name] = np.concatenate(rows, 0)
    out["E"] = out["A"][16:]
    return out


def audio(seconds, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(int(16000 * seconds)) / 16000.0
    x = 0.1 * np.sin(2 * np.pi * 220 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(t.shape)
    return x.astype(np.float32)
