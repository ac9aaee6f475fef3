"""The fp32 budget still catches front-end bugs at the edge widths (no GPU: the oracles on the CPU), the approach of
tests/test_numerics_budget_cpu.py applied to the 4x front end at F = 7 (F1 = 3, F2 = 1: one embed K chunk) and F = 128
(F1 = 63, F2 = 31: an embed contraction 1.6x longer than the 80-bin one the budget was measured on):
- the floor: the fp32 oracle against the float64 oracle stays below a tenth of F32_BUDGET;
- each of a few realistic front-end index bugs moves the float64 output by at least 5x F32_BUDGET, so a kernel with that
  bug fails tests/test_front_widths_gpu.py.
Mutations change a state-dict entry or patch a method on one oracle instance; the oracle sources stay as they are."""
import functools
import math
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import numerics as nm
from ppasr_amd.utils.synth import conformer_state_dict, synth_features

WIDTHS = [7, 128]
LENS = [131, 90, 23]
MARGIN = 5.0


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"\n[widths] {__name__}: {time.time() - t0:.1f} s wall")


@functools.lru_cache(maxsize=None)
def _sd(F):
    return conformer_state_dict(input_dim=F, vocab_size=97, num_blocks=1, seed=900 + F, perturb_norm=True)


@functools.lru_cache(maxsize=None)
def _inputs(F):
    return synth_features(len(LENS), max(LENS), n_mels=F, lens=LENS, seed=F)


def _oracle(F, dtype=torch.float64, sd=None):
    from oracle.conformer_oracle import ConformerOracle
    return ConformerOracle(_sd(F) if sd is None else sd, num_blocks=1, dtype=dtype)


def _logits(oracle, F):
    x, lens = _inputs(F)
    with torch.no_grad():
        return oracle.get_encoder_out(x, lens, return_logits=True)[1]


@functools.lru_cache(maxsize=None)
def _ref64(F):
    return _logits(_oracle(F), F)


def _err(F, out):
    ref = _ref64(F)
    lens_out = [min(ref.shape[1], (n + 3) // 4) for n in LENS]
    return max(nm.utt_rel(out, ref, lens_out),
               nm.logprob_err(torch.softmax(out.to(torch.float64), -1), ref, lens_out))


@pytest.mark.parametrize("F", WIDTHS)
def test_fp32_oracle_floor(F):
    e = _err(F, _logits(_oracle(F, torch.float32), F))
    print(f"[widths] F={F}: fp32 oracle vs float64 {e:.2e} (budget / 10 = {nm.F32_BUDGET / 10:.1e})")
    assert e < nm.F32_BUDGET / 10, e


def _embed4(o, x, offset, x_shift=0, y1_shift=0):
    """Conv2dSubsampling4 + RelPositionalEncoding of the oracle (conformer_oracle._embed, 4x case), with conv1 reading bin
    2 * f1 + j + x_shift and conv2 reading conv1 column 2 * f2 + j + y1_shift (out-of-range columns read zero)"""
    def shift(t, s):
        return torch.cat([t[..., s:], torch.zeros_like(t[..., :s])], -1) if s else t
    x = shift(x, x_shift).unsqueeze(1)
    y1 = F_.relu(F_.conv2d(x, o.p["encoder.embed.conv.0.weight"], o.p["encoder.embed.conv.0.bias"], stride=2))
    y2 = F_.relu(F_.conv2d(shift(y1, y1_shift), o.p["encoder.embed.conv.2.weight"], o.p["encoder.embed.conv.2.bias"],
                           stride=2))
    b, c, t, f = y2.shape
    out = o._linear(y2.permute(0, 2, 1, 3).reshape(b, t, c * f), "encoder.embed.out.0")
    return out * math.sqrt(o.d), o.pe[:, offset:offset + t]


def _mutant(F, name):
    if name in ("embed_drops_last_f2", "embed_chunk_added_twice"):
        sd = dict(_sd(F))
        w = np.array(sd["encoder.embed.out.0.weight"], copy=True)
        d = w.shape[1]
        if name == "embed_drops_last_f2":
            # the last f2 block of the embed input (K index c * F2 + F2 - 1) dropped
            w.reshape(256, -1, d)[:, -1, :] = 0.0
        else:
            # the embed's only K chunk (F2 = 1: K = 256) summed by two of the K slices, e.g. a slice that owns no chunk
            # taking its neighbour's
            w *= 2.0
        sd["encoder.embed.out.0.weight"] = w
        return _oracle(F, sd=sd)
    o = _oracle(F)
    if name == "conv1_reads_next_bin":
        o._embed = lambda x, offset: _embed4(o, x, offset, x_shift=1)
    elif name == "conv2_window_off_by_one":
        o._embed = lambda x, offset: _embed4(o, x, offset, y1_shift=1)
    elif name == "cmvn_skips_last_read_bin":
        # the last bin conv1 reads (2 * F1: at F = 128 bin 127 is never read) left un-normalised
        last = 2 * ((F - 1) // 2)
        cmvn = o._cmvn

        def skip(x):
            y = cmvn(x)
            y[..., last] = torch.as_tensor(x, dtype=y.dtype)[..., last]
            return y
        o._cmvn = skip
    else:
        raise ValueError(name)
    return o


# (at F = 7 there is one f2 block -- dropping "the last" one would drop the whole embed input -- so the embed mutation
# there is the one-chunk slice bug instead)
COMMON = ["conv1_reads_next_bin", "conv2_window_off_by_one", "cmvn_skips_last_read_bin"]
MUTATIONS = [(7, n) for n in COMMON + ["embed_chunk_added_twice"]] + [(128, n) for n in COMMON + ["embed_drops_last_f2"]]


@pytest.mark.parametrize("F", WIDTHS)
def test_the_replacement_embed_is_the_oracles(F):
    """_embed4 without a shift reproduces the oracle's own front end (so the mutations differ from it by the shift only)"""
    o = _oracle(F)
    o._embed = lambda x, offset: _embed4(o, x, offset)
    assert _err(F, _logits(o, F)) < 1e-12


@pytest.mark.parametrize("F,name", MUTATIONS)
def test_front_end_mutations_exceed_the_budget(F, name):
    e = _err(F, _logits(_mutant(F, name), F))
    print(f"[widths] F={F} {name}: {e:.2e} = {e / nm.F32_BUDGET:.0f} x budget")
    assert e >= MARGIN * nm.F32_BUDGET, (F, name, e)
