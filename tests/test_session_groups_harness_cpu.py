"""tests/session_groups.py has teeth: a stand-in group whose sessions are fp32 oracle streams on the CPU (the interface of
the library's groups: encode_chunks, offset, reset; its model hands out stream handles) passes drive,
replay_against_handles and reset_mid_stream against the float64 oracle, and each of a fixed list of faults seeded into it
-- the ways a round can go wrong that the per-family copies of the driver guarded against between them -- makes the
harness raise AssertionError."""
import pytest
import torch

import session_groups as sg
from numerics import F32_BUDGET, oracle64
from oracle.conformer_oracle import ConformerOracle
from ppasr_amd.utils.synth import conformer_state_dict

V, L = 50, 2
START = [0, 1, 2]  # round 0 lists one session, round 1 two, from round 2 on all three
FAULTS = ["swap", "offset", "argmax", "perturb", "extra_axis", "squeezed"]


class Handle:
    """One fp32 oracle stream with the stream handle's interface."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.reset()

    def reset(self):
        self.offset, self._att, self._cnn = 0, None, None

    def encode_chunk(self, x, required):
        probs, self._att, self._cnn = self.oracle.get_encoder_out_chunk(x, self.offset, required, self._att, self._cnn)
        self.offset += probs.shape[1]
        return probs


class Model:
    def __init__(self, oracle):
        self.oracle = oracle

    def new_stream(self):
        return Handle(self.oracle)


class Group:
    """n handles behind the session group's interface; `fault` seeds one of FAULTS into every round it applies to."""

    def __init__(self, model, n, max_frames=0, fault=None):
        self.sessions = [model.new_stream() for _ in range(n)]
        self.fault = fault
        self._before = {}  # session: its offset before its last chunk

    def offset(self, s):
        if self.fault == "offset" and s == 1:  # session 1's last chunk never shows in its offset
            return self._before.get(s, 0)
        return self.sessions[s].offset

    def reset(self, s=None):
        for h in self.sessions if s is None else [self.sessions[s]]:
            h.reset()

    def encode_chunks(self, ids, chunks, want_probs=False):
        self._before.update({s: self.sessions[s].offset for s in ids})
        probs = torch.cat([self.sessions[s].encode_chunk(chunks[k:k + 1], -16) for k, s in enumerate(ids)], 0)
        if self.fault == "swap" and len(ids) > 1:  # two sessions' outputs change places
            probs = probs[[1, 0] + list(range(2, len(ids)))]
        if self.fault == "perturb":
            probs = probs * (1 + 1e-3)
        fa, fp = probs.argmax(-1).to(torch.int32), probs.max(-1).values
        if self.fault == "argmax":  # off by one on one frame
            fa[0, 3] = (fa[0, 3] + 1) % V
        if self.fault == "extra_axis":
            probs = probs[:, None]
        if self.fault == "squeezed" and len(ids) == 1:
            probs = probs[0]
        return fa, fp, probs if want_probs else None


@pytest.fixture(scope="module")
def fake():
    sd = conformer_state_dict(vocab_size=V, num_blocks=L, seed=11, perturb_norm=True)
    utts = [sg.feats(sg.STRIDE * (3 + s % 2) + sg.WINDOW, 40 + s, device="cpu") for s in range(3)]
    oracle = oracle64("conformer", sd, num_blocks=L)
    return Model(ConformerOracle(sd, num_blocks=L)), utts, [sg.OracleStream(oracle, u) for u in utts]


def _make(fault):
    return lambda model, n, max_frames=0: Group(model, n, max_frames, fault)


def test_the_fp32_stand_in_passes(fake, capsys):
    model, utts, streams = fake
    g = Group(model, 3)
    worst, done = sg.drive(g, utts, START, 8, 5, streams, subset=lambda r, s: (r + s) % 4 != 0 or s == 0)
    with capsys.disabled():
        print(f"\n[session-group harness] fp32 stand-in against float64: worst {worst:.2e} (budget {F32_BUDGET:.0e})")
    assert done == {0: 4, 1: 5, 2: 4}
    assert 0.0 < worst < F32_BUDGET  # (measured 5.5e-6: the worse of both metrics over every chunk of every session)
    sg.replay_against_handles(model, _make(None), utts, streams, g)
    sg.reset_mid_stream(model, _make(None), utts[0], utts[1], fresh_chunk=3, offsets=16)
    sg.reset_mid_stream(model, _make(None), utts[0], utts[1], fresh_chunk=0, offsets=16)


@pytest.mark.parametrize("fault", FAULTS)
def test_drive_flags(fake, fault):
    model, utts, streams = fake
    with pytest.raises(AssertionError):
        sg.drive(Group(model, 3, fault=fault), utts, START, 8, 5, streams)


@pytest.mark.parametrize("fault", ["swap", "offset", "perturb", "extra_axis"])
def test_replay_and_reset_flag(fake, fault):
    """The faults the two handle comparisons can see (they do not look at frame_argmax, and list more than one session)."""
    model, utts, streams = fake
    g = Group(model, 3)
    sg.drive(g, utts, START, 8, 5, streams)
    with pytest.raises(AssertionError):
        sg.replay_against_handles(model, _make(fault), utts, streams, g)
    with pytest.raises(AssertionError):
        sg.reset_mid_stream(model, _make(fault), utts[0], utts[1], fresh_chunk=3, offsets=16)
