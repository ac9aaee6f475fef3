"""No streaming result depends on what the chunk workspace and the output buffers held on entry (tests/poison.py): stream
handles of the four transformer routes and session groups of all five families, chunk by chunk / round by round against
the same calls on zero-filled buffers of a fresh handle, byte for byte.

``stale``: the handle / group under test first carries ANOTHER, longer stream (other features, the cache trimmed to 32
frames on handles, the 8-way split route where accepted), is reset, and then runs the stream under test on the workspace
and the cache slots that stream left behind.  Handle-owned buffers (K / V caches, conv caches, recurrent state) cannot be
filled from here before the library first uses them: reset-and-reuse is the only way they are reached."""
import pytest
import torch

import numerics as nm
import poison
import test_ragged_gpu as rg
from test_buffer_contents_gpu import _accepted, _ds2
from ppasr_amd.utils.synth import synth_features

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
V = 131
WINDOWS = [(0, 67), (64, 131), (128, 195), (192, 227)]  # predict_stream's windowing, a short last chunk (35 frames)
HANDLES = ["conformer", "squeezeformer", "efficient", "conformer512"]


def _feats(n, T, seed):
    return torch.from_numpy(synth_features(n, T, seed=seed)[0]).cuda()


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("required", [-16, 32])
@pytest.mark.parametrize("ffn_split", [-1, 0])
@pytest.mark.parametrize("family", HANDLES)
def test_stream_handle(family, ffn_split, required, pattern, monkeypatch):
    x = _feats(1, 227, 31)
    other = _feats(1, 64 * 6 + 67, 32)

    def run(s):
        model = rg.FAMILIES[family](V)[0]
        stream = model.new_stream()
        if s.stale:
            _accepted(lambda: model.set_ffn_split(8))
            for k in range(7):
                stream.encode_chunk(other[:, 64 * k:64 * k + 67], 32, want_frames=True)
            stream.export_caches()
            stream.reset()
        model.set_ffn_split(ffn_split)
        outs = {}
        for k, (a, b) in enumerate(WINDOWS):
            s.scratch(stream)
            probs, fa, fp = stream.encode_chunk(x[:, a:b], required, want_frames=True)
            s.observe(stream, f"chunk {k}")
            att, cnn = stream.export_caches()
            torch.cuda.synchronize()
            outs.update({f"{k}/probs": probs, f"{k}/frame_argmax": fa, f"{k}/frame_maxprob": fp, f"{k}/att_cache": att,
                         f"{k}/cnn_cache": cnn, f"{k}/offset": torch.tensor([stream.offset, stream.cache_frames])})
        return outs, stream

    poison.check(f"stream {family} ffn_split={ffn_split} required={required}", run, pattern, monkeypatch, MEMO)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_stateless_chunk_signature(pattern, monkeypatch):
    """get_encoder_out_chunk: the caches go through a scratch stream object the model keeps (import, chunk, export)."""
    x = _feats(1, 227, 33)

    def run(s):
        model = rg.FAMILIES["conformer"](V)[0]
        if s.stale:
            o = _feats(1, 131, 34)
            _, a, c = model.get_encoder_out_chunk(o[:, :67], 0, 32)
            model.get_encoder_out_chunk(o[:, 64:131], 16, 32, a, c)
        outs, att, cnn, off = {}, None, None, 0
        for k, (a, b) in enumerate(WINDOWS):
            s.scratch(model)
            probs, att, cnn = model.get_encoder_out_chunk(x[:, a:b], off, -16, att, cnn)
            s.observe(model, f"chunk {k}")
            off += probs.shape[1]
            outs.update({f"{k}/probs": probs, f"{k}/att_cache": att, f"{k}/cnn_cache": cnn})
        return outs, model

    poison.check("stateless chunks conformer", run, pattern, monkeypatch, MEMO)


# ---- session groups ----------------------------------------------------------------------------------------------------
GROUPS = HANDLES + ["deepspeech2-lstm", "deepspeech2-gru"]


def _group(family, model, n=3):
    from ppasr_amd.model_utils.conformer.model import GeneralConformerStreamGroup, StreamHandleSet, make_stream_group
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup
    if family in ("conformer", "deepspeech2-lstm", "deepspeech2-gru"):
        g = make_stream_group(model, n, max_frames=256)
        assert not isinstance(g, StreamHandleSet)
        return g
    cls = {"squeezeformer": SqueezeformerStreamGroup, "efficient": EfficientConformerStreamGroup,
           "conformer512": GeneralConformerStreamGroup}[family]
    return cls(model, n, max_frames=256)


def _group_model(family):
    if family.startswith("deepspeech2"):
        return _ds2(True, family.endswith("gru"))
    return rg.FAMILIES[family](V)[0]


# rounds that list a changing subset of the sessions; the last round is a shorter chunk
ROUNDS = [([0, 2], 67), ([1], 67), ([0, 1, 2], 67), ([2, 1], 67), ([0], 67), ([1, 0, 2], 35)]


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("family", GROUPS)
def test_session_group(family, pattern, monkeypatch):
    utts = [_feats(1, 64 * len(ROUNDS) + 67, 50 + u) for u in range(3)]
    other = _feats(3, 64 * 5 + 67, 60)

    def run(s):
        g = _group(family, _group_model(family))
        if s.stale:
            for k in range(5):
                act = [[0, 1, 2], [2, 0], [1, 2, 0]][k % 3]
                g.encode_chunks(act, other[act, 64 * k:64 * k + 67], want_probs=True)
            g.reset()
        outs, pos = {}, [0, 0, 0]
        for r, (act, T) in enumerate(ROUNDS):
            chunk = torch.cat([utts[i][:, 64 * pos[i]:64 * pos[i] + T] for i in act], 0)
            s.scratch(g)
            fa, fp, probs = g.encode_chunks(act, chunk, want_probs=True)
            s.observe(g, f"round {r} {act}")
            torch.cuda.synchronize()
            for i in act:
                pos[i] += 1
            outs.update({f"{r}/probs": probs, f"{r}/frame_argmax": fa, f"{r}/frame_maxprob": fp,
                         f"{r}/offsets": torch.tensor([g.offset(i) for i in act])})
        return outs, g

    poison.check(f"group {family}", run, pattern, monkeypatch, MEMO)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("family", GROUPS)
def test_session_group_slot_reuse_mid_stream(family, pattern, monkeypatch):
    """One slot is reset while the others carry on (in every pattern: the reset is part of the case).  The clean
    reference does not reset: its group has a fourth slot that nothing used before, and the restarted session runs
    there, next to the same two sessions at the same places of the round."""
    utts = [_feats(1, 64 * 5 + 67, 70 + u) for u in range(3)]
    other = _feats(3, 64 * 2 + 67, 80)

    def run(s):
        clean = s.pattern == "zero"
        g = _group(family, _group_model(family), 4 if clean else 3)
        if s.stale:
            for k in range(3):
                g.encode_chunks([2, 1, 0], other[:, 64 * k:64 * k + 67], want_probs=True)
            g.reset()
        outs = {}
        for k in range(5):
            if k == 2 and not clean:
                g.reset(1)
            # from round 2 on the middle session starts over with utterance 0's features; sessions 0 and 2 go on
            mid = utts[1][:, 64 * k:64 * k + 67] if k < 2 else utts[0][:, 64 * (k - 2):64 * (k - 2) + 67]
            chunk = torch.cat([utts[0][:, 64 * k:64 * k + 67], mid, utts[2][:, 64 * k:64 * k + 67]], 0)
            s.scratch(g)
            fa, fp, p = g.encode_chunks([0, 3 if clean and k >= 2 else 1, 2], chunk, want_probs=True)
            s.observe(g, f"round {k}")
            outs.update({f"{k}/probs": p, f"{k}/frame_argmax": fa, f"{k}/frame_maxprob": fp})
        torch.cuda.synchronize()
        return outs, g

    poison.check(f"group slot reuse {family}", run, pattern, monkeypatch, MEMO)
