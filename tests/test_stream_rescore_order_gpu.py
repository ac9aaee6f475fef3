"""ppasr_encode_chunk_group_mem, ppasr_prob_arena_read_many and ppasr_beam_sessions_nbest do all their work on the caller's
stream: tests/stream_gate.py, both modes, one small case each."""
import numpy as np
import pytest
import torch

import stream_gate as sg
import stream_rescore_cases as sc
from numerics import Memo
from ppasr_amd.utils.synth import synth_vocabulary

pytestmark = pytest.mark.gpu
_memo = Memo()


def _model():
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    return _memo.get("model", lambda: ConformerModel(80, sc.V, streaming=True, encoder_conf=sc.ENC,
                                                     state_dict=sc.checkpoint(), device="cuda:0"))


def _windows():
    f = _memo.get("feats", sc.features)
    real = np.concatenate([sc.windows(f["A"])[0], sc.windows(f["B"])[0]], 0)
    decoy = np.concatenate([sc.windows(f["C"])[0], sc.windows(f["D"])[0]], 0)
    return real, decoy


def _group_mem(ctx):
    from ppasr_amd.decoders.ctc_alignment import ProbArena
    from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
    group, arena = ConformerStreamGroup(_model(), 2), ProbArena(2, 256, page_frames=5, n_pages=8, device="cuda:0")
    x = ctx.input(*_windows())
    fa, fp, probs = ctx.call(lambda: group.encode_chunks([1, 0], x, want_probs=True, memory_arena=arena,
                                                         memory_frames=[16, 9]), [x], label="encode_chunk_group_mem")
    memory, lens = ctx.call(lambda: arena.read_many([0, 1]), label="read_many")
    return dict(fa=fa, fp=fp, probs=probs, memory=memory, lens=lens)


def _table(seed, n=2, T=12, V=37):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.softmax(torch.from_numpy(2.0 * rng.standard_normal((n, T, V)).astype(np.float32)), -1)


def _read_many(ctx):
    from ppasr_amd.decoders.ctc_alignment import ProbArena
    arena = ProbArena(3, 37, page_frames=5, n_pages=8, device="cuda:0")
    p = ctx.input(_table(1), _table(2))
    ctx.call(lambda: arena.append([2, 0], p, [12, 7]), [p], label="append")
    dense, lens = ctx.call(lambda: arena.read_many([0, 2, 1], 14), label="read_many")
    return dict(dense=dense, lens=lens)


def _nbest(ctx):
    from ppasr_amd.decoders.beam_search_decoder import BeamSearchSessions
    pool = BeamSearchSessions(3, 0.0, 0.0, 5, 0.99, 40, synth_vocabulary(37), init_frames=16)
    p = ctx.input(_table(3), _table(4))
    ctx.call(lambda: pool.decode_chunks([2, 0], p), [p], syncs="beam_search_decoder.py decode_chunks reads its results back",
             label="decode_chunks")
    tokens, lens, scores = ctx.call(lambda: pool.nbest([0, 2], 3, max_tokens=12), label="nbest")
    return dict(tokens=tokens, lens=lens, scores=scores)


CASES = {"group_mem": _group_mem, "read_many": _read_many, "nbest": _nbest}


@pytest.mark.parametrize("mode", sg.MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_all_work_is_on_the_callers_stream(case, mode):
    sg.check(f"stream_rescore/{case}", CASES[case], mode, memo=_memo)
