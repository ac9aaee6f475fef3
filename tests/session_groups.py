"""Shared harness of the session-group tests (a plain module, imported by tests/test_*_session_groups_gpu.py): what a
round of ppasr_encode_chunk_group must guarantee whatever the family -- every session follows its own float64
forward_chunk and its own stream handle, a refused round changes nothing, a round stays inside its workspace, a
StreamPool on the group equals predict_stream.  A family file keeps its models, its `make_group(model, n, max_frames=0)`,
its constants and its parametrisations; every function here asserts the union of what the per-family copies it replaced
asserted.  tests/test_session_groups_harness_cpu.py runs the driver on a CPU stand-in and seeds faults into it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ref_cases as rc
from numerics import F32_BUDGET, logprob_err, rel
from ppasr_amd import _lib
from ppasr_amd.utils.synth import synth_features

HERE = os.path.dirname(os.path.abspath(__file__))
WINDOW, STRIDE = 67, 64  # predict.py:277-283: 67 frames -> 16 encoder frames per chunk (8 behind a stride layer)
EINVAL = _lib.PPASR_EINVAL


def feats(frames, seed, device="cuda"):
    return torch.from_numpy(synth_features(1, frames, seed=seed)[0]).to(device)


def win(x, k):
    return x[:, k * STRIDE:k * STRIDE + WINDOW]


def status_of(fn):
    try:
        fn()
    except _lib.PPASRHipError as e:
        return e.status
    return _lib.PPASR_OK


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize()


def _np(t):
    _sync(t)
    return t.cpu().numpy()


class OracleStream:
    """forward_chunk of one utterance by the oracle (float64 in the GPU tests), chunk by chunk (memoised: sessions that
    replay an utterance share it)."""

    def __init__(self, oracle, x):
        self.oracle, self.x, self.outs = oracle, x, []
        self._att = self._cnn = None
        self._off = 0

    def chunk(self, k):
        while len(self.outs) <= k:
            with torch.no_grad():
                xs, self._att, self._cnn = self.oracle.forward_chunk(win(self.x, len(self.outs)), self._off, -16, self._att,
                                                                     self._cnn)
                logits = self.oracle.ctc_logits(xs)
            self._off += xs.shape[1]
            self.outs.append((logits[0].numpy(), self._off))
        return self.outs[k]


def drive(group, utts, start, rounds, order_seed, oracle_streams, budget=F32_BUDGET, subset=None):
    """Round r advances session s (utterance utts[s], chunk r - start[s]) when it has started, has audio left and (subset)
    is picked this round; the sessions of a round are listed in a shuffled order.  Every output is checked against the
    oracle: its shape, probabilities relative to their largest magnitude and log-probabilities (tests/numerics.py), the
    frame argmax and the session's offset.  -> (worst error, chunks done per session)"""
    rng = np.random.Generator(np.random.PCG64(order_seed))
    n_chunks = {s: len(range(0, utts[s].shape[1] - WINDOW + 1, STRIDE)) for s in range(len(utts))}
    done = {s: 0 for s in range(len(utts))}
    worst = 0.0
    for r in range(rounds):
        act = [s for s in range(len(utts)) if r >= start[s] and done[s] < n_chunks[s] and (subset is None or subset(r, s))]
        if not act:
            continue
        act = [act[i] for i in rng.permutation(len(act))]
        fa, fp, probs = group.encode_chunks(act, torch.cat([win(utts[s], done[s]) for s in act], 0), want_probs=True)
        probs, fa = _np(probs), _np(fa)
        for k, s in enumerate(act):
            logits, off = oracle_streams[s].chunk(done[s])
            assert probs[k].shape == logits.shape, (probs[k].shape, logits.shape)
            ref_p = torch.softmax(torch.as_tensor(logits), -1).numpy()
            e_p, e_l = rel(probs[k], ref_p), logprob_err(probs[k], logits)
            worst = max(worst, e_p, e_l)
            assert e_p < budget and e_l < budget, (r, s, e_p, e_l)
            assert np.array_equal(fa[k], probs[k].argmax(-1))
            done[s] += 1
            assert group.offset(s) == off, (r, s)
    return worst, done


def replay_against_handles(model, make_group, utts, streams, first_group):
    """Single stream handles (same route setting) fed the same audio: the same offsets and, chunk by chunk, the same
    probabilities as a group's sessions -- a second group replays every session of `first_group` (driven through
    `streams`) in lockstep."""
    n = len(utts)
    g2 = make_group(model, n)
    hs = [model.new_stream() for _ in range(n)]
    for k in range(max(len(streams[s].outs) for s in range(n))):
        act = [s for s in range(n) if k < len(streams[s].outs)]
        _, _, p = g2.encode_chunks(act, torch.cat([win(utts[s], k) for s in act], 0), want_probs=True)
        for j, s in enumerate(act):
            want = hs[s].encode_chunk(win(utts[s], k), -16)
            assert rel(_np(p[j:j + 1]), _np(want)) < F32_BUDGET, (k, s)
    for s in range(n):
        assert hs[s].offset == first_group.offset(s) == g2.offset(s), s


def reference_pin(family, make_group, must_run, must_refuse, label, capsys):
    """Three sessions replay each streaming fixture of `family` in tests/golden/ref_small.npz, started one round apart,
    listed in a different order every round: each reproduces the fixture's probs and frame counts (chunk-16 = full
    history).  A case whose group is refused must be refused with EUNSUPPORTED while its own stream handle still works;
    `must_run` have to run and `must_refuse` have to be refused.  -> (ran, refused)"""
    from test_ref_pin_gpu import _make_model
    with np.load(os.path.join(HERE, "golden", "ref_small.npz")) as z:
        ref = {k: z[k] for k in z.files}
    cases = sorted({k.split("/")[0] for k in ref if "/chunk-16/" in k and rc.SMALL[k.split("/")[0]]["family"] == family})
    assert set(must_run) | set(must_refuse) <= set(cases)
    refused, ran = [], []
    for name in cases:
        case = rc.SMALL[name]
        model = _make_model(case, rc.state_dict(case))
        x = torch.from_numpy(rc.chunk_features(case)).cuda()
        wins = rc.windows(x.shape[1])
        try:
            g = make_group(model, 3)
        except _lib.PPASRHipError as e:
            assert e.status == _lib.PPASR_EUNSUPPORTED, name
            assert name not in must_run, name
            assert model.new_stream() is not None
            refused.append(name)
            continue
        ran.append(name)
        outs = {s: [] for s in range(3)}
        rng = np.random.Generator(np.random.PCG64(7))
        for r in range(len(wins) + 2):
            act = [s for s in range(3) if 0 <= r - s < len(wins)]
            act = [act[i] for i in rng.permutation(len(act))]
            chunks = [x[:, wins[r - s][0]:wins[r - s][1]] for s in act]
            if len({f.shape[1] for f in chunks}) > 1:  # (a shorter last window: one call per length)
                for s, f in zip(act, chunks):
                    outs[s].append(g.encode_chunks([s], f, want_probs=True)[2][0].cpu().numpy())
                continue
            probs = g.encode_chunks(act, torch.cat(chunks, 0), want_probs=True)[2].cpu().numpy()
            for k, s in enumerate(act):
                outs[s].append(probs[k])
        k = f"{name}/chunk-16"
        for s in range(3):
            assert [o.shape[0] for o in outs[s]] == ref[k + "/n"].tolist(), (name, s)
            e = rel(np.concatenate(outs[s], 0)[None], ref[k + "/probs"])
            assert e < F32_BUDGET, (name, s, e)
    with capsys.disabled():
        print(f"\n[{label}] reference pin ran: {ran}; EUNSUPPORTED: {refused}")
    assert set(must_run) <= set(ran) and set(must_refuse) <= set(refused)
    return ran, refused


def reset_mid_stream(model, make_group, x0, x1, fresh_chunk, offsets):
    """Two sessions advance two chunks, session 0 is reset, and the next round (session 1 listed first) gives session 0
    a fresh handle's result on chunk `fresh_chunk` of its utterance while session 1 carries on undisturbed.  `offsets`:
    encoder frames per chunk."""
    g = make_group(model, 2)
    for k in range(2):
        g.encode_chunks([0, 1], torch.cat([win(x0, k), win(x1, k)], 0))
    g.reset(0)
    assert g.offset(0) == 0 and g.offset(1) == 2 * offsets
    _, _, p = g.encode_chunks([1, 0], torch.cat([win(x1, 2), win(x0, fresh_chunk)], 0), want_probs=True)
    fresh = model.new_stream().encode_chunk(win(x0, fresh_chunk), -16)
    assert rel(_np(p[1:2]), _np(fresh)) < F32_BUDGET
    h = model.new_stream()
    for k in range(3):
        want = h.encode_chunk(win(x1, k), -16)
    assert rel(_np(p[0:1]), _np(want)) < F32_BUDGET
    assert g.offset(0) == offsets and g.offset(1) == 3 * offsets


# (sessions listed, (session, chunk) of each window) of the rounds refusals_leave_state expects EINVAL for: a repeated
# session; session 0 could advance but session 1 is full, in either order -- nothing happens to either; an index past
# the group; and REFUSED_NEGATIVE, a negative index
REFUSED_CALLS = [([0, 0], [(0, 1), (0, 1)]), ([0, 1], [(0, 1), (1, 3)]), ([1, 0], [(1, 3), (0, 1)]), ([2], [(0, 1)])]
REFUSED_NEGATIVE = ([-1], [(0, 1)])


def refusals_leave_state(model, make_group, x, refused_calls, offsets):
    """A group of two with room for three chunks per session: session 1 is filled, session 0 holds one chunk.  Each of
    `refused_calls` is refused with EINVAL, moves no offset, and the next two valid rounds give bit for bit what they
    give when the refused calls were never made."""
    runs = []
    for with_refusals in (False, True):
        g = make_group(model, 2, max_frames=48)  # room for three 16-frame chunks per session
        g.encode_chunks([0, 1], torch.cat([win(x[0], 0), win(x[1], 0)], 0))
        g.encode_chunks([1], win(x[1], 1))
        g.encode_chunks([1], win(x[1], 2))  # session 1 full (48 frames), session 0 at 16
        if with_refusals:
            for ids, wins in refused_calls:
                chunks = torch.cat([win(x[s], k) for s, k in wins], 0)
                assert status_of(lambda: g.encode_chunks(ids, chunks)) == EINVAL, ids
            assert g.offset(0) == offsets and g.offset(1) == 3 * offsets
        _, _, p = g.encode_chunks([0], win(x[0], 1), want_probs=True)
        _, _, p2 = g.encode_chunks([0], win(x[0], 2), want_probs=True)
        runs.append((p.cpu(), p2.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def max_len_refusal(model, make_group, x, tries, refused_at, offset):
    """A handle and session 1 of a group of two take the chunks of `x`: the chunk the handle refuses (EINVAL, chunk
    `refused_at` of at most `tries`) is the one the group refuses, both stay at `offset` and session 0 at 0."""
    h, g = model.new_stream(), make_group(model, 2)
    for k in range(tries):
        chunk = win(x, k)
        sh = status_of(lambda: h.encode_chunk(chunk, -16))
        sg = status_of(lambda: g.encode_chunks([1], chunk, want_probs=True))
        assert sh == sg, (k, sh, sg)
        if sh != _lib.PPASR_OK:
            break
    assert sh == EINVAL and k == refused_at
    assert g.offset(1) == h.offset == offset and g.offset(0) == 0


def odd_lengths(model, make_group, x, lengths, advance_when_refused):
    """A handle and session 2 of a group of three take windows of `lengths` frames, each starting 3 frames before the end
    of the last one taken (`advance_when_refused`: also of a refused one): the group refuses a round exactly when the
    handle refuses that chunk, the accepted chunks agree and the offsets stay equal.  -> the statuses"""
    h, g = model.new_stream(), make_group(model, 3)
    a, statuses = 0, []
    for T in lengths:
        chunk = x[:, a:a + T]
        out_h, out_g = [], []
        sh = status_of(lambda: out_h.append(h.encode_chunk(chunk, -16)))
        sg = status_of(lambda: out_g.append(g.encode_chunks([2], chunk, want_probs=True)[2]))
        assert sh == sg, (T, sh, sg)
        statuses.append(sh)
        if sh == _lib.PPASR_OK:
            assert rel(_np(out_g[0]), _np(out_h[0])) < F32_BUDGET, T
        if sh == _lib.PPASR_OK or advance_when_refused:
            a += T - 3
        assert g.offset(2) == h.offset, T
    return statuses


def workspace_canary(model, make_group, utts, n, c, check_c_out=False):
    """ppasr_group_chunk_workspace_bytes is monotone in n and T; two rounds of n sessions through the raw
    ppasr_encode_chunk_group call fit in exactly that many bytes (c frames out per session, reported through c_out where
    the family checks it), one byte less is ENOSPACE, and the 4 KiB behind the workspace are never written."""
    lib = model.lib
    need = int(lib.ppasr_group_chunk_workspace_bytes(model._h, n, WINDOW))
    assert need > 0
    sizes = [int(lib.ppasr_group_chunk_workspace_bytes(model._h, m, T)) for m in (1, 2, 8, 64, 256) for T in (7, 31, 67, 130)]
    for m in range(5):  # monotone in n (rows) and T (columns)
        row = sizes[4 * m:4 * m + 4]
        assert row == sorted(row)
        if m:
            assert all(a >= b for a, b in zip(row, sizes[4 * (m - 1):4 * m]))
    g = make_group(model, n)
    canary = 4096
    ws = torch.full((need + canary,), 0xA5, dtype=torch.uint8, device="cuda:0")
    x = torch.cat([utts[s % len(utts)][:, :WINDOW] for s in range(n)], 0).contiguous()
    probs = torch.empty(n, c, model.vocab_size, device="cuda:0")
    fa = torch.empty(n, c, dtype=torch.int32, device="cuda:0")
    fp = torch.empty(n, c, device="cuda:0")
    ids = (ctypes.c_int * n)(*range(n))
    c_out = ctypes.c_int(0)
    st = torch.cuda.current_stream().cuda_stream

    def call(ws_bytes, c_ptr=None):
        return lib.ppasr_encode_chunk_group(g._g, ids, n, x.data_ptr(), WINDOW, probs.data_ptr(), fa.data_ptr(),
                                            fp.data_ptr(), c_ptr, ws.data_ptr(), ws_bytes, st)
    for _ in range(2):
        _lib.check(call(need, ctypes.byref(c_out) if check_c_out else None))
        assert not check_c_out or c_out.value == c
    assert call(need - 1) == _lib.PPASR_ENOSPACE
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all())
    assert g.offset(0) == 2 * c


def predict_stream_reference(cfg, sd, vocab, wavs, step=16000):
    """-> (predictor, PCM16 bytes per utterance, predict_stream's final result per utterance fed in packets of `step`
    bytes (0.5 s)); the predictor's stream is reset behind the last one."""
    from ppasr_amd.predict import PPASRPredictor
    p = PPASRPredictor(configs=cfg, state_dict=sd, vocab_list=vocab, warmup=False)
    pcms = [(np.clip(w, -1, 1) * 32767).astype(np.int16).tobytes() for w in wavs]
    want = []
    for pcm in pcms:
        p.reset_stream()
        out = None
        for i in range(0, len(pcm), step):
            out = p.predict_stream(audio_data=pcm[i:i + step], is_end=(i + step >= len(pcm))) or out
        want.append(out)
    p.reset_stream()
    return p, pcms, want


def pool_equals_predict_stream(cfg, sd, vocab, make_group, wavs, oversize):
    """One StreamPool session per utterance on a group of make_group, all fed in lockstep: every session's text equals its
    own PPASRPredictor.predict_stream, its score within 1e-3.  `oversize`: a pool of one session more than its group
    holds is a ValueError."""
    from ppasr_amd.serving import StreamPool
    step = 16000
    p, pcms, want = predict_stream_reference(cfg, sd, vocab, wavs, step)
    model, n = p.predictor.model, len(wavs)
    if oversize:
        with pytest.raises(ValueError):
            StreamPool(model, vocab, n_sessions=n + 1, preprocess_conf=cfg["preprocess_conf"], group=make_group(model, n))
    grp = make_group(model, n)
    pool = StreamPool(model, vocab, n_sessions=n, preprocess_conf=cfg["preprocess_conf"], group=grp)
    assert pool.group is grp
    for i in range(0, max(len(x) for x in pcms), step):
        for s, pcm in enumerate(pcms):
            if i < len(pcm):
                pool.feed(s, pcm[i:i + step])
        pool.step()
    for s in range(n):
        got = pool.finish(s)
        assert got is not None and want[s] is not None and got["text"] == want[s]["text"], s
        assert abs(got["score"] - want[s]["score"]) < 1e-3


def f16x3_group(model_f32_handle, model, make_group, utts, streams):
    """ppasr_set_gemm_mode(F16X3) on `model` (`model_f32_handle`: a stream handle of it, still unused): groups of 1 and 3
    sessions stay within 1e-3 of the float64 oracle and equal the handle in that mode within the fp32 budget, the handle's
    chunks differ from the fp32 handle's (the mode is in effect on it), and no guard fallback is counted: streaming
    chunks are never re-run."""
    ref32 = [model_f32_handle.encode_chunk(win(utts[0], k), -16).cpu().numpy() for k in range(3)]
    model.set_gemm_mode("f16x3")
    fb0, _ = model.gemm_guard_stats()
    for n in (1, 3):
        g = make_group(model, n)
        u = [utts[s % len(utts)] for s in range(n)]
        drive(g, u, [0] * n, 3, 200 + n, [streams[s % len(utts)] for s in range(n)], budget=1e-3)
        g.reset()
        h = model.new_stream()
        for k in range(3):
            _, _, p = g.encode_chunks(list(range(n)), torch.cat([win(x, k) for x in u], 0), want_probs=True)
            want = _np(h.encode_chunk(win(utts[0], k), -16))
            assert rel(_np(p[0:1]), want) < F32_BUDGET, (n, k)
            if n == 1:
                assert not np.array_equal(want, ref32[k])
    fb1, _ = model.gemm_guard_stats()
    assert fb1 == fb0


def launches_by_kernel(fn, strip=None):
    """-> {kernel name: launches} of fn() inside the library's kernel profile (strip: a pattern cut out of every name,
    such as the template arguments, the counts of equal names added up)."""
    with _lib.kernel_profile() as kp:
        fn()
        torch.cuda.synchronize()
    out = {}
    for name, (_ms, launches) in kp.kernels.items():
        name = re.sub(strip, "", name) if strip else name
        out[name] = out.get(name, 0) + launches
    return out
