"""GPU: Squeezeformer session groups (ppasr_sq_stream_group_create + ppasr_encode_chunk_group) -- many streaming sessions
advanced with one set of launches per round.  Every session must follow its own SqueezeformerEncoder.forward_chunk
(squeezeformer/encoder.py:260-381) with the full history kept (required_cache_size < 0), whatever the other sessions in
the round are doing: against the reference-source fixtures, the float64 oracle and single stream handles."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ref_cases as rc
from numerics import F32_BUDGET, logprob_err, oracle64
from ppasr_amd import _lib
from ppasr_amd.utils.synth import (conformer_state_dict, efficient_conformer_state_dict, squeezeformer_state_dict,
                                   synth_features, synth_vocabulary)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WINDOW, STRIDE = 67, 64  # predict.py:277-283: 67 frames -> 16 encoder frames per chunk


def _sq_model(sd, V, L, red, rec, ks=31, streaming=True, **extra):
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel
    conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=L, reduce_idx=red, recover_idx=rec,
                feed_forward_expansion_factor=8, cnn_module_kernel=ks, **extra)
    return SqueezeformerModel(80, V, streaming=streaming, encoder_conf=conf, state_dict=sd, device="cuda:0")


def _group(model, n, max_frames=0):
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup
    return SqueezeformerStreamGroup(model, n, max_frames=max_frames)


def _feats(frames, seed):
    return torch.from_numpy(synth_features(1, frames, seed=seed)[0]).cuda()


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _status(fn):
    try:
        fn()
    except _lib.PPASRHipError as e:
        return e.status
    return _lib.PPASR_OK


class _OracleStream:
    """float64 forward_chunk of one utterance, chunk by chunk (memoised: sessions that replay an utterance share it)."""

    def __init__(self, oracle, x):
        self.oracle, self.x, self.outs = oracle, x, []
        self._att = self._cnn = None
        self._off = 0

    def chunk(self, k):
        while len(self.outs) <= k:
            a = len(self.outs) * STRIDE
            with torch.no_grad():
                xs, self._att, self._cnn = self.oracle.forward_chunk(self.x[:, a:a + WINDOW], self._off, -16, self._att,
                                                                     self._cnn)
                logits = self.oracle.ctc_logits(xs)
            self._off += xs.shape[1]
            self.outs.append((logits[0].numpy(), self._off))
        return self.outs[k]


def _drive(group, utts, start, rounds, order_seed, oracle_streams, budget=F32_BUDGET, subset=None):
    """Round r advances session s (utterance utts[s], chunk r - start[s]) when it has started, has audio left and (subset)
    is picked this round; the sessions of a round are listed in a shuffled order.  Every output is checked against the
    oracle: probabilities relative to their largest magnitude and log-probabilities (tests/numerics.py)."""
    rng = np.random.Generator(np.random.PCG64(order_seed))
    n_chunks = {s: len(range(0, utts[s].shape[1] - WINDOW + 1, STRIDE)) for s in range(len(utts))}
    done = {s: 0 for s in range(len(utts))}
    worst = 0.0
    for r in range(rounds):
        act = [s for s in range(len(utts)) if r >= start[s] and done[s] < n_chunks[s] and (subset is None or subset(r, s))]
        if not act:
            continue
        act = [act[i] for i in rng.permutation(len(act))]
        feats = torch.cat([utts[s][:, done[s] * STRIDE:done[s] * STRIDE + WINDOW] for s in act], 0)
        fa, fp, probs = group.encode_chunks(act, feats, want_probs=True)
        torch.cuda.synchronize()
        probs = probs.cpu().numpy()
        for k, s in enumerate(act):
            logits, off = oracle_streams[s].chunk(done[s])
            ref_p = torch.softmax(torch.as_tensor(logits), -1).numpy()
            e_p, e_l = _rel(probs[k], ref_p), logprob_err(probs[k], logits)
            worst = max(worst, e_p, e_l)
            assert e_p < budget and e_l < budget, (r, s, e_p, e_l)
            assert np.array_equal(fa[k].cpu().numpy(), probs[k].argmax(-1))
            done[s] += 1
            assert group.offset(s) == off, (r, s)
    return worst, done


# ---- 1. reference-source pin ---------------------------------------------------------------------------------------
REF_CASES = sorted({k.split("/")[0] for k in np.load(os.path.join(HERE, "golden", "ref_small.npz")).files
                    if "/chunk-16/" in k and rc.SMALL[k.split("/")[0]]["family"] == "squeezeformer"})


def test_reference_source_pin_three_staggered_sessions(capsys):
    """Three sessions replay each streaming Squeezeformer fixture's utterance, started one round apart, listed in a
    different order every round: each reproduces the fixture's probs and frame counts (chunk-16 = full history)."""
    from test_ref_pin_gpu import _make_model
    with np.load(os.path.join(HERE, "golden", "ref_small.npz")) as z:
        ref = {k: z[k] for k in z.files}
    assert {"sq_s", "sq_opt", "sq_gelu_s", "sq_pre_s", "sq_abs_s"} <= set(REF_CASES)
    refused, ran = [], []
    for name in REF_CASES:
        case = rc.SMALL[name]
        model = _make_model(case, rc.state_dict(case))
        x = torch.from_numpy(rc.chunk_features(case)).cuda()
        wins = rc.windows(x.shape[1])
        try:
            g = _group(model, 3)
        except _lib.PPASRHipError as e:
            assert e.status == _lib.PPASR_EUNSUPPORTED, name
            # only the general layer route is outside the groups: the same handle's stream is fine
            assert model.new_stream() is not None
            refused.append(name)
            continue
        ran.append(name)
        outs = {s: [] for s in range(3)}
        rng = np.random.Generator(np.random.PCG64(7))
        for r in range(len(wins) + 2):
            act = [s for s in range(3) if 0 <= r - s < len(wins)]
            act = [act[i] for i in rng.permutation(len(act))]
            feats = [x[:, wins[r - s][0]:wins[r - s][1]] for s in act]
            lens = {f.shape[1] for f in feats}
            if len(lens) > 1:  # (the last, shorter window: one call per length)
                for s, f in zip(act, feats):
                    outs[s].append(g.encode_chunks([s], f, want_probs=True)[2][0].cpu().numpy())
                continue
            probs = g.encode_chunks(act, torch.cat(feats, 0), want_probs=True)[2].cpu().numpy()
            for k, s in enumerate(act):
                outs[s].append(probs[k])
        k = f"{name}/chunk-16"
        for s in range(3):
            assert [o.shape[0] for o in outs[s]] == ref[k + "/n"].tolist(), (name, s)
            e = _rel(np.concatenate(outs[s], 0)[None], ref[k + "/probs"])
            assert e < F32_BUDGET, (name, s, e)
    with capsys.disabled():
        print(f"\n[sq groups] reference pin ran: {ran}; EUNSUPPORTED (general route): {refused}")
    assert "sq_s" in ran and "sq_opt" in ran


# ---- 2. float64 oracle: kernel 31, kernel 15, no time reduction --------------------------------------------------
# route: "default" = by grid size (these small rounds: the split route), "fused" = ppasr_set_ffn_split(0), the fused
# k_sq_mid / k_sq_tail kernels with the per-session conv histories on every layer (full- and half-rate)
ROUTES = ["default", "fused"]


def _set_route(model, route):
    model.set_ffn_split(0 if route == "fused" else -1)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("L,red,rec,ks", [(4, 1, 3, 31), (4, 1, 3, 15), (3, None, None, 31)])
def test_staggered_subsets_match_oracle_and_handles(L, red, rec, ks, route):
    V = 180
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=L, cnn_module_kernel=ks, seed=90 + ks + L, perturb_norm=True)
    model = _sq_model(sd, V, L, red, rec, ks)
    _set_route(model, route)
    oracle = oracle64("squeezeformer", sd, num_blocks=L, cnn_module_kernel=ks, reduce_idx=red, recover_idx=rec)
    n = 5
    utts = [_feats(STRIDE * (4 + s % 3) + WINDOW, 300 + s) for s in range(n)]
    streams = [_OracleStream(oracle, u.cpu()) for u in utts]
    g = _group(model, n)
    start = [0, 1, 0, 2, 3]
    # each round advances a different subset
    _drive(g, utts, start, 12, 11, streams, subset=lambda r, s: (r + s) % 3 != 0 or s == 0)
    # single stream handles (same route setting) fed the same audio: the same offsets and, chunk by chunk, the same
    # probabilities as the group's sessions (a second group replays every session in lockstep)
    g2 = _group(model, n)
    hs = [model.new_stream() for _ in range(n)]
    for k in range(max(len(streams[s].outs) for s in range(n))):
        act = [s for s in range(n) if k < len(streams[s].outs)]
        _, _, p = g2.encode_chunks(act, torch.cat([utts[s][:, k * STRIDE:k * STRIDE + WINDOW] for s in act], 0),
                                   want_probs=True)
        for j, s in enumerate(act):
            want = hs[s].encode_chunk(utts[s][:, k * STRIDE:k * STRIDE + WINDOW], -16)
            torch.cuda.synchronize()
            assert _rel(p[j:j + 1].cpu().numpy(), want.cpu().numpy()) < F32_BUDGET, (k, s)
    for s in range(n):
        assert hs[s].offset == g.offset(s) == g2.offset(s), s


# ---- 3. route thresholds ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sq4():
    V = 180
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=131, perturb_norm=True)
    model = _sq_model(sd, V, 4, 1, 3)
    oracle = oracle64("squeezeformer", sd, num_blocks=4, reduce_idx=1, recover_idx=3)
    utts = [_feats(STRIDE * 3 + WINDOW, 400 + u) for u in range(5)]
    streams = [_OracleStream(oracle, u.cpu()) for u in utts]
    return model, utts, streams, sd


@pytest.mark.parametrize("n,route", [(1, "default"), (2, "default"), (3, "default"), (33, "default"), (64, "default"),
                                     (260, "default"), (1, "fused"), (3, "fused"), (64, "fused")])
def test_route_thresholds(sq4, n, route):
    """n x 16 full-rate rows and n x 8 half-rate rows, several rounds each.  By default n <= 64 (16 .. 1 024 rows) stays
    on the split route (ffn_split_for: <= 128 row blocks) with 8, 4 or 2 slices; n = 260 puts the full-rate layers
    (4 160 rows) on the fused kernels and keeps the half-rate ones (2 080 rows) on the split route, so one round
    switches route at the reduction and back at the recovery.  route = "fused" (ppasr_set_ffn_split(0)): every layer,
    full- and half-rate, on the fused k_sq_mid / k_sq_tail kernels with one streaming history per session."""
    model, utts, streams, _ = sq4
    _set_route(model, route)
    try:
        g = _group(model, n, max_frames=16 * 6)
        u = [utts[s % len(utts)] for s in range(n)]
        st = [streams[s % len(utts)] for s in range(n)]
        worst, done = _drive(g, u, [0] * n, 4, 100 + n, st)
    finally:
        _set_route(model, "default")
    assert all(v == 4 for v in done.values())
    print(f"n={n} {route}: worst {worst:.2e}")


# ---- 4. state -------------------------------------------------------------------------------------------------------
def test_reset_mid_stream_matches_a_fresh_handle(sq4):
    model, utts, _, _ = sq4
    g = _group(model, 2)
    x0, x1 = utts[0], utts[1]
    for k in range(2):
        g.encode_chunks([0, 1], torch.cat([x0[:, k * STRIDE:k * STRIDE + WINDOW], x1[:, k * STRIDE:k * STRIDE + WINDOW]], 0))
    g.reset(0)
    assert g.offset(0) == 0 and g.offset(1) == 32
    _, _, p = g.encode_chunks([1, 0], torch.cat([x1[:, 2 * STRIDE:2 * STRIDE + WINDOW], x0[:, :WINDOW]], 0), want_probs=True)
    fresh = model.new_stream().encode_chunk(x0[:, :WINDOW], -16)
    torch.cuda.synchronize()
    assert _rel(p[1:2].cpu().numpy(), fresh.cpu().numpy()) < F32_BUDGET
    # session 1 carried on undisturbed
    h = model.new_stream()
    for k in range(3):
        want = h.encode_chunk(x1[:, k * STRIDE:k * STRIDE + WINDOW], -16)
    assert _rel(p[0:1].cpu().numpy(), want.cpu().numpy()) < F32_BUDGET
    assert g.offset(0) == 16 and g.offset(1) == 48


def test_refusals_leave_every_session_as_it_was(sq4):
    """A repeated session, a capacity overrun and a max_len overrun are refused with EINVAL, and the next valid call gives
    bit for bit what it gives when the refused calls were never made."""
    model, utts, _, _ = sq4
    x = [utts[0], utts[1]]
    win = lambda s, k: x[s][:, k * STRIDE:k * STRIDE + WINDOW]
    runs = []
    for with_refusals in (False, True):
        g = _group(model, 2, max_frames=48)  # room for three 16-frame chunks per session
        g.encode_chunks([0, 1], torch.cat([win(0, 0), win(1, 0)], 0))
        g.encode_chunks([1], win(1, 1))
        g.encode_chunks([1], win(1, 2))  # session 1 full (48 frames), session 0 at 16
        if with_refusals:
            assert _status(lambda: g.encode_chunks([0, 0], torch.cat([win(0, 1), win(0, 1)], 0))) == _lib.PPASR_EINVAL
            # session 0 could advance, session 1 cannot: nothing happens to either
            assert _status(lambda: g.encode_chunks([0, 1], torch.cat([win(0, 1), win(1, 3)], 0))) == _lib.PPASR_EINVAL
            assert _status(lambda: g.encode_chunks([1, 0], torch.cat([win(1, 3), win(0, 1)], 0))) == _lib.PPASR_EINVAL
            assert _status(lambda: g.encode_chunks([2], win(0, 1))) == _lib.PPASR_EINVAL
            assert g.offset(0) == 16 and g.offset(1) == 48
        _, _, p = g.encode_chunks([0], win(0, 1), want_probs=True)
        _, _, p2 = g.encode_chunks([0], win(0, 2), want_probs=True)
        runs.append((p.cpu(), p2.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_max_len_and_odd_lengths_refused_exactly_where_a_handle_refuses():
    """max_len: the chunk a single handle refuses (offset + chunk >= max_len) is the one the group refuses.  Odd cache
    lengths: chunks of odd frame counts (c = 15, 13, 1, 16, ...) on both -- the group refuses a round exactly when the
    handle refuses that chunk (with the full history the reference's trim of the reduced cache keeps every length in
    line, so neither does) and their outputs agree."""
    V = 180
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=141, perturb_norm=True)
    model = _sq_model(sd, V, 4, 1, 3, max_len=72)
    x = _feats(64 * 6 + 67, 142)
    h, g = model.new_stream(), _group(model, 2)
    got_h, got_g = [], []
    for k in range(6):
        chunk = x[:, k * 64:k * 64 + 67]
        sh = _status(lambda: got_h.append(h.encode_chunk(chunk, -16)))
        sg = _status(lambda: got_g.append(g.encode_chunks([1], chunk, want_probs=True)[2]))
        assert sh == sg, (k, sh, sg)
        if sh != _lib.PPASR_OK:
            break
    assert sh == _lib.PPASR_EINVAL and k == 4  # offsets 0, 16, 32, 48 fit; 64 + 16 >= 72 does not
    assert g.offset(1) == h.offset == 64
    # odd frame counts
    model = _sq_model(sd, V, 4, 1, 3)
    h, g = model.new_stream(), _group(model, 3)
    a = 0
    for T in (63, 59, 7, 67, 55, 11, 63, 67):
        chunk = x[:, a:a + T]
        a += T - 3
        out_h = []
        sh = _status(lambda: out_h.append(h.encode_chunk(chunk, -16)))
        sg = _status(lambda: got_g.append(g.encode_chunks([2], chunk, want_probs=True)[2]))
        assert sh == sg, (T, sh, sg)
        if sh == _lib.PPASR_OK:
            torch.cuda.synchronize()
            assert _rel(got_g[-1].cpu().numpy(), out_h[0].cpu().numpy()) < F32_BUDGET, T
    assert g.offset(2) == h.offset


# ---- 5. workspace guard ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64])
def test_workspace_canary(sq4, n):
    model, utts, _, _ = sq4
    lib = model.lib
    need = int(lib.ppasr_group_chunk_workspace_bytes(model._h, n, WINDOW))
    assert need > 0
    sizes = [int(lib.ppasr_group_chunk_workspace_bytes(model._h, m, T)) for m in (1, 2, 8, 64, 256) for T in (7, 31, 67, 130)]
    for m in range(5):  # monotone in n (rows) and T (columns)
        row = sizes[4 * m:4 * m + 4]
        assert row == sorted(row)
        if m:
            assert all(a >= b for a, b in zip(row, sizes[4 * (m - 1):4 * m]))
    g = _group(model, n)
    canary = 4096
    ws = torch.full((need + canary,), 0xA5, dtype=torch.uint8, device="cuda:0")
    x = torch.cat([utts[s % len(utts)][:, :WINDOW] for s in range(n)], 0).contiguous()
    c = 16
    probs = torch.empty(n, c, model.vocab_size, device="cuda:0")
    fa = torch.empty(n, c, dtype=torch.int32, device="cuda:0")
    fp = torch.empty(n, c, device="cuda:0")
    ids = (ctypes.c_int * n)(*range(n))
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        _lib.check(lib.ppasr_encode_chunk_group(g._g, ids, n, x.data_ptr(), WINDOW, probs.data_ptr(), fa.data_ptr(),
                                                fp.data_ptr(), None, ws.data_ptr(), need, st))
    assert lib.ppasr_encode_chunk_group(g._g, ids, n, x.data_ptr(), WINDOW, probs.data_ptr(), fa.data_ptr(), fp.data_ptr(),
                                        None, ws.data_ptr(), need - 1, st) == _lib.PPASR_ENOSPACE
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all())
    assert g.offset(0) == 32


# ---- 6. serving ------------------------------------------------------------------------------------------------------
def test_stream_pool_with_a_squeezeformer_group_equals_predict_stream():
    from test_predictor_gpu import _audio, _cfg
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup
    from ppasr_amd.predict import PPASRPredictor
    from ppasr_amd.serving import StreamPool
    V = 300
    vocab = synth_vocabulary(V)
    cfg = _cfg(use_model="squeezeformer", L=4)
    cfg["encoder_conf"] = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=4, reduce_idx=1,
                               recover_idx=3, feed_forward_expansion_factor=8, cnn_module_kernel=31)
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=5)
    p = PPASRPredictor(configs=cfg, state_dict=sd, vocab_list=vocab, warmup=False)
    wavs = [_audio(2.4, seed=21), _audio(1.93, seed=22)]
    pcms = [(np.clip(w, -1, 1) * 32767).astype(np.int16).tobytes() for w in wavs]
    step = 16000  # 0.5 s packets
    want = []
    for pcm in pcms:
        p.reset_stream()
        out = None
        for i in range(0, len(pcm), step):
            out = p.predict_stream(audio_data=pcm[i:i + step], is_end=(i + step >= len(pcm))) or out
        want.append(out)
    p.reset_stream()
    model = p.predictor.model
    with pytest.raises(ValueError):
        StreamPool(model, vocab, n_sessions=3, preprocess_conf=cfg["preprocess_conf"],
                   group=SqueezeformerStreamGroup(model, 2))
    grp = SqueezeformerStreamGroup(model, 2)
    pool = StreamPool(model, vocab, n_sessions=2, preprocess_conf=cfg["preprocess_conf"], group=grp)
    assert pool.group is grp
    for i in range(0, max(len(x) for x in pcms), step):
        for s, pcm in enumerate(pcms):
            if i < len(pcm):
                pool.feed(s, pcm[i:i + step])
        pool.step()
    for s in range(2):
        got = pool.finish(s)
        assert got is not None and got["text"] == want[s]["text"], s
        assert abs(got["score"] - want[s]["score"]) < 1e-3


# ---- 7. refusals and defaults ----------------------------------------------------------------------------------------
def test_other_handles_are_refused_and_the_default_stays():
    from ppasr_amd.model_utils.conformer.model import ConformerModel, StreamHandleSet, make_stream_group
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel
    V = 120
    conf = ConformerModel(80, V, streaming=True, state_dict=conformer_state_dict(vocab_size=V, num_blocks=2, seed=3),
                          encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2,
                                            cnn_module_kernel=15), device="cuda:0")
    eff = EfficientConformerModel(
        80, V, streaming=True, device="cuda:0",
        state_dict=efficient_conformer_state_dict(vocab_size=V, num_blocks=4, seed=5, stride_layer_idx=1, group_layer_idx=(0, 1)),
        encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                          cnn_module_norm="layer_norm", efficient_conf=dict(stride_layer_idx=[1], stride=[2],
                                                                            group_layer_idx=[0, 1], group_size=3,
                                                                            stride_kernel=True)))
    sq_n = _sq_model(squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=6, streaming=False), V, 4, 1, 3,
                     streaming=False)
    for m in (conf, eff, sq_n):
        with pytest.raises(_lib.PPASRHipError) as e:
            _group(m, 2)
        assert e.value.status == _lib.PPASR_EUNSUPPORTED
    sq = _sq_model(squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=7), V, 4, 1, 3)
    assert isinstance(make_stream_group(sq, 2), StreamHandleSet)
    g = ctypes.c_void_p()
    assert sq.lib.ppasr_stream_group_create(sq._h, 2, 0, ctypes.byref(g)) == _lib.PPASR_EUNSUPPORTED


# ---- 8. fp16 x3 ------------------------------------------------------------------------------------------------------
def test_f16x3_group_matches_oracle_and_handle(sq4):
    """ppasr_set_gemm_mode(F16X3): a Squeezeformer stream handle runs its split-route feed-forward slices on the fp16 x3
    route (its chunks do NOT keep fp32 arithmetic: they differ from the fp32 handle's), and the group uses the same rule --
    within 1e-3 of the float64 oracle and equal to the handle in that mode within the fp32 budget."""
    _, utts, streams, sd = sq4
    model = _sq_model(sd, 180, 4, 1, 3)
    f32_handle = model.new_stream()
    ref32 = [f32_handle.encode_chunk(utts[0][:, k * STRIDE:k * STRIDE + WINDOW], -16).cpu().numpy() for k in range(3)]
    model.set_gemm_mode("f16x3")
    fb0, _ = model.gemm_guard_stats()
    for n in (1, 3):
        g = _group(model, n)
        u = [utts[s % len(utts)] for s in range(n)]
        _drive(g, u, [0] * n, 3, 200 + n, [streams[s % len(utts)] for s in range(n)], budget=1e-3)
        g.reset()
        h = model.new_stream()
        for k in range(3):
            _, _, p = g.encode_chunks(list(range(n)), torch.cat([x[:, k * STRIDE:k * STRIDE + WINDOW] for x in u], 0),
                                      want_probs=True)
            want = h.encode_chunk(utts[0][:, k * STRIDE:k * STRIDE + WINDOW], -16)
            torch.cuda.synchronize()
            assert _rel(p[0:1].cpu().numpy(), want.cpu().numpy()) < F32_BUDGET, (n, k)
            if n == 1:
                assert not np.array_equal(want.cpu().numpy(), ref32[k])  # the mode is in effect on the handle
    # streaming chunks are never re-run: no fallbacks counted, as on handles
    fb1, _ = model.gemm_guard_stats()
    assert fb1 == fb0
