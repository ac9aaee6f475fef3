"""GPU: Efficient-Conformer session groups (ppasr_eff_stream_group_create + ppasr_encode_chunk_group) -- many streaming
sessions advanced with one set of launches per round.  Every session must follow its own
EfficientConformerEncoder.forward_chunk (efficient_conformer/encoder.py:266-393) with the full history kept
(required_cache_size < 0), whatever the other sessions in the round are doing: grouped attention re-cut from the start of
each session's own cache, the stride layer's causal context from each session's own history, 7-tap convs behind it.
Checked against the reference-source fixtures, the float64 oracle and single stream handles."""
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
WINDOW, STRIDE = 67, 64  # predict.py:277-283: 67 frames -> 16 encoder frames per chunk (8 behind a stride layer)


def _eff_model(sd, V, L, stride_idx, groups, group_size=3, streaming=True, **extra):
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel
    strides = [] if stride_idx is None else ([stride_idx] if isinstance(stride_idx, int) else list(stride_idx))
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=L, cnn_module_kernel=15,
                cnn_module_norm="layer_norm",
                efficient_conf=dict(stride_layer_idx=strides, stride=[2] * len(strides), group_layer_idx=list(groups),
                                    group_size=group_size, stride_kernel=True))
    conf.update(extra)
    return EfficientConformerModel(80, V, streaming=streaming, encoder_conf=conf, state_dict=sd, device="cuda:0")


def _sd(V, L, stride_idx, groups, group_size=3, seed=0, **kw):
    return efficient_conformer_state_dict(vocab_size=V, num_blocks=L, seed=seed, perturb_norm=True, stride_layer_idx=stride_idx,
                                          group_layer_idx=groups, group_size=group_size, **kw)


def _oracle(sd, L, stride_idx, groups, group_size=3):
    return oracle64("efficient_conformer", sd, num_blocks=L, stride_layer_idx=stride_idx, group_layer_idx=groups,
                    group_size=group_size)


def _group(model, n, max_frames=0):
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup
    return EfficientConformerStreamGroup(model, n, max_frames=max_frames)


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


def _win(x, k):
    return x[:, k * STRIDE:k * STRIDE + WINDOW]


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
        feats = torch.cat([_win(utts[s], done[s]) for s in act], 0)
        fa, fp, probs = group.encode_chunks(act, feats, want_probs=True)
        torch.cuda.synchronize()
        probs = probs.cpu().numpy()
        for k, s in enumerate(act):
            logits, off = oracle_streams[s].chunk(done[s])
            assert probs[k].shape == logits.shape, (probs[k].shape, logits.shape)
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
                    if "/chunk-16/" in k and rc.SMALL[k.split("/")[0]]["family"] == "efficient_conformer"})


def test_reference_source_pin_three_staggered_sessions(capsys):
    """Three sessions replay each streaming Efficient-Conformer fixture's utterance, started one round apart, listed in a
    different order every round: each reproduces the fixture's probs and frame counts (chunk-16 = full history).  The
    general-route fixture (output_size 512) is refused while its own stream handle still works."""
    from test_ref_pin_gpu import _make_model
    with np.load(os.path.join(HERE, "golden", "ref_small.npz")) as z:
        ref = {k: z[k] for k in z.files}
    assert {"eff_s", "eff_g4", "eff512_s"} <= set(REF_CASES)
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
            if len(lens) > 1:  # (a shorter last window: one call per length)
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
        print(f"\n[eff groups] reference pin ran: {ran}; EUNSUPPORTED: {refused}")
    assert "eff_s" in ran and "eff_g4" in ran and "eff512_s" in refused


# ---- 2. float64 oracle and single handles ----------------------------------------------------------------------------
# route: "default" = by grid size (these small rounds: the split route), "fused" = ppasr_set_ffn_split(0): the fused
# k_ffn_qkv / k_out_glu / k_conv_ffn / k_conv_ffn_stride kernels with the per-session conv histories on every layer
ROUTES = ["default", "fused"]
CONFIGS = {  # L, stride layer, grouped layers, group size
    "stride1_g3": (4, 1, (0, 1), 3),
    "stride1_g2": (3, 1, (0, 1), 2),
    "g4_behind_stride": (4, 1, (0, 2), 4),
    "groups_no_stride": (3, None, (0, 2), 3),
    "stride_no_groups": (3, 0, (), 3),
}


def _set_route(model, route):
    model.set_ffn_split(0 if route == "fused" else -1)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_staggered_subsets_match_oracle_and_handles(cfg, route):
    L, stride_idx, groups, G = CONFIGS[cfg]
    V = 180
    sd = _sd(V, L, stride_idx, groups, G, seed=70 + 3 * L + G + (stride_idx or 0))
    model = _eff_model(sd, V, L, stride_idx, groups, G)
    _set_route(model, route)
    oracle = _oracle(sd, L, stride_idx, groups, G)
    n = 5
    utts = [_feats(STRIDE * (4 + s % 3) + WINDOW, 500 + s) for s in range(n)]
    streams = [_OracleStream(oracle, u.cpu()) for u in utts]
    g = _group(model, n)
    start = [0, 1, 0, 2, 3]
    # each round advances a different subset
    _drive(g, utts, start, 12, 13, streams, subset=lambda r, s: (r + s) % 3 != 0 or s == 0)
    # single stream handles (same route setting) fed the same audio: the same offsets and, chunk by chunk, the same
    # probabilities as the group's sessions (a second group replays every session in lockstep)
    g2 = _group(model, n)
    hs = [model.new_stream() for _ in range(n)]
    for k in range(max(len(streams[s].outs) for s in range(n))):
        act = [s for s in range(n) if k < len(streams[s].outs)]
        _, _, p = g2.encode_chunks(act, torch.cat([_win(utts[s], k) for s in act], 0), want_probs=True)
        for j, s in enumerate(act):
            want = hs[s].encode_chunk(_win(utts[s], k), -16)
            torch.cuda.synchronize()
            assert _rel(p[j:j + 1].cpu().numpy(), want.cpu().numpy()) < F32_BUDGET, (k, s)
    for s in range(n):
        assert hs[s].offset == g.offset(s) == g2.offset(s), s


# ---- 3. route thresholds ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eff4():
    """4 blocks, grouped attention (group size 3) on layers 0-1, stride layer 1, 7-tap convs on layers 2-3."""
    V = 180
    sd = _sd(V, 4, 1, (0, 1), 3, seed=131)
    model = _eff_model(sd, V, 4, 1, (0, 1))
    oracle = _oracle(sd, 4, 1, (0, 1))
    utts = [_feats(STRIDE * 3 + WINDOW, 600 + u) for u in range(5)]
    streams = [_OracleStream(oracle, u.cpu()) for u in utts]
    return model, utts, streams, sd


@pytest.mark.parametrize("n,route", [(1, "default"), (3, "default"), (64, "default"), (256, "default"), (257, "default"),
                                     (512, "default"), (513, "default"), (1, "fused"), (3, "fused"), (64, "fused")])
def test_route_thresholds(eff4, n, route):
    """n x 16 full-rate rows and n x 8 half-rate rows.  By default ffn_split_for keeps up to 4 096 rows (128 row blocks)
    on the split route: n <= 256 puts every layer there; n = 257 / 512 run the full-rate layers (4 112 / 8 192 rows) on the
    fused kernels and the stride layer's feed-forward module and the half-rate layers (2 056 / 4 096 rows) on the split
    route; n = 513 runs everything fused.  route = "fused" (ppasr_set_ffn_split(0)): every layer on the fused kernels."""
    model, utts, streams, _ = eff4
    _set_route(model, route)
    try:
        g = _group(model, n, max_frames=16 * 5)
        u = [utts[s % len(utts)] for s in range(n)]
        st = [streams[s % len(utts)] for s in range(n)]
        worst, done = _drive(g, u, [0] * n, 4, 100 + n, st)
    finally:
        _set_route(model, "default")
    assert all(v == 4 for v in done.values())
    print(f"n={n} {route}: worst {worst:.2e}")


# ---- 4. state -------------------------------------------------------------------------------------------------------
def test_reset_mid_stream_matches_a_fresh_handle(eff4):
    """After a reset the session's cache slot still holds the keys of its two earlier chunks (32 frames); its fresh chunk
    has 16 key frames, so the grouped layers' tail group (frames 15 - 17) must read zeros behind frame 15, not those rows."""
    model, utts, _, _ = eff4
    g = _group(model, 2)
    x0, x1 = utts[0], utts[1]
    for k in range(2):
        g.encode_chunks([0, 1], torch.cat([_win(x0, k), _win(x1, k)], 0))
    g.reset(0)
    assert g.offset(0) == 0 and g.offset(1) == 16
    _, _, p = g.encode_chunks([1, 0], torch.cat([_win(x1, 2), _win(x0, 3)], 0), want_probs=True)
    fresh = model.new_stream().encode_chunk(_win(x0, 3), -16)
    torch.cuda.synchronize()
    assert _rel(p[1:2].cpu().numpy(), fresh.cpu().numpy()) < F32_BUDGET
    # session 1 carried on undisturbed
    h = model.new_stream()
    for k in range(3):
        want = h.encode_chunk(_win(x1, k), -16)
    torch.cuda.synchronize()
    assert _rel(p[0:1].cpu().numpy(), want.cpu().numpy()) < F32_BUDGET
    assert g.offset(0) == 8 and g.offset(1) == 24


def test_refusals_leave_every_session_as_it_was(eff4):
    """A repeated session, an index out of range and a capacity overrun are refused with EINVAL, and the next valid calls
    give bit for bit what they give when the refused calls were never made."""
    model, utts, _, _ = eff4
    x = [utts[0], utts[1]]
    runs = []
    for with_refusals in (False, True):
        g = _group(model, 2, max_frames=48)  # room for three 16-frame chunks per session
        g.encode_chunks([0, 1], torch.cat([_win(x[0], 0), _win(x[1], 0)], 0))
        g.encode_chunks([1], _win(x[1], 1))
        g.encode_chunks([1], _win(x[1], 2))  # session 1 full (48 frames), session 0 at 16
        if with_refusals:
            assert _status(lambda: g.encode_chunks([0, 0], torch.cat([_win(x[0], 1), _win(x[0], 1)], 0))) == _lib.PPASR_EINVAL
            # session 0 could advance, session 1 cannot: nothing happens to either
            assert _status(lambda: g.encode_chunks([0, 1], torch.cat([_win(x[0], 1), _win(x[1], 3)], 0))) == _lib.PPASR_EINVAL
            assert _status(lambda: g.encode_chunks([1, 0], torch.cat([_win(x[1], 3), _win(x[0], 1)], 0))) == _lib.PPASR_EINVAL
            assert _status(lambda: g.encode_chunks([2], _win(x[0], 1))) == _lib.PPASR_EINVAL
            assert _status(lambda: g.encode_chunks([-1], _win(x[0], 1))) == _lib.PPASR_EINVAL
            assert g.offset(0) == 8 and g.offset(1) == 24
        _, _, p = g.encode_chunks([0], _win(x[0], 1), want_probs=True)
        _, _, p2 = g.encode_chunks([0], _win(x[0], 2), want_probs=True)
        runs.append((p.cpu(), p2.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_max_len_and_odd_lengths_refused_exactly_where_a_handle_refuses():
    """max_len: the chunk a single handle refuses (2 offset + chunk >= max_len) is the one the group refuses.  Odd
    lengths: shorter windows with odd frame counts (c = 15, 13, 1, ...) on both -- after one the half-rate cache no longer
    lines up with the strided positional table for some next chunks; the group refuses a round exactly when the handle
    refuses that chunk, nothing changes then, and the accepted chunks agree."""
    V = 180
    sd = _sd(V, 4, 1, (0, 1), 3, seed=141)
    model = _eff_model(sd, V, 4, 1, (0, 1), max_len=72)
    x = _feats(64 * 8 + 67, 142)
    h, g = model.new_stream(), _group(model, 2)
    for k in range(6):
        chunk = _win(x, k)
        sh = _status(lambda: h.encode_chunk(chunk, -16))
        sg = _status(lambda: g.encode_chunks([1], chunk, want_probs=True))
        assert sh == sg, (k, sh, sg)
        if sh != _lib.PPASR_OK:
            break
    assert sh == _lib.PPASR_EINVAL and k == 4  # offsets 0, 8, 16, 24 fit (2 * 24 + 16 < 72); 2 * 32 + 16 does not
    assert g.offset(1) == h.offset == 32
    # odd frame counts
    model = _eff_model(sd, V, 4, 1, (0, 1))
    h, g = model.new_stream(), _group(model, 3)
    a, statuses = 0, []
    for T in (63, 63, 67, 59, 67, 7, 67, 55, 55, 67):
        chunk = x[:, a:a + T]
        out_h, out_g = [], []
        sh = _status(lambda: out_h.append(h.encode_chunk(chunk, -16)))
        sg = _status(lambda: out_g.append(g.encode_chunks([2], chunk, want_probs=True)[2]))
        assert sh == sg, (T, sh, sg)
        statuses.append(sh)
        if sh == _lib.PPASR_OK:
            a += T - 3
            torch.cuda.synchronize()
            assert _rel(out_g[0].cpu().numpy(), out_h[0].cpu().numpy()) < F32_BUDGET, T
        assert g.offset(2) == h.offset, T
    assert _lib.PPASR_EINVAL in statuses and statuses.count(_lib.PPASR_OK) >= 5, statuses


# ---- 5. workspace guard ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64])
def test_workspace_canary(eff4, n):
    model, utts, _, _ = eff4
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
    c = model.out_frames(WINDOW)
    assert c == 8
    probs = torch.empty(n, c, model.vocab_size, device="cuda:0")
    fa = torch.empty(n, c, dtype=torch.int32, device="cuda:0")
    fp = torch.empty(n, c, device="cuda:0")
    ids = (ctypes.c_int * n)(*range(n))
    c_out = ctypes.c_int(0)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        _lib.check(lib.ppasr_encode_chunk_group(g._g, ids, n, x.data_ptr(), WINDOW, probs.data_ptr(), fa.data_ptr(),
                                                fp.data_ptr(), ctypes.byref(c_out), ws.data_ptr(), need, st))
        assert c_out.value == c
    assert lib.ppasr_encode_chunk_group(g._g, ids, n, x.data_ptr(), WINDOW, probs.data_ptr(), fa.data_ptr(), fp.data_ptr(),
                                        None, ws.data_ptr(), need - 1, st) == _lib.PPASR_ENOSPACE
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all())
    assert g.offset(0) == 16


# ---- 6. serving ------------------------------------------------------------------------------------------------------
def test_stream_pool_with_an_efficient_conformer_group_equals_predict_stream():
    from test_predictor_gpu import _audio, _cfg
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup
    from ppasr_amd.predict import PPASRPredictor
    from ppasr_amd.serving import StreamPool
    V = 300
    vocab = synth_vocabulary(V)
    cfg = _cfg(use_model="efficient_conformer", L=4)
    cfg["encoder_conf"] = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                               cnn_module_norm="layer_norm",
                               efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3,
                                                   stride_kernel=True))
    sd = efficient_conformer_state_dict(vocab_size=V, num_blocks=4, seed=5, stride_layer_idx=1, group_layer_idx=(0, 1))
    p = PPASRPredictor(configs=cfg, state_dict=sd, vocab_list=vocab, warmup=False)
    wavs = [_audio(2.4, seed=21), _audio(1.93, seed=22), _audio(3.1, seed=23)]
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
        StreamPool(model, vocab, n_sessions=4, preprocess_conf=cfg["preprocess_conf"],
                   group=EfficientConformerStreamGroup(model, 3))
    grp = EfficientConformerStreamGroup(model, 3)
    pool = StreamPool(model, vocab, n_sessions=3, preprocess_conf=cfg["preprocess_conf"], group=grp)
    assert pool.group is grp
    for i in range(0, max(len(x) for x in pcms), step):
        for s, pcm in enumerate(pcms):
            if i < len(pcm):
                pool.feed(s, pcm[i:i + step])
        pool.step()
    for s in range(3):
        got = pool.finish(s)
        assert got is not None and want[s] is not None and got["text"] == want[s]["text"], s
        assert abs(got["score"] - want[s]["score"]) < 1e-3


# ---- 7. refusals and defaults ----------------------------------------------------------------------------------------
def test_other_handles_are_refused_and_the_default_stays():
    from ppasr_amd.model_utils.conformer.model import ConformerModel, StreamHandleSet, make_stream_group
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel
    V = 120
    conf = ConformerModel(80, V, streaming=True, state_dict=conformer_state_dict(vocab_size=V, num_blocks=2, seed=3),
                          encoder_conf=dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2,
                                            cnn_module_kernel=15), device="cuda:0")
    sq = SqueezeformerModel(80, V, streaming=True, device="cuda:0",
                            state_dict=squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=6),
                            encoder_conf=dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=4,
                                              reduce_idx=1, recover_idx=3, feed_forward_expansion_factor=8,
                                              cnn_module_kernel=31))
    non_causal = _eff_model(_sd(V, 3, 1, (0,), seed=7), V, 3, 1, (0,), streaming=False)
    two_strides = _eff_model(_sd(V, 4, [0, 2], (0,), seed=8), V, 4, [0, 2], (0,))
    general = _eff_model(_sd(V, 2, 1, (0,), seed=9, output_size=512, attention_heads=8), V, 2, 1, (0,),
                         output_size=512, attention_heads=8)
    for m in (conf, sq, non_causal, two_strides, general):
        with pytest.raises(_lib.PPASRHipError) as e:
            _group(m, 2)
        assert e.value.status == _lib.PPASR_EUNSUPPORTED
    g = ctypes.c_void_p()
    assert conf.lib.ppasr_eff_stream_group_create(conf._h, 0, 0, ctypes.byref(g)) == _lib.PPASR_EINVAL
    assert not g.value
    eff = _eff_model(_sd(V, 3, 1, (0, 1), seed=10), V, 3, 1, (0, 1))
    assert isinstance(make_stream_group(eff, 2), StreamHandleSet)
    for create in ("ppasr_stream_group_create", "ppasr_sq_stream_group_create"):
        assert getattr(eff.lib, create)(eff._h, 2, 0, ctypes.byref(g)) == _lib.PPASR_EUNSUPPORTED
    assert eff.lib.ppasr_eff_stream_group_create(eff._h, 0, 0, ctypes.byref(g)) == _lib.PPASR_EINVAL
    assert eff.lib.ppasr_eff_stream_group_create(eff._h, 2, 0, ctypes.byref(g)) == _lib.PPASR_OK
    assert g.value
    assert eff.lib.ppasr_stream_group_destroy(g) == _lib.PPASR_OK


# ---- 8. launches per round -------------------------------------------------------------------------------------------
@pytest.mark.skipif(bool(os.environ.get("PPASR_KCOV")), reason="conftest holds the library's kernel profile")
def test_launches_per_round_do_not_depend_on_the_session_count(eff4):
    """One round at n = 1, 8 and 64 launches the same number of kernels: the rows of all sessions are stacked into the
    same launches.  (Which form a launcher picks -- 16- or 32-row blocks, the one-chunk column split of the conv module --
    follows the stacked row count, as in the batched encoder; the number of launches does not.)"""
    from ppasr_amd._lib import kernel_profile
    model, utts, _, _ = eff4
    counts = {}
    for n in (1, 8, 64):
        g = _group(model, n)
        x = torch.cat([utts[s % len(utts)][:, :WINDOW] for s in range(n)], 0).contiguous()
        g.encode_chunks(list(range(n)), x)  # (warm: the workspace is allocated outside the profile)
        g.reset()
        torch.cuda.synchronize()
        with kernel_profile() as kp:
            g.encode_chunks(list(range(n)), x)
            torch.cuda.synchronize()
        counts[n] = {k: c for k, (_, c) in kp.kernels.items()}
        print(n, sum(counts[n].values()), sorted(counts[n].items()))
    totals = {n: sum(c.values()) for n, c in counts.items()}
    assert totals[1] == totals[8] == totals[64], totals
    L = 4
    assert totals[1] <= 16 * L, totals  # a bounded set per layer, not one per session
    for n in (1, 8, 64):  # the grouped attention: one launch per layer, whatever n
        assert sum(c for k, c in counts[n].items() if "k_attention_t" in k) == L, counts[n]
        assert sum(c for k, c in counts[n].items() if "k_conv_ffn_stride" in k) == 1, counts[n]
        assert sum(c for k, c in counts[n].items() if "k_pw1_glu_layers" in k) == 1, counts[n]


# ---- 9. fp16 x3 ------------------------------------------------------------------------------------------------------
def test_f16x3_group_matches_oracle_and_handle(eff4):
    """ppasr_set_gemm_mode(F16X3): an Efficient-Conformer stream handle runs its split-route units on the fp16 x3 route
    (its chunks differ from the fp32 handle's), and the group uses the same rule -- within 1e-3 of the float64 oracle and
    equal to the handle in that mode within the fp32 budget; no guard fallbacks are counted."""
    _, utts, streams, sd = eff4
    model = _eff_model(sd, 180, 4, 1, (0, 1))
    f32_handle = model.new_stream()
    ref32 = [f32_handle.encode_chunk(_win(utts[0], k), -16).cpu().numpy() for k in range(3)]
    model.set_gemm_mode("f16x3")
    fb0, _ = model.gemm_guard_stats()
    for n in (1, 3):
        g = _group(model, n)
        u = [utts[s % len(utts)] for s in range(n)]
        _drive(g, u, [0] * n, 3, 200 + n, [streams[s % len(utts)] for s in range(n)], budget=1e-3)
        g.reset()
        h = model.new_stream()
        for k in range(3):
            _, _, p = g.encode_chunks(list(range(n)), torch.cat([_win(x, k) for x in u], 0), want_probs=True)
            want = h.encode_chunk(_win(utts[0], k), -16)
            torch.cuda.synchronize()
            assert _rel(p[0:1].cpu().numpy(), want.cpu().numpy()) < F32_BUDGET, (n, k)
            if n == 1:
                assert not np.array_equal(want.cpu().numpy(), ref32[k])  # the mode is in effect on the handle
    fb1, _ = model.gemm_guard_stats()
    assert fb1 == fb0
