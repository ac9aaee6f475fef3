"""GPU: session groups on the general Conformer layer route (ppasr_gen_stream_group_create + ppasr_encode_chunk_group) --
many streaming sessions of a 512 / 768 / 1024-wide model, or of one with ConformerEncoder options the fused 256-wide
kernels do not cover, advanced with one set of launches per round.  Every session must follow its own
ConformerEncoder.forward_chunk (conformer/encoder.py:208-283) with the full history kept (required_cache_size < 0),
whatever the other sessions in the round are doing: its own keys / values, its own conv-module history and, with abs_pos,
its own positional rows.  Checked against the reference-source fixtures, the float64 oracle and single stream handles."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ref_cases as rc
from numerics import F32_BUDGET, logprob_err, oracle64
from ppasr_amd import _lib
from ppasr_amd.utils.synth import conformer_state_dict, synth_features, synth_vocabulary

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WINDOW, STRIDE = 67, 64  # predict.py:277-283: 67 frames -> 16 encoder frames per chunk

# name: (output_size, heads, layers, conv kernel, constructor options)
CONFIGS = {
    "w512": (512, 8, 2, 15, {}),
    "w768": (768, 12, 1, 15, {}),
    "w1024_small": (1024, 16, 1, 8, {}),
    "w256_abs_post": (256, 4, 2, 15, dict(pos_enc_layer_type="abs_pos", normalize_before=False)),
    "w256_k9": (256, 4, 2, 9, {}),
    "w512_nocnn_concat": (512, 8, 2, 15, dict(use_cnn_module=False, concat_after=True, macaron_style=False,
                                              pos_enc_layer_type="no_pos")),
}


def _build(cfg, V=97, seed=0, **extra):
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    D, heads, L, ks, opts = CONFIGS[cfg]
    opts = dict(opts, **extra)
    sd_keys = {k: opts[k] for k in ("pos_enc_layer_type", "macaron_style", "use_cnn_module", "concat_after") if k in opts}
    sd = conformer_state_dict(vocab_size=V, num_blocks=L, seed=300 + seed, perturb_norm=True, output_size=D,
                              attention_heads=heads, cnn_module_kernel=ks, **sd_keys)
    conf = dict(output_size=D, attention_heads=heads, linear_units=2048, num_blocks=L, cnn_module_kernel=ks, **opts)
    model = ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    oracle_opts = {k: v for k, v in opts.items() if k != "max_len"}
    oracle = oracle64("conformer", sd, num_blocks=L, causal=True, attention_heads=heads, cnn_module_kernel=ks, **oracle_opts)
    return model, oracle


def _group(model, n, max_frames=0):
    from ppasr_amd.model_utils.conformer.model import GeneralConformerStreamGroup
    return GeneralConformerStreamGroup(model, n, max_frames=max_frames)


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
    """float64 get_encoder_out_chunk of one utterance, chunk by chunk (memoised: sessions that replay an utterance share it)."""

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


def _drive(group, utts, start, rounds, order_seed, oracle_streams, subset=None):
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
            assert e_p < F32_BUDGET and e_l < F32_BUDGET, (r, s, e_p, e_l)
            assert np.array_equal(fa[k].cpu().numpy(), probs[k].argmax(-1))
            done[s] += 1
            assert group.offset(s) == off, (r, s)
    return worst, done


# ---- 1. reference-source pin ---------------------------------------------------------------------------------------
GENERAL_PIN = {"conf512", "opt_abs", "opt_nopos_post", "opt_nocnn", "act_relu6"}
REF_CASES = sorted({k.split("/")[0] for k in np.load(os.path.join(HERE, "golden", "ref_small.npz")).files
                    if "/chunk-16/" in k and rc.SMALL[k.split("/")[0]]["family"] == "conformer"})


def test_reference_source_pin_three_staggered_sessions(capsys):
    """Three sessions replay each streaming Conformer fixture's utterance, started one round apart, listed in a different
    order every round: each general-route case reproduces the fixture's probs and frame counts (chunk-16 = full
    history).  Fused-route and 6x / 8x front-end cases are refused while their stream handles still work."""
    from test_ref_pin_gpu import _make_model
    with np.load(os.path.join(HERE, "golden", "ref_small.npz")) as z:
        ref = {k: z[k] for k in z.files}
    assert GENERAL_PIN <= set(REF_CASES)
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
            assert name not in GENERAL_PIN, name
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
            if len({f.shape[1] for f in feats}) > 1:  # (a shorter last window: one call per length)
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
        print(f"\n[general groups] reference pin ran: {ran}; EUNSUPPORTED: {refused}")
    assert GENERAL_PIN <= set(ran)


# ---- 2. float64 oracle and single handles ----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_staggered_subsets_match_oracle_and_handles(cfg):
    model, oracle = _build(cfg, seed=len(cfg))
    n = 5
    utts = [_feats(STRIDE * (3 + s % 3) + WINDOW, 700 + s) for s in range(n)]
    streams = [_OracleStream(oracle, u.cpu()) for u in utts]
    g = _group(model, n)
    start = [0, 1, 0, 2, 3]
    worst, _ = _drive(g, utts, start, 10, 17, streams, subset=lambda r, s: (r + s) % 3 != 0 or s == 0)
    print(f"{cfg}: worst vs oracle {worst:.2e}")
    # single stream handles fed the same audio: the same offsets and, chunk by chunk, the same probabilities as the
    # group's sessions (a second group replays every session in lockstep)
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


# ---- 3. state -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def w512():
    model, oracle = _build("w512", seed=41)
    utts = [_feats(STRIDE * 3 + WINDOW, 800 + u) for u in range(5)]
    streams = [_OracleStream(oracle, u.cpu()) for u in utts]
    return model, utts, streams


@pytest.mark.parametrize("cfg", ["w512", "w256_abs_post"])
def test_reset_mid_stream_matches_a_fresh_handle(cfg):
    """After a reset the session's next chunk is a fresh handle's first (cache slot, history and positions start over,
    whatever its slot still holds); the other session carries on undisturbed."""
    model, _ = _build(cfg, seed=43)
    x0, x1 = _feats(STRIDE * 4 + WINDOW, 901), _feats(STRIDE * 4 + WINDOW, 902)
    g = _group(model, 2)
    for k in range(2):
        g.encode_chunks([0, 1], torch.cat([_win(x0, k), _win(x1, k)], 0))
    g.reset(0)
    assert g.offset(0) == 0 and g.offset(1) == 32
    _, _, p = g.encode_chunks([1, 0], torch.cat([_win(x1, 2), _win(x0, 3)], 0), want_probs=True)
    fresh = model.new_stream().encode_chunk(_win(x0, 3), -16)
    torch.cuda.synchronize()
    assert _rel(p[1:2].cpu().numpy(), fresh.cpu().numpy()) < F32_BUDGET
    h = model.new_stream()
    for k in range(3):
        want = h.encode_chunk(_win(x1, k), -16)
    torch.cuda.synchronize()
    assert _rel(p[0:1].cpu().numpy(), want.cpu().numpy()) < F32_BUDGET
    assert g.offset(0) == 16 and g.offset(1) == 48


def test_refusals_leave_every_session_as_it_was(w512):
    """A repeated session, an index out of range and a capacity overrun are refused with EINVAL, and the next valid calls
    give bit for bit what they give when the refused calls were never made."""
    model, utts, _ = w512
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
            assert g.offset(0) == 16 and g.offset(1) == 48
        _, _, p = g.encode_chunks([0], _win(x[0], 1), want_probs=True)
        _, _, p2 = g.encode_chunks([0], _win(x[0], 2), want_probs=True)
        runs.append((p.cpu(), p2.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_max_len_refused_exactly_where_a_handle_refuses():
    """The chunk a single handle refuses (offset + chunk >= max_len) is the one the group refuses, and nothing changes."""
    model, _ = _build("w256_abs_post", seed=45, max_len=56)
    x = _feats(STRIDE * 5 + WINDOW, 903)
    h, g = model.new_stream(), _group(model, 2)
    for k in range(5):
        chunk = _win(x, k)
        sh = _status(lambda: h.encode_chunk(chunk, -16))
        sg = _status(lambda: g.encode_chunks([1], chunk, want_probs=True))
        assert sh == sg, (k, sh, sg)
        if sh != _lib.PPASR_OK:
            break
    assert sh == _lib.PPASR_EINVAL and k == 3  # offsets 0, 16, 32 fit (32 + 16 < 56); 48 + 16 does not
    assert g.offset(1) == h.offset == 48 and g.offset(0) == 0


# ---- 4. launches ----------------------------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_the_session_count(w512):
    """A round at n = 1, 8 and 64 launches the same kernels the same number of times; k_attention once per layer, the
    per-session kernels once per layer (the front end's positional rows: none with rel_pos), nothing per session."""
    import re
    model, utts, _ = w512
    L = 2
    seen = {}
    for n in (1, 8, 64):
        g = _group(model, n)
        x = torch.cat([_win(utts[s % len(utts)], 0) for s in range(n)], 0)
        g.encode_chunks(list(range(n)), x)  # (warm: workspace allocated outside the profile)
        torch.cuda.synchronize()
        with _lib.kernel_profile() as kp:
            g.encode_chunks(list(range(n)), torch.cat([_win(utts[s % len(utts)], 1) for s in range(n)], 0))
            torch.cuda.synchronize()
        seen[n] = {}
        for k, v in kp.kernels.items():
            base = re.sub(r"<.*", "", k)
            seen[n][base] = seen[n].get(base, 0) + v[1]
        print(f"n={n}: {sum(seen[n].values())} launches {seen[n]}")
    assert seen[1] == seen[8] == seen[64]
    kinds = seen[64]
    assert sum(v for k, v in kinds.items() if "k_attention" in k) == L
    for kern in ("k_g_kv_append_group", "k_g_conv_in_group", "k_g_hist_update_group"):
        assert sum(v for k, v in kinds.items() if k.endswith(kern)) == L, (kern, kinds)
    assert not any(k.endswith("k_g_kv_append") for k in kinds)
    assert sum(kinds.values()) <= 8 + 14 * L  # (2 layers: 35 -- front end and head 7, a 512-wide layer 14)


# ---- 5. workspace ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["w512", "w256_abs_post", "w512_nocnn_concat"])
def test_round_stays_inside_its_workspace(cfg):
    GUARD, SENTINEL = 1 << 20, 0xA5
    model, _ = _build(cfg, seed=47)
    for n in (1, 64):
        g = _group(model, n, max_frames=64)
        x = torch.cat([_win(_feats(STRIDE * 2 + WINDOW, 950 + (s % 4)), 0) for s in range(n)], 0)
        need = int(model.lib.ppasr_group_chunk_workspace_bytes(model._h, n, WINDOW))
        assert need > 0
        ws = torch.full((need + GUARD,), SENTINEL, dtype=torch.uint8, device=model.device)
        g._ws = {torch.cuda.current_stream(model.device).cuda_stream: ws[:need]}
        for _ in range(2):
            _, _, p = g.encode_chunks(list(range(n)), x, want_probs=True)
        torch.cuda.synchronize()
        assert bool((ws[need:] == SENTINEL).all()), (cfg, n)
        assert bool(torch.isfinite(p).all())


# ---- 6. scale -------------------------------------------------------------------------------------------------------
def test_three_hundred_sessions_match_the_oracle(w512):
    """300 sessions x 16 frames = 4 800 stacked rows (past the 4 096-row threshold of the row-block routes) for a few
    rounds, every session against the float64 oracle of its utterance."""
    model, utts, streams = w512
    n = 300
    g = _group(model, n, max_frames=16 * 3)
    u = [utts[s % len(utts)] for s in range(n)]
    st = [streams[s % len(utts)] for s in range(n)]
    worst, done = _drive(g, u, [0] * n, 3, 300, st)
    assert all(v == 3 for v in done.values())
    print(f"n=300: worst {worst:.2e}")


# ---- 7. serving ------------------------------------------------------------------------------------------------------
def test_stream_pool_with_a_general_group_equals_predict_stream():
    from test_predictor_gpu import _audio, _cfg
    from ppasr_amd.model_utils.conformer.model import GeneralConformerStreamGroup
    from ppasr_amd.predict import PPASRPredictor
    from ppasr_amd.serving import StreamPool
    V = 300
    vocab = synth_vocabulary(V)
    cfg = _cfg(use_model="conformer", L=2)
    cfg["encoder_conf"] = dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
    sd = conformer_state_dict(vocab_size=V, num_blocks=2, seed=5, output_size=512, attention_heads=8)
    p = PPASRPredictor(configs=cfg, state_dict=sd, vocab_list=vocab, warmup=False)
    wavs = [_audio(2.4, seed=31), _audio(1.93, seed=32), _audio(3.1, seed=33)]
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
    grp = GeneralConformerStreamGroup(model, 3)
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


# ---- 8. refusals and defaults ----------------------------------------------------------------------------------------
def test_other_handles_are_refused_and_the_default_stays():
    from ppasr_amd.model_utils.conformer.model import ConformerModel, StreamHandleSet, make_stream_group
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
    from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel
    from ppasr_amd.utils.synth import (deepspeech2_state_dict, efficient_conformer_state_dict,
                                       squeezeformer_state_dict)
    V = 120

    def conformer(D, heads, streaming=True, **kw):
        sd_kw = {k: v for k, v in kw.items() if k == "input_layer"}
        sd = conformer_state_dict(vocab_size=V, num_blocks=1, seed=3, output_size=D, attention_heads=heads, **sd_kw)
        return ConformerModel(80, V, streaming=streaming, state_dict=sd, device="cuda:0",
                              encoder_conf=dict(output_size=D, attention_heads=heads, linear_units=2048, num_blocks=1,
                                                cnn_module_kernel=15, **kw))

    fused = conformer(256, 4)
    non_causal = conformer(512, 8, streaming=False)
    conv6 = conformer(512, 8, input_layer="conv2d6")
    conv8 = conformer(512, 8, input_layer="conv2d8")
    linear = conformer(512, 8, input_layer="linear")
    sq = SqueezeformerModel(80, V, streaming=True, device="cuda:0",
                            state_dict=squeezeformer_state_dict(vocab_size=V, num_blocks=3, seed=6, encoder_dim=512,
                                                                attention_heads=8),
                            encoder_conf=dict(encoder_dim=512, output_size=512, attention_heads=8, num_blocks=3,
                                              reduce_idx=1, recover_idx=2, feed_forward_expansion_factor=8,
                                              cnn_module_kernel=31))
    eff = EfficientConformerModel(
        80, V, streaming=True, device="cuda:0",
        state_dict=efficient_conformer_state_dict(vocab_size=V, num_blocks=2, seed=9, stride_layer_idx=1, group_layer_idx=(0,),
                                                  output_size=512, attention_heads=8),
        encoder_conf=dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=2, cnn_module_kernel=15,
                          cnn_module_norm="layer_norm", efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0], group_size=3,
                                              stride_kernel=True)))
    ds2 = DeepSpeech2Model(80, V, streaming=True, device="cuda:0",
                           state_dict=deepspeech2_state_dict(vocab_size=V, num_rnn_layers=1, rnn_size=1024, seed=4),
                           encoder_conf=dict(num_rnn_layers=1, rnn_size=1024, use_gru=False))
    g = ctypes.c_void_p()
    for m in (fused, non_causal, conv6, conv8, linear, sq, eff, ds2):
        assert m.lib.ppasr_gen_stream_group_create(m._h, 2, 0, ctypes.byref(g)) == _lib.PPASR_EUNSUPPORTED
        assert not g.value
    general = conformer(512, 8)
    assert general.lib.ppasr_gen_stream_group_create(general._h, 0, 0, ctypes.byref(g)) == _lib.PPASR_EINVAL
    assert not g.value
    for create in ("ppasr_stream_group_create", "ppasr_sq_stream_group_create", "ppasr_eff_stream_group_create"):
        assert getattr(general.lib, create)(general._h, 2, 0, ctypes.byref(g)) == _lib.PPASR_EUNSUPPORTED
    assert isinstance(make_stream_group(general, 2), StreamHandleSet)
    assert _group(general, 2).offset(1) == 0
