"""GPU: DeepSpeech2 session groups (ppasr_ds2_stream_group_create + ppasr_encode_chunk_group) -- many streaming sessions
advanced with one set of launches per round.  Every session must follow CRNNEncoder.forward (deepspeech2/encoder.py:61-104)
on its windows with its own state boxes carried between calls (what InferencePredictor.predict_chunk_deepspeech does,
inference_predictor.py:147-182), whatever the other sessions in the round are doing.  Checked against the
reference-source fixtures, the batched call bit for bit, and the float64 oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ref_cases as rc
from numerics import F32_BUDGET_DS2, oracle64, rel
from ppasr_amd import _lib
from ppasr_amd.utils.synth import deepspeech2_state_dict, synth_features, synth_vocabulary
from session_groups import predict_stream_reference, status_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WINDOW = 67  # predict.py:277-283: 67 frames -> 16 output frames per window


def _model(V, L, H=1024, gru=False, seed=0, streaming=True):
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
    sd = deepspeech2_state_dict(vocab_size=V, num_rnn_layers=L, rnn_size=H, streaming=streaming, seed=seed, perturb_norm=True,
                                use_gru=gru)
    model = DeepSpeech2Model(80, V, streaming=streaming, encoder_conf=dict(num_rnn_layers=L, rnn_size=H, use_gru=gru),
                             state_dict=sd, device="cuda:0")
    return model, sd


def _group(model, n):
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2StreamGroup
    return DeepSpeech2StreamGroup(model, n)


def _feats(n, T, seed):
    return torch.from_numpy(synth_features(n, T, seed=seed)[0]).cuda()


def _check_frames(fa, fp, probs):
    """frame argmax / max-prob are taken from the returned probabilities (first maximum wins)."""
    p = probs.cpu()
    assert torch.equal(fa.cpu().long(), p.argmax(-1))
    assert torch.equal(fp.cpu(), p.max(-1).values)


# ---- 1. reference-source pin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ds2_s", "ds2g_s"])
def test_reference_source_three_sessions(name):
    """The fixture's 3 utterances as 3 sessions of one group, listed in a different order every round (rc.windows, the
    last one shorter): probs and per-round frame counts as the reference's CRNNEncoder gave them.  The final states are
    checked through one more window: from them the group must give what the batched call gives from the fixture's h / c
    boxes."""
    from test_ref_pin_gpu import _make_model
    with np.load(os.path.join(HERE, "golden", "ref_small.npz")) as z:
        ref = {k: z[k] for k in z.files if k.startswith(name + "/chunk/")}
    case = rc.SMALL[name]
    gru = case["kw"].get("use_gru", False)
    model = _make_model(case, rc.state_dict(case))
    xc = torch.from_numpy(rc.chunk_features(case)).cuda()
    group = _group(model, 3)
    outs, counts = [[] for _ in range(3)], []
    for r, (a, b) in enumerate(rc.windows(xc.shape[1])):
        order = [(r + k) % 3 for k in range(3)]
        fa, fp, probs = group.encode_chunks(order, xc[order, a:b], want_probs=True)
        _check_frames(fa, fp, probs)
        counts.append(int(probs.shape[1]))
        for k, s in enumerate(order):
            outs[s].append(probs[k].cpu().numpy())
    assert counts == ref[f"{name}/chunk/n"].tolist()
    got = np.stack([np.concatenate(o, 0) for o in outs])
    e_p = rel(got, ref[f"{name}/chunk/probs"])
    assert e_p < F32_BUDGET_DS2, e_p
    assert [group.offset(s) for s in range(3)] == [sum(counts)] * 3
    nxt = _feats(3, WINDOW, seed=77)
    _, _, p_group = group.encode_chunks([0, 1, 2], nxt, want_probs=True)
    h = torch.from_numpy(ref[f"{name}/chunk/h"]).cuda()
    c = torch.from_numpy(ref[f"{name}/chunk/c"]).cuda()
    p_ref, _, _, _ = model.get_encoder_out_chunk(nxt, np.full(3, WINDOW, np.int64), h, c)
    e_s = rel(p_group.cpu().numpy(), p_ref.cpu().numpy())
    print(f"{name} ({'GRU' if gru else 'LSTM'}): probs {e_p:.2e}, next window from the final states {e_s:.2e}")
    assert e_s < F32_BUDGET_DS2


# ---- 2. bit for bit against the batched call -----------------------------------------------------------------------
@pytest.mark.parametrize("H,n", [(1024, 4), (1024, 33), (1024, 64), (1024, 130), (2048, 4), (2048, 64)])
@pytest.mark.parametrize("gru", [False, True])
def test_round_is_the_batched_call_bit_for_bit(H, n, gru):
    """Two rounds of n sessions (scattered, shuffled slots of a larger group) against get_encoder_out_chunk on the stacked
    windows: the first from zero states, the second from the first batched call's final boxes.  B >= 4 takes the
    wavefront route there, which the group runs for every n: probabilities identical bit for bit, frame argmax / max-prob
    taken from them."""
    V, L = 61, 3 if H == 1024 else 2
    model, _ = _model(V, L, H, gru, seed=600 + n + H // 1024 + 7 * gru)
    N = n + 5
    slots = [int(s) for s in np.random.default_rng(n).permutation(N)[:n]]
    group = _group(model, N)
    lens = np.full(n, WINDOW, np.int64)
    h = c = None
    for r in range(2):
        x = _feats(n, WINDOW, seed=700 + 10 * n + r)
        fa, fp, probs = group.encode_chunks(slots, x, want_probs=True)
        p_ref, _, h, c = model.get_encoder_out_chunk(x, lens, h, c)
        torch.cuda.synchronize()
        assert torch.equal(probs, p_ref), (r, float((probs - p_ref).abs().max()))
        _check_frames(fa, fp, probs)
    assert all(group.offset(s) == 32 for s in slots)
    assert all(group.offset(s) == 0 for s in set(range(N)) - set(slots))


# ---- 3. float64 oracle, staggered subsets --------------------------------------------------------------------------
ROUNDS = [([0, 1, 2, 3, 4, 5], 67), ([2], 67), ([4, 0], 67), ([5, 1, 3], 67), ([0, 2, 4, 5], 67), ([3], 40),
          ([1, 5], 67), ([5, 4, 3, 2, 1, 0], 67), ([0, 2], 23)]


@pytest.mark.parametrize("gru", [False, True])
def test_staggered_subsets_against_the_float64_oracle(gru):
    """6 sessions, each round a different subset in a shuffled order (n = 1 .. 6), shorter last windows (finish): every
    session against its own chained float64 CRNNEncoder.  A session not listed in a round is untouched (its next round
    still matches)."""
    V, L = 53, 3
    model, sd = _model(V, L, 1024, gru, seed=811)
    oracle = oracle64("deepspeech2", sd, num_rnn_layers=L, rnn_size=1024, streaming=True, use_gru=gru)
    group = _group(model, 6)
    rng = np.random.default_rng(812)
    state = {s: (None, None) for s in range(6)}
    frames = {s: 0 for s in range(6)}
    worst = 0.0
    for r, (act, T) in enumerate(ROUNDS):
        act = [act[i] for i in rng.permutation(len(act))]
        x = _feats(len(act), T, seed=820 + r)
        fa, fp, probs = group.encode_chunks(act, x, want_probs=True)
        torch.cuda.synchronize()
        _check_frames(fa, fp, probs)
        for k, s in enumerate(act):
            rp, rl, rh, rc_ = oracle.forward(x[k:k + 1].cpu().double(), np.array([T]), *state[s])
            state[s] = (rh, rc_)
            e = rel(probs[k].cpu().numpy(), rp[0].numpy())
            worst = max(worst, e)
            assert e < F32_BUDGET_DS2, (r, s, e)
            frames[s] += int(rl[0])
            assert group.offset(s) == frames[s], (r, s)
    print(f"gru={gru}: worst probs error {worst:.2e}")


# ---- 4. reset and refusals -----------------------------------------------------------------------------------------
def test_reset_and_refusals():
    V, L = 47, 2
    model, sd = _model(V, L, 1024, False, seed=901)
    oracle = oracle64("deepspeech2", sd, num_rnn_layers=L, rnn_size=1024, streaming=True)
    group = _group(model, 3)
    state = {s: (None, None) for s in range(3)}

    def advance(act, T, seed):
        x = _feats(len(act), T, seed=seed)
        _, _, probs = group.encode_chunks(act, x, want_probs=True)
        torch.cuda.synchronize()
        for k, s in enumerate(act):
            rp, _, rh, rc_ = oracle.forward(x[k:k + 1].cpu().double(), np.array([T]), *state[s])
            state[s] = (rh, rc_)
            assert rel(probs[k].cpu().numpy(), rp[0].numpy()) < F32_BUDGET_DS2, s

    advance([0, 1, 2], WINDOW, 902)
    # reset(1): session 1 starts again from zero state, the others go on
    group.reset(1)
    state[1] = (None, None)
    assert [group.offset(s) for s in range(3)] == [16, 0, 16]
    advance([2, 1, 0], WINDOW, 903)
    # refusals: create on a bidirectional handle; the other families' create calls on a streaming DeepSpeech2 handle
    lib = model.lib
    g = ctypes.c_void_p()
    bi, _ = _model(V, L, 1024, False, seed=904, streaming=False)
    assert lib.ppasr_ds2_stream_group_create(bi._h, 2, 0, ctypes.byref(g)) == _lib.PPASR_EUNSUPPORTED and not g.value
    for sym in ("ppasr_stream_group_create", "ppasr_sq_stream_group_create", "ppasr_eff_stream_group_create"):
        assert getattr(lib, sym)(model._h, 2, 0, ctypes.byref(g)) == _lib.PPASR_EUNSUPPORTED and not g.value, sym
    assert lib.ppasr_ds2_stream_group_create(model._h, 0, 0, ctypes.byref(g)) == _lib.PPASR_EINVAL and not g.value
    # refused rounds change no session
    x2 = _feats(2, WINDOW, seed=905)
    assert status_of(lambda: group.encode_chunks([0, 0], x2)) == _lib.PPASR_EINVAL
    assert status_of(lambda: group.encode_chunks([0, 3], x2)) == _lib.PPASR_EINVAL
    assert status_of(lambda: group.encode_chunks([-1, 1], x2)) == _lib.PPASR_EINVAL
    x6 = _feats(2, 6, seed=906)
    ids = (ctypes.c_int * 2)(0, 1)
    ws = torch.empty(int(lib.ppasr_group_chunk_workspace_bytes(model._h, 2, WINDOW)), dtype=torch.uint8, device="cuda")
    fa = torch.empty(2, 16, dtype=torch.int32, device="cuda")
    fp = torch.empty(2, 16, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.ppasr_encode_chunk_group(group._g, ids, 2, x6.data_ptr(), 6, None, fa.data_ptr(), fp.data_ptr(), None,
                                        ws.data_ptr(), ws.numel(), stream) == _lib.PPASR_EINVAL
    assert lib.ppasr_encode_chunk_group(group._g, ids, 2, x2.data_ptr(), WINDOW, None, fa.data_ptr(), fp.data_ptr(), None,
                                        ws.data_ptr(), ws.numel() - 1, stream) == _lib.PPASR_ENOSPACE
    assert [group.offset(s) for s in range(3)] == [32, 16, 32]
    advance([1, 0, 2], WINDOW, 907)
    # reset of every session
    group.reset()
    state = {s: (None, None) for s in range(3)}
    assert [group.offset(s) for s in range(3)] == [0, 0, 0]
    advance([0, 2], WINDOW, 908)


# ---- 5. StreamPool end to end --------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder,scorer", [("ctc_greedy", False), ("ctc_beam_search", False), ("ctc_beam_search", True)])
def test_stream_pool_equals_predict_stream(tmp_path, decoder, scorer):
    """3 staggered PCM streams through StreamPool on a DeepSpeech2 model (make_stream_group's choice: the session group):
    each session's text equals its own PPASRPredictor.predict_stream, its score within 1e-4 relative."""
    from lm_util import write_synthetic_arpa
    from test_predictor_gpu import _audio, _cfg
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2StreamGroup
    from ppasr_amd.serving import StreamPool
    V = 300
    vocab = synth_vocabulary(V)
    cfg = _cfg(use_model="deepspeech2", decoder=decoder)
    sd = deepspeech2_state_dict(vocab_size=V, num_rnn_layers=2, streaming=True, seed=7)
    conf = cfg["ctc_beam_search_decoder_conf"]
    if scorer:
        conf["language_model_path"] = write_synthetic_arpa(str(tmp_path / "lm.arpa"), vocab[2:150], order=3, seed=6)
    n = 3
    p, pcms, want = predict_stream_reference(cfg, sd, vocab, [_audio(2.4, seed=21), _audio(1.93, seed=22), _audio(3.1, seed=23)])
    step = 16000  # 0.5 s packets
    model = p.predictor.model
    kw = dict(decoder="ctc_beam_search", decoder_conf=dict(conf)) if decoder == "ctc_beam_search" else {}
    pool = StreamPool(model, vocab, n_sessions=n, preprocess_conf=cfg["preprocess_conf"], **kw)
    assert isinstance(pool.group, DeepSpeech2StreamGroup)
    for i in range(0, max(len(x) for x in pcms) + step, step):
        for s, pcm in enumerate(pcms):
            j = i - step if s == 2 else i  # session 2 starts one packet late
            if 0 <= j < len(pcm):
                pool.feed(s, pcm[j:j + step])
        pool.step()
    got = [pool.finish(s) for s in range(n)]
    for s in range(n):
        assert want[s] is not None and got[s]["text"] == want[s]["text"], (s, got[s], want[s])
        assert abs(got[s]["score"] - want[s]["score"]) <= 1e-4 * max(1.0, abs(want[s]["score"])), (s, got[s], want[s])
    pool.reset(0)
    assert pool.group.offset(0) == 0 and pool.sessions[0].result is None


# ---- 6. launches do not scale with n -------------------------------------------------------------------------------
@pytest.mark.parametrize("gru", [False, True])
def test_launches_do_not_depend_on_the_session_count(gru):
    """One round at n = 1, 64 and 256: the same kernels with the same launch counts, no persistent recurrence.  The one
    exception is launch_dense's K-split join of the CTC head, which ppasr_ds2_encode's route adds when the stacked frames
    are few (<= 512: n = 1 here) -- at most one launch."""
    model, _ = _model(47, 3, 1024, gru, seed=1001)
    group = _group(model, 256)
    seen = {}
    for n in (1, 64, 256):
        x = _feats(n, WINDOW, seed=1002 + n)
        group.encode_chunks(list(range(n)), x)  # (warm: workspace allocated outside the profile)
        torch.cuda.synchronize()
        with _lib.kernel_profile() as kp:
            group.encode_chunks(list(range(n)), x)
            torch.cuda.synchronize()
        print(f"n={n}: {sum(v[1] for v in kp.kernels.values())} launches {sorted(kp.kernels)}")
        seen[n] = {}
        for k, v in kp.kernels.items():  # (template arguments dropped: k_lstm_wave takes 1 row tile per workgroup up to 32 rows)
            base = re.sub(r"<[^<>]*>", "", k)
            seen[n][base] = seen[n].get(base, 0) + v[1]
    for n in seen:
        assert not any("k_lstm_persist" in k for k in seen[n]), n
        assert sum(v for k, v in seen[n].items() if "k_lstm_wave" in k) == 16 + 3 - 1
        for kern in ("k_ds2_state_gather", "k_ds2_state_scatter"):
            assert sum(v for k, v in seen[n].items() if kern in k) == 1, (n, kern, seen[n])
    assert seen[64] == seen[256]
    small = {k: v for k, v in seen[1].items() if "k_dense_join" not in k}
    assert small == seen[64] and sum(seen[1].values()) - sum(seen[64].values()) <= 1
