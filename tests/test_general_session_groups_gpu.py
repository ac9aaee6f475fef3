"""GPU: session groups on the general Conformer layer route (ppasr_gen_stream_group_create + ppasr_encode_chunk_group) --
many streaming sessions of a 512 / 768 / 1024-wide model, or of one with ConformerEncoder options the fused 256-wide
kernels do not cover, advanced with one set of launches per round.  Every session must follow its own
ConformerEncoder.forward_chunk (conformer/encoder.py:208-283) with the full history kept (required_cache_size < 0),
whatever the other sessions in the round are doing: its own keys / values, its own conv-module history and, with abs_pos,
its own positional rows.  Checked against the reference-source fixtures, the float64 oracle and single stream handles.  The
rounds and what they must guarantee are tests/session_groups.py; this file holds the route's models, cases and constants."""
import ctypes

import pytest
import torch

import session_groups as sg
from numerics import oracle64
from ppasr_amd import _lib
from ppasr_amd.utils.synth import conformer_state_dict, synth_vocabulary
from session_groups import STRIDE, WINDOW, OracleStream, feats, win

pytestmark = pytest.mark.gpu

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


# ---- 1. reference-source pin ---------------------------------------------------------------------------------------
GENERAL_PIN = {"conf512", "opt_abs", "opt_nopos_post", "opt_nocnn", "act_relu6"}


def test_reference_source_pin_three_staggered_sessions(capsys):
    """Three sessions replay each streaming Conformer fixture's utterance, started one round apart, listed in a different
    order every round: each general-route case reproduces the fixture's probs and frame counts (chunk-16 = full
    history).  Fused-route and 6x / 8x front-end cases are refused while their stream handles still work."""
    sg.reference_pin("conformer", _group, GENERAL_PIN, (), "general groups", capsys)


# ---- 2. float64 oracle and single handles ----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_staggered_subsets_match_oracle_and_handles(cfg):
    model, oracle = _build(cfg, seed=len(cfg))
    utts = [feats(STRIDE * (3 + s % 3) + WINDOW, 700 + s) for s in range(5)]
    streams = [OracleStream(oracle, u.cpu()) for u in utts]
    g = _group(model, 5)
    worst, _ = sg.drive(g, utts, [0, 1, 0, 2, 3], 10, 17, streams, subset=lambda r, s: (r + s) % 3 != 0 or s == 0)
    print(f"{cfg}: worst vs oracle {worst:.2e}")
    sg.replay_against_handles(model, _group, utts, streams, g)


# ---- 3. state -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def w512():
    model, oracle = _build("w512", seed=41)
    utts = [feats(STRIDE * 3 + WINDOW, 800 + u) for u in range(5)]
    streams = [OracleStream(oracle, u.cpu()) for u in utts]
    return model, utts, streams


@pytest.mark.parametrize("cfg", ["w512", "w256_abs_post"])
def test_reset_mid_stream_matches_a_fresh_handle(cfg):
    """After a reset the session's next chunk is a fresh handle's first (cache slot, history and positions start over,
    whatever its slot still holds); the other session carries on undisturbed."""
    model, _ = _build(cfg, seed=43)
    sg.reset_mid_stream(model, _group, feats(STRIDE * 4 + WINDOW, 901), feats(STRIDE * 4 + WINDOW, 902), fresh_chunk=3,
                        offsets=16)


def test_refusals_leave_every_session_as_it_was(w512):
    """A repeated session, an index out of range and a capacity overrun are refused with EINVAL, and the next valid calls
    give bit for bit what they give when the refused calls were never made."""
    model, utts, _ = w512
    sg.refusals_leave_state(model, _group, utts[:2], sg.REFUSED_CALLS + [sg.REFUSED_NEGATIVE], offsets=16)


def test_max_len_refused_exactly_where_a_handle_refuses():
    """The chunk a single handle refuses (offset + chunk >= max_len) is the one the group refuses, and nothing changes."""
    model, _ = _build("w256_abs_post", seed=45, max_len=56)
    # offsets 0, 16, 32 fit (32 + 16 < 56); 48 + 16 does not
    sg.max_len_refusal(model, _group, feats(STRIDE * 5 + WINDOW, 903), tries=5, refused_at=3, offset=48)


# ---- 4. launches ----------------------------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_the_session_count(w512):
    """A round at n = 1, 8 and 64 launches the same kernels the same number of times; k_attention once per layer, the
    per-session kernels once per layer (the front end's positional rows: none with rel_pos), nothing per session."""
    model, utts, _ = w512
    L = 2
    seen = {}
    for n in (1, 8, 64):
        g = _group(model, n)
        x = torch.cat([win(utts[s % len(utts)], 0) for s in range(n)], 0)
        g.encode_chunks(list(range(n)), x)  # (warm: workspace allocated outside the profile)
        torch.cuda.synchronize()
        x = torch.cat([win(utts[s % len(utts)], 1) for s in range(n)], 0)
        seen[n] = sg.launches_by_kernel(lambda: g.encode_chunks(list(range(n)), x), strip=r"<.*")
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
        x = torch.cat([win(feats(STRIDE * 2 + WINDOW, 950 + (s % 4)), 0) for s in range(n)], 0)
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
    worst, done = sg.drive(g, u, [0] * n, 3, 300, st)
    assert all(v == 3 for v in done.values())
    print(f"n=300: worst {worst:.2e}")


# ---- 7. serving ------------------------------------------------------------------------------------------------------
def test_stream_pool_with_a_general_group_equals_predict_stream():
    from test_predictor_gpu import _audio, _cfg
    V = 300
    cfg = _cfg(use_model="conformer", L=2)
    cfg["encoder_conf"] = dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
    sd = conformer_state_dict(vocab_size=V, num_blocks=2, seed=5, output_size=512, attention_heads=8)
    sg.pool_equals_predict_stream(cfg, sd, synth_vocabulary(V), _group,
                                  [_audio(2.4, seed=31), _audio(1.93, seed=32), _audio(3.1, seed=33)], oversize=False)


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
