"""GPU: Squeezeformer session groups (ppasr_sq_stream_group_create + ppasr_encode_chunk_group) -- many streaming sessions
advanced with one set of launches per round.  Every session must follow its own SqueezeformerEncoder.forward_chunk
(squeezeformer/encoder.py:260-381) with the full history kept (required_cache_size < 0), whatever the other sessions in
the round are doing: against the reference-source fixtures, the float64 oracle and single stream handles.  The rounds
and what they must guarantee are tests/session_groups.py; this file holds the family's models, cases and constants."""
import ctypes

import pytest

import session_groups as sg
from numerics import oracle64
from ppasr_amd import _lib
from ppasr_amd.utils.synth import (conformer_state_dict, efficient_conformer_state_dict, squeezeformer_state_dict,
                                   synth_vocabulary)
from session_groups import STRIDE, WINDOW, OracleStream, feats

pytestmark = pytest.mark.gpu


def _sq_model(sd, V, L, red, rec, ks=31, streaming=True, **extra):
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel
    conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=L, reduce_idx=red, recover_idx=rec,
                feed_forward_expansion_factor=8, cnn_module_kernel=ks, **extra)
    return SqueezeformerModel(80, V, streaming=streaming, encoder_conf=conf, state_dict=sd, device="cuda:0")


def _group(model, n, max_frames=0):
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup
    return SqueezeformerStreamGroup(model, n, max_frames=max_frames)


# ---- 1. reference-source pin ---------------------------------------------------------------------------------------
def test_reference_source_pin_three_staggered_sessions(capsys):
    """Three sessions replay each streaming Squeezeformer fixture's utterance, started one round apart, listed in a
    different order every round: each reproduces the fixture's probs and frame counts (chunk-16 = full history).  Only
    the general layer route is outside the groups: a refused case's own stream handle is fine."""
    ran, refused = sg.reference_pin("squeezeformer", _group, {"sq_s", "sq_opt"}, (), "sq groups", capsys)
    assert {"sq_s", "sq_opt", "sq_gelu_s", "sq_pre_s", "sq_abs_s"} <= set(ran) | set(refused)


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
    utts = [feats(STRIDE * (4 + s % 3) + WINDOW, 300 + s) for s in range(5)]
    streams = [OracleStream(oracle, u.cpu()) for u in utts]
    g = _group(model, 5)
    # each round advances a different subset
    sg.drive(g, utts, [0, 1, 0, 2, 3], 12, 11, streams, subset=lambda r, s: (r + s) % 3 != 0 or s == 0)
    sg.replay_against_handles(model, _group, utts, streams, g)


# ---- 3. route thresholds ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sq4():
    V = 180
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=131, perturb_norm=True)
    model = _sq_model(sd, V, 4, 1, 3)
    oracle = oracle64("squeezeformer", sd, num_blocks=4, reduce_idx=1, recover_idx=3)
    utts = [feats(STRIDE * 3 + WINDOW, 400 + u) for u in range(5)]
    streams = [OracleStream(oracle, u.cpu()) for u in utts]
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
        worst, done = sg.drive(g, u, [0] * n, 4, 100 + n, st)
    finally:
        _set_route(model, "default")
    assert all(v == 4 for v in done.values())
    print(f"n={n} {route}: worst {worst:.2e}")


# ---- 4. state -------------------------------------------------------------------------------------------------------
def test_reset_mid_stream_matches_a_fresh_handle(sq4):
    model, utts, _, _ = sq4
    sg.reset_mid_stream(model, _group, utts[0], utts[1], fresh_chunk=0, offsets=16)


def test_refusals_leave_every_session_as_it_was(sq4):
    """A repeated session, a capacity overrun and a max_len overrun are refused with EINVAL, and the next valid call gives
    bit for bit what it gives when the refused calls were never made."""
    model, utts, _, _ = sq4
    sg.refusals_leave_state(model, _group, utts[:2], sg.REFUSED_CALLS, offsets=16)


def test_max_len_and_odd_lengths_refused_exactly_where_a_handle_refuses():
    """max_len: the chunk a single handle refuses (offset + chunk >= max_len) is the one the group refuses.  Odd cache
    lengths: chunks of odd frame counts (c = 15, 13, 1, 16, ...) on both -- the group refuses a round exactly when the
    handle refuses that chunk (with the full history the reference's trim of the reduced cache keeps every length in
    line, so neither does) and their outputs agree."""
    V = 180
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=141, perturb_norm=True)
    x = feats(64 * 6 + 67, 142)
    # offsets 0, 16, 32, 48 fit; 64 + 16 >= 72 does not
    sg.max_len_refusal(_sq_model(sd, V, 4, 1, 3, max_len=72), _group, x, tries=6, refused_at=4, offset=64)
    statuses = sg.odd_lengths(_sq_model(sd, V, 4, 1, 3), _group, x, (63, 59, 7, 67, 55, 11, 63, 67), advance_when_refused=True)
    assert statuses == [_lib.PPASR_OK] * 8, statuses


# ---- 5. workspace guard ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64])
def test_workspace_canary(sq4, n):
    model, utts, _, _ = sq4
    sg.workspace_canary(model, _group, utts, n, c=16)


# ---- 6. serving ------------------------------------------------------------------------------------------------------
def test_stream_pool_with_a_squeezeformer_group_equals_predict_stream():
    from test_predictor_gpu import _audio, _cfg
    V = 300
    cfg = _cfg(use_model="squeezeformer", L=4)
    cfg["encoder_conf"] = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=4, reduce_idx=1,
                               recover_idx=3, feed_forward_expansion_factor=8, cnn_module_kernel=31)
    sd = squeezeformer_state_dict(vocab_size=V, num_blocks=4, seed=5)
    sg.pool_equals_predict_stream(cfg, sd, synth_vocabulary(V), _group, [_audio(2.4, seed=21), _audio(1.93, seed=22)],
                                  oversize=True)


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
    sg.f16x3_group(model.new_stream(), model, _group, utts, streams)
