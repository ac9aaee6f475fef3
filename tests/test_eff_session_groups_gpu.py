"""GPU: Efficient-Conformer session groups (ppasr_eff_stream_group_create + ppasr_encode_chunk_group) -- many streaming
sessions advanced with one set of launches per round.  Every session must follow its own
EfficientConformerEncoder.forward_chunk (efficient_conformer/encoder.py:266-393) with the full history kept
(required_cache_size < 0), whatever the other sessions in the round are doing: grouped attention re-cut from the start of
each session's own cache, the stride layer's causal context from each session's own history, 7-tap convs behind it.
Checked against the reference-source fixtures, the float64 oracle and single stream handles.  The rounds and what they
must guarantee are tests/session_groups.py; this file holds the family's models, cases and constants."""
import ctypes
import os

import pytest
import torch

import session_groups as sg
from numerics import oracle64
from ppasr_amd import _lib
from ppasr_amd.utils.synth import (conformer_state_dict, efficient_conformer_state_dict, squeezeformer_state_dict,
                                   synth_vocabulary)
from session_groups import STRIDE, WINDOW, OracleStream, feats

pytestmark = pytest.mark.gpu


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


# ---- 1. reference-source pin ---------------------------------------------------------------------------------------
def test_reference_source_pin_three_staggered_sessions(capsys):
    """Three sessions replay each streaming Efficient-Conformer fixture's utterance, started one round apart, listed in a
    different order every round: each reproduces the fixture's probs and frame counts (chunk-16 = full history).  The
    general-route fixture (output_size 512) is refused while its own stream handle still works."""
    sg.reference_pin("efficient_conformer", _group, {"eff_s", "eff_g4"}, {"eff512_s"}, "eff groups", capsys)


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
    utts = [feats(STRIDE * (4 + s % 3) + WINDOW, 500 + s) for s in range(5)]
    streams = [OracleStream(oracle, u.cpu()) for u in utts]
    g = _group(model, 5)
    # each round advances a different subset
    sg.drive(g, utts, [0, 1, 0, 2, 3], 12, 13, streams, subset=lambda r, s: (r + s) % 3 != 0 or s == 0)
    sg.replay_against_handles(model, _group, utts, streams, g)


# ---- 3. route thresholds ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eff4():
    """4 blocks, grouped attention (group size 3) on layers 0-1, stride layer 1, 7-tap convs on layers 2-3."""
    V = 180
    sd = _sd(V, 4, 1, (0, 1), 3, seed=131)
    model = _eff_model(sd, V, 4, 1, (0, 1))
    oracle = _oracle(sd, 4, 1, (0, 1))
    utts = [feats(STRIDE * 3 + WINDOW, 600 + u) for u in range(5)]
    streams = [OracleStream(oracle, u.cpu()) for u in utts]
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
        worst, done = sg.drive(g, u, [0] * n, 4, 100 + n, st)
    finally:
        _set_route(model, "default")
    assert all(v == 4 for v in done.values())
    print(f"n={n} {route}: worst {worst:.2e}")


# ---- 4. state -------------------------------------------------------------------------------------------------------
def test_reset_mid_stream_matches_a_fresh_handle(eff4):
    """After a reset the session's cache slot still holds the keys of its two earlier chunks (32 frames); its fresh chunk
    has 16 key frames, so the grouped layers' tail group (frames 15 - 17) must read zeros behind frame 15, not those rows."""
    model, utts, _, _ = eff4
    sg.reset_mid_stream(model, _group, utts[0], utts[1], fresh_chunk=3, offsets=8)


def test_refusals_leave_every_session_as_it_was(eff4):
    """A repeated session, an index out of range and a capacity overrun are refused with EINVAL, and the next valid calls
    give bit for bit what they give when the refused calls were never made."""
    model, utts, _, _ = eff4
    sg.refusals_leave_state(model, _group, utts[:2], sg.REFUSED_CALLS + [sg.REFUSED_NEGATIVE], offsets=8)


def test_max_len_and_odd_lengths_refused_exactly_where_a_handle_refuses():
    """max_len: the chunk a single handle refuses (2 offset + chunk >= max_len) is the one the group refuses.  Odd
    lengths: shorter windows with odd frame counts (c = 15, 13, 1, ...) on both -- after one the half-rate cache no longer
    lines up with the strided positional table for some next chunks; the group refuses a round exactly when the handle
    refuses that chunk, nothing changes then, and the accepted chunks agree."""
    V = 180
    sd = _sd(V, 4, 1, (0, 1), 3, seed=141)
    x = feats(64 * 8 + 67, 142)
    # offsets 0, 8, 16, 24 fit (2 * 24 + 16 < 72); 2 * 32 + 16 does not
    sg.max_len_refusal(_eff_model(sd, V, 4, 1, (0, 1), max_len=72), _group, x, tries=6, refused_at=4, offset=32)
    statuses = sg.odd_lengths(_eff_model(sd, V, 4, 1, (0, 1)), _group, x, (63, 63, 67, 59, 67, 7, 67, 55, 55, 67),
                              advance_when_refused=False)
    assert _lib.PPASR_EINVAL in statuses and statuses.count(_lib.PPASR_OK) >= 5, statuses


# ---- 5. workspace guard ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64])
def test_workspace_canary(eff4, n):
    model, utts, _, _ = eff4
    assert model.out_frames(WINDOW) == 8
    sg.workspace_canary(model, _group, utts, n, c=8, check_c_out=True)


# ---- 6. serving ------------------------------------------------------------------------------------------------------
def test_stream_pool_with_an_efficient_conformer_group_equals_predict_stream():
    from test_predictor_gpu import _audio, _cfg
    V = 300
    cfg = _cfg(use_model="efficient_conformer", L=4)
    cfg["encoder_conf"] = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                               cnn_module_norm="layer_norm",
                               efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3,
                                                   stride_kernel=True))
    sd = efficient_conformer_state_dict(vocab_size=V, num_blocks=4, seed=5, stride_layer_idx=1, group_layer_idx=(0, 1))
    sg.pool_equals_predict_stream(cfg, sd, synth_vocabulary(V), _group,
                                  [_audio(2.4, seed=21), _audio(1.93, seed=22), _audio(3.1, seed=23)], oversize=True)


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
    model, utts, _, _ = eff4
    counts = {}
    for n in (1, 8, 64):
        g = _group(model, n)
        x = torch.cat([utts[s % len(utts)][:, :WINDOW] for s in range(n)], 0).contiguous()
        g.encode_chunks(list(range(n)), x)  # (warm: the workspace is allocated outside the profile)
        g.reset()
        torch.cuda.synchronize()
        counts[n] = sg.launches_by_kernel(lambda: g.encode_chunks(list(range(n)), x))
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
    sg.f16x3_group(model.new_stream(), model, _group, utts, streams)
