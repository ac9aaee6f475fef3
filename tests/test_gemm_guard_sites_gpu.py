"""GPU: the fp16 x3 mode's range guard at EVERY GEMM input it covers (tests/guard_sites.py: the site table, the recipes
and their CPU isolation check), the refusal of weights and positional-table entries that do not fit the fp16 pieces, and
the balanced power-of-two rescaling case.

Per site, route and setting:
  push, guard on, batched    the call counts one fallback and > 0 events and returns logits, probabilities and greedy
                             tokens BYTE-identical to the same handle in "f32" mode; the handle is still in the mode
                             afterwards (the guard-off call right behind it saturates and counts again)
  push, guard off, batched   events rise, fallbacks do not, finite output (NOT required to differ from fp32: the pushed
                             channel meets a zero weight, which hides the saturated value)
  push, stream / group       events are counted, nothing is run again (no fallback, no fp32 form of the kernel), finite
  control                    no event, no fallback, bytes different from "f32" mode (the mode ran), per-utterance
                             utt_rel / logprob_err against the float64 oracle within F32_BUDGET, frame_ids_ok; a second
                             call returns the same bytes.  This is the large-operand case: an activation of 3 000 through
                             the 2^4 / 2^8 / 2^-12 scaling.
A recipe pushes through the CHECKPOINT, so no input of a pushed handle is in range: "an in-range call after a fallback
returns the mode's own bytes" is asserted where the features drive the range (tests/test_gemm_mode_gpu.py, conv2 input).
The intended <.., true> / _h3 kernels are confirmed through kernel_profile.  Every case prints events, fallbacks and errors."""
import numpy as np
import pytest
import torch

import guard_sites as gs
import numerics as nm
from ppasr_amd import _lib
from ppasr_amd._lib import kernel_profile

pytestmark = pytest.mark.gpu
_LAST = {}  # the handles and references of the recipe being run (one recipe at a time: its routes share them)


def _fixture(family, site, layer):
    key = (family, site, layer)
    if _LAST.get("key") != key:
        _LAST.clear()
        torch.cuda.empty_cache()
        _LAST["key"] = key
        _LAST["push"] = gs.make_model(family, gs.edited(family, site, layer, gs.PUSH))
        sd_c = gs.edited(family, site, layer, gs.CONTROL)
        _LAST["control"] = gs.make_model(family, sd_c)
        _LAST["oracle"] = gs.make_oracle64(family, sd_c)
        _LAST["memo"] = nm.Memo()
    return _LAST


def _np(t):
    return t.cpu().numpy()


def _batched(m):
    x, lens = gs.batch_features()
    probs, logits = m.get_encoder_out(x, lens, return_logits=True)
    torch.cuda.synchronize()
    return _np(probs), _np(logits)


def _greedy(m):
    x, lens = gs.batch_features()
    tokens, n, _ = m.encode_greedy(x, lens)
    torch.cuda.synchronize()
    return _np(tokens), _np(n)


def _batched_case(fx, family, site, layer, route, what):
    push, ctl = fx["push"], fx["control"]
    expect = gs.expected_kernels(family, site, layer, route)
    # ---- push ----
    gs.set_route(push, route)
    push.set_gemm_mode("f32")
    p32, l32 = _batched(push)
    t32, n32 = _greedy(push)
    assert np.isfinite(l32).all() and np.isfinite(p32).all()
    push.set_gemm_mode("f16x3")
    assert "layers" in push.gemm_coverage()
    push.set_gemm_guard(True)
    f0, e0 = push.gemm_guard_stats()
    with kernel_profile() as kp:
        ph, lh = _batched(push)
    f1, e1 = push.gemm_guard_stats()
    assert gs.launched(kp.kernels, expect), (expect, sorted(kp.kernels))
    th, nh = _greedy(push)
    f2, e2 = push.gemm_guard_stats()
    print(f"[guard] {what} push, guard on: fallbacks +{f1 - f0} +{f2 - f1}, events +{e1 - e0} +{e2 - e1}")
    assert f1 - f0 == 1 and e1 > e0, (f0, e0, f1, e1)
    assert np.array_equal(lh, l32) and np.array_equal(ph, p32)
    assert f2 - f1 == 1 and e2 > e1
    assert np.array_equal(th, t32) and np.array_equal(nh, n32)
    push.set_gemm_guard(False)
    ps, ls = _batched(push)
    f3, e3 = push.gemm_guard_stats()
    push.set_gemm_guard(True)
    print(f"[guard] {what} push, guard off: fallbacks +{f3 - f2}, events +{e3 - e2}")
    assert f3 == f2 and e3 > e2  # (the fallback left the handle in the mode: its kernels counted again)
    assert np.isfinite(ls).all() and np.isfinite(ps).all()
    push.set_gemm_mode("f32")
    # ---- control ----
    gs.set_route(ctl, route)
    ctl.set_gemm_mode("f32")
    _, c32 = _batched(ctl)
    ctl.set_gemm_mode("f16x3")
    f0, e0 = ctl.gemm_guard_stats()
    with kernel_profile() as kp:
        pc, lc = _batched(ctl)
    assert gs.launched(kp.kernels, expect), (expect, sorted(kp.kernels))
    _, lc2 = _batched(ctl)
    f1, e1 = ctl.gemm_guard_stats()
    ctl.set_gemm_mode("f32")
    x, lens = gs.batch_features()
    ref = fx["memo"].get("batched", lambda: fx["oracle"].get_encoder_out(x, lens, return_logits=True)[1])
    errs = (nm.utt_rel(lc, ref), nm.logprob_err(pc, ref))
    e32 = nm.utt_rel(c32, ref)
    ok, near = nm.frame_ids_ok(lc, ref, nm.F32_BUDGET)
    print(f"[guard] {what} control: fallbacks +{f1 - f0}, events +{e1 - e0}, logits {errs[0]:.2e} logprobs {errs[1]:.2e} "
          f"(f32 mode: {e32:.2e}) near-ties {near}")
    assert (f1, e1) == (f0, e0)
    assert not np.array_equal(lc, c32) and np.array_equal(lc, lc2)
    assert max(errs) < nm.F32_BUDGET, errs
    assert ok


def _ref_chunks(fx, session, x, wins):
    def run():
        att = cnn = None
        off = 0
        out = []
        with torch.no_grad():
            for a, b in wins:
                xs, att, cnn = fx["oracle"].forward_chunk(x[session:session + 1, a:b], off, -16, att, cnn)
                out.append(fx["oracle"].ctc_logits(xs))
                off += xs.shape[1]
        return out
    return fx["memo"].get(("chunks", session), run)


def _stream_rounds(m, route, x, wins):
    """-> per chunk, probabilities [sessions, c, V] of a stream handle (session 0) or a two-session group"""
    if route == gs.STREAM:
        s = m.new_stream()
        out = [_np(s.encode_chunk(x[:1, a:b], -16)) for a, b in wins]
    else:
        from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup
        grp = ConformerStreamGroup(m, 2, max_frames=16 * 8)
        out = [_np(grp.encode_chunks([0, 1], x[:, a:b], want_probs=True)[2]) for a, b in wins]
    torch.cuda.synchronize()
    return out


def _stream_case(fx, family, site, layer, route, what):
    push, ctl = fx["push"], fx["control"]
    expect = gs.expected_kernels(family, site, layer, gs.SPLIT)
    x, wins = gs.stream_features(2)
    gs.set_route(push, route)
    push.set_gemm_mode("f16x3")
    f0, e0 = push.gemm_guard_stats()
    with kernel_profile() as kp:
        got = _stream_rounds(push, route, x, wins)
    f1, e1 = push.gemm_guard_stats()
    push.set_gemm_mode("f32")
    print(f"[guard] {what} push: fallbacks +{f1 - f0}, events +{e1 - e0}")
    assert gs.launched(kp.kernels, expect), (expect, sorted(kp.kernels))
    assert not any(k.startswith("k_ffn_part<false>") for k in kp.kernels), sorted(kp.kernels)  # nothing was run again
    assert f1 == f0 and e1 > e0
    assert all(np.isfinite(g).all() for g in got)
    # ---- control ----
    gs.set_route(ctl, route)
    ctl.set_gemm_mode("f32")
    base = _stream_rounds(ctl, route, x, wins)
    ctl.set_gemm_mode("f16x3")
    f0, e0 = ctl.gemm_guard_stats()
    with kernel_profile() as kp:
        got = _stream_rounds(ctl, route, x, wins)
    f1, e1 = ctl.gemm_guard_stats()
    ctl.set_gemm_mode("f32")
    assert gs.launched(kp.kernels, expect), (expect, sorted(kp.kernels))
    worst = w32 = 0.0
    for s in range(got[0].shape[0]):
        for g, b, r in zip(got, base, _ref_chunks(fx, s, x, wins)):
            assert g[s:s + 1].shape == tuple(r.shape)
            worst = max(worst, nm.utt_rel(g[s:s + 1], torch.softmax(r, -1)), nm.logprob_err(g[s:s + 1], r))
            w32 = max(w32, nm.utt_rel(b[s:s + 1], torch.softmax(r, -1)), nm.logprob_err(b[s:s + 1], r))
            assert nm.frame_ids_ok(np.log(np.maximum(g[s], 1e-38)), r[0], nm.F32_BUDGET)[0]
    print(f"[guard] {what} control: fallbacks +{f1 - f0}, events +{e1 - e0}, worst chunk error {worst:.2e} (f32 mode: {w32:.2e})")
    assert (f1, e1) == (f0, e0)
    assert any(not np.array_equal(g, b) for g, b in zip(got, base))
    assert worst < nm.F32_BUDGET, worst


@pytest.mark.parametrize("case", gs.CASES, ids=gs.case_id)
def test_guard_site(case):
    family, site, layer, route = case
    fx = _fixture(family, site, layer)
    what = gs.case_id(case)
    if route in gs.BATCHED:
        _batched_case(fx, family, site, layer, route, what)
    else:
        _stream_case(fx, family, site, layer, route, what)


# ---- refusal matrix ----------------------------------------------------------------------------------------------------
def _accuracy(family, sd, model, what):
    x, lens = gs.batch_features()
    ref = gs.make_oracle64(family, sd).get_encoder_out(x, lens, return_logits=True)[1]
    probs, logits = model.get_encoder_out(x, lens, return_logits=True)
    errs = (nm.utt_rel(logits, ref), nm.logprob_err(probs, ref))
    print(f"[refusal] {what}: logits {errs[0]:.2e} logprobs {errs[1]:.2e}")
    assert max(errs) < nm.F32_BUDGET, errs
    assert nm.frame_ids_ok(logits, ref, nm.F32_BUDGET)[0]


@pytest.mark.parametrize("family,name,element,repacked", gs.WEIGHTS, ids=lambda v: str(v).replace("encoder.", "").replace(" ", ""))
def test_weight_at_the_fp16_boundary(family, name, element, repacked):
    """|w| = 255.5 < 65 504 / 2^8 = 255.875 is accepted and accurate; |w| = 256.0 is refused with PPASR_EUNSUPPORTED where the
    class is re-packed (coverage stays empty, the next call is byte-identical to the call before the attempt) and accepted
    with the family's coverage bits where the class keeps fp32 arithmetic."""
    sign = -1.0 if sum(element) % 2 else 1.0
    x, lens = gs.batch_features()
    sd = gs.weight_edited(family, name, element, sign * 255.5)
    m = gs.make_model(family, sd)
    m.set_gemm_mode("f16x3")
    assert m.gemm_coverage() == {"layers", "front", "head"}
    _accuracy(family, sd, m, f"{family} {name} = {sign * 255.5}")
    f, e = m.gemm_guard_stats()
    print(f"[refusal] {family} {name} = {sign * 255.5}: accepted, fallbacks {f} events {e}")
    assert (f, e) == (0, 0)
    del m
    sd = gs.weight_edited(family, name, element, sign * 256.0)
    m = gs.make_model(family, sd)
    _, before = m.get_encoder_out(x, lens, return_logits=True)
    if repacked:
        with pytest.raises(_lib.PPASRHipError) as ei:
            m.set_gemm_mode("f16x3")
        assert ei.value.status == _lib.PPASR_EUNSUPPORTED
        assert m.gemm_coverage() == set()
        _, after = m.get_encoder_out(x, lens, return_logits=True)
        assert torch.equal(before, after)
        print(f"[refusal] {family} {name} = {sign * 256.0}: refused")
    else:
        m.set_gemm_mode("f16x3")
        assert m.gemm_coverage() == {"layers", "front", "head"}
        _, after = m.get_encoder_out(x, lens, return_logits=True)
        assert torch.isfinite(after).all() and m.gemm_guard_stats() == (0, 0)
        print(f"[refusal] {family} {name} = {sign * 256.0}: accepted (fp32 arithmetic on this family)")


@pytest.mark.parametrize("family,layer,repacked", [("conformer", 1, True), ("efficient", 0, True), ("efficient", 2, True),
                                                   ("squeezeformer", 1, False)])
def test_positional_table_entry_at_the_fp16_boundary(family, layer, repacked):
    """The layers' projected positional tables are re-packed as operand planes on the Conformer families (grouped-attention
    layers included): an entry past 4 094 refuses the mode like a weight; at 0.9 x 4 094 it is accepted.  A Squeezeformer
    handle keeps its tables in fp32 and accepts both."""
    x, lens = gs.batch_features()
    m = gs.make_model(family, gs.table_scaled(family, layer, 0.9))
    m.set_gemm_mode("f16x3")
    assert m.gemm_coverage() == {"layers", "front", "head"}
    gs.set_route(m, gs.FUSED)
    _, out = m.get_encoder_out(x, lens, return_logits=True)
    assert torch.isfinite(out).all() and m.gemm_guard_stats() == (0, 0)
    del m
    m = gs.make_model(family, gs.table_scaled(family, layer, 1.05))
    gs.set_route(m, gs.FUSED)
    _, before = m.get_encoder_out(x, lens, return_logits=True)
    if repacked:
        with pytest.raises(_lib.PPASRHipError) as ei:
            m.set_gemm_mode("f16x3")
        assert ei.value.status == _lib.PPASR_EUNSUPPORTED
        assert m.gemm_coverage() == set()
        _, after = m.get_encoder_out(x, lens, return_logits=True)
        assert torch.equal(before, after)
    else:
        m.set_gemm_mode("f16x3")
        assert m.gemm_coverage() == {"layers", "front", "head"}
        _, after = m.get_encoder_out(x, lens, return_logits=True)
        assert torch.isfinite(after).all() and m.gemm_guard_stats() == (0, 0)
    print(f"[refusal] {family} layer {layer} positional table: 0.9 x accepted, 1.05 x {'refused' if repacked else 'accepted (fp32 table)'}")


# ---- balanced rescaling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [gs.FUSED, gs.SPLIT])
@pytest.mark.parametrize("k", [11, -9])
def test_balanced_rescaling(k, route):
    """CPU emulation of the mode (tools/experiments/r05/split_bf16_numerics.py, mode "h3", scales (16, 256)): 5.2 - 5.5e-7 of
    float64 for k = 0 .. 11 with activations shrinking (max |w1| = 128 at k = 11, still accepted) and for k = 0 .. 9 with
    them growing; fp32 arithmetic 5.3e-7.  Here: no event, no refusal, the error within F32_BUDGET, bytes different from
    "f32" mode."""
    from ppasr_amd.utils.synth import synth_features
    sd = gs.rescaled(k)
    feats = [synth_features(1, 200, seed=s)[0] for s in (11, 12)]
    x, lens = np.concatenate(feats, 0), np.array([200, 200], np.int64)
    m = gs.make_model("conformer", sd)
    gs.set_route(m, route)
    _, l32 = m.get_encoder_out(x, lens, return_logits=True)
    m.set_gemm_mode("f16x3")
    with kernel_profile() as kp:
        probs, logits = m.get_encoder_out(x, lens, return_logits=True)
        torch.cuda.synchronize()
    assert gs.launched(kp.kernels, ("k_ffn_qkv_h3",) if route == gs.FUSED else ("k_ffn_part<",)), sorted(kp.kernels)
    ref = gs.make_oracle64("conformer", sd).get_encoder_out(x, lens, return_logits=True)[1]
    errs = (nm.utt_rel(logits, ref), nm.logprob_err(probs, ref))
    e32 = nm.utt_rel(l32, ref)
    print(f"[rescale] k={k} {route}: f16x3 logits {errs[0]:.2e} logprobs {errs[1]:.2e}, f32 mode {e32:.2e}, stats {m.gemm_guard_stats()}")
    assert m.gemm_guard_stats() == (0, 0)
    assert not torch.equal(logits, l32)
    assert max(errs) < nm.F32_BUDGET, errs
    assert nm.frame_ids_ok(logits, ref, nm.F32_BUDGET)[0]
