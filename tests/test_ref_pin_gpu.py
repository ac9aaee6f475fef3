"""GPU: the HIP path (through the C-ABI) against fixtures produced by the REFERENCE's OWN model source
(tests/golden/ref_small.npz / ref_full.npz; tests/golden/make_ref_goldens.py runs /root/reference/ppasr/model_utils
unmodified on oracle/paddle_shim).  No oracle is involved at run time.

Tolerances: encoder logits / probabilities within the fp32 error budget of tests/numerics.py (F32_BUDGET; the
recurrences F32_BUDGET_DS2) relative to the tensor's largest magnitude; greedy ids bit-exact (frames whose reference top-2 logit margin is below 1e-3 are near-ties of the fp32
reference itself and are compared through the margin instead).

The batched tests run twice: in the default arithmetic and with the opt-in fp16 x 3 GEMM mode (ppasr_set_gemm_mode,
NOTES 9.8) -- the same fixtures, the frozen mode's own 1e-3 and the same greedy-id criteria."""
import os

import numpy as np
import pytest
import torch

import ref_cases as rc
from numerics import F32_BUDGET, F32_BUDGET_DS2, rel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = {"f32": F32_BUDGET, "f16x3": 1e-3}  # per GEMM mode: the opt-in fp16 x 3 mode keeps its 1e-3 (out of scope)


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(HERE, "golden", "ref_small.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ref_full():
    with np.load(os.path.join(HERE, "golden", "ref_full.npz")) as z:
        return {k: z[k] for k in z.files}


GEMM_MODES = ["f32", "f16x3"]


def make_model(case, sd, gemm="f32", force_rows=False):
    """gemm = "f16x3": the handle in the opt-in GEMM mode (skip where the route has none: general layer route,
    DeepSpeech2); force_rows: small fixtures on the 8-wave 32-row kernels, the ones the mode is built into."""
    model = _make_model(case, sd)
    if gemm != "f32":
        from ppasr_amd import _lib
        try:
            model.set_gemm_mode(gemm)
        except _lib.PPASRHipError as e:
            if e.status == _lib.PPASR_EUNSUPPORTED:
                pytest.skip("no fp16 x 3 GEMMs on this route")
            raise
        if force_rows:
            model.set_row_block(32)
            model.set_ffn_split(0)
    return model


def _make_model(case, sd):
    fam = case["family"]
    conf = rc.product_encoder_conf(case)
    if fam == "conformer":
        from ppasr_amd.model_utils.conformer.model import ConformerModel as M
    elif fam == "efficient_conformer":
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
    elif fam == "squeezeformer":
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
    else:
        from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model as M
    return M(80, case["V"], streaming=case["streaming"], encoder_conf=conf, state_dict=sd, device="cuda:0")


FORMERS = [k for k, c in rc.SMALL.items() if c["family"] != "deepspeech2"]
DS2 = [k for k, c in rc.SMALL.items() if c["family"] == "deepspeech2"]


@pytest.mark.parametrize("gemm", GEMM_MODES)
@pytest.mark.parametrize("name", FORMERS)
def test_former_batched_matches_reference_source(ref, name, gemm):
    case = rc.SMALL[name]
    model = make_model(case, rc.state_dict(case), gemm, force_rows=True)
    x, lens = rc.features(case)
    probs, logits = model.get_encoder_out(x, lens, return_logits=True)
    torch.cuda.synchronize()
    e_l, e_p = rel(logits.cpu().numpy(), ref[f"{name}/logits"]), rel(probs.cpu().numpy(), ref[f"{name}/probs"])
    print(f"{name} [{gemm}]: logits {e_l:.2e} probs {e_p:.2e}")
    assert e_l < TOL[gemm] and e_p < TOL[gemm]
    got, want = probs.cpu().numpy().argmax(-1), ref[f"{name}/probs"].argmax(-1)
    if gemm == "f32":
        assert np.array_equal(got, want)
    else:  # (another rounding of the same sums: a frame may only differ where the reference's own top two are a near-tie)
        top2 = np.sort(ref[f"{name}/probs"], axis=-1)[..., -2:]
        assert np.array_equal(got[(top2[..., 1] - top2[..., 0]) > 1e-5], want[(top2[..., 1] - top2[..., 0]) > 1e-5])


@pytest.mark.parametrize("gemm", GEMM_MODES)
@pytest.mark.parametrize("name,required", [(k, r) for k in FORMERS for r in rc.SMALL[k]["required"]])
def test_former_chunks_match_reference_source(ref, name, required, gemm):
    """gemm = "f16x3": the stream handle's split-route kernels on the fp16 x3 route (Conformer / Efficient-Conformer; on a
    Squeezeformer handle the mode covers batched launches only and the chunks keep fp32 arithmetic) -- same fixtures, same
    criteria."""
    case = rc.SMALL[name]
    model = make_model(case, rc.state_dict(case), gemm)
    x = rc.chunk_features(case)
    stream = model.new_stream()
    outs = []
    for (a, b) in rc.windows(x.shape[1]):
        outs.append(stream.encode_chunk(x[:, a:b], required).cpu().numpy())
    k = f"{name}/chunk{required}"
    assert [o.shape[1] for o in outs] == ref[k + "/n"].tolist()
    e_p = rel(np.concatenate(outs, 1), ref[k + "/probs"])
    att, cnn = stream.export_caches()
    assert tuple(att.shape) == ref[k + "/att"].shape and tuple(cnn.shape) == ref[k + "/cnn"].shape
    e_a = rel(att.cpu().numpy(), ref[k + "/att"]) if ref[k + "/att"].size else 0.0
    e_c = rel(cnn.cpu().numpy(), ref[k + "/cnn"]) if ref[k + "/cnn"].size else 0.0  # (use_cnn_module=False: empty)
    print(f"{k} [{gemm}]: probs {e_p:.2e} att {e_a:.2e} cnn {e_c:.2e}")
    assert e_p < TOL[gemm] and e_a < TOL[gemm] and e_c < TOL[gemm]


@pytest.mark.parametrize("name", DS2)
def test_ds2_matches_reference_source(ref, name):
    case = rc.SMALL[name]
    model = make_model(case, rc.state_dict(case))
    x, lens = rc.features(case)
    probs = model.get_encoder_out(x, lens)
    torch.cuda.synchronize()
    e = rel(probs.cpu().numpy(), ref[f"{name}/probs"])
    print(f"{name}: probs {e:.2e}")
    assert e < F32_BUDGET_DS2
    assert np.array_equal(probs.cpu().numpy().argmax(-1), ref[f"{name}/probs"].argmax(-1))
    if case["chunk_frames"]:
        xc = rc.chunk_features(case)
        B = xc.shape[0]
        h = torch.zeros(case["L"], B, 1024)
        c = torch.zeros(case["L"], B, 1024)
        outs = []
        for (a, b) in rc.windows(xc.shape[1]):
            p, _, h, c = model.get_encoder_out_chunk(xc[:, a:b], np.full(B, b - a, np.int64), h, c)
            outs.append(p.cpu().numpy())
        assert [o.shape[1] for o in outs] == ref[f"{name}/chunk/n"].tolist()
        e_p = rel(np.concatenate(outs, 1), ref[f"{name}/chunk/probs"])
        e_h = rel(h.cpu().numpy(), ref[f"{name}/chunk/h"])
        print(f"{name}/chunk: probs {e_p:.2e} h {e_h:.2e}")
        assert e_p < F32_BUDGET_DS2 and e_h < F32_BUDGET_DS2
        if not case["kw"].get("use_gru"):
            assert rel(c.cpu().numpy(), ref[f"{name}/chunk/c"]) < F32_BUDGET_DS2


# ---- BASELINE.json configs at full size ------------------------------------------------------------------------------
MEASURED_ERR = 2e-6  # relative logit error of the HIP path against the reference's source (printed by every test here)
MEASURED_ERR_MODE = {"f32": MEASURED_ERR, "f16x3": 4e-6}  # (the fp16 x 3 mode: the fp32 kernels' error + its own 1e-6 .. 2e-6)


def _check_frames(logits, ids, margin, lse, sampled, cols, what, measured_err=None):
    """logits [n, V] of the HIP path vs the reference's per-frame summary.  Greedy ids must equal the reference's on
    EVERY frame; a differing id is tolerated only on a near-tie frame of the reference (top-2 margin <= 1e-3) where the
    HIP path's own top-2 gap is below 2 x the measured logit error -- and the count of such frames is printed."""
    l64 = logits.astype(np.float64)
    scale = max(float(np.abs(sampled).max()), 1e-30)
    e_s = float(np.abs(l64[:, cols] - sampled).max() / scale)
    m = l64.max(-1, keepdims=True)
    got_lse = m[:, 0] + np.log(np.exp(l64 - m).sum(-1))
    e_z = float(np.abs(got_lse - lse).max() / max(float(np.abs(lse).max()), 1e-30))
    got_ids = l64.argmax(-1)
    clear = margin > 1e-3
    assert np.array_equal(got_ids[clear], ids[clear]), what
    near = ~clear
    differ = np.nonzero(near & (got_ids != ids))[0]
    top2 = np.sort(l64[differ], axis=-1)[:, -2:] if len(differ) else np.zeros((0, 2))
    gaps = top2[:, 1] - top2[:, 0]
    absmax = float(np.abs(l64).max())
    print(f"{what}: near-tie frames {int(near.sum())}/{len(ids)} (min reference margin {float(margin.min()):.2e}); "
          f"ids differing from the reference on them: {len(differ)}"
          + (f" (HIP top-2 gaps {np.array2string(gaps, precision=2)})" if len(differ) else ""))
    # a differing id needs a HIP gap inside the arithmetic's own noise, and the reference's winner must be our runner-up
    assert np.all(gaps <= 2 * (measured_err or MEASURED_ERR) * absmax), (what, differ, gaps)
    for f in differ:
        assert ids[f] in np.argsort(l64[f])[-2:], (what, f)
    return e_s, e_z, int(near.sum()), set(int(f) for f in differ)


def _check_probs_against_summary(p, z, key, what):
    """probabilities [n, V] against the reference-source summary of a full-size case (per-frame greedy id, top-2 logit
    margin, log-sum-exp, logits of the sampled columns): the reference's probabilities on those columns are
    exp(logit - lse)."""
    ids, margin, lse, sampled, cols = (z[f"{key}/{k}"].reshape((-1,) + z[f"{key}/{k}"].shape[2:]) if k != "cols" else z[f"{key}/cols"]
                                       for k in ("ids", "margin", "lse", "sampled", "cols"))
    want = np.exp(sampled.astype(np.float64) - lse.astype(np.float64)[:, None])
    e_p = float(np.abs(p[:, cols].astype(np.float64) - want).max() / max(want.max(), 1e-30))
    e_m = float(np.abs(p.max(-1) - z[f"{key}/maxprob"].reshape(-1)).max())
    clear = margin > 1e-3
    assert np.array_equal(p.argmax(-1)[clear], ids[clear]), what
    print(f"{what}: sampled probs {e_p:.2e} max-prob {e_m:.2e}; near-tie frames {int((~clear).sum())}/{len(ids)}")
    return e_p, e_m


def test_cfg1_deepspeech2_full_size_matches_reference_source(ref_full):
    """configs[0] at full size: DeepSpeech2 non-streaming, 5 x 1024 bidirectional LSTM (deepspeech2/encoder.py:61-104),
    B = 1, one 5 s utterance (498 frames -> 123), V = 4233 -- the reference's CRNNEncoder + CTC head run from source on the
    shim (whose LSTM cell is second-sourced against torch.nn.LSTM, tests/test_second_source_cpu.py), every frame: greedy id,
    sampled probabilities, max probability; then the greedy decoder's tokens == collapse of the reference's ids."""
    from ppasr_amd.decoders.ctc_greedy_decoder import greedy_decode_ids
    case = rc.FULL["cfg1"]
    model = make_model(case, rc.state_dict(case))
    x, lens = rc.features(case)
    probs = model.get_encoder_out(x, lens)
    torch.cuda.synchronize()
    assert tuple(probs.shape) == (1, 123, 4233)
    e_p, e_m = _check_probs_against_summary(probs.cpu().numpy()[0], ref_full, "cfg1", "cfg1")
    assert e_p < F32_BUDGET_DS2 and e_m < F32_BUDGET_DS2
    tokens, n, _, _, _ = greedy_decode_ids(probs)
    rid = ref_full["cfg1/ids"][0]
    if (ref_full["cfg1/margin"][0] > 1e-3).all():
        keep = np.concatenate([[True], rid[1:] != rid[:-1]]) & (rid != 0)
        assert np.array_equal(tokens[0, :int(n[0])].cpu().numpy(), rid[keep])


@pytest.mark.parametrize("gemm", GEMM_MODES)
def test_cfg2_all_utterances_logits_and_tokens(ref_full, gemm):
    """configs[1] at full size: 12 blocks, 32 x 1000 frames, V = 4233 -- logits of every frame of all 32 utterances
    (sampled vocabulary columns + log-sum-exp), greedy ids of every frame, and the fused greedy route's tokens."""
    case = rc.FULL["cfg2"]
    model = make_model(case, rc.state_dict(case), gemm)
    x, lens = rc.features(case)
    probs, logits = model.get_encoder_out(x, lens, return_logits=True)
    tokens, n_tokens, score = model.encode_greedy(x, lens)
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    B, Tp, V = lg.shape
    cols = ref_full["cfg2/cols"]
    e_s, e_z, near, differ = _check_frames(lg.reshape(B * Tp, V), ref_full["cfg2/ids"].reshape(-1),
                                           ref_full["cfg2/margin"].reshape(-1), ref_full["cfg2/lse"].reshape(-1),
                                           ref_full["cfg2/sampled"].reshape(B * Tp, -1), cols, f"cfg2 [{gemm}]",
                                           MEASURED_ERR_MODE[gemm])
    print(f"cfg2: sampled logits {e_s:.2e} lse {e_z:.2e} near-ties {near}/{B * Tp}")
    assert e_s < TOL[gemm] and e_z < TOL[gemm]
    e_m = float(np.abs(probs.cpu().numpy().max(-1) - ref_full["cfg2/maxprob"]).max())
    assert e_m < TOL[gemm]
    # fused greedy tokens of EVERY utterance == collapse of the HIP path's own frame ids (the fused route and the
    # materialised logits agree), and == collapse of the reference's frame ids wherever no frame of the utterance
    # differed above (near-tie utterances included: their ids were just compared frame by frame)
    hip_ids = lg.argmax(-1)
    n_ref_checked = 0
    for b in range(B):
        got = tokens[b, :int(n_tokens[b])].cpu().numpy()
        ids = hip_ids[b]
        keep = np.concatenate([[True], ids[1:] != ids[:-1]]) & (ids != 0)
        assert np.array_equal(ids[keep], got), b
        if not any(b * Tp <= f < (b + 1) * Tp for f in differ):
            rid = ref_full["cfg2/ids"][b]
            keep = np.concatenate([[True], rid[1:] != rid[:-1]]) & (rid != 0)
            assert np.array_equal(rid[keep], got), b
            n_ref_checked += 1
    n_near_utts = int((ref_full["cfg2/margin"] <= 1e-3).any(axis=1).sum())
    print(f"cfg2: encode_greedy tokens == reference collapse for {n_ref_checked}/{B} utterances "
          f"({n_near_utts} of them contain a near-tie frame)")
    assert n_ref_checked >= B - len(differ)


@pytest.mark.parametrize("gemm", GEMM_MODES)
def test_cfg4_efficient_conformer_beam_all_utterances(ref_full, gemm):
    """configs[3]: Efficient-Conformer 12 blocks, B = 64, beam 10 / 0.99 / top-40: HIP probabilities -> HIP beam search
    tokens == the C oracle's tokens on the REFERENCE's probabilities, for every utterance."""
    from ppasr_amd.decoders.beam_search_decoder import beam_search_ids
    case = rc.FULL["cfg4"]
    model = make_model(case, rc.state_dict(case), gemm)
    x, lens = rc.features(case)
    probs, logits = model.get_encoder_out(x, lens, return_logits=True)
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    B, Tp, V = lg.shape
    assert (B, Tp) == (64, 125)
    e_s, e_z, near, _ = _check_frames(lg.reshape(B * Tp, V), ref_full["cfg4/ids"].reshape(-1),
                                      ref_full["cfg4/margin"].reshape(-1), ref_full["cfg4/lse"].reshape(-1),
                                      ref_full["cfg4/sampled"].reshape(B * Tp, -1), ref_full["cfg4/cols"], f"cfg4 [{gemm}]",
                                      MEASURED_ERR_MODE[gemm])
    print(f"cfg4: sampled logits {e_s:.2e} lse {e_z:.2e} near-ties {near}/{B * Tp}")
    assert e_s < TOL[gemm] and e_z < TOL[gemm]
    toks, n, _, _ = beam_search_ids(probs, beam_size=rc.BEAM["beam_size"], cutoff_prob=rc.BEAM["cutoff_prob"],
                                    cutoff_top_n=rc.BEAM["cutoff_top_n"])
    toks, n = toks[:, 0].cpu().numpy(), n[:, 0].cpu().numpy()
    bad = [b for b in range(B) if not np.array_equal(toks[b, :n[b]], ref_full["cfg4/beam_tokens"][b, :ref_full["cfg4/beam_n"][b]])]
    # The probabilities agree with the reference's to ~1e-6, not bit for bit, and the search is discontinuous in them
    # (the 0.99 cumulative cut-off and the top-40 cut decide which tokens a frame may extend a prefix with; on
    # random-weight models some frame sits on such an edge).  So: at most 2 of the 64 utterances may differ from the
    # fixture, and each of those must be exactly what the C oracle finds on the SAME (HIP) probabilities -- the search
    # itself stays bit-exact.
    from test_ctc_beam_gpu import _oracle, _oracle_decode
    assert len(bad) <= 2, f"beam tokens differ from the oracle-on-reference-probs for utterances {bad}"
    pr = probs.cpu().numpy()
    print(f"cfg4: beam tokens == fixture for {B - len(bad)}/{B} utterances; pruning-edge utterances: {bad}")
    ref_pr = None
    for b in bad:
        top = _oracle_decode(_oracle(), pr[b], rc.BEAM["beam_size"], rc.BEAM["cutoff_prob"], rc.BEAM["cutoff_top_n"], 0, 1)
        assert top[0][0] == toks[b, :n[b]].tolist(), b
        # the deciding frame: the first frame whose pruned candidate SET (cumulative 0.99 cut / top-40) differs between
        # neighbouring roundings of the HIP probabilities -- found by perturbing the cut by the measured error
        srt = -np.sort(-pr[b].astype(np.float64), axis=-1)[:, :40]
        cum = np.cumsum(srt, -1)
        edge = np.abs(cum - rc.BEAM["cutoff_prob"]).min(-1)
        f = int(np.argmin(edge))
        print(f"cfg4: utterance {b}: pruning-edge case (frame {f}: cumulative probability within {edge[f]:.1e} of the 0.99 "
              "cut), HIP search == C oracle on the HIP probabilities")


@pytest.mark.parametrize("gemm", GEMM_MODES)
@pytest.mark.parametrize("route", ["buckets", "skip_padding"])
def test_cfg5_squeezeformer_ragged_beam(ref_full, route, gemm):
    """configs[4], one GPU's share: Squeezeformer 12 blocks, 16 utterances of 2-30 s; (a) 200-frame length buckets,
    (b) ONE batch padded to the longest with skip_padding.  Valid frames' logits vs the reference run on the SAME batch
    composition (the reference's values depend on what an utterance is padded into: full-context attention sees the
    partially padded last frame), and for (a) HIP beam tokens == C oracle tokens on the reference's probabilities."""
    from ppasr_amd.decoders.beam_search_decoder import beam_search_ids
    case = rc.FULL["cfg5"]
    model = make_model(case, rc.state_dict(case), gemm)
    x, lens = rc.features(case)
    cols = ref_full["cfg5/cols"]
    B = len(lens)
    got_probs = [None] * B
    got_logits = [None] * B
    if route == "buckets":
        buckets = {}
        for i, ln in enumerate(lens):
            buckets.setdefault(rc.bucket_of(ln), []).append(i)
        for bk, idx in sorted(buckets.items()):
            Tb = int(lens[idx].max())
            p, l = model.get_encoder_out(x[idx, :Tb], lens[idx], return_logits=True)
            for j, i in enumerate(idx):
                got_probs[i], got_logits[i] = p[j], l[j]
    else:
        model.set_skip_padding(True)
        p, l = model.get_encoder_out(x, lens, return_logits=True)
        for i in range(B):
            got_probs[i], got_logits[i] = p[i], l[i]
    torch.cuda.synchronize()
    worst = 0.0
    key = "cfg5" if route == "buckets" else "cfg5pad"   # the reference of the same batch composition
    for i in range(B):
        n = ref_full[f"{key}/ids/{i}"].shape[0]
        lg = got_logits[i][:n].cpu().numpy()
        e_s, e_z, _, _ = _check_frames(lg, ref_full[f"{key}/ids/{i}"], ref_full[f"{key}/margin/{i}"], ref_full[f"{key}/lse/{i}"],
                                       ref_full[f"{key}/sampled/{i}"], cols, f"{key}[{i}] [{gemm}]", MEASURED_ERR_MODE[gemm])
        worst = max(worst, e_s, e_z)
    print(f"cfg5/{route}: worst rel err {worst:.2e}")
    assert worst < TOL[gemm]
    if route == "buckets":
        for i in range(B):
            n = ref_full[f"cfg5/ids/{i}"].shape[0]
            toks, cnt, _, _ = beam_search_ids(got_probs[i][:n].unsqueeze(0), beam_size=rc.BEAM["beam_size"],
                                              cutoff_prob=rc.BEAM["cutoff_prob"], cutoff_top_n=rc.BEAM["cutoff_top_n"])
            want = ref_full["cfg5/beam_tokens"][i, :ref_full["cfg5/beam_n"][i]]
            got = toks[0, 0, :int(cnt[0, 0])].cpu().numpy()
            if gemm == "f32":
                assert np.array_equal(got, want), i
            elif not np.array_equal(got, want):
                # another rounding of the probabilities may sit on the other side of a pruning edge (see the cfg4 test): the
                # search itself must then be exactly the C oracle's on the SAME probabilities
                from test_ctc_beam_gpu import _oracle, _oracle_decode
                top = _oracle_decode(_oracle(), got_probs[i][:n].cpu().numpy(), rc.BEAM["beam_size"], rc.BEAM["cutoff_prob"],
                                     rc.BEAM["cutoff_top_n"], 0, 1)
                assert top[0][0] == got.tolist(), i
                print(f"cfg5[{i}] [{gemm}]: pruning-edge utterance, HIP search == C oracle on the HIP probabilities")


@pytest.mark.parametrize("mode", ["buckets", "merged"])
def test_cfg5_decode_ragged_end_to_end(ref_full, mode):
    """configs[4] through the product's own driver (parallel.decode_ragged: plan -> encode -> beam -> pack, one rank):
    mode "buckets" must reproduce the per-bucket fixture tokens (reference probabilities -> C oracle), utterance order
    restored; mode "merged" (ONE ragged batch, skip_padding) is held to the C oracle on the HIP probabilities of the same
    batch composition, and its agreement with the per-bucket fixture is printed (the reference's values depend on what
    an utterance is padded into, so the two compositions may legitimately differ on pruning-edge frames)."""
    from ppasr_amd.parallel import RaggedPlan, beam_ids_decoder, decode_ragged
    from test_ctc_beam_gpu import _oracle, _oracle_decode
    case = rc.FULL["cfg5"]
    model = make_model(case, rc.state_dict(case))
    x, lens = rc.features(case)
    B = len(lens)
    feats = [x[i, :int(lens[i])] for i in range(B)]          # per-utterance arrays, caller's order
    perm = np.random.Generator(np.random.PCG64(3)).permutation(B)   # ... shuffled: the plan must restore the order
    dec = beam_ids_decoder(rc.BEAM["beam_size"], rc.BEAM["cutoff_prob"], rc.BEAM["cutoff_top_n"])
    tokens, n, score = decode_ragged(model, [feats[i] for i in perm], [int(lens[i]) for i in perm], dec, mode=mode)
    torch.cuda.synchronize()
    tokens, n = tokens.cpu().numpy(), n.cpu().numpy()
    assert tokens.shape == (B, model.out_frames(int(lens.max())))
    same = 0
    for j, i in enumerate(perm):
        want = ref_full["cfg5/beam_tokens"][i, :ref_full["cfg5/beam_n"][i]]
        got = tokens[j, :n[j]]
        assert np.all(tokens[j, n[j]:] == -1)
        if mode == "buckets":
            assert np.array_equal(got, want), i
        same += int(np.array_equal(got, want))
    print(f"cfg5 decode_ragged[{mode}]: tokens == per-bucket fixture for {same}/{B} utterances")
    if mode == "merged":
        model.set_skip_padding(True)
        probs = model.get_encoder_out(x, lens)
        model.set_skip_padding(False)
        fl = model.valid_out_frames(lens, x.shape[1]).cpu().numpy()
        pr = probs.cpu().numpy()
        for j, i in enumerate(perm):
            top = _oracle_decode(_oracle(), pr[i, :fl[i]], rc.BEAM["beam_size"], rc.BEAM["cutoff_prob"], rc.BEAM["cutoff_top_n"], 0, 1)
            assert top[0][0] == tokens[j, :n[j]].tolist(), i
        # the pipelined plan object (encoder and beam search on two streams) returns the same hypotheses, call after call
        model.set_front_fused(1)  # the caller's own setting: the pipelined plan switches it per call and must restore it
        plan = RaggedPlan(model, feats, [int(v) for v in lens], mode="merged", pipeline=True)
        for _ in range(3):
            t2, n2, _ = plan.run(dec)
        plan.sync()
        assert model.front_fused == 1
        model.set_front_fused(-1)
        t2, n2 = t2.cpu().numpy(), n2.cpu().numpy()
        for j, i in enumerate(perm):
            assert np.array_equal(t2[i, :n2[i]], tokens[j, :n[j]]), i
