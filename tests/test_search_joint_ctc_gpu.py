"""ppasr_attention_decode_joint against the float64 restatements (tests/ctc_prefix_oracle.py and
tests/joint_search_oracle.py, held to path enumeration and to their named bugs by tests/test_ctc_prefix_oracle_cpu.py):

  weight 0     through the joint entry: every output of ppasr_attention_decode, byte for byte
  replay       every case of joint_search_cases (CASES, EXACT_CASES, DEMO), none excluded: the device's trace is a top-N of
               the float64 candidates at every step up to joint_search_cases.score_tol, exactly min(N, finite candidates)
               rows are kept, trace_ctc is Psi of the traced hypotheses up to psi_tol
  final        token_logp against the float64 teacher-forced log-probabilities and token_ctc against the float64 Psi
               differences of the same hypotheses, scores against sum logp_att + w x Psi(final hypothesis)
  exact class  tokens, lens, order, ended, the trace and steps_run equal the float64 search (EXACT_CASES, DEMO)
  demo         the joint result is the table's transcript and differs from the plain call's empty hypothesis
  buffers      workspace and outputs pre-filled with NaN bytes and large finite values; NaN behind out_lens in the table
  the stream gate (both modes), every refusal, and predict / evaluate through the YAML key ctc_weight

This file is named to be collected behind tests/test_buffer_contents_*_gpu.py, test_ctc_loss_gpu.py and
test_prob_arena_gpu.py: their `stale` pattern (tests/poison.py) looks at what earlier calls of the same process left in
the caching allocator's blocks, and a scratch buffer that no call writes (fbank without dB normalisation) proves nothing
when it lands on memory that was never written.  Ahead of them this file's allocations moved that buffer.

The table and the memory are poisoned with NaN behind out_lens in every run.  The tolerances are those of
joint_search_cases (F32_BUDGET x S for one Psi); nothing is widened and no case is skipped."""
import numpy as np
import pytest
import torch

import attention_search_cases as ac
import ctc_prefix_oracle as cp
import joint_search_cases as jc
import joint_search_oracle as jo
import numerics as nm
import poison
import stream_gate as sg
import test_attention_decode_gpu as tad

pytestmark = pytest.mark.gpu

ALL = dict(jc.CASES, **jc.EXACT_CASES, demo=jc.DEMO)
_memo = nm.Memo()


def rescorer(name):
    return tad.rescorer("joint/" + name, ALL[name])


def oracle64(name):
    return tad.oracle64("joint/" + name, ALL[name])


def inputs(name):
    """memory and table with NaN behind out_lens"""
    def make():
        case = ALL[name]
        inp, tab = ac.inputs(case), jc.table(case).copy()
        for b, n in enumerate(inp["out_lens"]):
            tab[b, max(int(n), 0):] = np.nan
        return dict(inp, poisoned=tad.poisoned(inp), table=tab)
    return _memo.get(("in", name), make)


def decode(name, taps=True, **kw):
    case, inp = ALL[name], inputs(name)
    kw.setdefault("ctc_weight", case["w"])
    res = rescorer(name).decode(inp["poisoned"], inp["out_lens"], case["N"], case["P"], return_token_logp=taps,
                                return_trace=taps, ctc_probs=inp["table"], blank=case["blank"], **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def device(name):
    return _memo.get(("dev", name), lambda: decode(name))


def test_weight_zero_through_the_joint_entry_is_the_plain_call_byte_for_byte():
    name = "v67_n3_b2_t33_p12"
    case, inp = ALL[name], inputs(name)
    joint = decode(name, ctc_weight=0.0)
    plain = rescorer(name).decode(inp["poisoned"], inp["out_lens"], case["N"], case["P"], return_token_logp=True,
                                  return_trace=True)
    assert set(joint) == set(plain) | {"token_ctc", "trace_ctc"}
    for k, v in plain.items():
        assert joint[k].tobytes() == v.cpu().numpy().tobytes(), k
    assert not joint["token_ctc"].any() and not joint["trace_ctc"].any()
    # at weight 0 the plain call's workspace suffices
    r = rescorer(name)
    ws = torch.empty(r.decode_workspace_bytes(case["B"], case["Tp"], case["N"], case["P"]), dtype=torch.uint8, device=r.device)
    assert r.decode_workspace_bytes(case["B"], case["Tp"], case["N"], case["P"], joint=True) > ws.numel()
    res = r.decode(inp["poisoned"], inp["out_lens"], case["N"], case["P"], workspace=ws, ctc_probs=inp["table"], ctc_weight=0.0)
    for k, v in res.items():
        assert v.cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k


def check(name, got):
    """replay and final hypotheses -> (replay violation / tol, trace_ctc error / psi_tol, token_logp error / scale,
    token_ctc error / psi_tol, score error / score_tol)"""
    case, inp, o64 = ALL[name], inputs(name), oracle64(name)
    B, N, P, V, w, u = case["B"], case["N"], case["P"], case["V"], case["w"], jc.unit(name)
    tab = jc.table(case)
    w_rep = w_psi = w_lp = w_ctc = w_sc = 0.0
    steps_max = 0
    for b in range(B):
        ps = cp.PrefixScorer(tab[b], inp["out_lens"][b], case["blank"])
        ptol = jc.psi_tol(ps.S, u)
        rep = jo.replay(o64, inp["memory"][b], inp["out_lens"][b], tab[b], case["blank"], w, N, got["trace_parent"][:, b],
                        got["trace_token"][:, b], got["trace_score"][:, b], got["trace_ctc"][:, b],
                        lambda scale: jc.score_tol(case, scale, ps.S, u), ptol)
        assert not rep["problems"], (name, b, rep["problems"])
        w_rep, w_psi, steps_max = max(w_rep, rep["worst"]), max(w_psi, rep["worst_psi"]), max(steps_max, rep["steps"])
        for k in range(N):
            hyp = rep["hyps"][k]
            n = len(hyp)
            assert got["lens"][b, k] == n and got["ended"][b, k] == rep["ended"][k]
            assert got["tokens"][b, k, :n].tolist() == hyp and (got["tokens"][b, k, n:] == -1).all()
            tl, tcx = got["token_logp"][b, k], got["token_ctc"][b, k]
            if not np.isfinite(rep["scores64"][k]):  # a row at -inf: an empty hypothesis, nothing summed
                assert got["scores"][b, k] == -np.inf and n == 0 and not got["ended"][b, k] and not tl.any() and not tcx.any()
                continue
            m = n + 1 if got["ended"][b, k] else n
            assert not tl[m:].any() and not tcx[m:].any()
            lp64, lg64 = o64.token_logp(inp["memory"][b], inp["out_lens"][b], hyp)
            lp64 = lp64.numpy()
            scale = max(float((lg64 - lg64.mean(-1, keepdim=True)).abs().max()), 1e-30)
            st, psis = ps.empty(), [0.0]
            for c in hyp:
                st = ps.extend(st, c)
                psis.append(float(st.psi))
            if got["ended"][b, k]:
                psis.append(float(ps.psi_all(st)[V - 1]))
            d64 = np.diff(np.asarray(psis))
            if m:
                w_lp = max(w_lp, float(np.abs(tl[:m] - lp64[:m]).max() / scale))
                w_ctc = max(w_ctc, float(np.abs(tcx[:m] - d64[:m]).max() / (2 * ptol)))
            s64 = lp64[:m].sum() + w * psis[m]
            w_sc = max(w_sc, abs(got["scores"][b, k] - s64) / jc.score_tol(case, scale, ps.S, u))
            own = (tl[:m].astype(np.float64) + np.float32(w).astype(np.float64) * tcx[:m].astype(np.float64)).sum()
            assert got["scores"][b, k] == pytest.approx(own, abs=(P + 1) * 2.0 ** -22 * max(ps.S, scale, 1.0))
        fin = got["scores"][b][np.isfinite(got["scores"][b])]
        assert (np.diff(fin) <= 0).all() and not np.isfinite(got["scores"][b][fin.size:]).any()  # best first, -inf last
    assert got["steps_run"][0] == steps_max
    return w_rep, w_psi, w_lp, w_ctc, w_sc


@pytest.mark.parametrize("name", list(ALL))
def test_replay_and_final_hypotheses(name):
    worst = check(name, device(name))
    print(f"{name}: replay {worst[0]:.2e} x tol  trace_ctc {worst[1]:.2e} x psi_tol  token_logp {worst[2]:.2e}  "
          f"token_ctc {worst[3]:.2e} x 2 psi_tol  scores {worst[4]:.2e} x tol  steps_run {device(name)['steps_run'][0]}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0 and worst[2] <= tad.LOGP_BUDGET and worst[3] <= 1.0 and worst[4] <= 1.0, worst


@pytest.mark.parametrize("name", list(jc.EXACT_CASES) + ["demo"])
def test_exact_class_equals_the_float64_search(name):
    case, inp, got, o64 = ALL[name], inputs(name), device(name), oracle64(name)
    tab = jc.table(case)
    steps = 0
    for b in range(case["B"]):
        ref = jo.search(o64, inp["memory"][b], inp["out_lens"][b], tab[b], case["blank"], case["w"], case["N"], case["P"])
        steps = max(steps, ref["steps"])
        for k in range(case["N"]):
            n = len(ref["tokens"][k])
            assert got["lens"][b, k] == n and got["tokens"][b, k, :n].tolist() == ref["tokens"][k], (b, k)
        assert np.array_equal(got["ended"][b], ref["ended"])
        assert np.array_equal(got["trace_parent"][:, b], ref["trace_parent"])
        assert np.array_equal(got["trace_token"][:, b], ref["trace_token"])
    assert got["steps_run"][0] == steps


def test_demonstration_case_differs_from_the_plain_call():
    case, inp, got = jc.DEMO, inputs("demo"), device("demo")
    plain = rescorer("demo").decode(inp["poisoned"], inp["out_lens"], case["N"], case["P"])
    assert int(plain["lens"][0, 0]) == 0 and int(plain["ended"][0, 0]) == 1  # the attention decoder alone: empty
    n = int(got["lens"][0, 0])
    assert got["tokens"][0, 0, :n].tolist() == jc.DEMO_TRANSCRIPT and got["ended"][0, 0] == 1


def test_rows_at_minus_inf():
    """vocab_2 has no token but blank and eos: step 1 keeps one candidate (eos), row 1 stays at -inf and the search is over"""
    got = device("vocab_2")
    assert got["steps_run"][0] == 1 and got["ended"][0].tolist() == [1, 0] and got["lens"][0].tolist() == [0, 0]
    assert np.isfinite(got["scores"][0, 0]) and got["scores"][0, 1] == -np.inf
    assert got["trace_parent"][0, 0].tolist() == [0, -1] and got["trace_token"][0, 0].tolist() == [1, -1]
    # T = 0: Psi(eos) = 0 for the empty hypothesis, every other candidate is infeasible
    got = device("lens_0_1_2_tp")
    assert got["ended"][0].tolist() == [1, 0, 0] and got["token_ctc"][0, 0, 0] == 0.0 and (got["lens"][0] == 0).all()
    assert (got["lens"][1] <= 1).all() and (got["lens"][2] <= 2).all()  # L + repeats <= T


@pytest.mark.parametrize("name", ["v67_n3_b2_t33_p12", "frames_b4_t129", "repeats_tight", "rows_65"])
def test_results_do_not_depend_on_buffer_contents_or_taps(name):
    case = ALL[name]
    r = rescorer(name)
    B, N, P = case["B"], case["N"], case["P"]
    need = r.decode_workspace_bytes(B, case["Tp"], N, P, joint=True)
    assert need > 0
    runs = []
    for pat in ("ff", "7f"):
        ws = poison.fill(torch.empty(need, dtype=torch.uint8, device=r.device), poison.BYTES[pat])
        e = lambda shape, dt: poison.fill(torch.empty(shape, dtype=dt, device=r.device), poison.BYTES[pat])
        out = dict(tokens=e((B, N, P), torch.int32), lens=e((B, N), torch.int32), scores=e((B, N), torch.float64),
                   ended=e((B, N), torch.int32), steps_run=e((1,), torch.int32), token_logp=e((B, N, P + 1), torch.float32),
                   token_ctc=e((B, N, P + 1), torch.float32), trace_parent=e((P, B, N), torch.int32),
                   trace_token=e((P, B, N), torch.int32), trace_score=e((P, B, N), torch.float64),
                   trace_ctc=e((P, B, N), torch.float32))
        runs.append({k: v.tobytes() for k, v in decode(name, workspace=ws, out=out).items()})
    ref = {k: v.tobytes() for k, v in device(name).items()}
    for k in ref:
        assert runs[0][k] == runs[1][k] == ref[k], k
    plain = decode(name, taps=False)
    assert set(plain) == {"tokens", "lens", "scores", "ended", "steps_run"}
    for k in plain:
        assert plain[k].tobytes() == ref[k], k


def test_out_lens_null_means_every_frame():
    name = "v67_n3_b2_t33_p12"
    case = ALL[name]
    inp, tab, r = ac.inputs(case), jc.table(case), rescorer(name)
    full = np.full(case["B"], case["Tp"], np.int32)
    kw = dict(return_token_logp=True, return_trace=True, ctc_probs=tab, ctc_weight=case["w"])
    a = r.decode(inp["memory"], None, case["N"], case["P"], **kw)
    b = r.decode(inp["memory"], full, case["N"], case["P"], **kw)
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


GATE_CASE = "v67_n3_b2_t33_p12"
GATE_MEMO = nm.Memo()


@pytest.mark.parametrize("mode", sg.MODES)
def test_joint_decode_is_ordered_on_the_callers_stream(mode):
    case = ALL[GATE_CASE]

    def ins(shift):
        c = dict(case, seed=case["seed"] + shift)
        inp = ac.inputs(c)
        return [torch.from_numpy(inp["memory"]), torch.from_numpy(inp["out_lens"]), torch.from_numpy(jc.table(c))]

    def run(ctx):
        r = rescorer(GATE_CASE)
        memory, lens, tab = [ctx.input(a, b) for a, b in zip(ins(0), ins(1))]
        return dict(ctx.call(lambda: r.decode(memory, lens, case["N"], case["P"], return_token_logp=True, return_trace=True,
                                              ctc_probs=tab, ctc_weight=case["w"]), [memory, lens, tab]))

    sg.check("attention_decode_joint " + GATE_CASE, run, mode, GATE_MEMO)


def test_refusals_leave_the_outputs_untouched():
    from ppasr_amd import _lib
    name = "v67_n3_b2_t33_p12"
    case, inp, r = ALL[name], inputs(name), rescorer(name)
    B, V = case["B"], case["V"]

    def refused(status, N=3, P=12, workspace=None, **kw):
        out = dict(tokens=torch.full((B, N, P), 7, dtype=torch.int32, device=r.device),
                   lens=torch.full((B, N), 7, dtype=torch.int32, device=r.device),
                   scores=torch.full((B, N), 7.0, dtype=torch.float64, device=r.device),
                   ended=torch.full((B, N), 7, dtype=torch.int32, device=r.device),
                   steps_run=torch.full((1,), 7, dtype=torch.int32, device=r.device))
        if workspace is None:
            workspace = torch.empty(1 << 22, dtype=torch.uint8, device=r.device)
        args = dict(ctc_probs=inp["table"], ctc_weight=0.5, blank=0)
        args.update(kw)
        with pytest.raises(_lib.PPASRHipError) as e:
            r.decode(inp["poisoned"], inp["out_lens"], N, P, out=out, workspace=workspace, **args)
        assert e.value.status == status, e.value
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in out.values())

    refused(_lib.PPASR_EINVAL, ctc_probs=None)  # NULL table with a positive weight
    refused(_lib.PPASR_EINVAL, blank=-1)
    refused(_lib.PPASR_EINVAL, blank=V - 1)  # eos cannot be the blank
    refused(_lib.PPASR_EINVAL, ctc_probs=inp["table"][:, :, :V - 1].copy())  # V_ctc != V
    refused(_lib.PPASR_EINVAL, ctc_weight=-0.5)
    refused(_lib.PPASR_EINVAL, ctc_weight=float("nan"))
    # the refusals of the plain call stay
    refused(_lib.PPASR_EINVAL, N=0)
    refused(_lib.PPASR_EINVAL, N=68)
    refused(_lib.PPASR_EINVAL, P=0)
    refused(_lib.PPASR_EUNSUPPORTED, N=33)
    refused(_lib.PPASR_EUNSUPPORTED, P=256)
    refused(_lib.PPASR_ENOSPACE, workspace=torch.empty(1024, dtype=torch.uint8, device=r.device))
    plain_ws = torch.empty(r.decode_workspace_bytes(B, case["Tp"], 3, 12), dtype=torch.uint8, device=r.device)
    refused(_lib.PPASR_ENOSPACE, workspace=plain_ws)  # the plain call's workspace is too small for the joint one
    assert r.decode_workspace_bytes(B, case["Tp"], 32, 255, joint=True) > 0
    assert r.decode_workspace_bytes(B, case["Tp"], 33, 12, joint=True) == 0


# ---- the YAML key: predict and evaluate on a synthetic checkpoint -------------------------------------------------------------
def test_predict_and_evaluate_read_ctc_weight_from_the_configuration():
    import test_predict_attention_gpu as tpa
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    from ppasr_amd.decoders import attention_decode
    from ppasr_amd.evaluate import evaluate
    from ppasr_amd.predict import PPASRPredictor
    from ppasr_amd.utils.metrics import cer, labels_to_string
    from ppasr_amd.utils.synth import synth_features, synth_vocabulary
    conf = dict(tpa.ATTENTION, ctc_weight=0.5)
    cfg = dict(tpa._cfg(), attention_decoder_conf=conf)
    vocab = synth_vocabulary(tpa.V)
    p = PPASRPredictor(configs=cfg, state_dict=tpa._checkpoint(), vocab_list=vocab, warmup=False)
    wav = tpa._audio(1.2, seed=5)
    res = p.predict(audio_data=wav)
    feat = AudioFeaturizer(**cfg["preprocess_conf"]).featurize(wav)
    x, lens = feat[None].astype(np.float32), np.array([feat.shape[0]], np.int64)
    model, r = p.predictor.model, p.predictor.rescorer
    probs, memory = model.get_encoder_out(x, lens, return_memory=True)
    got = r.decode(memory, None, tpa.ATTENTION["beam_size"], tpa.ATTENTION["max_steps"], ctc_probs=probs, ctc_weight=0.5)
    plain = r.decode(memory, None, **tpa.ATTENTION)
    n = int(got["lens"][0, 0])
    ids = got["tokens"][0, 0, :n].cpu().tolist()
    assert res["text"] == "".join(vocab[i] for i in ids) and res["score"] == float(got["scores"][0, 0])
    assert float(got["scores"][0, 0]) != float(plain["scores"][0, 0])  # the CTC term is in the score
    ts = p.predict(audio_data=wav, timestamps=True)
    assert ts["text"] == res["text"] and [e["text"] for e in ts["timestamps"]] == [vocab[i] for i in ids]
    with pytest.raises(NotImplementedError, match="decoder: attention scores whole utterances"):
        p.predict_stream(audio_data=tpa._audio(0.5), is_end=False)
    batches, errs = [], []
    for seed, labels in ((13, [[5, 9, 17, 3, -1], [8, 8, 21, -1, -1]]), (14, [[7, 7, 2, -1, -1], [30, 4, 4, 4, 11]])):
        x, lens = synth_features(2, 99, lens=[99, 99], seed=seed)
        labels = np.array(labels, np.int64)
        batches.append((x, labels, lens, (labels >= 0).sum(1)))
        outs = model.get_encoder_out(x, lens, return_memory=True)
        texts = [t for _, t in attention_decode(model, r, outs[1], None, vocab, probs=outs[0], **conf)]
        errs += [cer(t, l) for t, l in zip(texts, labels_to_string(labels, vocab, eos=len(vocab) - 1))]
    assert evaluate(model, batches, vocab, decoder="attention", rescorer=r, attention_conf=conf) == \
        pytest.approx(float(np.mean(errs)), abs=1e-12)
