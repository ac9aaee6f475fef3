"""The loss half end to end: model_loss on a tiny Conformer (with the attention decoder) and a tiny DeepSpeech2 against the
float64 pipeline -- numerics.oracle64 for the encoder, tests/decoder_oracle.py for the decoder, tests/loss_oracle.py for the
two losses and their combination --, evaluate(return_loss=True), and PPASRPredictor.score.

Tolerances (absolute, per utterance, from the budgets the encoder and decoder tests already hold):
  * ctc_nll: the library's log-probabilities lie within F32_BUDGET x logit scale of the float64 ones on every frame
    (numerics.logprob_err), so a sum over T frames moves by at most T x F32_BUDGET x scale; plus the kernel's own
    F32_BUDGET x max(|ref|, 1) (tests/test_ctc_loss_gpu.py);
  * att_kl: F32_BUDGET x rows x max(logit scale, 1) for the decoder (tests/test_att_loss_gpu.py), once more for the
    encoder output it attends to, which is itself within F32_BUDGET of the float64 one.
"""
import numpy as np
import pytest
import torch

import decoder_cases as dc
import loss_oracle as lo
import numerics as nm
from decoder_oracle import DecoderOracle
from ppasr_amd.utils.synth import conformer_state_dict, deepspeech2_state_dict, synth_features, synth_vocabulary

pytestmark = pytest.mark.gpu
_memo = nm.Memo()
V, UNITS, BLOCKS = 120, 256, (1, 1)
ENC = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
CONF = dict(ctc_weight=0.3, lsm_weight=0.1, reverse_weight=0.3)
LABELS = np.array([[5, 9, 9, 17, 3, 40, 118], [8, 8, 21, 2, -1, -1, -1], [7, -1, -1, -1, -1, -1, -1]], np.int64)
LABEL_LENS = np.array([7, 4, 1], np.int64)


def checkpoint():
    def go():
        sd = conformer_state_dict(vocab_size=V, num_blocks=2, seed=3, perturb_norm=True)
        sd.update(dc.decoder_state_dict(78, V, UNITS, *BLOCKS))
        return sd
    return _memo.get("sd", go)


def batch():
    return _memo.get("batch", lambda: synth_features(3, 131, lens=[131, 100, 60], seed=9))


def conformer():
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    return _memo.get("model", lambda: ConformerModel(80, V, streaming=True, encoder_conf=ENC, state_dict=checkpoint()))


def rescorer():
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    conf = dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0], r_num_blocks=BLOCKS[1])
    return _memo.get("rescorer", lambda: AttentionRescorer(checkpoint(), V, conf))


def labels_of(b):
    return LABELS[b, :LABEL_LENS[b]].tolist()


def pipeline64():
    """-> per utterance (ctc nll, ctc tolerance, att kl, r_att kl, att tolerance, rows, frames), all float64"""
    def go():
        x, lens = batch()
        o = nm.oracle64("conformer", checkpoint(), num_blocks=2)
        with torch.no_grad():
            enc, masks = o.encoder_forward(x, lens)
            logits = o.ctc_logits(enc)
            probs = torch.softmax(logits, dim=2).numpy()
        frames = masks.squeeze(1).sum(1).numpy()
        dec = DecoderOracle(checkpoint(), V, *BLOCKS, heads=4, dtype=torch.float64)
        out = []
        for b in range(3):
            T, tok = int(frames[b]), labels_of(b)
            nll, st = lo.ctc_nll(probs[b].astype(np.float32), tok, T)
            assert st == lo.OK
            lg = logits[b, :T].numpy()
            ctc_tol = T * nm.F32_BUDGET * float(np.abs(lg - lg.mean(-1, keepdims=True)).max()) + nm.F32_BUDGET * max(abs(nll), 1.0)
            kls, scale = [], 1.0
            for right in (False, True):
                xl = dec.logits(enc[b].numpy(), T, tok, right=right).numpy()
                kls.append(lo.att_kl(xl, tok, CONF["lsm_weight"], reverse=right)[0])
                scale = max(scale, float(np.abs(xl - xl.mean(-1, keepdims=True)).max()))
            rows = len(tok) + 1
            out.append(dict(nll=float(nll), ctc_tol=ctc_tol, kl=kls[0], r_kl=kls[1], att_tol=2 * nm.F32_BUDGET * rows * scale,
                            rows=rows, frames=T))
        return out
    return _memo.get("ref", go)


def test_model_loss_of_a_conformer_against_the_float64_pipeline():
    from ppasr_amd.model_utils.loss import model_loss
    x, lens = batch()
    ref = pipeline64()
    got = model_loss(conformer(), rescorer(), x, lens, LABELS, LABEL_LENS, **CONF)
    assert got["frames"].tolist() == [r["frames"] for r in ref] and got["rows"].tolist() == [r["rows"] for r in ref]
    assert got["ctc_status"].tolist() == [0, 0, 0]
    for b, r in enumerate(ref):
        print(f"[model_loss] b={b} ctc {got['ctc_nll'][b]:.9g} ref {r['nll']:.9g} tol {r['ctc_tol']:.2e} | att {got['att_kl'][b]:.9g} "
              f"ref {r['kl']:.9g} r_att {got['r_att_kl'][b]:.9g} ref {r['r_kl']:.9g} tol {r['att_tol']:.2e}")
        assert abs(got["ctc_nll"][b] - r["nll"]) <= r["ctc_tol"]
        assert abs(got["att_kl"][b] - r["kl"]) <= r["att_tol"] and abs(got["r_att_kl"][b] - r["r_kl"]) <= r["att_tol"]
    want = lo.combine([r["nll"] for r in ref], [r["kl"] for r in ref], [r["r_kl"] for r in ref], [r["rows"] for r in ref],
                      CONF["ctc_weight"], CONF["reverse_weight"])
    tol = CONF["ctc_weight"] * sum(r["ctc_tol"] for r in ref) / 3 + (1 - CONF["ctc_weight"]) * sum(r["att_tol"] for r in ref) / 3
    for k in ("loss", "loss_att", "loss_ctc"):
        print(f"[model_loss] {k}: got {got[k]:.9g} ref64 {want[k]:.9g}")
    assert abs(got["loss"] - want["loss"]) <= tol
    # the combination itself, from the call's own pieces: exact up to the rounding of a few double operations
    own = lo.combine(got["ctc_nll"], got["att_kl"], got["r_att_kl"], got["rows"], CONF["ctc_weight"], CONF["reverse_weight"])
    for k in ("loss", "loss_att", "loss_ctc"):
        assert got[k] == pytest.approx(own[k], rel=1e-12)
    norm = model_loss(conformer(), rescorer(), x, lens, LABELS, LABEL_LENS, length_normalized_loss=True, **CONF)
    own = lo.combine(norm["ctc_nll"], norm["att_kl"], norm["r_att_kl"], norm["rows"], CONF["ctc_weight"], CONF["reverse_weight"],
                     length_normalized_loss=True)
    assert norm["loss_att"] == pytest.approx(own["loss_att"], rel=1e-12) and norm["loss_att"] < got["loss_att"]


def test_model_loss_branches():
    from ppasr_amd.model_utils.loss import model_loss
    x, lens = batch()
    full = model_loss(conformer(), rescorer(), x, lens, LABELS, LABEL_LENS, **CONF)
    ctc_only = model_loss(conformer(), None, x, lens, LABELS, LABEL_LENS, 1.0)
    assert ctc_only["loss_att"] is None and ctc_only["loss"] == ctc_only["loss_ctc"] == full["loss_ctc"]
    att_only = model_loss(conformer(), rescorer(), x, lens, LABELS, LABEL_LENS, 0.0, 0.1, 0.3)
    assert att_only["loss_ctc"] is None and att_only["loss"] == att_only["loss_att"] == full["loss_att"]
    with pytest.raises(ValueError):
        model_loss(conformer(), None, x, lens, LABELS, LABEL_LENS, 0.3)
    # an utterance whose label does not fit makes the CTC loss inf, as warp-ctc does
    long = np.tile(np.arange(1, 41), (3, 1))
    inf = model_loss(conformer(), None, x, lens, long, np.array([40, 40, 40]), 1.0)
    assert inf["ctc_status"].tolist() == [1, 1, 1] or inf["ctc_status"][2] == 1
    assert inf["loss_ctc"] == np.inf and inf["loss"] == np.inf


def test_model_loss_of_a_deepspeech2():
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
    from ppasr_amd.model_utils.loss import model_loss
    sd = deepspeech2_state_dict(vocab_size=V, num_rnn_layers=2, streaming=True, seed=7)
    model = DeepSpeech2Model(80, V, streaming=True, encoder_conf=dict(num_rnn_layers=2, rnn_size=1024), state_dict=sd)
    x, lens = batch()
    got = model_loss(model, None, x, lens, LABELS, LABEL_LENS, ctc_weight=0.3)  # DeepSpeech2Model.forward is the CTCLoss alone
    assert got["loss_att"] is None and got["loss"] == got["loss_ctc"]
    probs, out_lens = nm.oracle64("deepspeech2", sd, num_rnn_layers=2, streaming=True).forward(x, lens)[:2]
    probs = probs.numpy()
    total = 0.0
    for b in range(3):
        T = int(out_lens[b])
        assert got["frames"][b] == T
        ref, st = lo.ctc_nll(probs[b].astype(np.float32), labels_of(b), T)
        lg = np.log(np.maximum(probs[b, :T], 1e-300))
        tol = T * nm.F32_BUDGET_DS2 * float(np.abs(lg - lg.mean(-1, keepdims=True)).max()) + nm.F32_BUDGET * max(abs(ref), 1.0)
        print(f"[model_loss] ds2 b={b} T={T} got {got['ctc_nll'][b]:.9g} ref64 {ref:.9g} tol {tol:.2e}")
        assert st == lo.OK and abs(got["ctc_nll"][b] - ref) <= tol
        total += ref
    assert got["loss"] == pytest.approx(float(np.sum(got["ctc_nll"]) / 3), rel=1e-12)


def _batches():
    x, lens = batch()
    x2, lens2 = synth_features(2, 99, lens=[99, 80], seed=13)
    return [(x, LABELS, lens, LABEL_LENS), (x2, LABELS[:2, :5], lens2, np.array([5, 4]))]


def test_evaluate_returns_the_pair():
    from ppasr_amd.evaluate import evaluate
    from ppasr_amd.model_utils.loss import model_loss
    vocab = synth_vocabulary(V)
    model, r = conformer(), rescorer()
    plain = evaluate(model, _batches(), vocab)
    assert isinstance(plain, float)
    conf = dict(CONF, accum_grad=2)
    loss, err = evaluate(model, _batches(), vocab, return_loss=True, loss_conf=conf, rescorer=r)
    assert err == plain
    want = np.mean([model_loss(model, r, x, n, y, yn, **CONF)["loss"] / 2 for x, y, n, yn in _batches()])
    assert loss == pytest.approx(float(want), rel=1e-12)
    assert evaluate(model, [], vocab, return_loss=True, loss_conf=conf, rescorer=r) == (-1, -1)
    # through the rescoring decoder too: the same loss, that decoder's error rate
    resc = dict(beam_size=3, ctc_weight=0.5, reverse_weight=0.3)
    loss2, err2 = evaluate(model, _batches(), vocab, decoder="attention_rescoring", rescorer=r, rescoring_conf=resc,
                           return_loss=True, loss_conf=conf)
    assert loss2 == loss
    assert err2 == evaluate(model, _batches(), vocab, decoder="attention_rescoring", rescorer=r, rescoring_conf=resc)
    ctc_only, err3 = evaluate(model, _batches(), vocab, return_loss=True, loss_conf=dict(ctc_weight=1.0))
    assert err3 == plain and np.isfinite(ctc_only)
    assert evaluate(model, _batches(), vocab, decoder="attention_rescoring", rescorer=r, rescoring_conf=resc, return_loss=True,
                    loss_conf=dict(ctc_weight=1.0)) == (ctc_only, err2)
    with pytest.raises(ValueError):
        evaluate(model, _batches(), vocab, return_loss=True, shard="buckets", loss_conf=conf, rescorer=r)
    with pytest.raises(ValueError):
        evaluate(model, _batches(), vocab, return_loss=True, loss_conf=conf)  # ctc_weight < 1 without a rescorer
    with pytest.raises(ValueError):
        evaluate(model, _batches(), vocab, return_loss=True, loss_conf=dict(conf, no_such_key=1), rescorer=r)


def _cfg(decoder):
    return dict(encoder_conf=ENC,
                decoder_conf=dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0], r_num_blocks=BLOCKS[1]),
                preprocess_conf=dict(feature_method="fbank", n_mels=80, sample_rate=16000, use_dB_normalization=True,
                                     target_dB=-20),
                use_model="conformer", streaming=True, decoder=decoder, metrics_type="cer")


def _audio(seconds, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(int(16000 * seconds)) / 16000.0
    x = 0.1 * np.sin(2 * np.pi * 220 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(t.shape)
    return x.astype(np.float32)


def test_predictor_score():
    from ppasr_amd.data_utils.featurizer import AudioFeaturizer
    from ppasr_amd.model_utils.loss import ctc_nll
    from ppasr_amd.predict import PPASRPredictor
    vocab = synth_vocabulary(V)
    p = PPASRPredictor(configs=_cfg("attention_rescoring"), state_dict=checkpoint(), vocab_list=vocab, warmup=False)
    wav = _audio(1.2, seed=5)
    ids = [5, 9, 9, 17, 3]
    text = "".join(vocab[i] for i in ids)
    got = p.score(audio_data=wav, text=text)
    assert set(got) == {"ctc_nll", "att_nll", "tokens", "frames"} and got["tokens"] == len(ids)
    feat = AudioFeaturizer(**_cfg("ctc_greedy")["preprocess_conf"]).featurize(wav)
    x, lens = feat[None].astype(np.float32), np.array([feat.shape[0]], np.int64)
    probs, memory = p.predictor.model.get_encoder_out(x, lens, return_memory=True)
    assert got["frames"] == probs.shape[1]
    lab, n = np.asarray([ids], np.int32), np.asarray([len(ids)], np.int32)
    assert got["ctc_nll"] == float(ctc_nll(probs, lab, n)["nll"][0])
    assert got["att_nll"] == float(p.predictor.rescorer.loss(memory, None, lab, n, 0.0, 0.0)["att_kl"][0])
    assert np.isfinite(got["ctc_nll"]) and got["att_nll"] > 0
    with pytest.raises(ValueError, match="not in the vocabulary"):
        p.score(audio_data=wav, text=text + "☃")
    with pytest.raises(ValueError, match="does not fit"):
        p.score(audio_data=wav, text=text * 20)
    # without decoder weights: the CTC half alone
    sd = {k: v for k, v in checkpoint().items() if not k.startswith("decoder.")}
    q = PPASRPredictor(configs=_cfg("ctc_greedy"), state_dict=sd, vocab_list=vocab, warmup=False)
    only = q.score(audio_data=wav, text=text)
    assert only["att_nll"] is None and only["ctc_nll"] == got["ctc_nll"]


@pytest.mark.parametrize("name", list(lo.MODEL_CASES))
def test_model_loss_against_the_reference_forward(name):
    """tests/golden/ref_loss.npz: the reference's own ConformerModel.forward on two tiny non-streaming checkpoints"""
    import os
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    from ppasr_amd.model_utils.loss import model_loss
    c, m = lo.MODEL_CASES[name], lo.model_case(name)
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_loss.npz"))
    model = ConformerModel(80, c["V"], streaming=False, encoder_conf=dict(ENC, num_blocks=c["num_blocks"]), state_dict=m["sd"])
    r = AttentionRescorer(m["sd"], c["V"], dict(attention_heads=4, linear_units=c["units"], num_blocks=c["blocks"][0],
                                                 r_num_blocks=c["blocks"][1]))
    got = model_loss(model, r, m["x"], m["lens"], m["labels"], m["label_lens"], **c["conf"])
    want, pieces = _memo.get(("pipe", name), lambda: lo.model_pipeline64(name, m))
    tols = lo.model_tolerances(name, pieces)
    assert got["frames"].tolist() == [p["frames"] for p in pieces]
    for k in ("loss", "loss_att", "loss_ctc"):
        ref = float(gold[f"{name}/{k}"])
        print(f"[model_loss] {name} {k}: got {got[k]:.7f} reference {ref:.7f} pipeline64 {want[k]:.7f} tol {tols[k]:.2e}")
        assert abs(got[k] - want[k]) <= tols[k] and abs(got[k] - ref) <= 2 * tols[k]  # (the reference's float32 has its own error)
