"""No batched-encode result depends on what the workspace and the output buffers held on entry (tests/poison.py).

Every case builds a fresh model, runs ``get_encoder_out(return_logits=True)`` and ``encode_greedy`` on every route the
handle accepts, and compares the raw bytes of every output with the same calls on zero-filled buffers: under 0xFF and
0x7F fills of every ``torch.empty`` the wrappers make (the kept workspace refilled before each call), and with the
buffers left as a DIFFERENT call on the same model left them (``stale``: a larger batch, other lengths, the split route
with padding skipped and a lengths hint, then the f16x3 arithmetic; from then on every route runs on what the route
before it left behind, so the split count, the block form and the ragged mode all change between calls).

Defined regions (include/ppasr_hip.h): every row of probs / logits (default mode: the reference computes the padded rows
too; ragged mode: zeros behind the valid frames), tokens with their -1 padding, n_tokens, score.  DeepSpeech2: probs in
full as well (the rows behind out_lens are written too), out_lens, the final state boxes -- through get_encoder_out_chunk,
which shares its one call path (DeepSpeech2Model._run) with get_encoder_out."""
import numpy as np
import pytest
import torch

import numerics as nm
import poison
import test_ragged_gpu as rg
from ppasr_amd import _lib
from ppasr_amd.utils.synth import conformer_state_dict, deepspeech2_state_dict, squeezeformer_state_dict, synth_features

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
V = 131

# (name, B, T, lens): one utterance; fully masked utterances (lengths 1 and 0); a ragged batch; two larger ragged batches
# whose LAST utterance is long -- the fused attention reads its values (vt) in whole 64-row sub-blocks of the batch's row
# space, so only the last utterance reads rows behind the batch, which nothing writes: 9x1000 takes the fused attention
# on the ffn_split=0 routes, 9x1900 (9 x 474 rows = 134 row blocks, past the 128 of the default rule) on every route;
# key counts off the 64-row sub-blocks (T' = 65 and 129) next to a 3-frame utterance
SHAPES = [
    ("1x67", 1, 67, [67]),
    ("3x131-masked", 3, 131, [131, 1, 0]),
    ("3x400", 3, 400, [400, 133, 36]),
    ("9x1000", 9, 1000, [873, 640, 36, 512, 7, 401, 259, 131, 1000]),
    ("9x1900", 9, 1900, [1900, 1203, 36, 900, 7, 611, 420, 133, 1899]),
    ("2x263-Tp65", 2, 263, [263, 12]),
    ("2x519-Tp129", 2, 519, [519, 12]),
]

# route knobs; what a handle refuses (PPASR_EUNSUPPORTED) is left out by status, in the clean and the poisoned run alike
ROUTES = [
    ("default", {}),
    ("ffn_split=0", dict(ffn_split=0)),
    ("ffn_split=2", dict(ffn_split=2)),
    ("ffn_split=8", dict(ffn_split=8)),
    ("row_block=16", dict(row_block=16)),
    ("row_block=32", dict(row_block=32)),
    ("row_block=1032", dict(row_block=1032)),
    ("front_fused=0", dict(front_fused=0)),
    ("front_fused=1", dict(front_fused=1)),
    ("skip", dict(skip=True)),
    ("skip+hint", dict(skip=True, hint=True)),
    ("ffn_split=0+skip", dict(ffn_split=0, skip=True)),  # the fused attention over rows a ragged batch skips
    ("ffn_split=0+skip+hint", dict(ffn_split=0, skip=True, hint=True)),
    ("f16x3+row_block=32", dict(gemm="f16x3", row_block=32)),
    ("f16x3+ffn_split=2", dict(gemm="f16x3", ffn_split=2)),
]
FRONT_ROUTES = [r for r in ROUTES if r[0] in ("default", "front_fused=0", "front_fused=1", "skip", "ffn_split=0")] + [
    ("front_fused=0+skip", dict(front_fused=0, skip=True))]


def _accepted(call):
    """Run a knob setter / an encode; False when the handle refuses it as unsupported."""
    try:
        call()
        return True
    except _lib.PPASRHipError as e:
        if e.status != _lib.PPASR_EUNSUPPORTED:
            raise
        return False


def _apply(model, knobs, lens):
    """Every knob to its default, then the route's; -> accepted"""
    _accepted(lambda: model.set_gemm_mode("f32"))
    _accepted(lambda: model.set_ffn_split(-1))
    _accepted(lambda: model.set_row_block(-1))
    _accepted(lambda: model.set_front_fused(-1))
    _accepted(lambda: model.set_skip_padding(False))
    model.set_lengths_hint(None)
    ok = True
    if "ffn_split" in knobs:
        ok &= _accepted(lambda: model.set_ffn_split(knobs["ffn_split"]))
    if "row_block" in knobs:
        ok &= _accepted(lambda: model.set_row_block(knobs["row_block"]))
    if "front_fused" in knobs:
        ok &= _accepted(lambda: model.set_front_fused(knobs["front_fused"]))
    if knobs.get("skip"):
        ok &= _accepted(lambda: model.set_skip_padding(True))
    if knobs.get("hint"):
        model.set_lengths_hint([int(v) for v in lens])
    if "gemm" in knobs:
        ok &= _accepted(lambda: model.set_gemm_mode(knobs["gemm"]))
    return ok


def _stale_calls(model, B, T):
    """What leaves state behind for the call under test: a larger batch with other lengths on the 8-way split route with
    padding skipped and a hint, the f16x3 arithmetic on 32-row blocks, the 2-way split."""
    F = model.input_dim
    Bb, Tb = B + 2, T + 160
    lens = [Tb] + [int(v) for v in np.linspace(Tb - 31, 9, Bb - 1)]
    x, la = synth_features(Bb, Tb, n_mels=F, lens=lens, seed=977)
    for knobs in (dict(ffn_split=8, skip=True, hint=True), dict(gemm="f16x3", row_block=32), dict(ffn_split=2)):
        if _apply(model, knobs, la):
            _accepted(lambda: model.get_encoder_out(x, la, return_logits=True))
            _accepted(lambda: model.encode_greedy(x, la, trim_to_length=True))
    _apply(model, {}, la)


def _encode_case(build, B, T, lens, routes):
    def run(s):
        model = build()
        x, la = synth_features(B, T, n_mels=model.input_dim, lens=lens, seed=B * 1000 + T)
        if s.stale:
            _stale_calls(model, B, T)
        outs = {}
        for name, knobs in routes:
            if not _apply(model, knobs, la):
                print(f"[poison] {name}: refused by the handle (PPASR_EUNSUPPORTED)")
                outs[name + "/refused"] = torch.zeros(1)
                continue
            got = {}

            def call():
                s.scratch(model)
                p, l = model.get_encoder_out(x, la, return_logits=True)
                s.observe(model, name + " get_encoder_out")
                got.update(probs=p, logits=l)
                for trim in sorted({bool(knobs.get("skip")), name == "default"}):
                    s.scratch(model)
                    t, n, sc = model.encode_greedy(x, la, trim_to_length=trim)
                    s.observe(model, name + f" encode_greedy trim={trim}")
                    got.update({f"tokens/trim={trim}": t, f"n_tokens/trim={trim}": n, f"score/trim={trim}": sc})

            if not _accepted(call):
                print(f"[poison] {name}: call refused by the handle (PPASR_EUNSUPPORTED)")
                outs[name + "/refused"] = torch.zeros(1)
                continue
            torch.cuda.synchronize()
            outs.update({f"{name}/{k}": v for k, v in got.items()})
        assert any(not k.endswith("/refused") for k in outs)
        return outs, model
    return run


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("family", list(rg.FAMILIES))
def test_batched_encode(family, shape, pattern, monkeypatch):
    name, B, T, lens = shape
    case = f"encode {family} {name}"
    poison.check(case, _encode_case(lambda: rg.FAMILIES[family](V)[0], B, T, lens, ROUTES), pattern, monkeypatch, MEMO)


# ---- the front ends' own scratch ---------------------------------------------------------------------------------------
def _conformer_front(F, input_layer="conv2d"):
    from ppasr_amd.model_utils.conformer.model import ConformerModel
    sd = conformer_state_dict(input_dim=F, vocab_size=V, num_blocks=1, seed=640 + F, perturb_norm=True, input_layer=input_layer)
    conf = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=1, cnn_module_kernel=15, input_layer=input_layer)
    return ConformerModel(F, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


def _squeezeformer_front(F):
    from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel
    sd = squeezeformer_state_dict(input_dim=F, vocab_size=V, num_blocks=2, seed=740 + F, perturb_norm=True)
    conf = dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=2, reduce_idx=None, recover_idx=None,
                feed_forward_expansion_factor=8, cnn_module_kernel=31)
    return SqueezeformerModel(F, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")


# the buffers the narrow-width fix resized: fewer than 16 conv1 bins (F = 12: F1 = 5), conv2d8 at F2 = 3 (F = 16);
# the quad-form conv2 at odd and even T' (T = 71 -> 17, T = 67 -> 16) and odd and even F2 (80 bins -> 19, 86 -> 20): the
# two-launch route reads y1 from the workspace, and a quad at an odd edge covers a frame or a bin that no launch wrote
FRONTS = {
    "conformer-F12": (lambda: _conformer_front(12), [(3, 131, [131, 77, 9]), (2, 67, [67, 30])]),
    "conv2d8-F16": (lambda: _conformer_front(16, "conv2d8"), [(4, 131, [131, 123, 60, 15]), (1, 67, [67])]),
    "conv2d8-F18": (lambda: _conformer_front(18, "conv2d8"), [(2, 101, [101, 93])]),
    "conformer-F80-quad": (lambda: _conformer_front(80), [(2, 71, [71, 30]), (2, 67, [67, 30]), (3, 131, [131, 1, 0])]),
    "conformer-F86-quad": (lambda: _conformer_front(86), [(2, 71, [71, 30]), (2, 67, [67, 30])]),
    "squeezeformer-F80-quad": (lambda: _squeezeformer_front(80), [(2, 71, [71, 30]), (2, 67, [67, 30])]),
    "squeezeformer-F86-quad": (lambda: _squeezeformer_front(86), [(2, 71, [71, 30]), (2, 67, [67, 30])]),
}


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("front", list(FRONTS))
def test_front_end_scratch(front, pattern, monkeypatch):
    build, shapes = FRONTS[front]
    for B, T, lens in shapes:
        poison.check(f"front {front} {B}x{T}", _encode_case(build, B, T, lens, FRONT_ROUTES), pattern, monkeypatch, MEMO)


# ---- DeepSpeech2 -------------------------------------------------------------------------------------------------------
def _ds2(streaming, gru):
    from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model
    L = 3
    sd = deepspeech2_state_dict(vocab_size=60, num_rnn_layers=L, streaming=streaming, seed=5, use_gru=gru)
    return DeepSpeech2Model(80, 60, streaming=streaming, encoder_conf=dict(num_rnn_layers=L, rnn_size=1024, use_gru=gru),
                            state_dict=sd, device="cuda:0")


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("B", [1, 3, 6])
@pytest.mark.parametrize("streaming", [True, False], ids=["streaming", "bidirectional"])
@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
def test_deepspeech2(gru, streaming, B, pattern, monkeypatch):
    """Two calls, the first one's final state boxes starting the second (what predict_chunk_deepspeech carries)."""
    T = 131
    lens = [T] + [int(v) for v in np.linspace(120, 5, B - 1)]
    x, la = synth_features(B, 2 * T, lens=[2 * n for n in lens], seed=B + 40)

    def run(s):
        m = _ds2(streaming, gru)
        if s.stale:
            xb, lb = synth_features(B + 2, T + 100, lens=[T + 100] + [int(v) for v in np.linspace(200, 30, B + 1)], seed=41)
            m.get_encoder_out_chunk(xb, lb)
            m.get_encoder_out(xb[:1, :67], lb[:1].clip(max=67))
        outs, h, c = {}, None, None
        for k in range(2):
            lk = np.clip(la - k * T, 0, T)
            s.scratch(m)
            probs, out_lens, h, c = m.get_encoder_out_chunk(x[:, k * T:(k + 1) * T], lk, h, c)
            s.observe(m, f"call {k}")
            torch.cuda.synchronize()
            outs.update({f"{k}/probs": probs, f"{k}/out_lens": out_lens, f"{k}/h": h, f"{k}/c": c})
        return outs, m

    kind = ("gru" if gru else "lstm") + ("-streaming" if streaming else "-bidirectional")
    poison.check(f"ds2 {kind} B={B}", run, pattern, monkeypatch, MEMO)
