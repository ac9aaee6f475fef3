"""Regenerate tests/golden/encode_routes.json: which kernels an offline encode launches, and how often, on every route the
host-side walks of ppasr_encode choose between (encode_impl, squeezeformer_encode, and gen_layers / sq_run of the general
route).

    PPASR_HIP_LIB=<the library of the commit the routes are to be pinned to> python tests/golden/make_encode_routes.py

Needs a GPU.  The fixture is recorded with the library the routes are pinned TO (a host-side refactor records it with its
parent's library and must reproduce it), never with the code under test.  `MODELS`, `CASES`, `cases_of`, `setup` and
`record` are shared with tests/test_encode_routes_gpu.py."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "encode_routes.json")

V, L = 150, 4
FUSED = ("conformer", "efficient", "squeezeformer")
W16 = 1032  # PPASR_ROW_BLOCK_32_W16
RAGGED = (400, 131, 67)  # lengths of a ragged batch, repeated over its utterances

# (B, T, settings): the smallest shape at which each route is chosen
CASES = {
    "1x67": (1, 67, {}),                                  # split route, S = 8, one row block; Squeezeformer: 16-row views
    "3x131": (3, 131, {}),                                # split route, several blocks
    "12x400": (12, 400, {}),                              # 38 blocks of 32 rows: 16-row kernels, stand-alone attention
    "17x1000": (17, 1000, {}),                            # 133 blocks: fused attention by the default rule
    "3x131-ff": (3, 131, dict(ffn_split=0)),              # fused attention, NEXT tails; efficient: the stride layer has none
    "3x131-w16": (3, 131, dict(ffn_split=0, row_block=W16)),  # 16-wave form
    "17x1000-s2": (17, 1000, dict(ffn_split=2)),          # forced split of a large batch: k_ln_qkv, two-kernel attention
    "3x131-ff-f16x3": (3, 131, dict(ffn_split=0, gemm="f16x3")),  # h3 fused units, h3 front end and head
    "1x67-f16x3": (1, 67, dict(gemm="f16x3")),            # h3 split units
    "3x400-ragged": (3, 400, dict(ragged=True)),          # block tables, conv2's tile table
    "3x400-ragged-ff": (3, 400, dict(ragged=True, ffn_split=0)),  # ... at two rates, the fused-route clear
    "12x400-ragged": (12, 400, dict(ragged=True)),        # ... 12 utterances
    "21x400-ragged": (21, 400, dict(ragged=True)),        # 38 blocks of 32 needed rows: a table of 16-row blocks
    "3x131-taps": (3, 131, dict(taps=True)),              # debug taps: 32-row blocks, two-kernel attention, outputs stored
    "3x131-ff-taps": (3, 131, dict(ffn_split=0, taps=True)),  # ... on the fused kernels: the exclusions change the route
    "3x131-front2": (3, 131, dict(front_fused=0)),        # conv1 + quad conv2
    "2x131": (2, 131, {}),
}
# model -> its cases
MODELS = {
    **{f: [c for c in CASES if c != "2x131"] for f in FUSED},
    "conformer-conv2d6": ["2x131"],                       # the other front ends of the fused route
    "conformer-conv2d8": ["2x131"],
    "conformer-512": ["2x131", "3x400-ragged"],           # general route: the tail of gen_layers
    "squeezeformer-512": ["2x131", "3x400-ragged"],       # ... and of sq_run
}
_models = {}


def cases_of():
    return [(m, c) for m in MODELS for c in MODELS[m]]


def _route_coverage():
    spec = importlib.util.spec_from_file_location("test_route_coverage_gpu",
                                                  os.path.join(ROOT, "tests", "test_route_coverage_gpu.py"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))  # (its `from numerics import ...`)
    try:
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "tests"))
    return mod


def _model(name):
    """The 4-layer models of tests/test_route_coverage_gpu.py::_model (15 taps, the Squeezeformer 31), their Conformer with the
    6x / 8x front end, and the width-512 ones of the general route; one per name and process."""
    if name in _models:
        return _models[name]
    from ppasr_amd.utils.synth import conformer_state_dict, squeezeformer_state_dict
    if name in FUSED:
        m = _route_coverage()._model(name, 31 if name == "squeezeformer" else 15, V, L)
    elif name == "squeezeformer-512":
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel
        conf = dict(encoder_dim=512, output_size=512, attention_heads=8, num_blocks=L, reduce_idx=1, recover_idx=3,
                    feed_forward_expansion_factor=4, cnn_module_kernel=31)
        sd = squeezeformer_state_dict(vocab_size=V, num_blocks=L, cnn_module_kernel=31, seed=551, perturb_norm=True,
                                      encoder_dim=512, attention_heads=8, feed_forward_expansion_factor=4)
        m = SqueezeformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    else:
        from ppasr_amd.model_utils.conformer.model import ConformerModel
        kw = dict(output_size=512, attention_heads=8) if name == "conformer-512" else dict(input_layer=name.split("-")[1])
        sd = conformer_state_dict(vocab_size=V, num_blocks=L, cnn_module_kernel=15, seed=550, **kw)
        conf = {**dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=L, cnn_module_kernel=15), **kw}
        m = ConformerModel(80, V, streaming=True, encoder_conf=conf, state_dict=sd, device="cuda:0")
    _models[name] = m
    return m


class setup:
    """``with setup(name, case) as (model, x, lens): ...`` -- the model with the case's settings and its batch; every setting
    is restored on the way out."""

    def __init__(self, name, case):
        self.name, self.case = name, case

    def __enter__(self):
        from ppasr_amd.utils.synth import synth_features
        B, T, s = CASES[self.case]
        self.model = m = _model(self.name)
        lens = [RAGGED[b % 3] for b in range(B)] if s.get("ragged") else None
        x, xl = synth_features(B, T, lens=lens, seed=800 + T + B)
        m.set_ffn_split(s.get("ffn_split", -1))
        m.set_row_block(s.get("row_block", -1))
        m.set_front_fused(s.get("front_fused", -1))
        m.set_gemm_mode(s.get("gemm", "f32"))
        if s.get("ragged"):
            m.set_skip_padding(True)
            m.set_lengths_hint(lens)
        if s.get("taps"):
            rows = B * m.out_frames(T)
            m.set_debug_taps((1 + 8 * L) * rows * 256)  # (x0, then at most 8 tensors of at most `rows` rows per layer)
        return m, x, xl

    def __exit__(self, *exc):
        m = self.model
        m.set_ffn_split(-1)
        m.set_row_block(-1)
        m.set_front_fused(-1)
        m.set_gemm_mode("f32")
        m.set_skip_padding(False)
        m.set_lengths_hint(None)
        m.set_debug_taps(0)
        return False


def record(name, case):
    """-> {kernel name: launches} of two encodes of `case`: probabilities + logits, then the greedy path (frame argmax /
    maxprob only, and the collapse kernel behind it)."""
    import torch
    from ppasr_amd._lib import kernel_profile
    with setup(name, case) as (model, x, lens):
        with kernel_profile(max_entries=512) as kp:
            model.get_encoder_out(x, lens, return_logits=True)
            model.encode_greedy(x, lens)
        torch.cuda.synchronize()
    return {k: n_launches for k, (_ms, n_launches) in sorted(kp.kernels.items())}


def main():
    out = {f"{name}/{case}": record(name, case) for name, case in cases_of()}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(out)} cases, {sum(sum(v.values()) for v in out.values())} launches")


if __name__ == "__main__":
    main()
