"""Regenerate tests/golden/stream_routes.json: which kernels a streaming round launches, and how often, on every route a
stream handle or a session group of the fused 256-wide families can take.

    PPASR_HIP_LIB=<the library of the commit the routes are to be pinned to> python tests/golden/make_stream_routes.py

Needs a GPU.  The fixture is recorded with the library the routes are pinned TO (a host-side refactor records it with its
parent's library and must reproduce it), never with the code under test.  `CASES` and `record` are shared with
tests/test_stream_routes_gpu.py."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "stream_routes.json")

FAMILIES = ("conformer", "efficient", "squeezeformer")
# (caller, sessions listed in a round or None for a handle, chunk frames, setting)
CASES = {
    "handle-67": ("handle", None, 67, "default"),          # c = 16, c_r = 8: consumer-side joins / 16-row weight views
    "handle-131": ("handle", None, 131, "default"),        # c = 32: the plain split route, K / V written in place
    "handle-67-fused": ("handle", None, 67, "fused"),      # ppasr_set_ffn_split(0): fused kernels + k_kv_append
    "handle-67-f16x3": ("handle", None, 67, "f16x3"),      # h3 views on the split units
    "group1-67": ("group", [0], 67, "default"),            # one session, 16 rows: the handle-only routes NOT taken
    "group3-67": ("group", [2, 0, 3], 67, "default"),      # 3 of 4 sessions, shuffled: descriptors, history GLU per layer / up front
    "group3-67-fused": ("group", [2, 0, 3], 67, "fused"),  # the S == 1 branch, the stride layer's included
    "group3-67-f16x3": ("group", [2, 0, 3], 67, "f16x3"),  # h3 on the group's split units
}
V, L = 150, 4
_models = {}


def _model(family):
    """The models of tests/test_route_coverage_gpu.py::_model, one per family and process."""
    if family not in _models:
        spec = importlib.util.spec_from_file_location("test_route_coverage_gpu",
                                                      os.path.join(ROOT, "tests", "test_route_coverage_gpu.py"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))  # (its `from numerics import ...`)
        try:
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        finally:
            sys.path.remove(os.path.join(ROOT, "tests"))
        _models[family] = mod._model(family, 31 if family == "squeezeformer" else 15, V, L)
    return _models[family]


def _group(family, model, n_sessions):
    if family == "conformer":
        from ppasr_amd.model_utils.conformer.model import ConformerStreamGroup as G
    elif family == "efficient":
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerStreamGroup as G
    else:
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerStreamGroup as G
    return G(model, n_sessions)


def record(family, case):
    """-> {kernel name: launches} of the SECOND round of `case` (the caches hold the first round's frames)."""
    import torch
    from ppasr_amd._lib import kernel_profile
    from ppasr_amd.utils.synth import synth_features
    caller, sessions, frames, setting = CASES[case]
    model = _model(family)
    model.set_ffn_split(0 if setting == "fused" else -1)
    model.set_gemm_mode("f16x3" if setting == "f16x3" else "f32")
    try:
        n = 1 if sessions is None else len(sessions)
        x, _ = synth_features(n, 2 * frames, seed=700 + frames)
        if caller == "handle":
            stream = model.new_stream()
            step = lambda r: stream.encode_chunk(x[:, r * frames:(r + 1) * frames], -16)
        else:
            group = _group(family, model, 4)
            step = lambda r: group.encode_chunks(sessions, x[:, r * frames:(r + 1) * frames], want_probs=True)
        step(0)
        with kernel_profile(max_entries=512) as kp:
            step(1)
        torch.cuda.synchronize()
    finally:
        model.set_ffn_split(-1)
        model.set_gemm_mode("f32")
    return {name: n_launches for name, (_ms, n_launches) in sorted(kp.kernels.items())}


def main():
    out = {f"{family}/{case}": record(family, case) for family in FAMILIES for case in CASES}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(out)} cases, {sum(sum(v.values()) for v in out.values())} launches")


if __name__ == "__main__":
    main()
