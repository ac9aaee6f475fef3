"""Regenerate tests/golden/ref_decoder.npz by running the REFERENCE's OWN attention decoder.

    python tests/golden/make_decoder_goldens.py

Like make_ref_goldens.py: `sys.path[:0] = [oracle/paddle_shim, /root/reference]`, so that
`ppasr/model_utils/transformer/decoder.py` (BiTransformerDecoder) imports and runs unmodified on the torch-backed shim.
For every case of decoder_cases.FIXTURE_CASES the reference decoder is built with the case's shape, the seeded synthetic
state dict (decoder_cases.weights) is loaded BY NAME -- every name and shape must be one of the decoder's own
`state_dict()` and none of its names may stay without a value -- the inputs are built with the reference's own
`add_sos_eos` / `reverse_pad_list`, and `forward(memory, memory_mask, ys_in, lens + 1, r_ys_in, reverse_weight)` is called.

Stored per case: `<name>/l_x`, `<name>/r_x`: the decoders' outputs on the valid rows, float32, [hypotheses that exist,
in (b, n) order][positions 0 .. len] concatenated -> [rows, V].  Inputs and weights come from the seed and are not
stored.  Needs /root/reference, so it runs in the build container only; the .npz travels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import decoder_cases as dc  # noqa: E402


def main():
    if not os.path.isdir(REFERENCE):
        raise SystemExit("needs /root/reference (build container only)")
    sys.path[:0] = [os.path.join(ROOT, "oracle", "paddle_shim"), REFERENCE]
    import paddle
    import torch
    torch.set_grad_enabled(False)
    from ppasr.model_utils.transformer.decoder import BiTransformerDecoder
    from ppasr.model_utils.utils.common import add_sos_eos, reverse_pad_list

    out = {}
    for name in dc.FIXTURE_CASES:
        case = dc.CASES[name]
        V = case["V"]
        sd = {k[len("decoder."):]: v for k, v in dc.weights(case).items()}
        dec = BiTransformerDecoder(V, dc.D, attention_heads=dc.HEADS, linear_units=case["units"],
                                   num_blocks=case["blocks"][0], r_num_blocks=case["blocks"][1], dropout_rate=0.1,
                                   positional_dropout_rate=0.1, self_attention_dropout_rate=0.1,
                                   src_attention_dropout_rate=0.1)
        own = dec.state_dict()
        for k, v in sd.items():
            assert k in own, f"{name}: synthetic parameter {k} is not a name of the reference decoder"
            assert list(own[k].shape) == list(v.shape), f"{name}: {k} shape {v.shape} vs reference {own[k].shape}"
        unset = [k for k in own if k not in sd]
        assert not unset, f"{name}: reference parameters without a synthetic value: {unset[:8]}"
        missing, unexpected = dec.set_state_dict(sd)
        assert not missing and not unexpected, (missing, unexpected)
        dec.eval()
        inp = dc.inputs(case)
        l_rows, r_rows = [], []
        for b in range(case["B"]):
            keep = [k for k in range(case["nbest"]) if inp["lens"][b, k] >= 0]
            lens = inp["lens"][b, keep].astype(np.int64)
            mt = max(int(lens.max()), 1)
            ys = np.full((len(keep), mt), -1, np.int64)
            for i, k in enumerate(keep):
                ys[i, :lens[i]] = inp["tokens"][b, k, :lens[i]]
            ys_pad = paddle.to_tensor(ys)
            ys_lens = paddle.to_tensor(lens)
            ys_in, _ = add_sos_eos(ys_pad, V - 1, V - 1, -1)
            # (the shim's pad_sequence does not take an empty sequence: the reverse of the empty hypothesis is a row of
            #  padding, put in by hand around the reference's own call on the others)
            some = np.nonzero(lens > 0)[0]
            r_np = np.full((len(keep), mt), -1, np.int64)
            if some.size:
                r_some = reverse_pad_list(paddle.to_tensor(ys[some]), paddle.to_tensor(lens[some]), -1.0).numpy()
                r_np[some, :r_some.shape[1]] = r_some
            r_ys = paddle.to_tensor(r_np)
            r_ys_in, _ = add_sos_eos(r_ys, V - 1, V - 1, -1)
            ol = int(inp["out_lens"][b])
            memory = paddle.to_tensor(np.repeat(inp["memory"][b:b + 1], len(keep), 0))
            mask = paddle.to_tensor((np.arange(case["Tp"]) < ol)[None, None, :].repeat(len(keep), 0))
            l_x, r_x, _ = dec(memory, mask, ys_in, ys_lens + 1, r_ys_in, case["reverse_weight"])
            for i in range(len(keep)):
                l_rows.append(l_x.numpy()[i, :lens[i] + 1])
                if case["reverse_weight"] > 0:
                    r_rows.append(r_x.numpy()[i, :lens[i] + 1])
        out[f"{name}/l_x"] = np.concatenate(l_rows).astype(np.float32)
        out[f"{name}/r_x"] = (np.concatenate(r_rows) if r_rows else np.zeros((0, V))).astype(np.float32)
        print(f"[ref] {name}: l_x {out[name + '/l_x'].shape} r_x {out[name + '/r_x'].shape}", flush=True)
    path = os.path.join(HERE, "ref_decoder.npz")
    np.savez_compressed(path, **out)
    print("wrote ref_decoder.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
