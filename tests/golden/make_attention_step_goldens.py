"""Regenerate tests/golden/ref_decoder_steps.npz by running the REFERENCE's OWN `TransformerDecoder.forward_one_step`
with its cache, the incremental step the attention beam search is built on.

    python tests/golden/make_attention_step_goldens.py

Like make_decoder_goldens.py: `sys.path[:0] = [oracle/paddle_shim, /root/reference]`, the reference decoder is built with
the case's shape and the seeded synthetic state dict (attention_search_cases.weights) is loaded by name.  For every case
of attention_search_cases.STEP_CASES and every utterance, a fixed prefix (step_prefix) is fed one token at a time: step t calls
`forward_one_step(memory, memory_mask, [sos] + prefix[:t], subsequent_mask(t + 1), cache)` and keeps the cache it returns.

Stored per case: `<name>/logp` float32 [B, len(prefix) + 1, V], the log-probabilities each step returned.  Inputs and
weights come from the seed and are not stored.  Needs /root/reference, so it runs in the build container only; the .npz
travels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attention_search_cases as ac  # noqa: E402
import decoder_cases as dc  # noqa: E402

from attention_search_cases import PREFIX_LEN, STEP_CASES, step_prefix  # noqa: E402


def main():
    if not os.path.isdir(REFERENCE):
        raise SystemExit("needs /root/reference (build container only)")
    sys.path[:0] = [os.path.join(ROOT, "oracle", "paddle_shim"), REFERENCE]
    import paddle
    import torch
    torch.set_grad_enabled(False)
    from ppasr.model_utils.transformer.decoder import BiTransformerDecoder
    from ppasr.model_utils.utils.mask import subsequent_mask

    out = {}
    for name in STEP_CASES:
        case = ac.CASES[name]
        V = case["V"]
        sd = {k[len("decoder."):]: v for k, v in ac.weights(case).items()}
        dec = BiTransformerDecoder(V, dc.D, attention_heads=dc.HEADS, linear_units=case["units"],
                                   num_blocks=case["blocks"][0], r_num_blocks=case["blocks"][1], dropout_rate=0.1,
                                   positional_dropout_rate=0.1, self_attention_dropout_rate=0.1,
                                   src_attention_dropout_rate=0.1)
        own = dec.state_dict()
        assert set(own) == set(sd), sorted(set(own) ^ set(sd))[:8]
        missing, unexpected = dec.set_state_dict(sd)
        assert not missing and not unexpected, (missing, unexpected)
        dec.eval()
        inp = ac.inputs(case)
        rows = np.zeros((case["B"], PREFIX_LEN + 1, V), np.float32)
        for b in range(case["B"]):
            memory = paddle.to_tensor(inp["memory"][b:b + 1])
            mask = paddle.to_tensor((np.arange(case["Tp"]) < int(inp["out_lens"][b]))[None, None, :])
            ys = [V - 1] + step_prefix(case, b)
            cache = None
            for t in range(PREFIX_LEN + 1):
                tgt = paddle.to_tensor(np.asarray([ys[:t + 1]], np.int64))
                tgt_mask = subsequent_mask(t + 1).unsqueeze(0)
                logp, cache = dec.left_decoder.forward_one_step(memory, mask, tgt, tgt_mask, cache)
                rows[b, t] = logp.numpy()[0]
        out[f"{name}/logp"] = rows
        print(f"[ref] {name}: logp {rows.shape}", flush=True)
    path = os.path.join(HERE, "ref_decoder_steps.npz")
    np.savez_compressed(path, **out)
    print("wrote ref_decoder_steps.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
