"""Attention beam-search decoding (csrc/attn_decode.hip) measured; one JSON line, run on one otherwise idle MI355X:

    python tools/bench_attention_decode.py [--reps R] [--warmup W] [--B 32] [--ctc-weight 0.5]
                                           [--out profiles/attention_decode.jsonl]

Workload: B = 32 utterances x T' = 250 x beam 10 x V = 4233, 3 + 3 decoder blocks of 1024 units, max_steps = T'.  The
decoder is synthetic (tests/decoder_cases.py); the output bias of the eos column is chosen by a scan, the first value at
which the search of this batch ends after 30 to 50 steps.
  hip          ``AttentionRescorer.decode`` with max_steps = 250: every step is enqueued, the steps behind ``steps_run``
               return at once (the dead tail)
  hip_live     the same with max_steps = steps_run: no dead tail.  time per live step = hip_live / steps_run; the dead
               tail costs hip - hip_live
  torch_f32    the same search in torch float32 on the same device with tests/decoder_oracle.py's weights, the way the
               reference's ``forward_one_step`` computes a step: a cache of layer outputs per row, the prefix's self-attention
               keys and values recomputed from it at every step, the caches gathered when the beam reorders, and one
               read-back per step for the stopping test (WeNet's ``recognize``).  The cross-attention keys and values are
               computed once, which the reference does not do: the stand-in is given that much.
  rescore      for scale: ``ppasr_rescore`` (left decoder only) of the hypotheses the search returned
``--ctc-weight W`` (W > 0) adds the CTC-joint search (csrc/attn_decode_joint.hip) of the same batch and decoder: the CTC table
is peaked (0.9) on a seeded transcript of 30 to 40 tokens per utterance, so the joint search follows the transcripts.
  hip_joint / hip_joint_live   ``AttentionRescorer.decode(..., ctc_probs, ctc_weight=W)``, as hip / hip_live
  torch_joint_f32              torch_search with the CTC prefix score in torch float32 on the same device: Psi of every
               (row, v) as one logsumexp over a [B, N, T, V] tensor per step, the state of the N new rows by a loop over
               the frames (the recurrence is sequential in t)
A host clock around work that ends in a device synchronise; W warm-up calls, then median and 10th / 90th percentile over R."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

V, TP, BEAM, UNITS, BLOCKS = 4233, 250, 10, 1024, (3, 3)
DEC_CONF = dict(attention_heads=4, linear_units=UNITS, num_blocks=BLOCKS[0], r_num_blocks=BLOCKS[1])


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "p10_p90_ms": [round(float(np.percentile(ms, q)), 3) for q in (10, 90)]}


def _timed(fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


@torch.no_grad()
def torch_search(o, memory, out_lens, N, P, ctc=None):
    """the beam search over DecoderOracle's weights (float32, on the device), a step computed as forward_one_step does
    -> (tokens [B, N, <= P], scores [B, N], steps).  ctc = (x [B, T, V] log emissions, blank, weight): the CTC-joint search
    (every frame valid)"""
    dev = memory.device
    B, Tp, d = memory.shape
    R, Vv, H = B * N, o.V, o.H
    eos, dk, L, p = Vv - 1, d // o.H, o.blocks["left"], "decoder.left_decoder"
    heads = lambda t: t.reshape(t.shape[0], t.shape[1], H, dk).transpose(1, 2)
    ck = [heads(o._lin(memory, f"{p}.decoders.{i}.src_attn.linear_k")).repeat_interleave(N, 0) for i in range(L)]
    cv = [heads(o._lin(memory, f"{p}.decoders.{i}.src_attn.linear_v")).repeat_interleave(N, 0) for i in range(L)]
    ol = torch.full((B,), Tp, device=dev) if out_lens is None else out_lens.to(dev).long()
    mask = (torch.arange(Tp, device=dev)[None] < ol[:, None]).repeat_interleave(N, 0)[:, None, None, :]
    scores = torch.full((B, N), float("-inf"), dtype=torch.float64, device=dev)
    scores[:, 0] = 0.0
    ended = torch.zeros(B, N, dtype=torch.bool, device=dev)
    toks = torch.full((R, 1), eos, dtype=torch.long, device=dev)
    cache = [None] * L
    base = (torch.arange(B, device=dev) * N)[:, None]
    neg = torch.full((B, N, N - 1), float("-inf"), dtype=torch.float64, device=dev)
    steps = 0
    if ctc is not None:
        assert out_lens is None
        xc, blank, w = ctc
        ninf = float("-inf")
        rn = torch.full((R, Tp), ninf, device=dev)
        rb = xc[:, :, blank].cumsum(1).repeat_interleave(N, 0)
        psi_g = torch.zeros(B, N, device=dev)
        last = torch.full((R,), -1, dtype=torch.long, device=dev)
        bidx = torch.arange(B, device=dev).repeat_interleave(N)
    for i in range(1, P + 1):
        x = o.w[p + ".embed.0.weight"][toks] * (d ** 0.5) + o.pe[:i]
        new_cache = []
        for l in range(L):
            lp = f"{p}.decoders.{l}"
            y = o._ln(x, lp + ".norm1")  # every prefix row: the keys and values are recomputed from the cached outputs
            q = heads(o._lin(y[:, -1:], lp + ".self_attn.linear_q"))
            k, v = heads(o._lin(y, lp + ".self_attn.linear_k")), heads(o._lin(y, lp + ".self_attn.linear_v"))
            a = torch.softmax(q @ k.transpose(2, 3) / dk ** 0.5, -1) @ v
            xl = x[:, -1:] + o._lin(a.transpose(1, 2).reshape(R, 1, d), lp + ".self_attn.linear_out")
            q = heads(o._lin(o._ln(xl, lp + ".norm2"), lp + ".src_attn.linear_q"))
            s = (q @ ck[l].transpose(2, 3) / dk ** 0.5).masked_fill(~mask, float("-inf"))
            a = torch.softmax(s, -1) @ cv[l]
            xl = xl + o._lin(a.transpose(1, 2).reshape(R, 1, d), lp + ".src_attn.linear_out")
            h = torch.relu(o._lin(o._ln(xl, lp + ".norm3"), lp + ".feed_forward.w_1"))
            xl = xl + o._lin(h, lp + ".feed_forward.w_2")
            x = xl if cache[l] is None else torch.cat([cache[l], xl], 1)
            new_cache.append(x)
        logp = torch.log_softmax(o._lin(o._ln(x[:, -1], p + ".after_norm"), p + ".output_layer"), -1).reshape(B, N, Vv)
        if ctc is not None:
            first = torch.full((R, 1), 0.0 if i == 1 else ninf, device=dev)
            php = torch.cat([first, torch.logaddexp(rn, rb)[:, :-1]], 1)  # phi[t - 1]
            pbp = torch.cat([first, rb[:, :-1]], 1)
            psi = torch.logsumexp(php.reshape(B, N, Tp, 1) + xc[:, None], 2)  # [B, N, V]
            at_last = torch.logsumexp(pbp + xc[bidx, :, last.clamp(min=0)], 1)
            psi.view(R, Vv)[last >= 0, last[last >= 0]] = at_last[last >= 0]
            psi[:, :, blank] = ninf
            psi[:, :, eos] = torch.logaddexp(rn[:, -1], rb[:, -1]).reshape(B, N)
            logp = logp + w * (psi - psi_g[:, :, None])
        top_lp, top_id = logp.topk(N, -1)
        cand = scores[:, :, None] + top_lp.double()
        cand = torch.where(ended[:, :, None], torch.cat([scores[:, :, None], neg], 2), cand)
        tok = torch.where(ended[:, :, None], torch.full_like(top_id, eos), top_id)
        scores, idx = cand.reshape(B, N * N).topk(N, 1)
        par = idx // N
        tok_new = tok.reshape(B, N * N).gather(1, idx)
        gidx = (base + par).reshape(-1)
        toks = torch.cat([toks[gidx], tok_new.reshape(R, 1)], 1)
        cache = [c[gidx] for c in new_cache]
        if ctc is not None:
            was = ended.gather(1, par).reshape(R)
            c = tok_new.reshape(R)
            keep = was | (c == eos) | ~torch.isfinite(scores.reshape(R))  # rows that take no token keep their parent's state
            cc = torch.where(keep, torch.zeros_like(c), c)
            ph = torch.where((cc == last[gidx])[:, None], pbp[gidx], php[gidx])
            x_c, x_b = xc[bidx, :, cc], xc[bidx, :, blank]
            prn = prb = torch.full((R,), ninf, device=dev)
            nrn, nrb = [], []
            for t in range(Tp):  # the recurrence is sequential in t
                prn, prb = torch.logaddexp(prn, ph[:, t]) + x_c[:, t], torch.logaddexp(prn, prb) + x_b[:, t]
                nrn.append(prn)
                nrb.append(prb)
            rn = torch.where(keep[:, None], rn[gidx], torch.stack(nrn, 1))
            rb = torch.where(keep[:, None], rb[gidx], torch.stack(nrb, 1))
            new_psi = psi.reshape(B, N * Vv).gather(1, par * Vv + tok_new)
            psi_g = torch.where(was.reshape(B, N), psi_g.gather(1, par), new_psi)
            last = torch.where(keep, last[gidx], c)
        ended = ended.gather(1, par) | (tok_new == eos)
        steps = i
        if bool((ended | ~torch.isfinite(scores)).all()):  # (the read-back of WeNet's loop)
            break
    return toks[:, 1:].reshape(B, N, -1), scores, steps


def main():
    import decoder_cases as dc
    from decoder_oracle import DecoderOracle
    from ppasr_amd.decoders.attention_rescoring import AttentionRescorer
    reps, warmup, B = _arg("--reps", 7), _arg("--warmup", 2), _arg("--B", 32)
    path = _arg("--out", None, str)
    sd = dc.decoder_state_dict(4321, V, UNITS, *BLOCKS)
    memory = torch.from_numpy(np.random.default_rng(B).standard_normal((B, TP, 256)).astype(np.float32)).cuda()
    bias0 = sd["decoder.left_decoder.output_layer.bias"].copy()
    chosen, scan = None, []
    for eb in np.arange(12.0, -8.25, -0.25):  # from "ends at once" downwards: the first value inside 30 .. 50 steps
        b = bias0.copy()
        b[V - 1] += np.float32(eb)
        sd["decoder.left_decoder.output_layer.bias"] = b
        r = AttentionRescorer(sd, V, DEC_CONF)
        steps = int(r.decode(memory, None, BEAM, TP)["steps_run"].cpu()[0])
        scan.append([float(eb), steps])
        if 30 <= steps <= 50:
            chosen = float(eb)
            break
        del r
        if steps > 50:
            break
    if chosen is None:
        print(json.dumps({"section": "attention_decode", "error": "no eos bias of the scan ends within 30 .. 50 steps",
                          "scan": scan}), flush=True)
        return
    res = r.decode(memory, None, BEAM, TP)
    steps = int(res["steps_run"].cpu()[0])
    lens = res["lens"].cpu().numpy()
    hip = _timed(lambda: r.decode(memory, None, BEAM, TP), reps, warmup)
    live = _timed(lambda: r.decode(memory, None, BEAM, steps), reps, warmup)
    zeros = torch.zeros(B, BEAM, dtype=torch.float64, device="cuda")
    tk, ln = res["tokens"][:, :, :max(int(lens.max()), 1)].clamp(min=0).contiguous(), res["lens"]
    resc = _timed(lambda: r.rescore(memory, None, tk, ln, zeros, 0.0, 0.0), reps, warmup)
    o32 = DecoderOracle(sd, V, *BLOCKS, dtype=torch.float32).to("cuda:0")
    tor = _timed(lambda: torch_search(o32, memory, None, BEAM, TP), reps, warmup)
    t_tok, t_sc, t_steps = torch_search(o32, memory, None, BEAM, TP)
    same = 0
    for b in range(B):
        n = int(lens[b, 0])
        row = t_tok[b, 0].cpu().numpy()
        same += int(row[:n].tolist() == res["tokens"][b, 0, :n].cpu().tolist() and (row[n:] == V - 1).all())
    rec = {"section": "attention_decode", "B": B, "Tp": TP, "V": V, "beam": BEAM, "blocks": list(BLOCKS), "units": UNITS,
           "max_steps": TP, "eos_bias": chosen, "steps_run": steps, "torch_steps": t_steps,
           "best_hypothesis_tokens_min_mean_max": [int(lens[:, 0].min()), round(float(lens[:, 0].mean()), 1), int(lens[:, 0].max())],
           "reps": reps, "hip": _stats(hip), "hip_live": _stats(live), "torch_f32": _stats(tor), "rescore_left": _stats(resc),
           "ratio_torch_over_hip": round(float(np.median(tor) / np.median(hip)), 2),
           "launches_per_step": 5 * BLOCKS[0] + 3,
           "ms_per_live_step": round(float(np.median(live)) / steps, 4),
           "dead_tail_ms": round(float(np.median(hip) - np.median(live)), 3),
           "dead_tail_us_per_step": round(float(np.median(hip) - np.median(live)) * 1e3 / max(TP - steps, 1), 2),
           "workspace_bytes": r.decode_workspace_bytes(B, TP, BEAM, TP),
           "same_best_hypothesis_as_torch": f"{same}/{B}",
           "max_abs_best_score_difference_to_torch": round(float((res["scores"][:, 0] - t_sc[:, 0]).abs().max()), 6)}
    cw = _arg("--ctc-weight", 0.0, float)
    if cw > 0:
        import joint_search_cases as jc
        rng = np.random.default_rng(1000 + B)
        tab = np.stack([jc._peaked(rng, TP, TP, V, 0, rng.integers(1, V - 1, int(rng.integers(30, 41))).tolist(), 0.9)
                        for _ in range(B)]).astype(np.float32)
        probs = torch.from_numpy(tab).cuda()
        jres = r.decode(memory, None, BEAM, TP, ctc_probs=probs, ctc_weight=cw)
        jsteps = int(jres["steps_run"].cpu()[0])
        jlens = jres["lens"].cpu().numpy()
        jhip = _timed(lambda: r.decode(memory, None, BEAM, TP, ctc_probs=probs, ctc_weight=cw), reps, warmup)
        jlive = _timed(lambda: r.decode(memory, None, BEAM, jsteps, ctc_probs=probs, ctc_weight=cw), reps, warmup)
        xlog = torch.log(probs.clamp(min=float(np.finfo(np.float32).tiny)))
        jtor = _timed(lambda: torch_search(o32, memory, None, BEAM, TP, (xlog, 0, cw)), reps, warmup)
        j_tok, j_sc, j_steps = torch_search(o32, memory, None, BEAM, TP, (xlog, 0, cw))
        jsame = 0
        for b in range(B):
            n = int(jlens[b, 0])
            row = j_tok[b, 0].cpu().numpy()
            jsame += int(row[:n].tolist() == jres["tokens"][b, 0, :n].cpu().tolist() and (row[n:] == V - 1).all())
        rec.update({"ctc_weight": cw, "joint_steps_run": jsteps, "torch_joint_steps": j_steps,
                    "joint_best_hypothesis_tokens_min_mean_max": [int(jlens[:, 0].min()), round(float(jlens[:, 0].mean()), 1),
                                                                  int(jlens[:, 0].max())],
                    "hip_joint": _stats(jhip), "hip_joint_live": _stats(jlive),
                    "torch_joint_f32": _stats(jtor),
                    "ratio_torch_joint_over_hip_joint": round(float(np.median(jtor) / np.median(jhip)), 2),
                    "joint_launches_per_step": 5 * BLOCKS[0] + 5,
                    "joint_ms_per_live_step": round(float(np.median(jlive)) / jsteps, 4),
                    "joint_workspace_bytes": r.decode_workspace_bytes(B, TP, BEAM, TP, joint=True),
                    "joint_same_best_hypothesis_as_torch": f"{jsame}/{B}",
                    "joint_max_abs_best_score_difference_to_torch": round(float((jres["scores"][:, 0] - j_sc[:, 0]).abs().max()), 6)})
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
