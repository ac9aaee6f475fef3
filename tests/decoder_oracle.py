"""Plain torch restatement of the reference's attention decoder (transformer/decoder.py: BiTransformerDecoder =
two TransformerDecoders of pre-norm DecoderLayers, `after_norm`, `output_layer`) and of WeNet's attention-rescoring score,
taking a dtype: float64 is the yardstick of the rescoring tests, float32 their floor.  One hypothesis at a time, so
that no padding, batch mask or launch shape takes part.

    sos = eos = V - 1
    left  input [sos, y0 .. y(n-1)], targets [y0 .. y(n-1), eos]
    right input [sos, y(n-1) .. y0], targets [y(n-1) .. y0, eos]
    att   = sum_j log_softmax(logits[j])[target_j]
    total = (1 - reverse_weight) * att + reverse_weight * r_att + ctc_weight * (-ctc_score)

`mut` names one deliberate bug (tests/test_rescore_oracle_cpu.py): MUTATIONS are bugs of the decoder's definition, EDGE_MUTATIONS
what a kernel could plausibly get wrong at a tile edge (a key tile, a key slice, a key / value slot, an FFN chunk, a
vocabulary tile, a tie) or on trained-like weights (fp32 one-pass LayerNorm statistics, a softmax without its maximum).

`rec` (a dict, set by decoder_cases.conditioning) collects what the trained-like cases state about themselves: the
smallest |row mean| / row std a LayerNorm saw, the widest attention-score row and the widest logit row."""
import math

import numpy as np
import torch

MUTATIONS = ("causal_no_diagonal", "one_frame_past_out_lens", "no_eos", "left_embedding_for_right", "no_after_norm",
             "no_sqrt_d")
EDGE_MUTATIONS = ("cross_keys_first_tile_only", "cross_every_eighth_slice_dropped", "right_reads_left_kv_slot",
                  "ffn_last_chunk_dropped", "target_column_mod_256", "vocab_padded_columns_counted", "last_index_on_tie",
                  "best_among_first_64", "ln_one_pass", "softmax_without_max")
EPS = 1e-12  # LayerNorm(epsilon=1e-12) of decoder.py


def pe_table(n, d, dtype):
    """PositionalEncoding.__init__ (conformer/embedding.py), computed in float32 as the reference and the library do"""
    pe = torch.zeros(n, d, dtype=torch.float32)
    pos = torch.arange(0, n, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe.to(dtype)


class DecoderOracle:
    def __init__(self, sd, vocab_size, num_blocks, r_num_blocks, heads=4, dtype=torch.float64, mut=None):
        assert mut is None or mut in MUTATIONS + EDGE_MUTATIONS, mut
        self.V, self.H, self.dtype, self.mut = vocab_size, heads, dtype, mut
        self.rec = None
        self.blocks = {"left": num_blocks, "right": r_num_blocks}
        self.w = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if k.startswith("decoder.")}
        self.d = self.w["decoder.left_decoder.embed.0.weight"].shape[1]
        self.pe = pe_table(512, self.d, dtype)

    def _ln(self, x, prefix):
        g, b = self.w[prefix + ".weight"], self.w[prefix + ".bias"]
        if self.rec is not None:
            r = x.double()
            ratio = r.mean(-1).abs() / r.std(-1, unbiased=False).clamp_min(1e-300)
            self.rec["ln"] = min(self.rec["ln"], float(ratio.min()))
        if self.mut == "ln_one_pass":  # fp32 statistics, var = max(E[x^2] - E[x]^2, 0)
            x32 = x.to(torch.float32)
            mu = x32.mean(-1, keepdim=True)
            var = ((x32 * x32).mean(-1, keepdim=True) - mu * mu).clamp_min(0.0)
            return ((x32 - mu) * torch.rsqrt(var + np.float32(EPS))).to(x.dtype) * g + b
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) / torch.sqrt(var + EPS) * g + b

    def _softmax(self, s, mask):
        """softmax over the last axis of s [.., Lk] with mask (True = attend) already applied as -inf"""
        if self.mut == "softmax_without_max":  # fp32 exp(s) / sum exp(s): inf / inf or 0 / 0 once |s| passes ~88
            e = torch.exp(s.to(torch.float32)).masked_fill(~mask, 0.0)
            return (e / e.sum(-1, keepdim=True)).to(s.dtype)
        return torch.softmax(s, -1)

    def _lin(self, x, prefix):
        return x @ self.w[prefix + ".weight"] + self.w[prefix + ".bias"]  # Paddle Linear: weight [in, out]

    def _mha(self, q_in, kv_in, mask, prefix, kv_prefix=None):
        """MultiHeadedAttention.forward (conformer/attention.py): mask [Lq, Lk] bool, True = attend; kv_prefix: the
        attention whose linear_k / linear_v are used (a mutation; None: the attention's own)"""
        Lq, Lk, H = q_in.shape[0], kv_in.shape[0], self.H
        dk = self.d // H
        kvp = kv_prefix or prefix
        q = self._lin(q_in, prefix + ".linear_q").reshape(Lq, H, dk).transpose(0, 1)
        k = self._lin(kv_in, kvp + ".linear_k").reshape(Lk, H, dk).transpose(0, 1)
        v = self._lin(kv_in, kvp + ".linear_v").reshape(Lk, H, dk).transpose(0, 1)
        s = q @ k.transpose(1, 2) / math.sqrt(dk)
        if self.rec is not None and Lk > 0:
            hi = s.masked_fill(~mask[None], float("-inf")).amax(-1)
            lo = s.masked_fill(~mask[None], float("inf")).amin(-1)
            spread = (hi - lo)[torch.isfinite(hi - lo)]
            if spread.numel():
                self.rec["score"] = max(self.rec["score"], float(spread.max()))
        s = s.masked_fill(~mask[None], float("-inf"))
        a = self._softmax(s, mask[None].expand_as(s))
        a = torch.nan_to_num(a, nan=0.0).masked_fill(~mask[None], 0.0)  # a row without keys attends to nothing
        ctx = (a @ v).transpose(0, 1).reshape(Lq, self.d)
        return self._lin(ctx, prefix + ".linear_out")

    def logits(self, memory, out_len, tokens, right=False):
        """one hypothesis -> [len(tokens) + 1, V] pre-softmax outputs of the left (right) decoder"""
        side = "right" if right else "left"
        p = f"decoder.{side}_decoder"
        toks = list(tokens)[::-1] if right else list(tokens)
        ys_in = torch.tensor([self.V - 1] + toks, dtype=torch.long)
        n = ys_in.shape[0]
        emb_side = "left" if (right and self.mut == "left_embedding_for_right") else side
        x = self.w[f"decoder.{emb_side}_decoder.embed.0.weight"][ys_in]
        x = x * (1.0 if self.mut == "no_sqrt_d" else math.sqrt(self.d)) + self.pe[:n]
        Tp = memory.shape[0]
        keys = min(int(out_len) + (1 if self.mut == "one_frame_past_out_lens" else 0), Tp)
        mem = torch.as_tensor(np.asarray(memory)).to(self.dtype)[:keys]
        if self.mut == "cross_keys_first_tile_only":
            mem = mem[:64]
        elif self.mut == "cross_every_eighth_slice_dropped":
            mem = mem[torch.arange(mem.shape[0]) % 8 != 7]
        keys = mem.shape[0]
        causal = torch.tril(torch.ones(n, n, dtype=torch.bool), diagonal=-1 if self.mut == "causal_no_diagonal" else 0)
        full = torch.ones(n, keys, dtype=torch.bool)
        for i in range(self.blocks[side]):
            lp = f"{p}.decoders.{i}"
            y = self._ln(x, lp + ".norm1")
            x = x + self._mha(y, y, causal, lp + ".self_attn")
            kvp = None
            if right and self.mut == "right_reads_left_kv_slot":
                kvp = f"decoder.left_decoder.decoders.{min(i, self.blocks['left'] - 1)}.src_attn"
            x = x + self._mha(self._ln(x, lp + ".norm2"), mem, full, lp + ".src_attn", kvp)
            y = self._ln(x, lp + ".norm3")
            h = torch.relu(self._lin(y, lp + ".feed_forward.w_1"))
            if self.mut == "ffn_last_chunk_dropped":
                h = torch.cat([h[:, :-256], torch.zeros_like(h[:, -256:])], 1)
            x = x + self._lin(h, lp + ".feed_forward.w_2")
        if self.mut != "no_after_norm":
            x = self._ln(x, p + ".after_norm")
        return self._lin(x, p + ".output_layer")

    def token_logp(self, memory, out_len, tokens, right=False):
        """-> (log-probabilities of the targets [n + 1], logits [n + 1, V])"""
        lg = self.logits(memory, out_len, tokens, right)
        toks = list(tokens)[::-1] if right else list(tokens)
        tgt = torch.tensor(toks + [self.V - 1], dtype=torch.long)
        if self.rec is not None:
            self.rec["logit"] = max(self.rec["logit"], float((lg.amax(-1) - lg.amin(-1)).max()))
        if self.mut == "softmax_without_max":  # fp32 log(exp(v) / sum exp(v))
            e = torch.exp(lg.to(torch.float32))
            lsm = torch.log(e / e.sum(-1, keepdim=True)).to(lg.dtype)
        elif self.mut == "vocab_padded_columns_counted":  # the columns V .. Vp - 1 of the last 256-column tile, logit 0
            pad = (self.V + 255) // 256 * 256 - self.V
            lsm = lg - torch.logsumexp(torch.cat([lg, torch.zeros(lg.shape[0], pad, dtype=lg.dtype)], 1), -1, keepdim=True)
        else:
            lsm = torch.log_softmax(lg, -1)
        if self.mut == "target_column_mod_256":  # the target's logit from the column's place in its tile
            lp = lg.gather(1, (tgt % 256)[:, None])[:, 0] - (lg - lsm)[:, 0]
        else:
            lp = lsm.gather(1, tgt[:, None])[:, 0]
        if self.mut == "no_eos":
            lp = torch.cat([lp[:-1], torch.zeros(1, dtype=lp.dtype)])
        return lp, lg

    def to(self, device):
        """weights and positional table on `device` (rescore_batched: the torch stand-in of tools/bench_rescore.py)"""
        self.w = {k: v.to(device) for k, v in self.w.items()}
        self.pe = self.pe.to(device)
        return self

    def _mha_b(self, q_in, kv_in, mask, prefix):
        """_mha over a padded batch: q_in [N, Lq, d], kv_in [N, Lk, d], mask [N, Lq or 1, Lk]"""
        N, Lq, Lk, H = q_in.shape[0], q_in.shape[1], kv_in.shape[1], self.H
        dk = self.d // H
        q = self._lin(q_in, prefix + ".linear_q").reshape(N, Lq, H, dk).transpose(1, 2)
        k = self._lin(kv_in, prefix + ".linear_k").reshape(N, Lk, H, dk).transpose(1, 2)
        v = self._lin(kv_in, prefix + ".linear_v").reshape(N, Lk, H, dk).transpose(1, 2)
        s = (q @ k.transpose(2, 3) / math.sqrt(dk)).masked_fill(~mask[:, None], float("-inf"))
        a = torch.nan_to_num(torch.softmax(s, -1), nan=0.0).masked_fill(~mask[:, None], 0.0)
        return self._lin((a @ v).transpose(1, 2).reshape(N, Lq, self.d), prefix + ".linear_out")

    def rescore_batched(self, memory, out_lens, tokens, lens, ctc_scores, ctc_weight, reverse_weight):
        """The same scores the way the reference's own forward computes them: every hypothesis padded to max_tokens + 1
        rows, the memory repeated per hypothesis, the [B * nbest, L, V] logits materialised.  Tensors on the oracle's
        device in, (att, r_att, total, best) tensors out; no mutations."""
        B, nbest, mt = tokens.shape
        N, L, V, dev = B * nbest, mt + 1, self.V, memory.device
        ln = lens.reshape(N).long()
        n = ln.clamp(min=0)
        tok = tokens.reshape(N, mt).long()
        pos = torch.arange(L, device=dev)
        mem = memory.to(self.dtype).repeat_interleave(nbest, 0)
        Tp = mem.shape[1]
        ol = torch.full((B,), Tp, device=dev) if out_lens is None else out_lens.long()
        mem_mask = (torch.arange(Tp, device=dev)[None] < ol.repeat_interleave(nbest)[:, None])[:, None]  # [N, 1, Tp]
        tgt_mask = (pos[None] <= n[:, None])[:, None] & torch.tril(torch.ones(L, L, dtype=torch.bool, device=dev))[None]
        rev_idx = (n[:, None] - 1 - pos[None, :mt]).clamp(min=0)
        sides = [("left", tok)] + ([("right", tok.gather(1, rev_idx))] if reverse_weight > 0 else [])
        scores = []
        for side, y in sides:
            p = f"decoder.{side}_decoder"
            valid = pos[None, :mt] < n[:, None]
            y = torch.where(valid, y, torch.full_like(y, V - 1))
            ys_in = torch.cat([torch.full((N, 1), V - 1, device=dev, dtype=torch.long), y], 1)
            ys_out = torch.cat([y, torch.full((N, 1), V - 1, device=dev, dtype=torch.long)], 1)
            x = self.w[p + ".embed.0.weight"][ys_in] * math.sqrt(self.d) + self.pe[:L]
            for i in range(self.blocks[side]):
                lp = f"{p}.decoders.{i}"
                h = self._ln(x, lp + ".norm1")
                x = x + self._mha_b(h, h, tgt_mask, lp + ".self_attn")
                x = x + self._mha_b(self._ln(x, lp + ".norm2"), mem, mem_mask, lp + ".src_attn")
                h = self._ln(x, lp + ".norm3")
                x = x + self._lin(torch.relu(self._lin(h, lp + ".feed_forward.w_1")), lp + ".feed_forward.w_2")
            lg = self._lin(self._ln(x, p + ".after_norm"), p + ".output_layer")
            lp_ = torch.log_softmax(lg, -1).gather(2, ys_out[:, :, None])[:, :, 0]
            scores.append((lp_ * (pos[None] <= n[:, None])).double().sum(1))
        att = scores[0]
        r_att = scores[1] if len(scores) > 1 else torch.zeros_like(att)
        total = (1.0 - reverse_weight) * att + reverse_weight * r_att - ctc_weight * ctc_scores.reshape(N)
        total = torch.where(ln < 0, torch.full_like(total, float("-inf")), total)
        zero = torch.zeros_like(att)
        att, r_att = torch.where(ln < 0, zero, att), torch.where(ln < 0, zero, r_att)
        return (att.reshape(B, nbest), r_att.reshape(B, nbest), total.reshape(B, nbest),
                total.reshape(B, nbest).argmax(1).to(torch.int32))

    def rescore(self, memory, out_lens, tokens, lens, ctc_scores, ctc_weight, reverse_weight):
        """The arguments of ppasr_rescore as numpy arrays -> dict of numpy float64 arrays in its output layouts
        (att, r_att, total [B, nbest]; best [B]; token_logp [B, nbest, 2, max_tokens + 1]; logits [.., V], zeros where
        there is no row)."""
        B, nbest, mt = tokens.shape
        L = mt + 1
        att = np.zeros((B, nbest))
        r_att = np.zeros((B, nbest))
        total = np.full((B, nbest), -np.inf)
        tlp = np.zeros((B, nbest, 2, L))
        lgs = np.zeros((B, nbest, 2, L, self.V))
        for b in range(B):
            ol = memory.shape[1] if out_lens is None else int(out_lens[b])
            for k in range(nbest):
                n = int(lens[b, k])
                if n < 0:
                    continue
                y = [int(t) for t in tokens[b, k, :n]]
                for side in range(2 if reverse_weight > 0 else 1):
                    lp, lg = self.token_logp(memory[b], ol, y, right=bool(side))
                    tlp[b, k, side, :n + 1] = lp.double().numpy()
                    lgs[b, k, side, :n + 1] = lg.double().numpy()
                    (r_att if side else att)[b, k] = float(lp.double().sum())
                total[b, k] = ((1.0 - reverse_weight) * att[b, k] + reverse_weight * r_att[b, k]
                               + ctc_weight * (-float(ctc_scores[b, k])))
        best = total.argmax(1)  # the lowest index on a tie
        if self.mut == "last_index_on_tie":
            best = total.shape[1] - 1 - total[:, ::-1].argmax(1)
        elif self.mut == "best_among_first_64":  # the argmax without the stride over k_dec_score's 64 threads
            best = total[:, :64].argmax(1)
        return dict(att=att, r_att=r_att, total=total, best=best.astype(np.int32), token_logp=tlp, logits=lgs)
