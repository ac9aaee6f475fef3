// capi_attdecode.hip -- C-ABI of attention beam-search decoding on an existing rescorer (attn_decode.hip) and of its
// CTC-joint mode (attn_decode_joint.hip).
#include "attn_decode.h"
#include "capi_internal.h"
#include "rescorer_handle.h"

namespace {

constexpr size_t al256(size_t n) { return (n + 255) / 256 * 256; }

// workspace offsets in bytes: the plain search's share up to `total`, the joint mode's behind it up to `joint_total`
struct AttDecLayout {
  size_t x, q, ctx, qc, kv, cache, logits, cand_lp, cand_tok, score[2], ended[2], anc[2], live, last_tok, utt_live, utt_steps,
      tr_par, tr_tok, tr_lp, total;
  size_t state[2], psi[2], cpsi, cand_att, cand_psi, tr_ctc, joint_total;
};
AttDecLayout attdec_layout(const ppasr_rescorer_s* r, const AttDecDims& d) {
  AttDecLayout l;
  const size_t R = d.R(), Rp = d.Rp(), L = r->desc.num_blocks;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += al256(bytes);
    return at;
  };
  l.x = take(Rp * kD * 4);
  l.q = take(Rp * kD * 4);
  l.ctx = take(Rp * kD * 4);
  l.qc = take(Rp * kD * 4);
  l.kv = take((size_t)d.B * d.Tp * 512 * L * 4);
  l.cache = take(L * d.P * R * 512 * 4);
  l.logits = take(Rp * r->W.Vp * 4);
  l.cand_lp = take(R * d.N * 4);
  l.cand_tok = take(R * d.N * 4);
  for (int i = 0; i < 2; ++i) {
    l.score[i] = take(R * 8);
    l.ended[i] = take(R * 4);
    l.anc[i] = take(R * 256);
  }
  l.live = take(Rp * 4);
  l.last_tok = take(Rp * 4);
  l.utt_live = take((size_t)d.B * 4);
  l.utt_steps = take((size_t)d.B * 4);
  l.tr_par = take((size_t)d.P * R * 4);
  l.tr_tok = take((size_t)d.P * R * 4);
  l.tr_lp = take((size_t)d.P * R * 4);
  l.total = o;
  for (int i = 0; i < 2; ++i) {
    l.state[i] = take(R * d.Tp * 2 * 4);
    l.psi[i] = take(R * 4);
  }
  l.cpsi = take(R * r->W.Vp * 4);
  l.cand_att = take(R * d.N * 4);
  l.cand_psi = take(R * d.N * 4);
  l.tr_ctc = take((size_t)d.P * R * 4);
  l.joint_total = o;
  return l;
}

AttDecBufs attdec_bufs(void* workspace, const AttDecLayout& l) {
  char* ws = static_cast<char*>(workspace);
  auto f = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
  auto i32 = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
  AttDecBufs bf;
  bf.x = f(l.x);
  bf.q = f(l.q);
  bf.ctx = f(l.ctx);
  bf.qc = f(l.qc);
  bf.kv = f(l.kv);
  bf.cache = f(l.cache);
  bf.logits = f(l.logits);
  bf.cand_lp = f(l.cand_lp);
  bf.cand_tok = i32(l.cand_tok);
  for (int i = 0; i < 2; ++i) {
    bf.score[i] = reinterpret_cast<double*>(ws + l.score[i]);
    bf.ended[i] = i32(l.ended[i]);
    bf.anc[i] = reinterpret_cast<uint8_t*>(ws + l.anc[i]);
  }
  bf.live = i32(l.live);
  bf.last_tok = i32(l.last_tok);
  bf.utt_live = i32(l.utt_live);
  bf.utt_steps = i32(l.utt_steps);
  bf.tr_par = i32(l.tr_par);
  bf.tr_tok = i32(l.tr_tok);
  bf.tr_lp = f(l.tr_lp);
  return bf;
}

bool attdec_shape_ok(int B, int Tp, int beam_size, int max_steps) {
  return B > 0 && Tp > 0 && beam_size >= 1 && beam_size <= kAttDecMaxBeam && max_steps >= 1 && max_steps + 1 <= kRescoreMaxRows &&
         (size_t)B * beam_size <= ((size_t)1 << 20) && (size_t)B * Tp <= ((size_t)1 << 24);
}

// one call of either entry point; jb == nullptr: the plain search, else the caller's inputs and taps of the joint mode
// (its workspace views are filled in here)
ppasr_status attdec_run(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B, int Tp, int beam_size,
                        int max_steps, const AttDecOut& out, AttJointBufs* jb, void* workspace, size_t workspace_bytes,
                        void* stream) {
  if (!r) return fail(PPASR_EINVAL, "null rescorer");
  if (!memory || !out.tokens || !out.lens || !out.scores || !out.ended || !out.steps_run || !workspace)
    return fail(PPASR_EINVAL, "null argument");
  if (B <= 0 || Tp <= 0 || max_steps < 1) return fail(PPASR_EINVAL, "bad shape");
  if (beam_size < 1 || beam_size > r->desc.vocab_size) return fail(PPASR_EINVAL, "beam_size outside [1, vocab_size]");
  if (beam_size > kAttDecMaxBeam) return fail(PPASR_EUNSUPPORTED, "beam_size above the 32 the selection is built for");
  if (max_steps + 1 > r->desc.max_len) return fail(PPASR_EUNSUPPORTED, "max_steps + 1 exceeds the positional table (max_len)");
  if (max_steps + 1 > kRescoreMaxRows)
    return fail(PPASR_EUNSUPPORTED, "max_steps + 1 exceeds the 256 rows per hypothesis the kernels are built for");
  if (!attdec_shape_ok(B, Tp, beam_size, max_steps)) return fail(PPASR_EUNSUPPORTED, "batch too large");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(PPASR_EINVAL, "workspace not 16-byte aligned");
  const AttDecDims d{B, Tp, beam_size, max_steps};
  const AttDecLayout l = attdec_layout(r, d);
  if (workspace_bytes < (jb ? l.joint_total : l.total))
    return fail(PPASR_ENOSPACE, jb ? "workspace too small (ppasr_attention_decode_joint_workspace_bytes)"
                                   : "workspace too small (ppasr_attention_decode_workspace_bytes)");
  const AttDecBufs bf = attdec_bufs(workspace, l);
  if (jb) {
    char* ws = static_cast<char*>(workspace);
    auto f = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    for (int i = 0; i < 2; ++i) {
      jb->state[i] = f(l.state[i]);
      jb->psi[i] = f(l.psi[i]);
    }
    jb->cpsi = f(l.cpsi);
    jb->cand_att = f(l.cand_att);
    jb->cand_psi = f(l.cand_psi);
    jb->tr_ctc = f(l.tr_ctc);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY(configure_attention_decode_kernels());  // (a per-device attribute)
  // the taps are defined everywhere: -1 / 0.0 where the search wrote nothing
  const size_t tn = (size_t)max_steps * B * beam_size;
  if (out.trace_parent) HIP_TRY(hipMemsetAsync(out.trace_parent, 0xff, tn * sizeof(int32_t), st));
  if (out.trace_token) HIP_TRY(hipMemsetAsync(out.trace_token, 0xff, tn * sizeof(int32_t), st));
  if (out.trace_score) HIP_TRY(hipMemsetAsync(out.trace_score, 0, tn * sizeof(double), st));
  if (jb && jb->trace_ctc) HIP_TRY(hipMemsetAsync(jb->trace_ctc, 0, tn * sizeof(float), st));
  launch_attention_decode(r->W, d, bf, jb, memory, out_lens, out, st);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

}  // namespace

extern "C" {

size_t ppasr_attention_decode_workspace_bytes(ppasr_rescorer r, int B, int Tp, int beam_size, int max_steps) {
  if (!r || !attdec_shape_ok(B, Tp, beam_size, max_steps)) return 0;
  return attdec_layout(r, AttDecDims{B, Tp, beam_size, max_steps}).total;
}

ppasr_status ppasr_attention_decode(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B, int Tp, int beam_size,
                                    int max_steps, int32_t* tokens, int32_t* lens, double* scores, int32_t* ended,
                                    int32_t* steps_run, float* token_logp, int32_t* trace_parent, int32_t* trace_token,
                                    double* trace_score, void* workspace, size_t workspace_bytes, void* stream) {
  const AttDecOut out{tokens, lens, scores, ended, steps_run, token_logp, trace_parent, trace_token, trace_score};
  return attdec_run(r, memory, out_lens, B, Tp, beam_size, max_steps, out, nullptr, workspace, workspace_bytes, stream);
}

size_t ppasr_attention_decode_joint_workspace_bytes(ppasr_rescorer r, int B, int Tp, int beam_size, int max_steps) {
  if (!r || !attdec_shape_ok(B, Tp, beam_size, max_steps)) return 0;
  return attdec_layout(r, AttDecDims{B, Tp, beam_size, max_steps}).joint_total;
}

ppasr_status ppasr_attention_decode_joint(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B, int Tp,
                                          int beam_size, int max_steps, const float* ctc_probs, int V_ctc, int blank,
                                          double ctc_weight, int32_t* tokens, int32_t* lens, double* scores, int32_t* ended,
                                          int32_t* steps_run, float* token_logp, float* token_ctc, int32_t* trace_parent,
                                          int32_t* trace_token, double* trace_score, float* trace_ctc, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  if (!r) return fail(PPASR_EINVAL, "null rescorer");
  if (!(ctc_weight >= 0.0)) return fail(PPASR_EINVAL, "ctc_weight negative or NaN");
  if (V_ctc != r->desc.vocab_size) return fail(PPASR_EINVAL, "V_ctc differs from the decoder's vocab_size");
  if (blank < 0 || blank >= V_ctc - 1) return fail(PPASR_EINVAL, "blank outside [0, V - 1)");
  if (!ctc_probs && ctc_weight > 0.0) return fail(PPASR_EINVAL, "null ctc_probs with ctc_weight > 0");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float w = (float)ctc_weight;
  if (w == 0.0f) {  // the plain search, bit for bit: no CTC kernel, no 0 * inf
    const ppasr_status rc = ppasr_attention_decode(r, memory, out_lens, B, Tp, beam_size, max_steps, tokens, lens, scores, ended,
                                                   steps_run, token_logp, trace_parent, trace_token, trace_score, workspace,
                                                   workspace_bytes, stream);
    if (rc != PPASR_OK) return rc;
    if (token_ctc) HIP_TRY(hipMemsetAsync(token_ctc, 0, (size_t)B * beam_size * (max_steps + 1) * sizeof(float), st));
    if (trace_ctc) HIP_TRY(hipMemsetAsync(trace_ctc, 0, (size_t)max_steps * B * beam_size * sizeof(float), st));
    return PPASR_OK;
  }
  AttJointBufs jb{};
  jb.probs = ctc_probs;
  jb.out_lens = out_lens;
  jb.V = V_ctc;
  jb.blank = blank;
  jb.weight = w;
  jb.token_ctc = token_ctc;
  jb.trace_ctc = trace_ctc;
  const AttDecOut out{tokens, lens, scores, ended, steps_run, token_logp, trace_parent, trace_token, trace_score};
  return attdec_run(r, memory, out_lens, B, Tp, beam_size, max_steps, out, &jb, workspace, workspace_bytes, stream);
}

}  // extern "C"
