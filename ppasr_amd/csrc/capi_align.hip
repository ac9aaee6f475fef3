// capi_align.hip -- C-ABI of CTC forced alignment: ppasr_ctc_align_workspace_bytes and ppasr_ctc_align (ctc_align.hip),
// and of the CTC negative log-likelihood over the same trellis: ppasr_ctc_loss_workspace_bytes and ppasr_ctc_loss
// (ctc_loss.hip).
#include "capi_internal.h"
#include "ctc_align.h"
#include "ctc_loss.h"

extern "C" {

size_t ppasr_ctc_align_workspace_bytes(int B, int Tp, int max_tokens) {
  if (B <= 0 || Tp < 0 || max_tokens < 0 || max_tokens > kAlignMaxTokens) return 0;
  return align_layout(B, Tp, max_tokens).total;
}

ppasr_status ppasr_ctc_align(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank,
                             const int32_t* tokens, const int32_t* n_tokens, int max_tokens, int32_t* frame_token, int32_t* begin,
                             int32_t* end, int32_t* peak, float* conf, float* score, int32_t* status, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (B <= 0 || Tp < 0 || V < 2 || max_tokens < 0) return fail(PPASR_EINVAL, "ctc_align: bad shape (B > 0, Tp >= 0, V >= 2, max_tokens >= 0)");
  if (blank < 0 || blank >= V) return fail(PPASR_EINVAL, "ctc_align: blank outside [0, V)");
  if (max_tokens > kAlignMaxTokens)
    return fail(PPASR_EUNSUPPORTED, "ctc_align: max_tokens exceeds the 255 tokens per utterance the kernel is built for");
  if (!n_tokens || !score || !status || !workspace || (Tp > 0 && (!probs || !frame_token)) || (max_tokens > 0 && !tokens))
    return fail(PPASR_EINVAL, "ctc_align: null argument");
  if ((size_t)B * Tp > (size_t)1 << 26) return fail(PPASR_EUNSUPPORTED, "ctc_align: batch too large (B * Tp > 2^26)");
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(PPASR_EINVAL, "ctc_align: workspace must be 16-byte aligned");
  if (workspace_bytes < ppasr_ctc_align_workspace_bytes(B, Tp, max_tokens))
    return fail(PPASR_EINVAL, "ctc_align: workspace too small (ppasr_ctc_align_workspace_bytes)");
  launch_ctc_align(probs, frame_lens, B, Tp, V, blank, tokens, n_tokens, max_tokens, frame_token, begin, end, peak, conf, score,
                   status, workspace, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

size_t ppasr_ctc_loss_workspace_bytes(int B, int Tp, int max_tokens) {
  if (B <= 0 || Tp < 0 || max_tokens < 0 || max_tokens > kAlignMaxTokens) return 0;
  return ctc_loss_workspace(B, Tp, max_tokens);
}

ppasr_status ppasr_ctc_loss(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                            const int32_t* n_tokens, int max_tokens, float* nll, int32_t* status, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (B <= 0 || Tp < 0 || V < 2 || max_tokens < 0) return fail(PPASR_EINVAL, "ctc_loss: bad shape (B > 0, Tp >= 0, V >= 2, max_tokens >= 0)");
  if (blank < 0 || blank >= V) return fail(PPASR_EINVAL, "ctc_loss: blank outside [0, V)");
  if (max_tokens > kAlignMaxTokens)
    return fail(PPASR_EUNSUPPORTED, "ctc_loss: max_tokens exceeds the 255 tokens per utterance the kernel is built for");
  if (!n_tokens || !nll || !status || !workspace || (Tp > 0 && !probs) || (max_tokens > 0 && !tokens))
    return fail(PPASR_EINVAL, "ctc_loss: null argument");
  if ((size_t)B * Tp > (size_t)1 << 26) return fail(PPASR_EUNSUPPORTED, "ctc_loss: batch too large (B * Tp > 2^26)");
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(PPASR_EINVAL, "ctc_loss: workspace must be 16-byte aligned");
  if (workspace_bytes < ppasr_ctc_loss_workspace_bytes(B, Tp, max_tokens))
    return fail(PPASR_EINVAL, "ctc_loss: workspace too small (ppasr_ctc_loss_workspace_bytes)");
  launch_ctc_loss(probs, frame_lens, B, Tp, V, blank, tokens, n_tokens, max_tokens, nll, status, workspace,
                  static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

}  // extern "C"
