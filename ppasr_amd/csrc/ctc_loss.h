// ctc_loss.h -- CTC negative log-likelihood (ctc_loss.hip): the workspace and the launcher behind ppasr_ctc_loss.
#pragma once
#include "ctc_align.h"

namespace ppasr {

// The workspace is the alignment's emission rows alone: f32 [B][Tp][align_row_stride(max_tokens)].
inline size_t ctc_loss_workspace(int B, int Tp, int max_tokens) {
  const size_t n = ((size_t)B * Tp * align_row_stride(max_tokens) * sizeof(float) + 255) / 256 * 256;
  return n > 0 ? n : 256;
}

// Queues the gather (launch_ctc_gather) and the forward chain on `st`.  Arguments as ppasr_ctc_loss, already validated.
void launch_ctc_loss(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                     const int32_t* n_tokens, int max_tokens, float* nll, int32_t* status, void* workspace, hipStream_t st);

}  // namespace ppasr
